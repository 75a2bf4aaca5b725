"""Every arena record's layout function counts and carves the same bytes: tools/arena_layout_host_check.cpp, built with the host
sanitizers against the library and run as a program of its own (no GPU, no HIP call)."""
import os
import re
import subprocess

import imagestitch_amd as isa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_layouts_count_and_carve_alike(tmp_path):
    if not os.path.exists(isa.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    src = os.path.join(ROOT, "tools", "arena_layout_host_check.cpp")
    exe = str(tmp_path / "arena_layout_host_check")
    libdir = os.path.dirname(isa.LIB_PATH)
    # the sanitizer runtimes linked into the program itself: it runs whatever else the loader brings along
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe,
           "-L", libdir, "-lvfsms", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    m = re.search(r"arena_layout_host_check: (\d+) records ok", p.stdout)
    assert m and int(m.group(1)) >= 80, p.stdout + p.stderr
