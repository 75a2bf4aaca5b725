"""The owner of every long-lived device allocation (csrc/device_buf.h) and the records that hold their memory through it:
tools/device_buf_host_check.cpp, built with the host sanitizers over malloc-backed runtime calls and run as a program of its own
(no GPU, no HIP runtime, no libvfsms)."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_device_buf_grow_rule_moves_and_canvas_ownership(tmp_path):
    src = os.path.join(ROOT, "tools", "device_buf_host_check.cpp")
    exe = str(tmp_path / "device_buf_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, with nothing preloaded
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    m = re.search(r"device_buf_host_check: (\d+) log checks ok", p.stdout)
    assert m and int(m.group(1)) >= 30, p.stdout + p.stderr
