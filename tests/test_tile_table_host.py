"""The rules of the context's tile table (csrc/tile_table.h): tools/tile_table_host_check.cpp, built with the host sanitizers over
malloc-backed runtime calls and run as a program of its own (no GPU, no HIP runtime, no libvfsms).  It sends every short list over a pool
of tiles through tile_list under every rule and compares with a model of the order of checks, the runtime calls logged: a GPU test sees
that a call is refused, not whether it had already waited for a decoder thread or enqueued a stream wait by then."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_list_order_and_pool_return_under_injected_failures(tmp_path):
    src = os.path.join(ROOT, "tools", "tile_table_host_check.cpp")
    exe = str(tmp_path / "tile_table_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, with nothing preloaded
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    m = re.search(r"tile_table_host_check: (\d+) checks ok, (\d+) lists of up to (\d+) of (\d+) tiles x (\d+) ranges x (\d+) flags", p.stdout)
    assert m, p.stdout + p.stderr
    checks, lists, max_len, kinds, ranges, flags = (int(g) for g in m.groups())
    # the pool of the issue (five owned shapes, wrapped, pending, given up, unknown), lists of 0..4, two count ranges, the three rule
    # flags and the predicate; every list under every rule is at least three checks (the code, the message, the log)
    assert kinds >= 9 and max_len >= 4 and ranges >= 2 and flags >= 4, p.stdout
    assert lists == sum(kinds ** n for n in range(max_len + 1)), p.stdout
    assert checks >= 3 * lists * ranges * 2 ** flags, p.stdout
