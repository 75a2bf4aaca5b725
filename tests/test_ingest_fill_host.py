"""The transaction behind every vfsms_tile_fill* entry (csrc/ingest_fill.h): tools/ingest_fill_host_check.cpp, built with the host
sanitizers over malloc-backed runtime calls and run as a program of its own (no GPU, no HIP runtime, no libvfsms).  It drives every row
of the behaviour table with failures injected at every position; a GPU test cannot, since the orderings show only when a call fails."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_tile_fill_transaction_orderings_under_injected_failures(tmp_path):
    src = os.path.join(ROOT, "tools", "ingest_fill_host_check.cpp")
    exe = str(tmp_path / "ingest_fill_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, with nothing preloaded
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    m = re.search(r"ingest_fill_host_check: (\d+) checks ok, (\d+) table rows x (\d+) injection positions", p.stdout)
    assert m, p.stdout + p.stderr
    checks, rows, positions = (int(g) for g in m.groups())
    assert rows >= 8 and positions >= 6 and checks >= rows * positions, p.stdout
