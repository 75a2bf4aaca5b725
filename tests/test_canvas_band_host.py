"""The band walk behind the four write-out routes of a canvas (csrc/canvas_band.h): tools/canvas_band_host_check.cpp, built with the host
sanitizers over malloc-backed runtime calls and run as a program of its own (no GPU, no HIP runtime, no libvfsms).  It drives the band
check and PyrPending -- the only state of the library that survives between calls -- against a brute-force model over a sweep of canvases,
with every refusal and with failures injected into the grow, and the driver of a band of the tile route (canvas_tile_band) over a stub coder:
the capacity protocol, which consumes nothing when there is too little room; a GPU test sees that state only through a whole walk."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_band_check_and_pending_rows_against_the_model(tmp_path):
    src = os.path.join(ROOT, "tools", "canvas_band_host_check.cpp")
    exe = str(tmp_path / "canvas_band_host_check")
    # the sanitizer runtimes linked into the program itself: it runs as it is, with nothing preloaded
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    m = re.search(r"canvas_band_host_check: (\d+) checks ok, (\d+) walks, (\d+) bands, (\d+) injected failures", p.stdout)
    assert m, p.stdout + p.stderr
    checks, walks, bands, injected = (int(g) for g in m.groups())
    # the sweep's own size: rows 1..80 x 3 widths x 2 channel counts x levels 0..3, each with the band lengths 16, 32 and 48 (all are
    # multiples of 2^levels <= 8) and at least one walk that switches to a longer band; a band asserts a dozen things and more
    canvases = 80 * 3 * 2 * 4
    sweep_bands = 3 * 2 * 4 * sum(-(-rows // n) for rows in range(1, 81) for n in (16, 32, 48))
    assert walks >= canvases * 4 and bands >= sweep_bands and checks >= 12 * bands, p.stdout
    # the grow fails once at its allocation, at a copy and at its synchronisation, for levels 1..3 and both channel counts
    assert injected >= 3 * 3 * 2, p.stdout
    # the driver of a band of the tile route over a stub coder: rows 1..80 x 2 channel counts x levels 0..3 at one width, in bands of 16 and of
    # 48 rows; every band is refused twice for want of room (a byte, a record) before it goes through
    m = re.search(r"injected failures, (\d+) driver bands \((\d+) capacity refusals\)", p.stdout)
    assert m, p.stdout + p.stderr
    driver_bands, refusals = (int(g) for g in m.groups())
    assert driver_bands >= 2 * 4 * sum(-(-rows // n) for rows in range(1, 81) for n in (16, 48)) and refusals >= 2 * driver_bands, p.stdout
