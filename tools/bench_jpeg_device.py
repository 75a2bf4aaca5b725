"""JPEG results encoded on the device (Method.jpegEncoder = "device") against the host path, on the headline mosaic, gray and colour, in
one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised, uploaded and fused (fade) into a canvas that stays in HBM.
Per mode (gray, B G R) the script times the streamed write-out of that canvas, from the first band request to the closed file, alternated
A B A B after warm-up:
  A  host:   Engine.canvas_download_bands -> JpegBandWriter, its pool sized by io._usable_cpus() (the CPUs this process may use, recorded),
             not os.cpu_count()
  B  device: Engine.canvas_encode_jpeg_bands -> DeviceJpegFile, at --restart-mcus
For leg B it records the bytes that crossed the link and the file size, and -- in a pass with the library's event profiler on, bands without a
file -- the split of the "jpeg_encode" stage into transform, entropy and copy.  The transform is set against its compulsory bytes (mosaic
in, int16 coefficients out) as a fraction of the 8 TB/s HBM figure the other benchmarks use; the entropy pass against its own (the
coefficients read twice -- counting, writing -- and the stream written once), which shows how far it is from a memory bound: its lanes
run jchuff.c's serial coder, one restart interval each.  Then leg B is swept over jpegRestartMcus in {1, 2, 4, 8, 16, 32, 64}: time and
file size.
Writes profiles/jpeg_device_bench.json and prints the same JSON line.

    python tools/bench_jpeg_device.py [--rows 10 --cols 9 --tile 2048 --steps 3 --warmup 1 --band-rows 4096 --restart-mcus 8]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_GBPS = 8000.0
SWEEP = (1, 2, 4, 8, 16, 32, 64)
STAGES = ("transform", "entropy", "copy")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--band-rows", type=int, default=4096)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--restart-mcus", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions per leg (at least 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_device_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 2)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd import io as IO
    from imagestitch_amd.synthetic import SyntheticGrid

    cpus = IO._usable_cpus()
    threads = min(cpus, 32)
    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    gray = grid.tiles(threads=min(16, cpus))
    n = grid.n_tiles
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    shapes = [(grid.th, grid.tw)] * n
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    geom = isa.Stitcher._placements(shapes, offs, offsetList, rangeX, rangeY, isa.Engine.CANVAS_MODES["fadeInAndFadeOut"])
    eng = isa.Engine(0)
    outdir = args.dir or tempfile.mkdtemp(prefix="vfsms_jpeg_")
    os.makedirs(outdir, exist_ok=True)

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 1), "ms_min": round(float(v.min()), 1), "ms_max": round(float(v.max()), 1)}

    res = {"metric": "streamed JPEG write-out of the headline mosaic: bands downloaded and encoded by libjpeg-turbo on the host (A) against "
                     "bands encoded on the device and appended to the file (B)",
           "grid": [args.rows, args.cols, args.tile], "mosaic": [rows, cols], "band_rows": args.band_rows, "quality": args.quality,
           "restart_mcus": args.restart_mcus, "usable_cpus": cpus, "host_encoder_threads": threads, "os_cpu_count": os.cpu_count(),
           "steps": args.steps, "warmup": args.warmup, "hbm_GBps": HBM_GBPS}
    try:
        for mode, ch in (("gray", 1), ("color", 3)):
            handles = [eng.tile_upload(t) if ch == 1 else eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in gray]
            canvas = eng.canvas_create(rows, cols, ch)
            eng.canvas_assemble_resident(canvas, handles, geom)
            eng.sync()
            full = (rows, cols, ch) if ch > 1 else (rows, cols)

            def leg_host():
                path = os.path.join(outdir, "a.jpg")
                w = isa.JpegBandWriter(path, quality=args.quality, threads=threads)
                t0 = time.perf_counter()
                for r0, band in eng.canvas_download_bands(canvas, rows, cols, ch, args.band_rows, transient=True):
                    w(r0, band, full)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size

            def leg_device(R):
                path = os.path.join(outdir, "b.jpg")
                t0 = time.perf_counter()
                f = IO.DeviceJpegFile(path, full, args.quality, R)
                link = 0
                for _r0, _n, payload in eng.canvas_encode_jpeg_bands(canvas, rows, cols, ch, args.quality, R, args.band_rows):
                    f.append(payload)
                    link += payload.size
                f.close()
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size, link

            a, b = [], []
            for k in range(args.warmup + args.steps):
                (ta, size_a), (tb, size_b, link_b) = leg_host(), leg_device(args.restart_mcus)
                if k >= args.warmup:
                    a.append(ta); b.append(tb)
            # the "jpeg_encode" stages by HIP events: the bands of leg B without a file
            eng.profile_enable(True)
            eng.profile_read(reset=True)
            for _ in eng.canvas_encode_jpeg_bands(canvas, rows, cols, ch, args.quality, args.restart_mcus, args.band_rows):
                pass
            prof = eng.profile_read(reset=True)
            eng.profile_enable(False)
            stage = {s_: round(prof.get("jpeg_encode." + s_, (0.0, 0))[0], 3) for s_ in STAGES}
            mcu = 16 if ch == 3 else 8
            coef_bytes = -(-rows // mcu) * -(-cols // mcu) * (6 if ch == 3 else 1) * 128
            r = {"mosaic_MB": round(rows * cols * ch / 1e6, 1),
                 "host": dict(stats(a), file_MB=round(size_a / 1e6, 1), link_MB=round(rows * cols * ch / 1e6, 1)),
                 "device": dict(stats(b), file_MB=round(size_b / 1e6, 1), link_MB=round(link_b / 1e6, 1)),
                 "device_over_host": round(float(np.median(b)) / float(np.median(a)), 3),
                 "jpeg_encode_stage_ms": stage}
            if stage["transform"] > 0:
                comp = rows * cols * ch + coef_bytes
                gbps = comp / stage["transform"] / 1e6
                r["transform"] = {"compulsory_MB": round(comp / 1e6, 1), "GBps_of_compulsory": round(gbps, 1), "fraction_of_hbm": round(gbps / HBM_GBPS, 3)}
            if stage["entropy"] > 0:
                comp = 2 * coef_bytes + link_b
                gbps = comp / stage["entropy"] / 1e6
                r["entropy"] = {"compulsory_MB": round(comp / 1e6, 1), "GBps_of_compulsory": round(gbps, 1), "fraction_of_hbm": round(gbps / HBM_GBPS, 3),
                                "bound": "one lane per restart interval runs the serial Huffman coder twice (count, write): divergent issue, not memory"}
            sweep = []
            for R in SWEEP:
                if args.band_rows % (mcu * R):
                    continue
                leg_device(R)
                t = [leg_device(R) for _ in range(2)]
                sweep.append({"restart_mcus": R, "ms_min": round(min(v[0] for v in t), 1), "file_MB": round(t[0][1] / 1e6, 2)})
            r["restart_sweep"] = sweep
            res[mode] = r
            eng.canvas_free(canvas)
            for h in handles:
                eng.tile_free(h)
    finally:
        eng.close()
        if args.dir is None:
            shutil.rmtree(outdir, ignore_errors=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
