"""Pyramidal output (Stitcher.outputPyramid) on the headline mosaic, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised, uploaded and fused (fade) into a canvas that stays in HBM.
Per mode (gray, B G R) the script times the streamed write-out of that canvas, from the first band request to the closed file, alternated
A B A B after warm-up:
  A  Engine.canvas_download_bands -> TiffBandWriter (one strip per band, the file of today)
  B  Engine.canvas_download_pyramid_bands -> PyramidTiffBandWriter, uncompressed, default levels (tiles of 512)
Both legs write to the same directory (--dir, default: a temporary one) and remove the file again.  A further pass with the library's event
profiler on runs the bands of leg B without a writer and records the "pyramid" stage (vfsms_profile_read): the device time of the
reduction per mosaic, set against its compulsory traffic -- every band byte read once, every level byte written once -- as a fraction of
the 8 TB/s HBM figure the other benchmarks use.
Writes profiles/pyramid_bench.json and prints the same JSON line.

    python tools/bench_pyramid.py [--rows 10 --cols 9 --tile 2048 --steps 3 --warmup 1 --band-rows 4096]
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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--band-rows", type=int, default=4096)
    ap.add_argument("--pyramid-tile", type=int, default=512)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions per leg (at least 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 2)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.io import default_levels
    from imagestitch_amd.synthetic import SyntheticGrid

    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    gray = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    n = grid.n_tiles
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    shapes = [(grid.th, grid.tw)] * n
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    geom = isa.Stitcher._placements(shapes, offs, offsetList, rangeX, rangeY, isa.Engine.CANVAS_MODES["fadeInAndFadeOut"])
    eng = isa.Engine(0)
    outdir = args.dir or tempfile.mkdtemp(prefix="vfsms_pyramid_")
    os.makedirs(outdir, exist_ok=True)
    levels = default_levels(rows, cols, args.pyramid_tile)

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 1), "ms_min": round(float(v.min()), 1), "ms_max": round(float(v.max()), 1)}

    res = {"metric": "streamed write-out of the headline mosaic: strip TIFF (A) against tiled pyramidal TIFF with device-reduced levels (B)",
           "grid": [args.rows, args.cols, args.tile], "mosaic": [rows, cols], "band_rows": args.band_rows, "pyramid_tile": args.pyramid_tile,
           "levels": levels, "steps": args.steps, "warmup": args.warmup, "hbm_GBps": HBM_GBPS}
    try:
        for mode, ch in (("gray", 1), ("color", 3)):
            handles = [eng.tile_upload(t) if ch == 1 else eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in gray]
            canvas = eng.canvas_create(rows, cols, ch)
            eng.canvas_assemble_resident(canvas, handles, geom)
            eng.sync()
            full = (rows, cols, ch) if ch > 1 else (rows, cols)

            def leg_a():
                path = os.path.join(outdir, "a.tif")
                w = isa.TiffBandWriter(path)
                t0 = time.perf_counter()
                for r0, band in eng.canvas_download_bands(canvas, rows, cols, ch, args.band_rows, transient=True):
                    w(r0, band, full)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size

            def leg_b():
                path = os.path.join(outdir, "b.tif")
                w = isa.PyramidTiffBandWriter(path, tile=args.pyramid_tile)
                assert w.pyramid_levels(full) == levels
                t0 = time.perf_counter()
                for r0, band, lv in eng.canvas_download_pyramid_bands(canvas, rows, cols, ch, levels, args.band_rows, transient=True):
                    w(r0, band, full, levels=lv)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size

            a, b = [], []
            for k in range(args.warmup + args.steps):
                (ta, size_a), (tb, size_b) = leg_a(), leg_b()
                if k >= args.warmup:
                    a.append(ta); b.append(tb)
            # the "pyramid" stage by HIP events: the bands of leg B without a writer
            eng.profile_enable(True)
            eng.profile_read(reset=True)
            for _ in eng.canvas_download_pyramid_bands(canvas, rows, cols, ch, levels, args.band_rows, transient=True):
                pass
            stage = eng.profile_read(reset=True).get("pyramid", (0.0, 0))
            eng.profile_enable(False)
            level_bytes = sum(int(np.prod(s_)) for s_ in eng.pyramid_band_shapes(0, rows, cols, ch, levels))
            compulsory = rows * cols * ch + level_bytes
            r = {"mosaic_MB": round(rows * cols * ch / 1e6, 1), "strip_tiff": dict(stats(a), file_MB=round(size_a / 1e6, 1)),
                 "pyramid_tiff": dict(stats(b), file_MB=round(size_b / 1e6, 1)),
                 "pyramid_over_strip": round(float(np.median(b)) / float(np.median(a)), 3),
                 "pyramid_stage": {"ms": round(stage[0], 3), "launch_groups": stage[1], "compulsory_MB": round(compulsory / 1e6, 1)}}
            if stage[0] > 0:
                gbps = compulsory / stage[0] / 1e6
                r["pyramid_stage"]["GBps_of_compulsory"] = round(gbps, 1)
                r["pyramid_stage"]["fraction_of_hbm"] = round(gbps / HBM_GBPS, 3)
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
