"""Shading correction (Method.shadingCorrection = "estimate") on the headline grid, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised and uploaded to HBM.  Per mode (gray, B G R) the script
times, each from host to device-synchronised end after warm-up: the estimate over the 90 tiles (vfsms_shading_estimate), the in-place apply
(vfsms_shading_apply), and the fade mosaic from the true offsets without and with the correction in front of it, alternated A B A B.  A
further pass with the library's event profiler on records the "shading" stage (vfsms_profile_read).  Each time is set against the bytes
the kernel has to move: the estimate reads N h w ch bytes once, the apply reads and writes them and reads one gain table.  The apply works in
place, so the timed tiles are corrected again and again: the times do not depend on the pixel values.
Writes profiles/shading_bench.json and prints the same JSON line.

    python tools/bench_shading.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 2 --radius 32]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--percentile", type=int, default=50)
    ap.add_argument("--radius", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions per leg (at least 3)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shading_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 3)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid

    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    gray = grid.tiles(threads=min(16, os.cpu_count() or 1))
    n = grid.n_tiles
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([(grid.th, grid.tw)] * n, offs)
    geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
    for i in range(1, n):
        oy, ox = offsetList[i]
        geom.append((oy, ox, max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + grid.th, rangeX[i - 1][1]),
                     min(ox + grid.tw, rangeY[i - 1][1]), offs[i][0], offs[i][1], 0))
    geom = np.array(geom, np.int32)
    eng = isa.Engine(0)

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3)}

    res = {"metric": "shading correction: estimate, apply and the fade mosaic without / with it (resident tiles)",
           "grid": [args.rows, args.cols, args.tile], "percentile": args.percentile, "radius": args.radius, "steps": args.steps, "warmup": args.warmup}
    for mode, ch in (("gray", 1), ("color", 3)):
        if ch == 1:
            handles = [eng.tile_upload(t) for t in gray]
        else:
            handles = [eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in gray]
        eng.sync()
        stack_bytes = n * grid.th * grid.tw * ch
        gain_bytes = grid.th * grid.tw * ch * 2

        def timed(fn):
            eng.sync()
            t0 = time.perf_counter()
            out = fn()
            eng.sync()
            return (time.perf_counter() - t0) * 1e3, out

        def mosaic(correct):
            canvas = eng.canvas_create(rows, cols, ch)
            try:
                def run():
                    if correct:
                        f = eng.shading_estimate(handles, args.percentile, args.radius)
                        eng.shading_apply(f, handles)
                        eng.shading_free(f)
                    eng.canvas_assemble_resident(canvas, handles, geom)
                return timed(run)[0]
            finally:
                eng.canvas_free(canvas)

        est, app, plain, corrected = [], [], [], []
        for k in range(args.warmup + args.steps):
            t_est, f = timed(lambda: eng.shading_estimate(handles, args.percentile, args.radius))
            t_app, _ = timed(lambda: eng.shading_apply(f, handles))
            eng.shading_free(f)
            a, b = mosaic(False), mosaic(True)
            if k >= args.warmup:
                est.append(t_est); app.append(t_app); plain.append(a); corrected.append(b)
        # the "shading" stage by HIP events (event pairs around every launch group: not part of the timings above)
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        f = eng.shading_estimate(handles, args.percentile, args.radius)
        stage_est = eng.profile_read(reset=True).get("shading", (0.0, 0))
        eng.shading_apply(f, handles)
        stage_app = eng.profile_read(reset=True).get("shading", (0.0, 0))
        eng.shading_free(f)
        eng.profile_enable(False)
        for h in handles:
            eng.tile_free(h)
        r = {"tiles": n, "stack_MB": round(stack_bytes / 1e6, 1), "estimate": stats(est), "apply": stats(app),
             "fade_mosaic": stats(plain), "fade_mosaic_corrected": stats(corrected),
             "shading_stage_ms": {"estimate": round(stage_est[0], 3), "apply": round(stage_app[0], 3)}}
        # compulsory traffic: the estimate reads the stack once; the apply reads and writes it and reads one gain table
        r["estimate"]["compulsory_MB"] = round(stack_bytes / 1e6, 1)
        r["apply"]["compulsory_MB"] = round((2 * stack_bytes + gain_bytes) / 1e6, 1)
        if stage_est[0] > 0:
            r["estimate"]["stage_GBps_of_compulsory"] = round(stack_bytes / stage_est[0] / 1e6, 1)
        if stage_app[0] > 0:
            r["apply"]["stage_GBps_of_compulsory"] = round((2 * stack_bytes + gain_bytes) / stage_app[0] / 1e6, 1)
        r["correction_over_mosaic"] = round(float(np.median(corrected)) / float(np.median(plain)), 3)
        res[mode] = r
    eng.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
