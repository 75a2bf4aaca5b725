"""Exposure compensation (Method.exposureCompensation = "gain") on the headline grid, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised, every tile multiplied by an exposure drawn from a
committed seed (exp of a uniform +-0.2; for B G R after the three channels are formed), and uploaded to HBM.  Per mode (gray, B G R) the script records

  * the edge residual max |log(g_a Sa / (g_b Sb))| before and after one exposure.compensate on the fresh tiles, and the gains it found;
  * after warm-up, from host to device-synchronised end: the statistics of all edges (vfsms_overlap_stats_batch), the in-place apply
    (vfsms_exposure_apply), and in the SAME run the shading apply (vfsms_shading_apply with a constant gain plane), which moves the same
    tile bytes with more arithmetic and a gain plane on top: the new apply is expected at no more than 1.15 x of it, the margin being
    for the run-to-run spread recorded next to it (`apply_over_shading_apply`, `spread`);
  * the fade mosaic from the true offsets without and with the compensation in front of it, alternated A B A B, with the spread of the
    repeats.  The compensated leg is edges + statistics + solve + apply + mosaic.  The apply works in place, so the tiles are multiplied
    again and again and the gains solved in later repetitions drift towards one; the leg therefore solves on the pixels as they are but
    applies the gains of the first run (a gain of exactly 4096, which the apply skips, taken as 4097), so that every repetition
    moves the same bytes (times do not depend on pixel values);
  * a further pass with the library's event profiler on: the "exposure" stage of the statistics and of the apply (vfsms_profile_read),
    each against its compulsory bytes -- the statistics read the overlap rectangle of either tile once, the apply reads and writes
    every tile -- and the fraction of the 6.3 TB/s a streaming copy reaches on this device.
Writes profiles/exposure_bench.json and prints the same JSON line.

    python tools/bench_exposure.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 2 --seed 20]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 6.3          # measured stream bandwidth of the MI355X (8 TB/s is the specification)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--seed", type=int, default=20, help="seed of the per-tile exposures")
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions per leg (at least 3)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exposure_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 3)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd import exposure as EX
    from imagestitch_amd.synthetic import SyntheticGrid

    m = isa.Method
    band, min_pixels, max_gain = tuple(m.exposureBand), int(m.exposureMinPixels), float(m.exposureMaxGain)
    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    plain = grid.tiles(threads=min(16, os.cpu_count() or 1))
    n = grid.n_tiles
    truth = np.exp(np.random.default_rng(args.seed).uniform(-0.2, 0.2, n))

    def exposed(t, g):
        return np.clip(np.rint(t.astype(np.float32) * np.float32(g)), 0, 255).astype(np.uint8)
    path = [list(map(int, o)) for o in grid.true_offsets()]
    offs = [[0, 0]] + path
    shapes = [(grid.th, grid.tw)] * n
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    geom = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
    for i in range(1, n):
        oy, ox = offsetList[i]
        geom.append((oy, ox, max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + grid.th, rangeX[i - 1][1]),
                     min(ox + grid.tw, rangeY[i - 1][1]), offs[i][0], offs[i][1], 0))
    geom = np.array(geom, np.int32)
    edges = EX.overlap_edges(shapes, path, min_pixels)
    # pixels of the overlap rectangle of every edge: tile b stands at (dx, dy) against tile a
    overlap_px = int(sum(max(0, min(grid.th, dx + grid.th) - max(0, dx)) * max(0, min(grid.tw, dy + grid.tw) - max(0, dy))
                         for _a, _b, dx, dy in edges.tolist()))
    eng = isa.Engine(0)

    def summary(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3),
                "spread": round(float((v.max() - v.min()) / np.median(v)), 3)}

    res = {"metric": "exposure compensation: overlap statistics, apply and the fade mosaic without / with it (resident tiles)",
           "grid": [args.rows, args.cols, args.tile], "seed": args.seed, "band": list(band), "min_pixels": min_pixels, "max_gain": max_gain,
           "steps": args.steps, "warmup": args.warmup, "hbm_TBps": HBM_TBPS, "edges": int(len(edges))}
    for mode, ch in (("gray", 1), ("color", 3)):
        if ch == 1:
            handles = [eng.tile_upload(exposed(t, g)) for t, g in zip(plain, truth)]
        else:
            handles = [eng.tile_upload_color(exposed(np.stack([t, 255 - t, t // 2 + 64], -1), g)) for t, g in zip(plain, truth)]
        eng.sync()
        stack_bytes = n * grid.th * grid.tw * ch
        stats_bytes = 2 * overlap_px * ch
        jobs = [(handles[a], handles[b], dx, dy) for a, b, dx, dy in edges.tolist()]

        def timed(fn):
            eng.sync()
            t0 = time.perf_counter()
            out = fn()
            eng.sync()
            return (time.perf_counter() - t0) * 1e3, out

        # the compensation itself, once, on the fresh tiles
        q0, report = EX.compensate(eng, handles, shapes, path, band=band, min_pixels=min_pixels, max_gain=max_gain)
        q0 = np.where(q0 == 4096, 4097, q0).astype(np.uint16)      # (a tile at exactly 4096 would be skipped: every timed apply moves all tiles)
        field = eng.shading_from_gain(np.full((grid.th, grid.tw, ch) if ch > 1 else (grid.th, grid.tw), 4100, np.uint16))

        def mosaic(compensated):
            canvas = eng.canvas_create(rows, cols, ch)
            try:
                def run():
                    if compensated:
                        e = EX.overlap_edges(shapes, path, min_pixels)
                        st = eng.overlap_stats_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in e.tolist()], *band)
                        EX.solve_gains(n, e, st, min_pixels, max_gain)
                        eng.exposure_apply(handles, q0)
                    eng.canvas_assemble_resident(canvas, handles, geom)
                return timed(run)[0]
            finally:
                eng.canvas_free(canvas)

        t_stats, t_apply, t_shade, t_plain, t_comp = [], [], [], [], []
        for k in range(args.warmup + args.steps):
            a = timed(lambda: eng.overlap_stats_batch(jobs, *band))[0]
            b = timed(lambda: eng.exposure_apply(handles, q0))[0]
            c = timed(lambda: eng.shading_apply(field, handles))[0]
            d, e = mosaic(False), mosaic(True)
            if k >= args.warmup:
                t_stats.append(a); t_apply.append(b); t_shade.append(c); t_plain.append(d); t_comp.append(e)
        # the "exposure" stage by HIP events (event pairs around every launch group: not part of the timings above)
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        eng.overlap_stats_batch(jobs, *band)
        stage_stats = eng.profile_read(reset=True).get("exposure", (0.0, 0))
        eng.exposure_apply(handles, q0)
        stage_apply = eng.profile_read(reset=True).get("exposure", (0.0, 0))
        eng.shading_apply(field, handles)
        stage_shade = eng.profile_read(reset=True).get("shading", (0.0, 0))
        eng.profile_enable(False)
        eng.shading_free(field)
        for h in handles:
            eng.tile_free(h)
        r = {"tiles": n, "stack_MB": round(stack_bytes / 1e6, 1), "report": report,
             "gains_q12": [int(q0.min()), int(q0.max())],
             "statistics": summary(t_stats), "apply": summary(t_apply), "shading_apply": summary(t_shade),
             "fade_mosaic": summary(t_plain), "fade_mosaic_compensated": summary(t_comp),
             "stage_ms": {"statistics": round(stage_stats[0], 3), "apply": round(stage_apply[0], 3), "shading_apply": round(stage_shade[0], 3)}}
        r["statistics"]["compulsory_MB"] = round(stats_bytes / 1e6, 1)
        r["apply"]["compulsory_MB"] = round(2 * stack_bytes / 1e6, 1)
        for key, stage, nbytes in (("statistics", stage_stats, stats_bytes), ("apply", stage_apply, 2 * stack_bytes)):
            if stage[0] > 0:
                r[key]["stage_GBps_of_compulsory"] = round(nbytes / stage[0] / 1e6, 1)
                r[key]["fraction_of_hbm"] = round(nbytes / stage[0] / 1e9 / HBM_TBPS, 3)
        ratio = float(np.median(t_apply)) / float(np.median(t_shade))
        r["apply_over_shading_apply"] = round(ratio, 3)
        r["apply_within_1.15x_of_shading_apply"] = bool(ratio <= 1.15)
        if stage_shade[0] > 0:
            r["stage_apply_over_shading_apply"] = round(stage_apply[0] / stage_shade[0], 3)
        r["compensation_over_mosaic"] = round(float(np.median(t_comp)) / float(np.median(t_plain)), 3)
        res[mode] = r
    eng.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
