"""Lens correction (Method.lensCorrection = "estimate") on the headline grid, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised and uploaded to HBM, and every tile is distorted on the
device by the library's own resampling with the negated coefficient: vfsms_lens_apply with (-a, 3 a^2) makes the image a camera with
s = u (1 + a rho^2) would have taken, up to O(a^3) and one interpolation.  Per mode (gray, B G R) the script records

  * one lens.correct on the fresh distorted tiles: the fitted (a1, a2) against the injected (a, 0), spread_before and spread_after;
  * after warm-up, from host to device-synchronised end: the block field of all edges (vfsms_block_ncc_batch), the in-place resampling
    (vfsms_lens_apply), and the fade mosaic without and with the correction in front of it, alternated A B A B, with the spread of the
    repeats.  The corrected leg is edges + block field + fit + resampling + block field + mosaic.  The resampling works in place, so the
    leg fits on the pixels as they are but applies the coefficients of the first run: every repetition moves the same bytes (times do
    not depend on pixel values);
  * a further pass with the library's event profiler on: the stages "lens_blocks" and "lens_apply" (vfsms_profile_read), each against
    its compulsory bytes -- the block field reads the overlap samples of both tiles once, the resampling reads and writes every tile
    once -- the fraction of the 6.3 TB/s a streaming copy reaches on this device, and which bound holds: a stage far below the
    memory bound is bound by instruction issue, whose floor for the block field is counted from the kernel's inner loop;
  * the distribution of the best block scores on the 25 committed real dendritic strip pairs (tests/golden/real_path_strips), at the
    stored offsets: what lensThreshold = 0.5 -- the verifier's threshold re-used, provisional -- keeps of real material.
Writes profiles/lens_bench.json and prints the same JSON line.

    python tools/bench_lens.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 2 --a1 0.002]
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
VALU_TOPS = 39.3        # lane operations per second of 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz, in 10^12
BLOCK_LOOP_OPS = 6      # k_lens_blocks per four samples of a candidate: two LDS reads, alignbyte, sad_u8, two udot4


def dendritic_scores(eng, block, radius):
    """the best fixed-point block scores over the 25 committed real dendritic pairs (the recipe of tools/bench_stage_repair.py: 640-px
    crops of the accepted strips, at the raw vote of the stored SURF row)"""
    import numpy as np
    from imagestitch_amd import lens
    from imagestitch_amd.utility import roi_rect
    gdir = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(gdir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(gdir, "real_path_strips.npz"))
    scores, bracketed, pairs = [], 0, 0
    for nb in meta:
        def crop(tile, rect):
            for s in nb["strips"]:
                a = g[s["key"]]
                if s["tile"] == tile and s["y0"] >= rect[0] and s["x0"] >= rect[1] and s["y0"] + a.shape[0] <= rect[0] + rect[2] \
                        and s["x0"] + a.shape[1] <= rect[1] + rect[3]:
                    return a
            raise KeyError((tile, rect))
        H, W = nb["shape"]
        for k, e in enumerate(nb["expected"]):
            d, i = e["direction"], e["i"]
            a = np.ascontiguousarray(crop(nb["tiles"][k], roi_rect(nb["shape"], d, "first", i * 0.2)))
            b = np.ascontiguousarray(crop(nb["tiles"][k + 1], roi_rect(nb["shape"], d, "second", i * 0.2)))
            off = list(e["offset"])                           # the full-tile offset back to the raw vote of the strips
            if d == 1: off[0] -= H - int(i * 0.2 * H)
            elif d == 2: off[1] -= W - int(i * 0.2 * W)
            elif d == 3: off[0] += H - int(i * 0.2 * H)
            else: off[1] += W - int(i * 0.2 * W)
            if a.shape != b.shape or a.ndim != 2:
                continue
            first = lens.block_first(a.shape, [off], block, radius)
            if first[-1] == 0:
                continue
            ha, hb = eng.tile_upload(a), eng.tile_upload(b)
            try:
                best = eng.block_ncc_batch([(ha, hb, off[0], off[1])], first, block, radius)
            finally:
                eng.tile_free(ha); eng.tile_free(hb)
            pairs += 1
            scores += best[:, 2].tolist()
            bracketed += int(((abs(best[:, 0]) < radius) & (abs(best[:, 1]) < radius)).sum())
    if not scores:
        return {"pairs": 0}
    s = np.sort(np.array(scores, np.float64) / (1 << 20))
    q = lambda p: round(float(s[min(len(s) - 1, int(p * len(s)))]), 4)        # noqa: E731
    return {"pairs": pairs, "blocks": len(s), "block": block, "radius": radius, "bracketed": bracketed, "score_min": q(0.0), "score_p10": q(0.10),
            "score_p25": q(0.25), "score_median": q(0.5), "score_p75": q(0.75), "score_max": q(1.0),
            "fraction_at_least_0.5": round(float((s >= 0.5).mean()), 4), "fraction_at_least_0.8": round(float((s >= 0.8).mean()), 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--a1", type=float, default=0.002, help="the injected coefficient: a corner shift of a1 x the half-diagonal")
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions per leg (at least 3)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--modes", default="gray,color")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lens_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 3)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd import lens
    from imagestitch_amd.adjust import neighbour_edges
    from imagestitch_amd.synthetic import SyntheticGrid

    m = isa.Method
    block, radius, threshold = int(m.lensBlock), int(m.lensRadius), float(m.lensThreshold)
    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    plain = grid.tiles(threads=min(16, os.cpu_count() or 1))
    n = grid.n_tiles
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
    edges = neighbour_edges(shapes, np.asarray(path), radius)
    eoff = [(dx, dy) for _a, _b, dx, dy in edges.tolist()]
    first = lens.block_first(shapes[0], eoff, block, radius)
    overlap_px = int(sum(max(0, min(grid.th, dx + grid.th) - max(0, dx)) * max(0, min(grid.tw, dy + grid.tw) - max(0, dy)) for dx, dy in eoff))
    inject = lens.coefficients_q30(-args.a1, 3.0 * args.a1 * args.a1)
    eng = isa.Engine(0)

    def summary(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3),
                "spread": round(float((v.max() - v.min()) / np.median(v)), 3)}

    res = {"metric": "lens correction: block displacement field, resampling and the fade mosaic without / with it (resident tiles)",
           "grid": [args.rows, args.cols, args.tile], "injected": [args.a1, 0.0], "block": block, "radius": radius, "threshold": threshold,
           "interpolation": m.lensInterpolation, "steps": args.steps, "warmup": args.warmup, "hbm_TBps": HBM_TBPS, "edges": int(len(edges)),
           "blocks": int(first[-1])}
    for mode in args.modes.split(","):
        ch = 1 if mode == "gray" else 3
        if ch == 1:
            handles = [eng.tile_upload(t) for t in plain]
        else:
            handles = [eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in plain]
        eng.lens_apply(handles, inject[0], inject[1], (-1, -1), "cubic")       # the camera
        eng.sync()
        stack_bytes = n * grid.th * grid.tw * ch
        jobs = [(handles[a], handles[b], dx, dy) for a, b, dx, dy in edges.tolist()]

        def timed(fn):
            eng.sync()
            t0 = time.perf_counter()
            out = fn()
            eng.sync()
            return (time.perf_counter() - t0) * 1e3, out

        t_first, (_offs, pair, report) = timed(lambda: lens.correct(eng, handles, shapes, path, block=block, radius=radius, threshold=threshold,
                                                                   min_blocks=int(m.lensMinBlocks), min_shift=float(m.lensMinShift),
                                                                   interpolation=m.lensInterpolation))
        q = lens.coefficients_q30(*pair) if pair is not None else inject

        def mosaic(corrected):
            canvas = eng.canvas_create(rows, cols, ch)
            try:
                def run():
                    if corrected:
                        e = neighbour_edges(shapes, np.asarray(path), radius)
                        f = lens.block_first(shapes[0], [(dx, dy) for _a, _b, dx, dy in e.tolist()], block, radius)
                        best, surface = eng.block_ncc_batch(jobs, f, block, radius, want_surface=True)
                        lens.fit_radial(shapes[0], eoff, best, surface, block, radius, threshold)
                        eng.lens_apply(handles, q[0], q[1], (-1, -1), m.lensInterpolation)
                        best = eng.block_ncc_batch(jobs, f, block, radius)
                        lens.path_moves(n, e, f, best, radius, threshold)
                    eng.canvas_assemble_resident(canvas, handles, geom)
                return timed(run)[0]
            finally:
                eng.canvas_free(canvas)

        t_blocks, t_apply, t_plain, t_corr = [], [], [], []
        for k in range(args.warmup + args.steps):
            a = timed(lambda: eng.block_ncc_batch(jobs, first, block, radius, want_surface=True))[0]
            b = timed(lambda: eng.lens_apply(handles, q[0], q[1], (-1, -1), m.lensInterpolation))[0]
            c, d = mosaic(False), mosaic(True)
            if k >= args.warmup:
                t_blocks.append(a); t_apply.append(b); t_plain.append(c); t_corr.append(d)
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        eng.block_ncc_batch(jobs, first, block, radius, want_surface=True)
        stage_blocks = eng.profile_read(reset=True).get("lens_blocks", (0.0, 0))
        eng.lens_apply(handles, q[0], q[1], (-1, -1), m.lensInterpolation)
        stage_apply = eng.profile_read(reset=True).get("lens_apply", (0.0, 0))
        eng.lens_apply(handles, q[0], q[1], (-1, -1), "bilinear")
        stage_bilinear = eng.profile_read(reset=True).get("lens_apply", (0.0, 0))
        eng.profile_enable(False)
        for h in handles:
            eng.tile_free(h)
        blocks_bytes, apply_bytes = 2 * overlap_px * ch, 2 * stack_bytes
        valu_floor_ms = int(first[-1]) * block * block * (2 * radius + 1) ** 2 / 4.0 * BLOCK_LOOP_OPS / (VALU_TOPS * 1e12) * 1e3
        r = {"tiles": n, "stack_MB": round(stack_bytes / 1e6, 1), "report": report, "first_correct_ms": round(t_first, 3),
             "fitted": None if pair is None else [pair[0], pair[1]],
             "fitted_corner_over_injected": None if pair is None else round((pair[0] + pair[1]) / args.a1, 4),
             "blocks": summary(t_blocks), "apply": summary(t_apply), "fade_mosaic": summary(t_plain), "fade_mosaic_corrected": summary(t_corr),
             "stage_ms": {"lens_blocks": round(stage_blocks[0], 3), "lens_apply": round(stage_apply[0], 3), "lens_apply_bilinear": round(stage_bilinear[0], 3)}}
        r["blocks"]["compulsory_MB"] = round(blocks_bytes / 1e6, 1)
        r["apply"]["compulsory_MB"] = round(apply_bytes / 1e6, 1)
        r["blocks"]["valu_floor_ms"] = round(valu_floor_ms, 3)
        for key, stage, nbytes in (("blocks", stage_blocks, blocks_bytes), ("apply", stage_apply, apply_bytes)):
            if stage[0] > 0:
                frac = nbytes / stage[0] / 1e9 / HBM_TBPS
                r[key]["stage_GBps_of_compulsory"] = round(nbytes / stage[0] / 1e6, 1)
                r[key]["fraction_of_hbm"] = round(frac, 3)
                r[key]["bound"] = "memory" if frac >= 0.5 else "instruction issue (VALU / LDS; the split is not measured)"
        if stage_blocks[0] > 0:
            r["blocks"]["fraction_of_valu_floor"] = round(valu_floor_ms / stage_blocks[0], 3)
        r["correction_over_mosaic"] = round(float(np.median(t_corr)) / float(np.median(t_plain)), 3)
        res[mode] = r
    res["dendritic_block_scores"] = dendritic_scores(eng, block, radius)
    eng.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
