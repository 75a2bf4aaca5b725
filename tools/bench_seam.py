"""Mosaic assembly with fuseMethod "optimalSeamLine" (both seamLineBlend values) against "fadeInAndFadeOut" and "multiBandBlending" on the
same resident grid, in one process.

The headline grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap, gray) is synthesised, uploaded to HBM, and assembled from its
true offsets the way Stitcher.getStitchByOffset does it for resident tiles: one vfsms_canvas_assemble_resident call per mosaic, geom mode
0 (fade), 6 (multi-band) or 7 (optimal seam).  After warm-up the four legs alternate A B C D A B C D ...; every mosaic is timed from host to
device-synchronised end.  A further pass per seam leg runs with the library's event profiler on and records the per-kernel split
(seam_energy / seam_dp / seam_trace / seam_apply, from vfsms_profile_read) and the forward pass's time per seam step.
Writes profiles/seam_bench.json and prints the same JSON line.

    python tools/bench_seam.py [--rows 10 --cols 9 --tile 2048 --levels 4 --steps 5 --warmup 2]
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
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed mosaics per leg (at least 3)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seam_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 3)

    import numpy as np
    import torch
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid

    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    tiles = grid.tiles(threads=min(16, os.cpu_count() or 1))
    eng = isa.Engine(0)
    torch.cuda.init()
    n = grid.n_tiles
    handles = [eng.tile_upload(t) for t in tiles]
    eng.sync()
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([(grid.th, grid.tw)] * n, offs)
    rois = []
    for i in range(1, n):
        oy, ox = offsetList[i]
        rois.append((max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + grid.th, rangeX[i - 1][1]), min(ox + grid.tw, rangeY[i - 1][1])))

    def geom(mode):
        g = [(offsetList[0][0], offsetList[0][1], 0, 0, 0, 0, 0, 0, -1)]
        g += [(offsetList[i][0], offsetList[i][1]) + tuple(rois[i - 1]) + (offs[i][0], offs[i][1], mode) for i in range(1, n)]
        return np.array(g, np.int32)
    legs = {"fadeInAndFadeOut": (geom(0), "none"), "multiBandBlending": (geom(6), "none"),
            "optimalSeamLine": (geom(7), "none"), "optimalSeamLine+multiBandBlending": (geom(7), "multiBandBlending")}

    def assemble(name, download=False):
        canvas = eng.canvas_create(rows, cols, 1)
        try:
            eng.canvas_set_multiband_levels(canvas, args.levels)
            eng.canvas_set_seam_blend(canvas, legs[name][1])
            t0 = time.perf_counter()
            eng.canvas_assemble_resident(canvas, handles, legs[name][0])
            eng.sync(); torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            return eng.canvas_download(canvas, rows, cols, 1) if download else ms
        finally:
            eng.canvas_free(canvas)

    for _ in range(args.warmup):
        for name in legs:
            assemble(name)
    ms = {name: [] for name in legs}
    for _ in range(args.steps):
        for name in legs:
            ms[name].append(assemble(name))
    # the per-kernel split of the seam legs (event pairs around every launch group slow the mosaic down: not part of the timings above)
    split = {}
    for name in ("optimalSeamLine", "optimalSeamLine+multiBandBlending"):
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        assemble(name)
        prof = eng.profile_read(reset=True)
        eng.profile_enable(False)
        split[name] = {k: {"ms": round(v[0], 3), "launch_groups": v[1]} for k, v in prof.items() if k.startswith("seam_") or k.startswith("fuse")}
    mosaics = {name: assemble(name, download=True) for name in ("fadeInAndFadeOut", "optimalSeamLine")}
    for h in handles:
        eng.tile_free(h)
    eng.close()

    # seam steps of a mosaic: a strip ROI has one seam along its longer side (corner ROIs: both sides, an upper bound)
    def steps_of(r):
        h, w = r[2] - r[0], r[3] - r[1]
        return max(h, w)
    seam_steps = sum(steps_of(r) for r in rois)
    res = {"metric": "mosaic assembly, optimalSeamLine vs fadeInAndFadeOut and multiBandBlending (resident tiles, one assemble call per mosaic)",
           "grid": [args.rows, args.cols, args.tile], "levels": args.levels, "mosaic_px": rows * cols, "fused_regions": len(rois),
           "region_Mpx": round(sum((r[2] - r[0]) * (r[3] - r[1]) for r in rois) / 1e6, 1), "seam_steps_per_mosaic": seam_steps,
           "steps": args.steps, "warmup": args.warmup}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3),
                     "spread_pct": round(float((v.max() - v.min()) / np.median(v) * 100), 1)}
    med = {name: float(np.median(v)) for name, v in ms.items()}
    for name in ("optimalSeamLine", "optimalSeamLine+multiBandBlending"):
        res[name]["over_fade"] = round(med[name] / med["fadeInAndFadeOut"], 2)
        res[name]["over_multiband"] = round(med[name] / med["multiBandBlending"], 2)
        res[name]["ms_per_fused_region"] = round(med[name] / len(rois), 4)
        res[name]["kernel_split"] = split[name]
        dp = split[name].get("seam_dp")
        if dp:
            res[name]["dp_us_per_seam_step"] = round(dp["ms"] * 1e3 / seam_steps, 4)
    a, b = mosaics["fadeInAndFadeOut"], mosaics["optimalSeamLine"]
    res["mosaic_mean_grey"] = {"fadeInAndFadeOut": round(float(a.mean()), 3), "optimalSeamLine": round(float(b.mean()), 3)}
    res["bytes_differing_from_fade_pct"] = round(float(np.count_nonzero(a != b)) / a.size * 100, 3)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
