"""Mosaic assembly with fuseMethod "multiBandBlending" against "fadeInAndFadeOut" on the same resident grid, in one process.

The headline grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap, gray) is synthesised, uploaded to HBM, and assembled from its
true offsets the way Stitcher.getStitchByOffset does it for resident tiles: one vfsms_canvas_assemble_resident call per mosaic, geom mode
0 (fade) or 6 (multi-band).  After warm-up the two blends alternate A B A B; every mosaic is timed from host to device-synchronised end.
Prints one JSON line: ms per mosaic of each blend (median, spread), mosaic Gpx/s, the multi-band blend's algorithmic bytes per mosaic
(computed from the region shapes and the level count) and the fraction of 6.3 TB/s HBM bandwidth they make at the measured time.

    python tools/bench_multiband.py [--rows 10 --cols 9 --tile 2048 --levels 4 --steps 10 --warmup 3]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

HBM_TBPS = 6.3          # measured MI355X stream bandwidth


def multiband_bytes(r, c, ch, levels, th, tw):
    """algorithmic bytes of one multi-band fuse of an r x c ROI inside a th x tw tile (u8 canvas + validity byte, fp32 planes)"""
    px = [r * c]
    for _ in range(levels):
        h = (r + 1) // 2; w = (c + 1) // 2
        r, c = h, w
        px.append(h * w)
    plane = (2 * ch + 1) * 4                                  # GA, GB (ch floats) + M of one pixel
    b = (2 * ch + 1) * px[0] + plane * px[1]                  # level-0 pyrDown: canvas + validity + tile in, level 1 out
    for k in range(1, levels):
        b += plane * px[k] + plane * px[k + 1]                # pyrDown k -> k + 1
    for k in range(1, levels):
        b += plane * px[k] + 3 * ch * 4 * px[k + 1] + ch * 4 * px[k]     # reconstruct k: fine planes + O / GA / GB of k + 1 in, O_k out
    b += (2 * ch + 1) * px[0] + 3 * ch * 4 * px[1] + (ch + 1) * px[0]   # level-0 reconstruct: ROI in, coarse in, u8 + validity out
    b += (2 * ch + 1) * (th * tw - px[0])                     # paste outside the ROI: tile in, canvas + validity out
    return b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10, help="timed mosaics per blend")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()

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
    geoms = {"fadeInAndFadeOut": geom(0), "multiBandBlending": geom(6)}

    def assemble(name):
        canvas = eng.canvas_create(rows, cols, 1)
        try:
            eng.canvas_set_multiband_levels(canvas, args.levels)
            t0 = time.perf_counter()
            eng.canvas_assemble_resident(canvas, handles, geoms[name])
            eng.sync(); torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
        finally:
            eng.canvas_free(canvas)

    for _ in range(args.warmup):
        for name in geoms:
            assemble(name)
    ms = {name: [] for name in geoms}
    for _ in range(args.steps):
        for name in geoms:                                    # A B A B
            ms[name].append(assemble(name))
    # the download of one multi-band mosaic (outside the timing): a sanity check that the work happened
    canvas = eng.canvas_create(rows, cols, 1)
    try:
        eng.canvas_set_multiband_levels(canvas, args.levels)
        eng.canvas_assemble_resident(canvas, handles, geoms["multiBandBlending"])
        mosaic = eng.canvas_download(canvas, rows, cols, 1)
    finally:
        eng.canvas_free(canvas)
    for h in handles:
        eng.tile_free(h)
    eng.close()

    roi_px = [(r[2] - r[0]) * (r[3] - r[1]) for r in rois]
    mb_bytes = sum(multiband_bytes(r[2] - r[0], r[3] - r[1], 1, args.levels, grid.th, grid.tw) for r in rois) + 2 * grid.th * grid.tw
    res = {"metric": "mosaic assembly, multiBandBlending vs fadeInAndFadeOut (resident tiles, one assemble call per mosaic)",
           "grid": [args.rows, args.cols, args.tile], "levels": args.levels, "mosaic_px": rows * cols, "fused_regions": len(rois),
           "region_Mpx": round(sum(roi_px) / 1e6, 1), "steps": args.steps, "warmup": args.warmup}
    for name, v in ms.items():
        v = np.array(v)
        res[name] = {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3),
                     "spread_pct": round(float((v.max() - v.min()) / np.median(v) * 100), 1),
                     "mosaic_Gpx_per_s": round(rows * cols / (np.median(v) * 1e-3) / 1e9, 2)}
    t_mb = float(np.median(ms["multiBandBlending"])) * 1e-3
    res["multiBandBlending"].update({"algorithmic_bytes_per_mosaic": int(mb_bytes), "achieved_TB_per_s": round(mb_bytes / t_mb / 1e12, 3),
                                     "fraction_of_hbm": round(mb_bytes / t_mb / 1e12 / HBM_TBPS, 3)})
    res["multiband_over_fade"] = round(float(np.median(ms["multiBandBlending"]) / np.median(ms["fadeInAndFadeOut"])), 2)
    res["mosaic_mean_grey"] = round(float(mosaic.mean()), 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
