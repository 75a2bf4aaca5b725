"""featureMethod "sift" on the MI355X: detect + describe of a search strip and of a whole tile, and the per-pair registration rate.

  strip  the roiRatio 0.2 strip of a 2048 x 2048 tile (409 x 2048), Engine.sift_detect_describe from host array to host arrays
         (upload and download included), timed call by call after warm-up
  tile   the same for the whole 2048 x 2048 tile
  grid   Stitcher.calculateOffsetForFeatureSearchIncre with featureMethod "sift" over the 10 x 9 synthetic grid of 2048 x 2048 tiles
         (the generic per-pair path: detectAndDescribe -> matchDescriptors -> getOffsetByMode), pairs per second and the offsets'
         agreement with the synthetic truth
Prints one JSON line.

    python tools/bench_sift.py [--steps 20 --warmup 3 --no-grid]
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
    ap.add_argument("--steps", type=int, default=20, help="timed calls per image")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-grid", action="store_true", help="skip the 10 x 9 grid registration (profiling runs)")
    args = ap.parse_args()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid

    eng = isa.Engine(0)
    res = {"metric": "SIFT detect+describe (host arrays in and out) and per-pair SIFT registration", "steps": args.steps, "warmup": args.warmup}
    tile = SyntheticGrid(2, 1, 2048).tiles(threads=1)[0]
    for name, img in (("strip_409x2048", np.ascontiguousarray(tile[-409:])), ("tile_2048x2048", tile)):
        for _ in range(args.warmup):
            xy, _d = eng.sift_detect_describe(img)
        ms = []
        for _ in range(args.steps):
            t0 = time.perf_counter()
            xy, _d = eng.sift_detect_describe(img)
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = np.array(ms)
        res[name] = {"ms_median": round(float(np.median(ms)), 3), "ms_min": round(float(ms.min()), 3), "ms_max": round(float(ms.max()), 3),
                     "keypoints": int(len(xy))}
    if not args.no_grid:
        grid = SyntheticGrid(10, 9, 2048)
        tiles = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
        truth = grid.true_offsets()
        st = isa.Stitcher(); st._engine = eng
        st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = 1
        st.calculateOffsetForFeatureSearchIncre([tiles[0], tiles[1]])            # warm-up pair
        st.direction = 1
        within, n = 0, len(tiles) - 1
        t0 = time.perf_counter()
        for k in range(n):
            ok, off = st.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
            within += bool(ok) and abs(off[0] - truth[k][0]) <= 1 and abs(off[1] - truth[k][1]) <= 1
        dt = time.perf_counter() - t0
        res["grid_10x9_2048"] = {"pairs": n, "s": round(dt, 3), "pairs_per_s": round(n / dt, 2), "within_1px_of_truth": int(within)}
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
