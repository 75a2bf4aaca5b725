"""featureMethod "sift" on the MI355X: detect + describe of a search strip and of a whole tile, and the registration rate of the per-pair
path and of the fused attempt batch.

  strip  the roiRatio 0.2 strip of a 2048 x 2048 tile (409 x 2048), Engine.sift_detect_describe from host array to host arrays
         (upload and download included), timed call by call after warm-up
  tile   the same for the whole 2048 x 2048 tile
  grid   the 10 x 9 synthetic grid of 2048 x 2048 tiles, two legs ALTERNATED --reps times in this one process:
         per-pair  Stitcher.calculateOffsetForFeatureSearchIncre with featureMethod "sift" on an engine wrapper that hides
                   attempt_sift_batch, i.e. the generic operator path (detectAndDescribe -> matchDescriptors -> getOffsetByMode) that was the
                   only SIFT path before the fused batch existed
         fused     GridRegistrar(method="sift").register over the resident tiles, with the path memory of a warm-up run (as bench.py
                   measures SURF); per-stage HIP-event times of one extra run (vfsms_profile_*)
         then the fused leg once more in a fresh child process under VFSMS_BF_EXACT=1 (the exhaustive VALU 2-NN instead of the integer
         matrix-core kernel; the switch is read once per process), same tiles, same repetitions
Prints one JSON line; --out also writes it to a file.

    python tools/bench_sift.py [--steps 20 --warmup 3 --reps 3 --no-grid --out profiles/sift_batch_bench.json]
    python tools/bench_sift.py --fused-only --no-per-pair      # what a rocprofv3 --kernel-trace --stats run wraps
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class GenericOnly:
    """the engine without its fused SIFT batch: the Stitcher then takes the per-pair operator path"""

    def __init__(self, base):
        self.base = base

    def __getattr__(self, name):
        if name == "attempt_sift_batch":
            raise AttributeError(name)
        return getattr(self.base, name)


def per_pair_leg(isa, eng, tiles, truth):
    st = isa.Stitcher(); st._engine = GenericOnly(eng)
    st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = 1
    assert not st._usesStockOperators()
    within, n = 0, len(tiles) - 1
    t0 = time.perf_counter()
    for k in range(n):
        ok, off = st.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        within += bool(ok) and abs(off[0] - truth[k][0]) <= 1 and abs(off[1] - truth[k][1]) <= 1
    return time.perf_counter() - t0, int(within)


def fused_leg(reg, handles, shapes, truth):
    t0 = time.perf_counter()
    table, _d = reg.register(handles, shapes, 1)
    dt = time.perf_counter() - t0
    within = sum(bool(r[0]) and abs(r[1] - t[0]) <= 1 and abs(r[2] - t[1]) <= 1 for r, t in zip(table.tolist(), truth))
    return dt, int(within), table


def spread(xs):
    return {"median": round(float(sorted(xs)[len(xs) // 2]), 3), "min": round(min(xs), 3), "max": round(max(xs), 3), "all": [round(x, 3) for x in xs]}


def grid_legs(args, isa, eng, res):
    import numpy as np
    from imagestitch_amd.grid import GridRegistrar
    from imagestitch_amd.synthetic import SyntheticGrid
    grid = SyntheticGrid(10, 9, 2048)
    truth = grid.true_offsets()
    if args.tiles and os.path.exists(args.tiles):
        tiles = list(np.load(args.tiles))
    else:
        tiles = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    n = len(tiles) - 1
    handles = [eng.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    reg = GridRegistrar(eng, method="sift", roiRatio=0.2)
    _dt, _w, cold = fused_leg(reg, handles, shapes, truth)                       # warm-up: code objects, buffers, path memory
    if not args.no_per_pair:
        per_pair_leg(isa, eng, tiles[:3], truth)                                 # warm-up pairs
    pp, fu, within_pp, within_fu = [], [], 0, 0
    for _ in range(args.reps):
        if not args.no_per_pair:
            dt, within_pp = per_pair_leg(isa, eng, tiles, truth)
            pp.append(n / dt)
        dt, within_fu, table = fused_leg(reg, handles, shapes, truth)
        assert np.array_equal(table, cold)
        fu.append(n / dt)
    a0, b0 = reg.stats["attempts"], reg.stats["batches"]
    eng.profile_enable(True)
    fused_leg(reg, handles, shapes, truth)
    stages = {k: round(v[0], 3) for k, v in eng.profile_read().items()}
    eng.profile_enable(False)
    out = {"pairs": n, "reps": args.reps, "bf_exact": os.environ.get("VFSMS_BF_EXACT", "0"),
           "fused": {"pairs_per_s": spread(fu), "within_1px_of_truth": within_fu, "attempts_per_path": reg.stats["attempts"] - a0,
                     "batches_per_path": reg.stats["batches"] - b0, "stage_ms_of_one_path": stages}}
    if pp:
        out["per_pair"] = {"pairs_per_s": spread(pp), "within_1px_of_truth": within_pp}
        out["fused_over_per_pair"] = {"of_medians": round(out["fused"]["pairs_per_s"]["median"] / out["per_pair"]["pairs_per_s"]["median"], 2),
                                      "worst_case": round(min(fu) / max(pp), 2)}
    res["grid_10x9_2048"] = out
    if args.fused_only:
        return
    # the same fused leg under VFSMS_BF_EXACT=1, in a fresh child (this process has already read the switch)
    import subprocess
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "tiles.npy")
        np.save(path, np.stack(tiles))
        for h in handles:
            eng.tile_free(h)
        eng.close()
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--fused-only", "--no-per-pair", "--no-images", "--reps", str(args.reps), "--tiles", path],
                           env=dict(os.environ, VFSMS_BF_EXACT="1"), capture_output=True, text=True, timeout=900)
    if p.returncode != 0:
        raise SystemExit("the VFSMS_BF_EXACT=1 child failed:\n" + p.stderr[-2000:])
    child = json.loads(p.stdout.strip().splitlines()[-1])["grid_10x9_2048"]
    out["fused_bf_exact"] = child["fused"]
    out["integer_2nn_over_valu_2nn"] = {"path_rate_ratio_of_medians": round(out["fused"]["pairs_per_s"]["median"] / child["fused"]["pairs_per_s"]["median"], 2),
                                        "bf_stage_ms": {"bf_i8": stages.get("bf_i8"), "bf_l2": child["fused"]["stage_ms_of_one_path"].get("bf_l2")}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20, help="timed calls per image")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--no-grid", action="store_true", help="skip the 10 x 9 grid registration (profiling runs)")
    ap.add_argument("--reps", type=int, default=3, help="alternations of the per-pair and the fused leg")
    ap.add_argument("--fused-only", action="store_true", help="no VFSMS_BF_EXACT=1 child (this process is one, or a profiling run)")
    ap.add_argument("--no-per-pair", action="store_true", help="skip the per-pair leg")
    ap.add_argument("--no-images", action="store_true", help="skip the single-image timings")
    ap.add_argument("--tiles", default=None, help="a .npy stack of the grid's tiles (handed to the child process)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid

    eng = isa.Engine(0)
    res = {"metric": "SIFT detect+describe (host arrays in and out) and per-pair SIFT registration", "steps": args.steps, "warmup": args.warmup}
    tile = SyntheticGrid(2, 1, 2048).tiles(threads=1)[0]
    for name, img in (() if args.no_images else (("strip_409x2048", np.ascontiguousarray(tile[-409:])), ("tile_2048x2048", tile))):
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
        grid_legs(args, isa, eng, res)
    eng.close()
    line = json.dumps(res)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
