"""The 16-bit tiles (vfsms_deep_*) at the headline size: 90 tiles of 2048 x 2048 uint16, 755 MB.

One device process under a time limit of its own:
  stages  the three stages from the library's event profiler (vfsms_profile_read) against their compulsory bytes --
            deep_window  the tiles read once per pass, two passes
            deep_reduce  the tiles read, half as many bytes written
            deep_mosaic  the tiles read, the mosaic's bytes written: the whole headline mosaic in bands of 4096 rows, and two bands of ONE size
                         (2048 x 16384): 8 tiles side by side without overlap (every pixel a copy) and 9 tiles at a step of 1792 (an eighth of
                         every tile shared with its neighbour) -- the difference is what the divided overlap pixels cost
          and, in the same process, vfsms_shading_apply on the 90 tiles' 8-bit views as the yardstick (the project's best streaming kernel:
          one byte in, one byte out per sample); every stage's rate as a ratio to it.  The tiles are `--distinct` SyntheticGrid tiles deepened
          with fresh noise (tests/deep_ref.py: deepen): the values sit in 2000 .. 5071 like a 12-bit camera's, which is what the histogram sees.
Writes profiles/deep_bench.json and prints the same JSON line.

    python tools/bench_deep.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 1 --distinct 9 --limit 420]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def _med(v):
    import numpy as np
    return float(np.median(np.array(v, float)))


def stages(args):
    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid
    import deep_ref as DR
    T, n = args.tile, args.rows * args.cols
    g = SyntheticGrid(args.rows, args.cols, T)
    base = g.tiles(ks=range(min(args.distinct, n)), threads=16)
    rng = np.random.default_rng(1)
    eng = isa.Engine(0)
    deeps = [eng.deep_upload(DR.deepen(base[k % len(base)], rng)) for k in range(n)]
    tile_bytes = n * T * T * 2

    def stage(name, fn, reps):
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        ms = []
        for _ in range(reps):
            fn()
            ms.append(eng.profile_read(reset=True).get(name, (0.0, 0))[0])
        eng.profile_enable(False)
        return _med(ms), [round(v, 4) for v in ms]

    out = {"tiles": n, "tile": T, "distinct_tiles": len(base), "tile_MB": round(tile_bytes / 1e6, 1), "steps": args.steps}
    # window
    for _ in range(args.warmup):
        win = eng.deep_window(deeps, 1000, 999000)
    ms, all_ms = stage("deep_window", lambda: eng.deep_window(deeps, 1000, 999000), args.steps)
    out["window"] = {"window": list(win), "ms": round(ms, 4), "ms_all": all_ms, "compulsory_MB": round(2 * tile_bytes / 1e6, 1),
                     "GBps": round(2 * tile_bytes / ms / 1e6, 1)}
    # reduce (the views stay for the yardstick)
    views = []

    def reduce_once():
        for v in views:
            eng.tile_free(v)
        views[:] = eng.deep_reduce(deeps, win[0], win[1])
    for _ in range(args.warmup):
        reduce_once()
    ms, all_ms = stage("deep_reduce", reduce_once, args.steps)
    out["reduce"] = {"ms": round(ms, 4), "ms_all": all_ms, "compulsory_MB": round(1.5 * tile_bytes / 1e6, 1), "GBps": round(1.5 * tile_bytes / ms / 1e6, 1)}
    # the yardstick: shading_apply on the views, in place (one byte in, one out per sample, the gain plane read once)
    field = eng.shading_from_gain(np.full((T, T), 4096, np.uint16))
    for _ in range(args.warmup):
        eng.shading_apply(field, views)
    ms, all_ms = stage("shading", lambda: eng.shading_apply(field, views), args.steps)
    yard_bytes = 2 * n * T * T + 2 * T * T
    out["shading_apply"] = {"ms": round(ms, 4), "ms_all": all_ms, "compulsory_MB": round(yard_bytes / 1e6, 1), "GBps": round(yard_bytes / ms / 1e6, 1)}
    eng.shading_free(field)
    for v in views:
        eng.tile_free(v)
    # mosaic: two bands of one size
    H, W = T, 8 * T
    bands = {}
    for name, k, step in (("no_overlap", 8, T), ("overlap", 9, (W - T) // 8)):
        yx = [(0, i * step) for i in range(k)]
        buf = np.empty((H, W), np.uint16)
        for mode in ("feather", "paste"):
            call = lambda: eng.deep_mosaic_rows(deeps[:k], yx, H, W, mode, 0, 0, H, out=buf)      # noqa: E731
            for _ in range(args.warmup):
                call()
            ms, all_ms = stage("deep_mosaic", call, args.steps)
            nbytes = k * T * T * 2 + H * W * 2
            bands[name + "_" + mode] = {"tiles": k, "step": step, "band": [H, W], "ms": round(ms, 4), "ms_all": all_ms, "compulsory_MB": round(nbytes / 1e6, 1),
                                        "GBps": round(nbytes / ms / 1e6, 1)}
    over_px = 8 * (T - (W - T) // 8) * H
    bands["overlap_pixels"] = over_px
    bands["overlap_cost_ms"] = round(bands["overlap_feather"]["ms"] - bands["no_overlap_feather"]["ms"], 4)
    bands["overlap_cost_ns_per_divided_pixel"] = round(bands["overlap_cost_ms"] * 1e6 / over_px, 4)
    out["mosaic_bands"] = bands
    # mosaic: the headline grid's own layout, all bands
    shapes = [(T, T)] * n
    offs, _rx, _ry, rows, cols = isa.Stitcher._layout(shapes, [[0, 0]] + [list(o) for o in g.true_offsets()])
    buf = np.empty((min(4096, rows), cols), np.uint16)

    def whole():
        for r0 in range(0, rows, 4096):
            nr = min(4096, rows - r0)
            eng.deep_mosaic_rows(deeps, offs, rows, cols, "feather", 0, r0, nr, out=buf[:nr])
    for _ in range(args.warmup):
        whole()
    ms, all_ms = stage("deep_mosaic", whole, args.steps)
    nbytes = tile_bytes + rows * cols * 2
    t0 = time.perf_counter(); whole(); wall = (time.perf_counter() - t0) * 1e3
    out["mosaic"] = {"canvas": [rows, cols], "band_rows": 4096, "kernel_ms": round(ms, 4), "ms_all": all_ms, "compulsory_MB": round(nbytes / 1e6, 1),
                     "GBps": round(nbytes / ms / 1e6, 1), "wall_ms_with_downloads": round(wall, 1)}
    y = out["shading_apply"]["GBps"]
    out["ratio_to_shading_apply"] = {"window": round(out["window"]["GBps"] / y, 3), "reduce": round(out["reduce"]["GBps"] / y, 3),
                                     "mosaic_no_overlap_band": round(bands["no_overlap_feather"]["GBps"] / y, 3),
                                     "mosaic_headline": round(out["mosaic"]["GBps"] / y, 3)}
    for d in deeps:
        eng.deep_free(d)
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10); ap.add_argument("--cols", type=int, default=9); ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--distinct", type=int, default=9, help="distinct synthetic tiles behind the stages' 90 (each deepened with noise of its own)")
    ap.add_argument("--limit", type=int, default=420, help="seconds the device process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_bench.json"))
    ap.add_argument("--worker", choices=("stages",), default=None)
    args = ap.parse_args()
    if args.worker:
        return stages(args)
    res = {"metric": "16-bit tiles: window, reduce and mosaic stages against their compulsory bytes and against shading_apply"}
    passed = [a for a in sys.argv[1:]]
    for step in ("stages",):
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", step] + passed
        try:
            run = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit, cwd=ROOT)
        except subprocess.TimeoutExpired:
            print("the %s process ran into its limit of %d s: nothing written, nothing started behind it" % (step, args.limit), file=sys.stderr)
            return 124
        if run.returncode != 0:
            print("the %s process failed with status %d: nothing written, nothing started behind it" % (step, run.returncode), file=sys.stderr)
            return run.returncode
        res[step] = json.loads(run.stdout.decode().strip().splitlines()[-1])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
