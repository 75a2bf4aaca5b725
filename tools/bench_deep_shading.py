"""Flat-field correction of 16-bit tiles (vfsms_deep_shading_*) at the headline size: 90 tiles of 2048 x 2048 uint16, 755 MB, percentile 50,
radius 32, pedestal 2000.

One device process under a time limit of its own.  The two stages come from the library's event profiler (vfsms_profile_read): the deep
calls are booked under "deep_shading", the 8-bit ones under "shading".
  estimate  vfsms_deep_shading_estimate over the 90 deep tiles: the stack read once (755 MB) and the three planes written
  apply     vfsms_deep_shading_apply in place on the 90 deep tiles: 1510 MB moved and 8 MB of gain read
and, in the SAME process and alternated A B A B with them, the yardsticks: vfsms_shading_estimate and vfsms_shading_apply on the 90
8-bit views of the same tiles (deep_reduce through the dataset's window).  Median of `--steps` after `--warmup`; every stage's rate as a
ratio to its yardstick's.  The tiles are `--distinct` SyntheticGrid tiles deepened with fresh noise (tests/deep_ref.py: deepen): the values
sit in 2000 .. 5071 like a 12-bit camera's over its pedestal.  Only deep_* and shading_* entries are called: nothing is registered.
Writes profiles/deep_shading_bench.json and prints the same JSON line.

    python tools/bench_deep_shading.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 1 --distinct 9 --limit 420]
"""
import argparse
import json
import os
import subprocess
import sys

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
    win = eng.deep_window(deeps, 1000, 999000)
    views = eng.deep_reduce(deeps, win[0], win[1])
    plane = T * T
    pct, R, ped = args.percentile, args.radius, args.pedestal

    def timed(name, fn):
        """one call between two readings of the profiler -> the stage's milliseconds"""
        eng.profile_read(reset=True)
        fn()
        return eng.profile_read(reset=True).get(name, (0.0, 0))[0]

    def alternate(a, b, warmup, steps):
        """A B A B ...: -> (all of A's times, all of B's), the warm-up rounds dropped"""
        ta, tb = [], []
        for k in range(warmup + steps):
            x, y = timed("deep_shading", a), timed("shading", b)
            if k >= warmup:
                ta.append(x); tb.append(y)
        return ta, tb

    def estimate16():
        eng.deep_shading_free(eng.deep_shading_estimate(deeps, pct, R, ped))

    def estimate8():
        eng.shading_free(eng.shading_estimate(views, pct, R))

    def report(ms_all, nbytes):
        ms = _med(ms_all)
        return {"ms": round(ms, 4), "ms_all": [round(v, 4) for v in ms_all], "compulsory_MB": round(nbytes / 1e6, 1), "GBps": round(nbytes / ms / 1e6, 1)}

    out = {"tiles": n, "tile": T, "distinct_tiles": len(base), "tile_MB": round(n * plane * 2 / 1e6, 1), "steps": args.steps, "warmup": args.warmup,
           "percentile": pct, "radius": R, "pedestal": ped, "window": list(win)}
    eng.profile_enable(True)
    # estimate: the stack read once, the profile, the field and the gain written (uint16 each; the 8-bit path: u8, Q8 uint16, uint16)
    a, b = alternate(estimate16, estimate8, args.warmup, args.steps)
    out["estimate"] = report(a, n * plane * 2 + 3 * plane * 2)
    out["estimate_8bit"] = report(b, n * plane + plane * 5)
    # apply: every sample read and written once, the gain plane read once
    f16 = eng.deep_shading_estimate(deeps, pct, R, ped)
    f8 = eng.shading_estimate(views, pct, R)
    a, b = alternate(lambda: eng.deep_shading_apply(f16, deeps), lambda: eng.shading_apply(f8, views), args.warmup, args.steps)
    out["apply"] = report(a, 2 * n * plane * 2 + plane * 2)
    out["apply_8bit"] = report(b, 2 * n * plane + plane * 2)
    eng.profile_enable(False)
    out["ratio_to_8bit_GBps"] = {"estimate": round(out["estimate"]["GBps"] / out["estimate_8bit"]["GBps"], 3),
                                 "apply": round(out["apply"]["GBps"] / out["apply_8bit"]["GBps"], 3)}
    out["ratio_to_8bit_ms"] = {"estimate": round(out["estimate"]["ms"] / out["estimate_8bit"]["ms"], 3),
                               "apply": round(out["apply"]["ms"] / out["apply_8bit"]["ms"], 3)}
    eng.deep_shading_free(f16)
    eng.shading_free(f8)
    for v in views:
        eng.tile_free(v)
    for d in deeps:
        eng.deep_free(d)
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10); ap.add_argument("--cols", type=int, default=9); ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--percentile", type=int, default=50); ap.add_argument("--radius", type=int, default=32); ap.add_argument("--pedestal", type=int, default=2000)
    ap.add_argument("--distinct", type=int, default=9, help="distinct synthetic tiles behind the stages' 90 (each deepened with noise of its own)")
    ap.add_argument("--limit", type=int, default=420, help="seconds the device process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_shading_bench.json"))
    ap.add_argument("--worker", choices=("stages",), default=None)
    args = ap.parse_args()
    if args.worker:
        return stages(args)
    res = {"metric": "16-bit shading correction: estimate and apply against their compulsory bytes and against the 8-bit kernels in the same run"}
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
