"""The overlap-correlation acceptance check (offsetVerify = "ncc", csrc/verify_kernels.hip) on the MI355X.

The 10 x 9 grid of 2048 x 2048 tiles (bench.py's headline workload, fixed seed) through GridRegistrar.register, SURF and ORB (configs[2],
offsetEvaluate 3), verifier off / on alternated A B A B in ONE process.  Per leg: pairs per second over --steps timed registrations of the
whole path (after --warmup), attempts per registration (with the verifier on a rejected candidate continues the search, so ORB evaluates
MORE attempts: read attempts and pairs/s together), pairs off the synthetic truth (SURF: > 1 px; ORB: any difference), the "verify" and
"vote" stage milliseconds per fused batch (vfsms_profile_*).  Prints one JSON line; --out also writes it to a file.

    python tools/bench_verify.py [--steps 5 --warmup 2 --out profiles/verify_bench.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _leg(eng, reg, handles, shapes, steps, warmup):
    for _ in range(warmup):
        table, _d = reg.register(handles, shapes, 1)
    eng.sync()
    eng.profile_enable(True); eng.profile_read(reset=True)
    a0 = reg.stats["attempts"]
    t0 = time.perf_counter()
    for _ in range(steps):
        table, _d = reg.register(handles, shapes, 1)
    eng.sync()
    dt = time.perf_counter() - t0
    prof = eng.profile_read(reset=True); eng.profile_enable(False)
    return table, dt, prof, (reg.stats["attempts"] - a0) / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.grid import GridRegistrar
    from imagestitch_amd.synthetic import SyntheticGrid

    eng = isa.Engine(0)
    thr, minpx = isa.Method.verifyThreshold, isa.Method.verifyMinPixels
    res = {"metric": "offsetVerify ncc beside none, 10 x 9 grid of 2048^2, A B A B in one process", "steps": args.steps, "warmup": args.warmup,
           "verifyThreshold": thr, "verifyMinPixels": minpx}
    grid = SyntheticGrid(10, 9, 2048)
    tiles = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    truth = np.asarray(grid.true_offsets(), np.int64)
    handles = [eng.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    P = len(tiles) - 1
    for method in ("surf", "orb"):
        legs = []
        steps, warmup = (args.steps, args.warmup) if method == "surf" else (max(1, args.steps // 2), 1)
        for verify in ("none", "ncc", "none", "ncc"):
            reg = GridRegistrar(eng, method=method, roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1,
                                surfParams=eng.surf_params() if method == "surf" else eng.orb_params(), window=48,
                                offsetVerify=verify, verifyThreshold=thr, verifyMinPixels=minpx)
            table, dt, prof, attempts = _leg(eng, reg, handles, shapes, steps, warmup)
            ok = table[:, 0] == 1
            err = np.abs(table[:, 1:3].astype(np.int64) - truth).max(axis=1)
            ver_ms, ver_calls = prof.get("verify", (0.0, 0))
            vote_ms, vote_calls = prof.get("vote", (0.0, 0))
            legs.append({"offsetVerify": verify, "pairs_per_s": round(P * steps / dt, 2), "ms_per_path": round(1e3 * dt / steps, 3),
                         "attempts_per_path": attempts, "pairs_off_truth": int((~ok | (err > (1 if method == "surf" else 0))).sum()),
                         "pairs_failed": int((~ok).sum()), "verify_ms_per_batch": round(ver_ms / max(ver_calls, 1), 4), "verify_batches": ver_calls,
                         "verify_ms_per_path": round(ver_ms / steps, 4), "vote_ms_per_batch": round(vote_ms / max(vote_calls, 1), 4),
                         "stage_ms_per_path": round(sum(v[0] for v in prof.values()) / steps, 3)})
        res["surf_10x9_2048" if method == "surf" else "orb_configs2_10x9_2048"] = legs
    for h in handles:
        eng.tile_free(h)
    eng.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
