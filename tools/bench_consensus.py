"""The consensus vote tail (offsetCaculate = "ransac", csrc/consensus_kernels.hip) beside the mode on the MI355X.

  headline  the 10 x 9 grid of 2048 x 2048 SURF tiles (bench.py's headline workload) through GridRegistrar.register, once per estimator:
            pairs per second over --steps timed registrations of the whole path (after --warmup), the "vote" stage milliseconds per
            batch (vfsms_profile_*: merge + compaction + vote of every fused batch), pairs accepted off the synthetic truth (> 1 px)
  strips    the vote stage of one fused SURF batch of configs[4]-sized strips (819 x 4096 and 4096 x 819 ROIs of 4096^2 tiles) per
            estimator, with the matches and votes per job that the O(M^2) support pass sees
  orb       configs[2]: the same 10 x 9 grid with ORB at offsetEvaluate 3, per estimator: pairs accepted off the synthetic truth (any
            difference: BASELINE asks ORB for the exact truth) and failed pairs
Prints one JSON line.

    python tools/bench_consensus.py [--steps 5 --warmup 2 --tol 3 --skip orb]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _register(eng, reg, handles, shapes, steps, warmup):
    for _ in range(warmup):
        table, _d = reg.register(handles, shapes, 1)
    eng.sync()
    eng.profile_enable(True); eng.profile_read(reset=True)
    t0 = time.perf_counter()
    for _ in range(steps):
        table, _d = reg.register(handles, shapes, 1)
    eng.sync()
    dt = time.perf_counter() - t0
    prof = eng.profile_read(reset=True); eng.profile_enable(False)
    return table, dt, prof


def _off_truth(table, truth, tol):
    import numpy as np
    ok = table[:, 0] == 1
    err = np.abs(table[:, 1:3].astype(np.int64) - np.asarray(truth, np.int64)).max(axis=1)
    return int((ok & (err > tol)).sum()), int((~ok).sum()), int(err[ok].max()) if ok.any() else -1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5, help="timed registrations of the whole headline path per estimator")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--tol", type=int, default=3, help="Method.ransacThreshold")
    ap.add_argument("--skip", nargs="*", default=[], choices=["headline", "strips", "orb"])
    args = ap.parse_args()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.grid import GridRegistrar
    from imagestitch_amd.synthetic import SyntheticGrid

    eng = isa.Engine(0)
    res = {"metric": "consensus vote tail (offsetCaculate ransac) beside the mode", "tol": args.tol, "steps": args.steps, "warmup": args.warmup}
    threads = min(16, len(os.sched_getaffinity(0)))
    if not ("headline" in args.skip and "orb" in args.skip):
        grid = SyntheticGrid(10, 9, 2048)
        tiles = grid.tiles(threads=threads)
        truth = grid.true_offsets()
        handles = [eng.tile_upload(t) for t in tiles]
        shapes = [t.shape for t in tiles]
        P = len(tiles) - 1
        for method in ("surf", "orb"):
            if (method == "surf" and "headline" in args.skip) or (method == "orb" and "orb" in args.skip):
                continue
            out = {}
            for est in ("mode", "ransac"):
                reg = GridRegistrar(eng, method=method, roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1,
                                    surfParams=eng.surf_params() if method == "surf" else eng.orb_params(), window=48,
                                    offsetCaculate=est, ransacThreshold=args.tol)
                steps = args.steps if method == "surf" else 1
                table, dt, prof = _register(eng, reg, handles, shapes, steps, args.warmup if method == "surf" else 1)
                vote_ms, vote_calls = prof.get("vote", (0.0, 0))
                off, failed, max_err = _off_truth(table, truth, 1 if method == "surf" else 0)
                out[est] = {"pairs_per_s": round(P * steps / dt, 2), "vote_ms_per_batch": round(vote_ms / max(vote_calls, 1), 4),
                            "vote_batches": vote_calls, "vote_ms_per_path": round(vote_ms / steps, 3),
                            "stage_ms_per_path": round(sum(v[0] for v in prof.values()) / steps, 3),
                            "pairs_off_truth": off, "pairs_failed": failed, "max_err_px": max_err,
                            "off_truth_1px": _off_truth(table, truth, 1)[0]}
            res["headline_surf_10x9_2048" if method == "surf" else "orb_configs2_10x9_2048"] = out
        for h in handles:
            eng.tile_free(h)
    if "strips" not in args.skip:
        grid = SyntheticGrid(2, 2, 4096)
        tiles = grid.tiles(threads=threads)
        hs = [eng.tile_upload(t) for t in tiles]
        jobs = []
        for a, b, d in ((0, 1, 1), (2, 3, 1), (0, 2, 2), (1, 3, 2)):
            for d2 in (d, 1 if d == 2 else 2):
                ra = isa.roi_rect(tiles[a].shape, d2, "first", 0.2); rb = isa.roi_rect(tiles[b].shape, d2, "second", 0.2)
                jobs.append((hs[a], hs[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]))
        out = {}
        for est in ("mode", "ransac"):
            eng.set_offset_estimator(est, args.tol)
            try:
                for _ in range(args.warmup):
                    rows = eng.attempt_surf_batch(jobs)
                eng.sync()
                eng.profile_enable(True); eng.profile_read(reset=True)
                for _ in range(args.steps):
                    rows = eng.attempt_surf_batch(jobs)
                eng.sync()
                prof = eng.profile_read(reset=True); eng.profile_enable(False)
            finally:
                eng.set_offset_estimator("mode")
            vote_ms, vote_calls = prof.get("vote", (0.0, 0))
            out[est] = {"vote_ms_per_batch": round(vote_ms / max(vote_calls, 1), 4), "batch_stage_ms": round(sum(v[0] for v in prof.values()) / args.steps, 3),
                        "jobs": len(jobs), "matches_per_job": [int(r[6]) for r in rows], "keypoints_a": [int(r[4]) for r in rows],
                        "rows_status_dx_dy_count": [[int(v) for v in r[:4]] for r in rows]}
        res["strips_configs4_4096"] = out
        for h in hs:
            eng.tile_free(h)
    eng.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
