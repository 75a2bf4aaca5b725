"""The global placement (globalAdjust = "ncc", csrc/adjust_kernels.hip + adjust.py) on the MI355X.

The 10 x 9 grid of 2048 x 2048 tiles (bench.py's headline workload, fixed seed): GridRegistrar.register with SURF gives the path offsets,
GridRegistrar.adjust places the tiles.  Registration (A) and adjustment (B) alternate A B A B in ONE process.  Reported: milliseconds per
registration of the whole path; per adjustment the wall time, the "adjust" stage (vfsms_profile_*: the window search of every edge, one
launch group) and the host's least-squares solve; the edges found / measured / dropped; and the maximum and RMS error of the tile
POSITIONS against the synthetic truth, laid out from the voted offsets (before) and from the adjusted ones (after).  The one requirement
is after <= before.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_adjust.py [--steps 5 --warmup 2 --out profiles/adjust_bench.json]
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
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--radius", type=int, default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd import adjust as ADJ
    from imagestitch_amd.grid import GridRegistrar
    from imagestitch_amd.synthetic import SyntheticGrid

    eng = isa.Engine(0)
    R = int(args.radius or isa.Method.adjustRadius)
    thr, minpx = isa.Method.adjustThreshold, isa.Method.adjustMinPixels
    res = {"metric": "globalAdjust ncc behind SURF registration, 10 x 9 grid of 2048^2, A B A B in one process", "steps": args.steps,
           "warmup": args.warmup, "adjustRadius": R, "adjustThreshold": thr, "adjustMinPixels": minpx}
    grid = SyntheticGrid(10, 9, 2048)
    tiles = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    truth = ADJ.path_positions(grid.true_offsets()).astype(np.float64)
    handles = [eng.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    reg = GridRegistrar(eng, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1, surfParams=eng.surf_params(), window=48)

    def register(n):
        t0 = time.perf_counter()
        for _ in range(n):
            table, _d = reg.register(handles, shapes, 1)
        eng.sync()
        return table, (time.perf_counter() - t0) / max(n, 1)

    def adjust(table, n):
        eng.profile_enable(True); eng.profile_read(reset=True)
        t0 = time.perf_counter()
        for _ in range(n):
            out, report = reg.adjust(handles, shapes, table, radius=R, threshold=thr, min_pixels=minpx)
        dt = (time.perf_counter() - t0) / max(n, 1)
        prof = eng.profile_read(reset=True); eng.profile_enable(False)
        return out, report, dt, prof.get("adjust", (0.0, 0))

    table, _ = register(args.warmup)
    assert bool(np.all(table[:, 0] == 1)), "a pair of the synthetic grid was not registered"
    adjust(table, args.warmup)
    legs = []
    for _ in range(2):                                        # A B A B
        table, reg_s = register(args.steps)
        out, report, adj_s, (stage_ms, groups) = adjust(table, args.steps)
        edges = ADJ.neighbour_edges(shapes, table[:, 1:3], R)
        t0 = time.perf_counter()
        for _k in range(args.steps):
            ADJ.solve_positions(len(shapes), edges)
        solve_ms = 1e3 * (time.perf_counter() - t0) / args.steps

        def err(offsets):
            e = np.sqrt(((ADJ.path_positions(offsets) - truth) ** 2).sum(axis=1))
            return {"max": round(float(e.max()), 3), "rms": round(float(np.sqrt((e * e).mean())), 3)}
        legs.append({"register_ms_per_path": round(1e3 * reg_s, 3), "adjust_wall_ms": round(1e3 * adj_s, 3),
                     "adjust_stage_ms": round(stage_ms / max(groups, 1), 4), "adjust_launch_groups": groups, "host_solve_ms": round(solve_ms, 3),
                     "edges": report["edges"], "measured": report["measured"], "dropped": report["dropped"], "kept_votes": report["kept_votes"],
                     "candidates": report["edges"] * (2 * R + 1) ** 2,
                     "edge_residual_before": report["residual_before"], "edge_residual_after": report["residual_after"],
                     "position_error_before": err(table[:, 1:3]), "position_error_after": err(out)})
    res["surf_10x9_2048"] = legs
    res["position_error_after_le_before"] = all(l["position_error_after"]["max"] <= l["position_error_before"]["max"] and
                                                l["position_error_after"]["rms"] <= l["position_error_before"]["rms"] for l in legs)
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
