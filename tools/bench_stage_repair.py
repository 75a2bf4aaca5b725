"""The repair of failed pairs (failedPairRepair = "stage": stage.py + csrc/wide_kernels.hip) on the MI355X.

The 10 x 9 grid of 2048 x 2048 tiles (bench.py's headline workload, fixed seed) with three tiles replaced by seeded noise (128 +- sigma 2):
one in mid-column, one at a turn, one in the last column -- six pairs that cannot be registered.  "none" (register, stop at the first
failure: what flowStitch does today) and "stage" (register every pair, repair, cut at the first pair that stays failed) alternate
A B A B in ONE process.  Reported per setting: milliseconds per path with the spread, the pairs reported in front of the first break, the
pieces the dataset falls into; for "stage" the profile stages "repair" and "adjust", the position error of measured and predicted pairs
against the synthetic truth; the same grid WITHOUT blank tiles, both settings.  A run of its own under rocprofv3 --kernel-trace (a fresh
child process that only searches the six failed pairs) gives the reduce / coarse / fine split and k_wide_reduce's bytes per second
against its compulsory bytes.  On the 25 committed real dendritic pairs: the smallest and the median overlap sigma of the accepted
pairs, so that repairBlankRatio can be revisited.  Prints one JSON line; --out also writes it to a file.

    python tools/bench_stage_repair.py [--steps 5 --warmup 2 --out profiles/stage_repair_bench.json]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLANK = (4, 9, 85)            # mid-column, the turn behind column 0, the last column
CHILD_CALLS = 5


def blank_tile(seed, shape):
    import numpy as np
    return np.clip(np.rint(128.0 + np.random.default_rng(seed).normal(0.0, 2.0, shape)), 0, 255).astype(np.uint8)


def model_jobs(grid, handles_of):
    """the wide-search jobs of the six failed pairs as stage.repair_table would pose them from the true offsets of the other pairs"""
    import numpy as np
    from imagestitch_amd import stage
    true = np.array(grid.true_offsets(), np.int64)
    failed = sorted(set(k for t in BLANK for k in (t - 1, t) if 0 <= k < len(true)))
    ok = np.ones(len(true), bool); ok[failed] = False
    cls = stage.classes_of(true[ok], grid.th, grid.tw)
    M, avail, _count = stage.stage_model(true[ok], cls)
    return [(handles_of(k), handles_of(k + 1), int(M[c, 0]), int(M[c, 1])) for k in failed for c in stage.CLASSES if avail[c]], failed


def trace_child():
    """the run rocprofv3 wraps: the tiles of the six failed pairs, CHILD_CALLS wide searches of them, nothing else"""
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid
    grid = SyntheticGrid(10, 9, 2048)
    eng = isa.Engine(0)
    hs = {}

    def handle(k):
        if k not in hs:
            hs[k] = eng.tile_upload(blank_tile(k, (grid.th, grid.tw)) if k in BLANK else grid.tile(k))
        return hs[k]
    jobs, _failed = model_jobs(grid, handle)
    m = isa.Method
    for _ in range(CHILD_CALLS):
        eng.ncc_wide_batch(jobs, m.repairRadius, m.repairFactor, m.repairPeaks, m.repairMinPixels)
    for h in hs.values():
        eng.tile_free(h)
    eng.close()
    print(json.dumps({"jobs": len(jobs), "calls": CHILD_CALLS}))


def kernel_split():
    """rocprofv3 --kernel-trace --stats around trace_child (a fresh process) -> per-kernel milliseconds per call, the search's launches
    split into coarse (the first of each call) and fine (the second)"""
    exe = shutil.which("rocprofv3")
    if exe is None:
        return {"error": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="stage_repair_trace_")
    try:
        cmd = [exe, "--kernel-trace", "--stats", "-d", out, "-o", "trace", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--trace-child"]
        run = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if run.returncode != 0:
            return {"error": "rocprofv3 exited %d: %s" % (run.returncode, run.stderr[-300:])}
        child = json.loads([ln for ln in run.stdout.splitlines() if ln.startswith("{")][-1])
        files = glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_trace.csv under the output directory"}
        rows = list(csv.DictReader(open(files[0])))
        rows.sort(key=lambda r: int(r["Start_Timestamp"]))
        ms = {}
        seen = {}
        for r in rows:
            name = r["Kernel_Name"]
            short = next((s for s in ("k_wide_reduce", "k_wide_seeds", "k_wide_pick", "k_adjust_sums", "k_adjust_pick") if s in name), None)
            if short is None:
                continue
            if short.startswith("k_adjust"):
                n = seen.get(short, 0); seen[short] = n + 1
                short += "_coarse" if n % 2 == 0 else "_fine"
            ms.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
        res = {"jobs": child["jobs"], "calls": child["calls"], "ms_per_call": {k: round(sorted(v)[len(v) // 2], 4) for k, v in ms.items()},
               "launches": {k: len(v) for k, v in ms.items()}}
        per = res["ms_per_call"]
        res["reduce_ms"] = per.get("k_wide_reduce")
        res["coarse_ms"] = round(per.get("k_adjust_sums_coarse", 0.0) + per.get("k_adjust_pick_coarse", 0.0) + per.get("k_wide_seeds", 0.0), 4)
        res["fine_ms"] = round(per.get("k_adjust_sums_fine", 0.0) + per.get("k_adjust_pick_fine", 0.0) + per.get("k_wide_pick", 0.0), 4)
        return res
    except Exception as e:                                    # the record says what is missing; the timings above it stand
        return {"error": "%s: %s" % (type(e).__name__, e)}
    finally:
        shutil.rmtree(out, ignore_errors=True)


def dendritic_sigmas():
    """min(sigma_a, sigma_b) over the overlap of the 25 committed real dendritic pairs (tests/golden/real_path_strips: 640-px crops of the
    accepted (direction, i) strips, at the raw vote of the stored SURF row)"""
    import numpy as np
    from imagestitch_amd.utility import roi_rect
    gdir = os.path.join(ROOT, "tests", "golden")
    meta = json.load(open(os.path.join(gdir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(gdir, "real_path_strips.npz"))
    sig = []
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
            a = crop(nb["tiles"][k], roi_rect(nb["shape"], d, "first", i * 0.2)).astype(np.int64)
            b = crop(nb["tiles"][k + 1], roi_rect(nb["shape"], d, "second", i * 0.2)).astype(np.int64)
            off = list(e["offset"])                           # the full-tile offset back to the raw vote of the strips
            if d == 1: off[0] -= H - int(i * 0.2 * H)
            elif d == 2: off[1] -= W - int(i * 0.2 * W)
            elif d == 3: off[0] += H - int(i * 0.2 * H)
            else: off[1] += W - int(i * 0.2 * W)
            h, w = a.shape
            r0, r1, c0, c1 = max(0, -off[0]), min(h, h - off[0]), max(0, -off[1]), min(w, w - off[1])
            if r1 <= r0 or c1 <= c0:
                continue
            sig.append(min(float(a[r0 + off[0]:r1 + off[0], c0 + off[1]:c1 + off[1]].std()), float(b[r0:r1, c0:c1].std())))
    sig.sort()
    return {"pairs": len(sig), "sigma_min": round(sig[0], 3), "sigma_median": round(sig[len(sig) // 2], 3)} if sig else {"pairs": 0}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 run")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.trace_child:
        return trace_child()

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.grid import GridRegistrar, split_segments
    from imagestitch_amd.synthetic import SyntheticGrid

    m = isa.Method
    kw = dict(radius=m.repairRadius, factor=m.repairFactor, peaks=m.repairPeaks, threshold=m.repairThreshold, min_pixels=m.repairMinPixels,
              blank_ratio=m.repairBlankRatio)
    res = {"metric": "failedPairRepair none against stage behind SURF registration, 10 x 9 grid of 2048^2, A B A B in one process",
           "steps": args.steps, "warmup": args.warmup, "blank_tiles": list(BLANK), "repair": kw}
    eng = isa.Engine(0)
    grid = SyntheticGrid(10, 9, 2048)
    tiles = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    true = grid.true_offsets()
    clean = [eng.tile_upload(t) for t in tiles]
    blank = list(clean)
    for k in BLANK:
        blank[k] = eng.tile_upload(blank_tile(k, tiles[k].shape))
    shapes = [t.shape for t in tiles]
    reg = GridRegistrar(eng, method="surf", roiRatio=0.2, searchRatio=0.75, offsetEvaluate=3, directIncre=1, surfParams=eng.surf_params(), window=48)
    reg.remember = False                                      # every path registered cold: the two settings see the same registrar
    state = {}

    def none(handles):
        table, _d = reg.register(handles, shapes, 1, stop_on_fail=True)
        return table

    def stage(handles):
        table, _d = reg.register(handles, shapes, 1, stop_on_fail=False)
        state["full"] = table
        if not bool(np.all(table[:, 0] == 1)):
            table, state["report"] = reg.repair(handles, shapes, table, **kw)
            state["repaired"] = table.copy()
            bad = np.flatnonzero(table[:, 0] != 1)
            if len(bad):
                table[bad[0]:] = 0
        return table

    def timed(fn, handles, n):
        ms = []
        for _ in range(n):
            t0 = time.perf_counter()
            table = fn(handles)
            eng.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        return table, ms

    def summary(ms):
        s = sorted(ms)
        return {"median": round(s[len(s) // 2], 3), "min": round(s[0], 3), "max": round(s[-1], 3)}

    def leading(table):
        n = 0
        while n < len(table) and table[n][0]:
            n += 1
        return n

    for name, handles in (("blank", blank), ("clean", clean)):
        for fn in (none, stage):
            timed(fn, handles, args.warmup)
        legs = []
        for _ in range(2):                                    # A B A B
            t_none, ms_none = timed(none, handles, args.steps)
            state.pop("report", None); state.pop("repaired", None)
            t_stage, ms_stage = timed(stage, handles, args.steps)
            eng.profile_enable(True); eng.profile_read(reset=True)      # the stage times in a pass of their own: the profiler's events cost time
            timed(stage, handles, args.steps)
            prof = eng.profile_read(reset=True); eng.profile_enable(False)
            leg = {"none_ms_per_path": summary(ms_none), "stage_ms_per_path": summary(ms_stage),
                   "none_pairs_before_the_first_break": leading(t_none), "stage_pairs_before_the_first_break": leading(t_stage),
                   "none_pieces": len(split_segments(state["full"])), "stage_pieces": len(split_segments(state.get("repaired", state["full"]))),
                   "repair_stage_ms_per_call": round(prof["repair"][0] / max(prof["repair"][1], 1), 4) if "repair" in prof else None,
                   "repair_calls": prof.get("repair", (0.0, 0))[1]}
            rep = state.get("report")
            if rep is not None:
                leg["counts"] = rep["counts"]
                err = {"measured": [], "predicted": []}
                for e in rep["pairs"]:
                    if e["kind"] in err:
                        k = e["pair"]
                        err[e["kind"]].append(max(abs(int(t_stage[k][1]) - true[k][0]), abs(int(t_stage[k][2]) - true[k][1])) if t_stage[k][0] else None)
                leg["position_error_px"] = {kind: {"pairs": len(v), "max": max([x for x in v if x is not None], default=None)} for kind, v in err.items()}
                leg["period"], leg["ref_sigma"] = rep["period"], rep["ref_sigma"]
            legs.append(leg)
        res[name] = legs
    for h in set(clean) | set(blank):
        eng.tile_free(h)
    eng.close()

    if not args.no_trace:
        split = kernel_split()
        if "reduce_ms" in split and split["reduce_ms"]:
            f = int(m.repairFactor)
            per_job = 2 * 2048 * 2048 + 2 * (2048 // f) * (2048 // f)          # both tiles read once, both planes written once
            split["reduce_compulsory_bytes"] = per_job * split["jobs"]
            split["reduce_tb_per_s"] = round(per_job * split["jobs"] / (split["reduce_ms"] * 1e-3) / 1e12, 3)
        res["kernel_trace"] = split
    res["dendritic_overlap_sigma"] = dendritic_sigmas()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
