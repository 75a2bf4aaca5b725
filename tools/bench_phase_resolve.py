#!/usr/bin/env python
"""bench_phase_resolve.py -- what Stitcher.phaseResolve = "ncc" costs and what it buys on the headline grid (10 x 9 tiles of 2048^2, method
phase): the resolver off (the reference's reading: bench.py's phase line) and on, alternated A B A B in ONE process on the same resident
tiles, then a separate profiled pass for the "phase_resolve" stage, then both legs against the grid's true offsets.

The device work runs in a child process under a time limit of its own (--limit seconds); the parent only waits and writes
profiles/phase_resolve_bench.json.  No GPU: the child fails, nothing is written.

    python tools/bench_phase_resolve.py [--rows 10 --cols 9 --tile 2048 --steps 5 --warmup 2 --limit 420]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface_bytes(tile, roi_ratio, peaks):
    """what the stage must move per attempt, from the shapes: one read of the M x N float64 surface + at most 4 K overlap reads of two u8 strips"""
    from imagestitch_amd._lib import load_library
    import ctypes
    import numpy as np
    h = int(tile * roi_ratio)
    info = np.zeros(8, np.int32)
    load_library().vfsms_phase_plan(h, tile, info.ctypes.data_as(ctypes.c_void_p))
    M, N = int(info[2]), int(info[3])
    return dict(strip=[h, tile], surface=[M, N], surface_bytes=8 * M * N, strip_read_bytes_max=4 * peaks * 2 * h * tile)


def worker(args):
    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.grid import GridRegistrar
    from imagestitch_amd.synthetic import SyntheticGrid
    grid = SyntheticGrid(args.rows, args.cols, args.tile)
    t0 = time.perf_counter()
    tiles = list(grid.tiles(processes=16)) if args.rows * args.cols > 16 else grid.tiles(threads=8)
    truth = grid.true_offsets()
    eng = isa.Engine(0)
    handles = [eng.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    P = len(tiles) - 1
    setup_s = time.perf_counter() - t0
    kw = dict(method="phase", roiRatio=0.2, window=48, phaseResolveThreshold=args.threshold, phasePeaks=args.peaks, phaseResolveMinPixels=args.min_pixels)
    legs = {"off": GridRegistrar(eng, phaseResolve="none", **kw), "on": GridRegistrar(eng, phaseResolve="ncc", **kw)}

    def step(name):
        reg = legs[name]
        a0 = reg.stats["attempts"]
        eng.sync()
        t = time.perf_counter()
        table, _d = reg.register(handles, shapes, 1)
        eng.sync()
        return time.perf_counter() - t, table, reg.stats["attempts"] - a0
    for _ in range(args.warmup):                              # every shape and both legs, path memory included
        for name in ("off", "on"):
            step(name)
    times = {"off": [], "on": []}; tables = {}; attempts = {}
    for _ in range(args.steps):                               # A B A B
        for name in ("off", "on"):
            dt, tables[name], attempts[name] = step(name)
            times[name].append(dt)
    # the stage times, in a pass of their own (the event records slow the host)
    eng.profile_enable(True); eng.profile_read(reset=True)
    for _ in range(args.steps):
        step("on")
    prof = eng.profile_read(reset=True); eng.profile_enable(False)
    b0 = legs["on"].stats["batches"]
    step("on")
    batches = legs["on"].stats["batches"] - b0

    def against_truth(table):
        off, worst = 0, 0
        for row, t in zip(table, truth):
            e = max(abs(int(row[1]) - t[0]), abs(int(row[2]) - t[1])) if row[0] else None
            if e is None or e > 1:
                off += 1
            if e is not None:
                worst = max(worst, e)
        return dict(pairs_off_truth=off, unregistered=int(sum(1 for r in table if not r[0])), max_offset_error_px=worst)
    out = dict(grid=[args.rows, args.cols, args.tile], pairs=P, steps=args.steps, warmup=args.warmup, setup_s=round(setup_s, 2),
               resolver=dict(peaks=args.peaks, threshold=args.threshold, min_pixels=args.min_pixels), legs={})
    for name in ("off", "on"):
        ts = sorted(times[name])
        out["legs"][name] = dict(pairs_per_s=round(P / ts[len(ts) // 2], 1), step_ms_median=round(1e3 * ts[len(ts) // 2], 3),
                                 step_ms_min=round(1e3 * ts[0], 3), step_ms_max=round(1e3 * ts[-1], 3), attempts_per_path=attempts[name],
                                 **against_truth(tables[name]))
    n = args.steps
    out["stages_ms_per_path"] = {k: round(v[0] / n, 4) for k, v in sorted(prof.items())}
    out["batches_per_path"] = batches
    if "phase_resolve" in prof and batches:
        out["phase_resolve_ms_per_batch"] = round(prof["phase_resolve"][0] / n / batches, 4)
    sb = surface_bytes(args.tile, 0.2, args.peaks)
    out["bytes_per_attempt"] = sb
    if "phase_resolve" in prof:
        per_attempt_s = prof["phase_resolve"][0] * 1e-3 / n / max(attempts["on"], 1)
        out["phase_resolve_us_per_attempt"] = round(per_attempt_s * 1e6, 3)
        out["phase_resolve_gb_per_s_surface_only"] = round(sb["surface_bytes"] / per_attempt_s / 1e9, 1)
    for h in handles:
        eng.tile_free(h)
    eng.close()
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10); ap.add_argument("--cols", type=int, default=9); ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--steps", type=int, default=5); ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--peaks", type=int, default=2); ap.add_argument("--threshold", type=float, default=0.5); ap.add_argument("--min-pixels", type=int, default=4096)
    ap.add_argument("--limit", type=int, default=420, help="seconds the device process may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "phase_resolve_bench.json"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker"] + [a for a in sys.argv[1:] if a != "--worker"]
    try:
        res = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=args.limit, cwd=ROOT)
    except subprocess.TimeoutExpired:
        print("the device process ran into its limit of %d s: nothing written" % args.limit, file=sys.stderr)
        return 124
    if res.returncode != 0:
        print("the device process failed with status %d: nothing written" % res.returncode, file=sys.stderr)
        return res.returncode
    line = res.stdout.decode().strip().splitlines()[-1]
    out = json.loads(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
