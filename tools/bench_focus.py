"""Focus stacking (Method.focusStack) at production size, gray and colour, in one process.

A focus series of tests/focus_cases.py (2048 x 2048, N = 8 planes, "quad" depth map) is uploaded to HBM.  Per mode (gray, B G R) the script
  - reads the two stages "focus_select" and "focus_compose" from the library's event profiler (vfsms_profile_read), R = 4, median 1;
  - times the operator (Engine.focus_stack, host to device-synchronised end, the download of out, D and S included) against the numpy
    specification on the host (tests/focus_ref.py: the "parent" leg -- what a user has without this operator), alternated A B A B, and
    checks that both return the same bytes;
  - sets the stages against the compulsory bytes -- N h w ch read, h w (ch + 1) written -- as a rate and as a fraction of HBM bandwidth;
  - sweeps R in {1, 2, 4, 8, 16, 31} at N = 8 and N in {2, 4, 8, 16, 64} at R = 4 (N > 8 names the eight planes again: the kernels' time does
    not depend on the pixel values).  The compulsory bytes do not depend on R: a select time that grows with R is not HBM time.
The dataset leg writes the series of a few positions as PNG files and runs focus.fuse_dataset on them, split into decode (thread-seconds of
the decoder pool), fuse (upload of the planes excluded: Engine.focus_stack alone), file write and the whole wall clock.
Writes profiles/focus_bench.json and prints the same JSON line.

    python tools/bench_focus.py [--size 2048 --planes 8 --radius 4 --steps 5 --warmup 2 --host-steps 2 --positions 4]
"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_GBPS_MEASURED = 6300.0      # float4 copy on the MI355X; the data sheet says 8000
HBM_GBPS_SPEC = 8000.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--planes", type=int, default=8)
    ap.add_argument("--radius", type=int, default=4)
    ap.add_argument("--steps", type=int, default=5, help="timed repetitions per device leg (at least 3)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--host-steps", type=int, default=2, help="repetitions of the numpy specification (the parent leg)")
    ap.add_argument("--positions", type=int, default=4, help="stage positions of the dataset leg (0: skip it)")
    ap.add_argument("--dataset-planes", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "focus_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 3)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd import focus
    import focus_cases as FC
    import focus_ref as FR

    eng = isa.Engine(0)
    h = w = args.size
    N, R = args.planes, args.radius

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 3), "ms_min": round(float(v.min()), 3), "ms_max": round(float(v.max()), 3)}

    def stages(handles, radius, reps):
        """median per-call time of the two stages by HIP events"""
        eng.profile_enable(True)
        eng.profile_read(reset=True)
        sel, com = [], []
        for _ in range(reps):
            eng.focus_stack(handles, radius=radius, median=1)
            p = eng.profile_read(reset=True)
            sel.append(p.get("focus_select", (0.0, 0))[0]); com.append(p.get("focus_compose", (0.0, 0))[0])
        eng.profile_enable(False)
        return float(np.median(sel)), float(np.median(com))

    def rates(n, ch, sel_ms, com_ms):
        read, written = n * h * w * ch, h * w * (ch + 1)
        total = sel_ms + com_ms
        return {"compulsory_MB": round((read + written) / 1e6, 1),
                "GBps_of_compulsory": round((read + written) / total / 1e6, 1) if total > 0 else None,
                "fraction_of_hbm_measured_6.3TBps": round((read + written) / total / 1e6 / HBM_GBPS_MEASURED, 4) if total > 0 else None,
                "fraction_of_hbm_spec_8TBps": round((read + written) / total / 1e6 / HBM_GBPS_SPEC, 4) if total > 0 else None,
                "select_ns_per_pixel_plane": round(sel_ms * 1e6 / (n * h * w), 4)}

    res = {"metric": "focus stacking: select and compose stages, the operator against the numpy specification, sweeps over R and N, the dataset leg",
           "size": [h, w], "planes": N, "radius": R, "median": 1, "steps": args.steps, "warmup": args.warmup, "host_steps": args.host_steps}
    for mode, ch in (("gray", 1), ("color", 3)):
        planes, sharp, depth = FC.stack((h, w) if ch == 1 else (h, w, 3), N, "quad", seed=1)
        handles = [eng.tile_upload(p) if ch == 1 else eng.tile_upload_color(p) for p in planes]
        eng.sync()
        for _ in range(args.warmup):
            got = eng.focus_stack(handles, radius=R, median=1)
        dev, host, want = [], [], None
        for k in range(max(args.steps, args.host_steps)):            # A B A B
            if k < args.steps:
                eng.sync(); t0 = time.perf_counter()
                got = eng.focus_stack(handles, radius=R, median=1)
                eng.sync(); dev.append((time.perf_counter() - t0) * 1e3)
            if k < args.host_steps:
                t0 = time.perf_counter()
                want = FR.fuse(planes, R, 1)
                host.append((time.perf_counter() - t0) * 1e3)
        same = want is None or all(np.array_equal(a, b) for a, b in zip(got, want))
        sel, com = stages(handles, R, args.steps)
        r = {"stage_ms": {"focus_select": round(sel, 4), "focus_compose": round(com, 4)}, "operator": stats(dev),
             "numpy_specification_on_host": stats(host) if host else "not measured", "equal_to_specification": bool(same),
             "right_plane_fraction": round(float(np.mean(got[1] == depth)), 4)}
        r.update(rates(N, ch, sel, com))
        if host:
            r["host_over_operator"] = round(float(np.median(host)) / float(np.median(dev)), 1)
        sweepR = {}
        for rr in (1, 2, 4, 8, 16, 31):
            eng.focus_stack(handles, radius=rr, median=1)
            s, c = stages(handles, rr, 3)
            sweepR[str(rr)] = {"focus_select_ms": round(s, 4), "focus_compose_ms": round(c, 4), "select_ns_per_pixel_plane": round(s * 1e6 / (N * h * w), 4)}
        sweepN = {}
        for nn in (2, 4, 8, 16, 64):
            hs = [handles[k % N] for k in range(nn)]
            eng.focus_stack(hs, radius=R, median=1)
            s, c = stages(hs, R, 3)
            sweepN[str(nn)] = {"focus_select_ms": round(s, 4), "focus_compose_ms": round(c, 4), "select_ns_per_pixel_plane": round(s * 1e6 / (nn * h * w), 4)}
        r["sweep_radius"], r["sweep_planes"] = sweepR, sweepN
        for hd in handles:
            eng.tile_free(hd)
        res[mode] = r
        if ch == 1 and args.positions > 0:
            res["dataset"] = dataset_leg(eng, isa, focus, planes[:args.dataset_planes], args.positions, R)
    eng.close()
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


def dataset_leg(eng, isa, focus, planes, positions, radius):
    """focus.fuse_dataset over `positions` x len(planes) PNG files of the tile size, gray: where the wall clock goes"""
    import threading
    from PIL import Image
    K = len(planes)
    with tempfile.TemporaryDirectory() as tmp:
        files = []
        for p in range(positions):
            for z, img in enumerate(planes):
                files.append(os.path.join(tmp, "p%03d_z%d.png" % (p, z)))
                Image.fromarray(np_roll(img, 7 * p)).save(files[-1], compress_level=1)
        file_MB = sum(os.path.getsize(f) for f in files) / 1e6
        st = isa.Stitcher(); st._engine = eng
        st.printAndWrite = lambda c: None
        st.focusStack, st.focusRadius, st.focusMedian = "pixel", radius, 1
        t = {"decode": 0.0, "fuse": 0.0, "write": 0.0}
        lock = threading.Lock()
        real_read, real_write, real_fuse = focus._imread, focus._imwrite, eng.focus_stack

        def timed(key, fn):
            def run(*a, **k):
                t0 = time.perf_counter()
                try:
                    return fn(*a, **k)
                finally:
                    with lock:
                        t[key] += time.perf_counter() - t0
            return run
        focus._imread, focus._imwrite, eng.focus_stack = timed("decode", real_read), timed("write", real_write), timed("fuse", real_fuse)
        try:
            walls = []
            for rep in range(2):                                      # the second pass is the warm one
                for k in t:
                    t[k] = 0.0
                t0 = time.perf_counter()
                focus.fuse_dataset(st, files, K, os.path.join(tmp, "out%d" % rep))
                walls.append(time.perf_counter() - t0)
        finally:
            focus._imread, focus._imwrite = real_read, real_write
            del eng.focus_stack
        return {"positions": positions, "planes": K, "input_png_MB": round(file_MB, 1), "wall_ms": round(walls[-1] * 1e3, 1), "first_pass_wall_ms": round(walls[0] * 1e3, 1),
                "decode_thread_ms": round(t["decode"] * 1e3, 1), "fuse_ms": round(t["fuse"] * 1e3, 1), "write_ms": round(t["write"] * 1e3, 1),
                "note": "decode runs on the decoder pool beside the fuse of the position before: its thread time overlaps the wall clock; the upload of the planes is in neither leg"}


def np_roll(img, k):
    import numpy as np
    return np.ascontiguousarray(np.roll(img, k, axis=1))


if __name__ == "__main__":
    main()
