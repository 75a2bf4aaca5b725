"""JPEG tiles decoded on the device (Method.jpegDecoder = "device", "device-entropy") against the host decoder, decode inclusive, on the
headline grid, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is written as JPEG files (quality 90; gray files, and 4:2:0 colour files
tinted as bench.py --from-files --color tints them) and registered through the Stitcher's own ingest (Stitcher._registerBatched: tiles
reserved up front, a pool of decoder threads fills them while the registrar works), exactly as bench.py --from-files does.  Per mode and per
decoder-pool size (4 and 16 threads: 16 is what a job on a shared GPU host is granted; the pool is never sized by os.cpu_count()) the legs
  A  host:   vfsms_tile_fill_jpeg      (libjpeg-turbo up to the sample planes on the decoder thread)
  B  device: vfsms_tile_fill_jpeg_dct  (libjpeg-turbo up to the coefficients; dequantisation + inverse DCT in k_jpeg_idct)
  C  device-entropy: vfsms_tile_fill_jpeg_huff  (a marker scan on the decoder thread; Huffman decode, DC prediction, inverse DCT on the device)
are alternated A B C A B C after warm-up.  Recorded per leg: warm pairs/s, and the decoder threads' summed host seconds per tile
(Stitcher._ingestStats: wall time inside the fill call, which includes the upload and the wait for the device).
Then, with the library's event profiler on, the "jpeg_decode" stage on the coefficients of one tile of each mode (Engine.jpeg_idct per
component) against the bytes the kernel must move -- 2 B in, 1 B out per sample -- as a fraction of the 8 TB/s HBM figure the other
benchmarks use; and the bytes that cross the link per tile either way.
Then the bare entropy operator (Engine.jpeg_entropy_decode) over every file of the grid: the stages "jpeg_entropy_sync / _rounds / _scan /
_write" (the DC prefix is part of the scan), rounds_used, and the write pass against its compulsory bytes -- 2 B per coefficient slot zeroed
plus the stream read once.  --sweep 512=LIB,2048=LIB repeats that probe in a child process per library built with another
VFSMS_JPEG_HUFF_SUB_BITS (VFSMS_LIB).
Writes profiles/jpeg_entropy_bench.json (profiles/jpeg_decode_bench.json is the two-leg record of the change before) and prints the same line.

    python tools/bench_jpeg_decode.py [--rows 10 --cols 9 --tile 2048 --steps 8 --warmup 1 --threads 4,16 --sweep 512=a.so,2048=b.so]
"""
import argparse
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

HBM_GBPS = 8000.0
LEGS = ("host", "device", "device-entropy")
TOOK = {"host": None, "device": "dct", "device-entropy": "huff"}


def entropy_probe(eng, paths, reps=3):
    """the bare operator over `paths` with the event profiler on -> the stage split per file (ms), rounds_used, bytes"""
    import numpy as np
    from imagestitch_amd import _lib
    datas = [open(f, "rb").read() for f in paths]
    rounds, slots, stream, record, nsub = [], 0, 0, 0, 0
    for d in datas:                                             # warm: the arena has grown, the kernels are loaded
        rc, h, w, comps, used = eng.jpeg_entropy_decode(d, -1)
        assert rc == 0, rc
        rounds.append(used)
        rec = _lib.jpeg_scan(d)
        slots += sum(int(c.size) for c, _ in comps); stream += rec["stream_bytes"]; record += rec["total_bytes"]; nsub += rec["nsub"]
    sub_bits = rec["sub_bits"]
    eng.profile_enable(True)
    eng.profile_read(reset=True)
    for _ in range(reps):
        for d in datas:
            eng.jpeg_entropy_decode(d, -1)
    prof = eng.profile_read(reset=True)
    eng.profile_enable(False)
    n = len(datas) * reps
    stages = {k: round(prof.get(k, (0.0, 0))[0] / n, 4) for k in ("jpeg_entropy", "jpeg_entropy_sync", "jpeg_entropy_rounds", "jpeg_entropy_scan", "jpeg_entropy_write")}
    compulsory = (2 * slots + stream) / len(datas)
    wr = stages["jpeg_entropy_write"]
    return {"sub_bits": sub_bits, "files": len(datas), "ms_per_file": stages, "rounds_used": {"min": int(min(rounds)), "median": float(np.median(rounds)), "max": int(max(rounds))},
            "subsequences_per_file": round(nsub / len(datas), 1), "record_bytes_per_file": round(record / len(datas)),
            "write_pass": {"compulsory_MB": round(compulsory / 1e6, 3), "GBps_of_compulsory": round(compulsory / wr / 1e6, 1) if wr > 0 else None,
                           "fraction_of_hbm": round(compulsory / wr / 1e6 / HBM_GBPS, 4) if wr > 0 else None}}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--threads", default="4,16", help="decoder-pool sizes, comma separated")
    ap.add_argument("--steps", type=int, default=8, help="timed repetitions per leg (at least 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the tiles are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_entropy_bench.json"))
    ap.add_argument("--sweep", default="", help="BITS=LIBRARY,...: the entropy probe again per library built with another VFSMS_JPEG_HUFF_SUB_BITS")
    ap.add_argument("--probe", default=None, help="(internal) a file listing JPEG paths: run the entropy probe over them, print its JSON, stop")
    args = ap.parse_args()
    if args.probe:
        import imagestitch_amd as isa
        eng = isa.Engine(0)
        try:
            print(json.dumps(entropy_probe(eng, [ln.strip() for ln in open(args.probe) if ln.strip()])))
        finally:
            eng.close()
        return
    args.steps = max(args.steps, 2)
    pools = [int(v) for v in args.threads.split(",") if v]

    import numpy as np
    from PIL import Image
    import imagestitch_amd as isa
    from imagestitch_amd import _lib
    from imagestitch_amd import io as IO
    from imagestitch_amd.synthetic import SyntheticGrid

    cpus = IO._usable_cpus()
    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    tiles = grid.tiles(range(grid.n_tiles), threads=min(16, cpus))
    outdir = args.dir or tempfile.mkdtemp(prefix="vfsms_jpegdec_")
    os.makedirs(outdir, exist_ok=True)
    files = {"gray": [], "color": []}
    for k, t in enumerate(tiles):
        ft = t.astype(np.float32)
        rgb = np.clip(np.stack([0.6 * ft + 30, ft, 255 - 0.7 * ft], -1), 0, 255).astype(np.uint8)
        for mode, img in (("gray", t), ("color", rgb)):
            f = os.path.join(outdir, "%s_%03d.jpg" % (mode, k))
            Image.fromarray(img).save(f, quality=args.quality)
            files[mode].append(f)
    del tiles

    eng = isa.Engine(0)
    P, n = grid.n_pairs, grid.n_tiles
    res = {"metric": "decode-inclusive registration of the headline grid from JPEG files: host decoder (A, vfsms_tile_fill_jpeg) against the device "
                     "half of the decoder (B, vfsms_tile_fill_jpeg_dct) and the whole decoder on the device (C, vfsms_tile_fill_jpeg_huff), legs "
                     "alternated A B C A B C in one process",
           "grid": [args.rows, args.cols, args.tile], "pairs": P, "tiles": n, "quality": args.quality, "usable_cpus": cpus,
           "os_cpu_count": os.cpu_count(), "decoder_threads": pools, "steps": args.steps, "warmup": args.warmup, "hbm_GBps": HBM_GBPS}
    names = ("direction", "directIncre", "roiRatio", "featureMethod", "offsetEvaluate", "isColorMode", "fuseMethod")
    old = {k: getattr(isa.Stitcher, k) for k in names}
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.featureMethod, isa.Stitcher.offsetEvaluate = 1, 0.2, "surf", 3
        isa.Stitcher.fuseMethod = "notFuse"
        truth = grid.true_offsets()
        for mode in ("gray", "color"):
            color = mode == "color"
            isa.Stitcher.isColorMode = color
            res[mode] = {"files_MB": round(sum(os.path.getsize(f) for f in files[mode]) / 1e6, 1)}
            for nthreads in pools:
                s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False
                s.decodeThreads = nthreads

                def leg(decoder):
                    s.jpegDecoder = decoder
                    s.direction = 1
                    eng.sync(); t0 = time.perf_counter()
                    status, end, offs, _d = s._registerBatched(files[mode], s.calculateOffsetForFeatureSearchIncre)
                    eng.sync(); dt = time.perf_counter() - t0
                    for h, _shape in (s.__dict__.pop("_resident", None) or {}).values():
                        eng.tile_free(h)
                    ist = dict(s._ingestStats)
                    assert status and end == P, (decoder, status, end)
                    assert ist.get("native", 0) == n and all(ist.get(v, 0) == (n if v == TOOK[decoder] else 0) for v in ("dct", "huff")), (decoder, ist)
                    worst = max(max(abs(o[0] - t_[0]), abs(o[1] - t_[1])) for o, t_ in zip(offs, truth))
                    return dt, ist["decode_s"] / n, worst, [[int(v) for v in o] for o in offs]
                runs = {d: [] for d in LEGS}
                for k in range(args.warmup + args.steps):
                    for decoder in LEGS:
                        r = leg(decoder)
                        if k >= args.warmup:
                            runs[decoder].append(r)
                assert runs["host"][0][3] == runs["device"][0][3] == runs["device-entropy"][0][3]       # the same offsets every way
                entry = {}
                for decoder, rr in runs.items():
                    dts = np.array([r[0] for r in rr])
                    entry[decoder] = {"pairs_per_s_median": round(P / float(np.median(dts)), 1), "pairs_per_s_best": round(P / float(dts.min()), 1),
                                      "pairs_per_s_worst": round(P / float(dts.max()), 1), "ms_per_step": [round(float(v) * 1e3, 1) for v in dts],
                                      "host_ms_per_tile_summed_over_threads": round(float(np.median([r[1] for r in rr])) * 1e3, 3),
                                      "max_abs_offset_error_px": int(max(r[2] for r in rr))}
                for d, key in (("device", "device"), ("device-entropy", "entropy")):
                    entry[key + "_over_host_pairs_per_s"] = round(entry[d]["pairs_per_s_median"] / entry["host"]["pairs_per_s_median"], 3)
                    entry[key + "_over_host_host_ms_per_tile"] = round(entry[d]["host_ms_per_tile_summed_over_threads"] /
                                                                       entry["host"]["host_ms_per_tile_summed_over_threads"], 3)
                res[mode]["threads_%d" % nthreads] = entry
            # the kernel alone, on one tile's coefficients: every component the request needs (gray: luma; colour: all three)
            with open(files[mode][n // 2], "rb") as fh:
                data = fh.read()
            h, w, comps = _lib.jpeg_coefficients(data)
            comps = comps if color else comps[:1]
            for coef, quant in comps:
                eng.jpeg_idct(coef, quant)
            eng.profile_enable(True)
            eng.profile_read(reset=True)
            reps = 10
            for _ in range(reps):
                for coef, quant in comps:
                    eng.jpeg_idct(coef, quant)
            ms, calls = eng.profile_read(reset=True).get("jpeg_decode", (0.0, 0))
            eng.profile_enable(False)
            samples = sum(int(c.shape[0]) * int(c.shape[1]) * 64 for c, _ in comps)
            stage_ms = ms / reps
            px = h * w
            res[mode]["jpeg_decode_stage"] = {
                "ms_per_tile": round(stage_ms, 4), "launches_per_tile_in_this_probe": len(comps), "samples": samples,
                "compulsory_MB": round(3 * samples / 1e6, 2),
                "GBps_of_compulsory": round(3 * samples / stage_ms / 1e6, 1) if stage_ms > 0 else None,
                "fraction_of_hbm": round(3 * samples / stage_ms / 1e6 / HBM_GBPS, 3) if stage_ms > 0 else None,
                "bound": "memory: 2 B in + 1 B out per sample against about 110 integer operations; the figure is event time around launches "
                         "of 12 and 3 MB, so launch latency weighs on it"}
            res[mode]["jpeg_entropy"] = entropy_probe(eng, files[mode])
            res[mode]["link_bytes_per_pixel"] = {"host": 1.5 if color else 1.0, "device": round((2 * samples + 128 * len(comps)) / px, 3),
                                                 "device-entropy": round(res[mode]["jpeg_entropy"]["record_bytes_per_file"] / px, 3)}
            if args.sweep:
                listing = os.path.join(outdir, mode + "_files.txt")
                with open(listing, "w") as fh:
                    fh.write("\n".join(files[mode]) + "\n")
                res[mode]["jpeg_entropy_sweep"] = {}
                for item in args.sweep.split(","):
                    bits, lib = item.split("=", 1)
                    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--probe", listing], env=dict(os.environ, VFSMS_LIB=lib),
                                         capture_output=True, text=True, timeout=600)
                    assert out.returncode == 0, out.stderr
                    res[mode]["jpeg_entropy_sweep"][bits] = json.loads(out.stdout.strip().splitlines()[-1])
                    assert res[mode]["jpeg_entropy_sweep"][bits]["sub_bits"] == int(bits)
    finally:
        for k, v in old.items():
            setattr(isa.Stitcher, k, v)
        eng.close()
        if args.dir is None:
            shutil.rmtree(outdir, ignore_errors=True)
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
