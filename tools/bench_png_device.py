"""PNG results coded on the device (Method.pngEncoder = "device") against the host writer, on the headline mosaic, gray and colour, in one
process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised, uploaded and fused (fade) into a canvas that stays in HBM.
Per mode (gray, B G R) the script times the streamed write-out of that canvas, from the first band request to the closed file, alternated
A B A B after warm-up:
  A  Engine.canvas_download_bands     -> PngBandWriter (filter 0, ONE zlib stream at level 1 on one host thread)
  B  Engine.canvas_encode_png_bands   -> DevicePngFile (adaptive filters, segments coded and checksummed on the device; the host appends)
Both legs write to the same directory (--dir, default: a temporary one) and remove the file again.  Recorded beside the times: the file
sizes, the bytes that crossed the link, the stage split of leg B by the library's event profiler (png.choose / .filter / .symbols / .codes /
.write / .crc / .copy; bands without a file) with the time the generator took for those bands -- every stage beside the bytes it cannot avoid
moving and the rate that makes -- and a sweep of pngSegmentRows over {1, 4, 16, 64, 256}: time of leg B and file size.  The mosaic is
synthetic: its compression ratio says nothing about micrographs (tests/test_png_device_host.py measures the coder on real strips).
Writes profiles/png_device_bench.json and prints the same JSON line.

    python tools/bench_png_device.py [--rows 10 --cols 9 --tile 2048 --steps 2 --warmup 1 --band-rows 4096 --segment-rows 16]
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGES = ("png.choose", "png.filter", "png.symbols", "png.codes", "png.write", "png.crc", "png.copy")
SWEEP = (1, 4, 16, 64, 256)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--band-rows", type=int, default=4096)
    ap.add_argument("--segment-rows", type=int, default=16)
    ap.add_argument("--steps", type=int, default=2, help="timed repetitions per leg (at least 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--no-sweep", action="store_true")
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "png_device_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 2)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid

    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    gray = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    n = grid.n_tiles
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    shapes = [(grid.th, grid.tw)] * n
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    geom = isa.Stitcher._placements(shapes, offs, offsetList, rangeX, rangeY, isa.Engine.CANVAS_MODES["fadeInAndFadeOut"])
    eng = isa.Engine(0)
    outdir = args.dir or tempfile.mkdtemp(prefix="vfsms_png_device_")
    os.makedirs(outdir, exist_ok=True)
    S0 = args.segment_rows

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 1), "ms_min": round(float(v.min()), 1), "ms_max": round(float(v.max()), 1)}

    res = {"metric": "streamed write-out of the headline mosaic as one PNG: filter 0 and one zlib stream at level 1 on the host (host), "
                     "adaptive filters and segments coded on the device (device)",
           "grid": [args.rows, args.cols, args.tile], "mosaic": [rows, cols], "band_rows": args.band_rows, "segment_rows": S0,
           "steps": args.steps, "warmup": args.warmup, "content": "synthetic"}
    try:
        for mode, ch in (("gray", 1), ("color", 3)):
            handles = [eng.tile_upload(t) if ch == 1 else eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in gray]
            canvas = eng.canvas_create(rows, cols, ch)
            eng.canvas_assemble_resident(canvas, handles, geom)
            eng.sync()
            full = (rows, cols, ch) if ch > 1 else (rows, cols)
            rowbytes = 1 + cols * ch

            def leg_host():
                path = os.path.join(outdir, "host.png")
                w = isa.PngBandWriter(path)
                link = 0
                t0 = time.perf_counter()
                for r0, band in eng.canvas_download_bands(canvas, rows, cols, ch, args.band_rows, transient=True):
                    link += band.nbytes
                    w(r0, band, full)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size, link

            def leg_device(S=S0):
                path = os.path.join(outdir, "device.png")
                band_rows = max(S, args.band_rows // S * S)
                link = 0
                t0 = time.perf_counter()
                w = isa.DevicePngFile(path, full, S)
                for _r0, nr, payload, adler in eng.canvas_encode_png_bands(canvas, rows, cols, ch, S, band_rows):
                    link += payload.nbytes + 4
                    w.append(payload, adler, nr * rowbytes)
                w.close()
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size, link

            def staged():
                """the bands of leg B without a file, profiler on -> (generator ms, stage ms by name, payload bytes)"""
                eng.profile_enable(True)
                eng.profile_read(reset=True)
                t0 = time.perf_counter()
                nbytes = sum(p.nbytes for _r0, _n, p, _a in eng.canvas_encode_png_bands(canvas, rows, cols, ch, S0, max(S0, args.band_rows // S0 * S0)))
                ms = (time.perf_counter() - t0) * 1e3
                prof = eng.profile_read(reset=True)
                eng.profile_enable(False)
                return round(ms, 1), {s_.split(".")[1]: round(prof.get(s_, (0.0, 0))[0], 3) for s_ in STAGES}, nbytes

            legs = {"host": [], "device": []}
            sizes, link = {}, {}
            for k in range(args.warmup + args.steps):
                for name, leg in (("host", leg_host), ("device", leg_device)):
                    ms, sizes[name], link[name] = leg()
                    print("%s %s: %.1f ms, %.1f MB" % (mode, name, ms, sizes[name] / 1e6), file=sys.stderr, flush=True)
                    if k >= args.warmup:
                        legs[name].append(ms)
            pixels = rows * cols * ch
            r = {"mosaic_MB": round(pixels / 1e6, 1)}
            for name in legs:
                r[name] = dict(stats(legs[name]), file_MB=round(sizes[name] / 1e6, 1), link_MB=round(link[name] / 1e6, 1), file_over_raw=round(sizes[name] / pixels, 4))
            r["device_over_host"] = round(float(np.median(legs["device"])) / float(np.median(legs["host"])), 4)
            r["device_file_over_host_file"] = round(sizes["device"] / sizes["host"], 3)
            staged()                                               # (the ring and the scratch at their final sizes)
            ms, split, nb = staged()
            # what every stage cannot avoid moving: the pixels are read once by the filter choice and once more by the filter pass, which
            # stores the filtered bytes; the symbol pass reads those once, the write pass once more and stores the payload; the CRC reads the
            # payload and the copy carries it over the link
            filtered = rows * rowbytes
            must = {"choose": pixels, "filter": pixels + filtered, "symbols": filtered, "codes": 0, "write": filtered + nb, "crc": nb, "copy": nb}
            r["device_stages"] = dict(
                {name: {"ms": split[name], "compulsory_MB": round(must[name] / 1e6, 1),
                        "GB_per_s": round(must[name] / 1e6 / split[name], 1) if split[name] > 0 and must[name] else None} for name in split},
                generator_ms=ms, device_ms=round(sum(split.values()), 3), payload_MB=round(nb / 1e6, 1))
            if not args.no_sweep:
                sweep = {}
                for S in SWEEP:
                    leg_device(S)
                    runs = [leg_device(S) for _ in range(2)]
                    sweep[str(S)] = {"ms_min": round(min(x[0] for x in runs), 1), "file_MB": round(runs[0][1] / 1e6, 2), "file_over_raw": round(runs[0][1] / pixels, 4)}
                r["segment_rows_sweep"] = sweep
            res[mode] = r
            eng.canvas_free(canvas)
            for h in handles:
                eng.tile_free(h)
    finally:
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
