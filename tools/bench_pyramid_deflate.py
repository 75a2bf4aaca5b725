"""Lossless pyramidal output with deflate tiles coded on the device (Method.pyramidCompression = "deflate-device") against the "none" and
"deflate" host writers and the lossy "jpeg" tiles, on the headline mosaic, gray and colour, in one process.

The grid of bench.py (10 x 9 tiles of 2048 x 2048, 10 % overlap) is synthesised, uploaded and fused (fade) into a canvas that stays in HBM.
Per mode (gray, B G R) the script times the streamed write-out of that canvas, from the first band request to the closed file, alternated
A B C D A B C D after warm-up:
  A  Engine.canvas_download_pyramid_bands         -> PyramidTiffBandWriter(compression="none")
  B  the same bands                               -> PyramidTiffBandWriter(compression="deflate")
  C  Engine.canvas_encode_pyramid_tiles_deflate   -> PyramidTiffBandWriter(compression="deflate-device").tiles
  D  Engine.canvas_encode_pyramid_tiles           -> PyramidTiffBandWriter(compression="jpeg").tiles
All legs write to the same directory (--dir, default: a temporary one) and remove the file again.  Recorded beside the times: the file
sizes, the bytes that crossed the link (pixels of the band and its levels for A and B, tile streams and index for C and D), and the stage
split of leg C by the library's event profiler (pyramid_deflate.levels, deflate.symbols / .codes / .write / .copy; bands without a writer)
with the time the generator took for those bands -- every stage beside the bytes it cannot avoid moving (the pixels of all levels for the
symbol pass, which reads them once; the predicted bytes for the write pass; the payload for the copy) and the rate that makes.  The mosaic is
synthetic: its compression ratio says nothing about micrographs (tests/test_deflate_host.py measures the coder on real strips).
Writes profiles/pyramid_deflate_bench.json and prints the same JSON line.

    python tools/bench_pyramid_deflate.py [--rows 10 --cols 9 --tile 2048 --steps 3 --warmup 1 --band-rows 4096]
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

STAGES = ("pyramid_deflate.levels", "deflate.symbols", "deflate.codes", "deflate.write", "deflate.copy")
LEGS = ("none", "deflate", "deflate-device", "jpeg")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=10)
    ap.add_argument("--cols", type=int, default=9)
    ap.add_argument("--tile", type=int, default=2048)
    ap.add_argument("--overlap", type=float, default=0.10)
    ap.add_argument("--band-rows", type=int, default=4096)
    ap.add_argument("--pyramid-tile", type=int, default=512)
    ap.add_argument("--quality", type=int, default=95)
    ap.add_argument("--restart-mcus", type=int, default=8)
    ap.add_argument("--steps", type=int, default=3, help="timed repetitions per leg (at least 2)")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--dir", default=None, help="where the files are written (default: a temporary directory)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pyramid_deflate_bench.json"))
    args = ap.parse_args()
    args.steps = max(args.steps, 2)

    import numpy as np
    import imagestitch_amd as isa
    from imagestitch_amd.io import default_levels
    from imagestitch_amd.synthetic import SyntheticGrid

    grid = SyntheticGrid(args.rows, args.cols, args.tile, overlap=args.overlap)
    gray = grid.tiles(threads=min(16, len(os.sched_getaffinity(0))))
    n = grid.n_tiles
    offs = [[0, 0]] + [list(map(int, o)) for o in grid.true_offsets()]
    shapes = [(grid.th, grid.tw)] * n
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, offs)
    geom = isa.Stitcher._placements(shapes, offs, offsetList, rangeX, rangeY, isa.Engine.CANVAS_MODES["fadeInAndFadeOut"])
    eng = isa.Engine(0)
    outdir = args.dir or tempfile.mkdtemp(prefix="vfsms_pyramid_deflate_")
    os.makedirs(outdir, exist_ok=True)
    T, Q, R = args.pyramid_tile, args.quality, args.restart_mcus
    levels = default_levels(rows, cols, T)

    def stats(v):
        v = np.array(v)
        return {"ms_median": round(float(np.median(v)), 1), "ms_min": round(float(v.min()), 1), "ms_max": round(float(v.max()), 1)}

    res = {"metric": "streamed write-out of the headline mosaic as tiled pyramidal TIFF: tiles raw (none), zlib on the host (deflate), "
                     "deflate coded on the device (deflate-device), JPEG encoded on the device (jpeg)",
           "grid": [args.rows, args.cols, args.tile], "mosaic": [rows, cols], "band_rows": args.band_rows, "pyramid_tile": T, "levels": levels,
           "quality": Q, "restart_mcus": R, "steps": args.steps, "warmup": args.warmup, "content": "synthetic"}
    try:
        for mode, ch in (("gray", 1), ("color", 3)):
            handles = [eng.tile_upload(t) if ch == 1 else eng.tile_upload_color(np.stack([t, 255 - t, t // 2 + 64], -1)) for t in gray]
            canvas = eng.canvas_create(rows, cols, ch)
            eng.canvas_assemble_resident(canvas, handles, geom)
            eng.sync()
            full = (rows, cols, ch) if ch > 1 else (rows, cols)

            def leg_pixels(compression):
                path = os.path.join(outdir, compression + ".tif")
                w = isa.PyramidTiffBandWriter(path, tile=T, compression=compression)
                link = 0
                t0 = time.perf_counter()
                for r0, band, lv in eng.canvas_download_pyramid_bands(canvas, rows, cols, ch, levels, args.band_rows, transient=True):
                    link += band.nbytes + sum(x.nbytes for x in lv)
                    w(r0, band, full, levels=lv)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size, link

            def bands(compression):
                if compression == "jpeg":
                    return eng.canvas_encode_pyramid_tiles(canvas, rows, cols, ch, levels, T, Q, R, args.band_rows)
                return eng.canvas_encode_pyramid_tiles_deflate(canvas, rows, cols, ch, levels, T, args.band_rows)

            def leg_tiles(compression):
                path = os.path.join(outdir, compression + ".tif")
                w = isa.PyramidTiffBandWriter(path, tile=T, compression=compression, quality=Q, restart_mcus=R)
                link = 0
                t0 = time.perf_counter()
                for r0, nr, payload, index in bands(compression):
                    link += payload.nbytes + index.nbytes
                    w.tiles(r0, nr, payload, index, full)
                ms = (time.perf_counter() - t0) * 1e3
                size = os.path.getsize(path)
                os.remove(path)
                return ms, size, link

            def staged():
                """the bands of leg C without a writer, profiler on -> (generator ms, stage ms by name, payload bytes)"""
                eng.profile_enable(True)
                eng.profile_read(reset=True)
                t0 = time.perf_counter()
                nbytes = sum(p.nbytes for _r0, _n, p, _i in bands("deflate-device"))
                ms = (time.perf_counter() - t0) * 1e3
                prof = eng.profile_read(reset=True)
                eng.profile_enable(False)
                return round(ms, 1), {s_.split(".")[1]: round(prof.get(s_, (0.0, 0))[0], 3) for s_ in STAGES}, nbytes

            legs = {name: [] for name in LEGS}
            sizes, link = {}, {}
            for k in range(args.warmup + args.steps):
                for name in LEGS:
                    ms, sizes[name], link[name] = leg_tiles(name) if name in ("deflate-device", "jpeg") else leg_pixels(name)
                    if k >= args.warmup:
                        legs[name].append(ms)
            r = {"mosaic_MB": round(rows * cols * ch / 1e6, 1)}
            for name in legs:
                r[name] = dict(stats(legs[name]), file_MB=round(sizes[name] / 1e6, 1), link_MB=round(link[name] / 1e6, 1))
            med = {name: float(np.median(legs[name])) for name in legs}
            r["deflate_device_over_none"] = round(med["deflate-device"] / med["none"], 3)
            r["deflate_device_over_deflate"] = round(med["deflate-device"] / med["deflate"], 3)
            r["deflate_device_over_jpeg"] = round(med["deflate-device"] / med["jpeg"], 3)
            r["deflate_device_file_over_deflate_file"] = round(sizes["deflate-device"] / sizes["deflate"], 3)
            staged()                                               # (the ring and the scratch at their final sizes)
            ms, split, nb = staged()
            # what every stage cannot avoid moving: the pixels of all levels, tile padding included, are read once by the symbol pass and
            # once more, as predicted bytes, by the write pass, which stores the payload; the copy carries the payload over the link
            padded, rr, cc = 0, rows, cols
            for _k in range(levels + 1):
                padded += -(-rr // T) * -(-cc // T) * T * T * ch
                rr, cc = (rr + 1) >> 1, (cc + 1) >> 1
            must = {"levels": rows * cols * ch, "symbols": padded, "codes": 0, "write": padded + nb, "copy": nb}
            r["deflate_device_stages"] = dict(
                {name: {"ms": split[name], "compulsory_MB": round(must[name] / 1e6, 1),
                        "GB_per_s": round(must[name] / 1e6 / split[name], 1) if split[name] > 0 and must[name] else None} for name in split},
                generator_ms=ms, device_ms=round(sum(split.values()), 3), payload_MB=round(nb / 1e6, 1))
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
