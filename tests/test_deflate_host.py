"""CPU tests of lossless pyramidal TIFF with tiles coded on the device (Method.pyramidCompression = "deflate-device"): the specification
tests/deflate_ref.py against zlib's inflate and a plain heapq Huffman; csrc/deflate_core.h -- the lines the kernels compile -- through
tools/deflate_core_host_check.cpp under the host sanitizers; PyramidTiffBandWriter fed the specification's streams and read back by the
parser of tests/test_tiff_jpeg_host.py and by Pillow (libtiff), page by page against tests/pyramid_ref.py and against the file the "deflate"
host writer makes of the same bands; and the Stitcher's wiring through a fake engine.  All comparisons are of bytes."""
import heapq
import os
import struct
import subprocess
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_ref as ref                 # noqa: E402
import pyramid_ref as PR                  # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from test_pyramid_host import PyramidOracleEngine, _Project, read_tiff, stream as stream_pixels      # noqa: E402
from test_tiff_jpeg_host import TileOracleEngine, _image, parse_tiff                                 # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO_RUNS = (1, 2, 3, 4, 5, 259, 260, 261, 262, 517, 518, 519, 520, 4096)


def _strips():
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_full_strips.npz"))
    return [z[k] for k in z.files]


def depth_limit_tile():
    """a 112 x 112 gray tile whose predicted bytes have the counts 1, 3, 5, 9, 15, ... (a_n = a_(n-1) + a_(n-2) + 1: with the end-of-block
    symbol's 1 every merge of the two-queue construction deepens the same branch) plus fillers no smaller than the largest of them, no two
    equal bytes adjacent: -> (the image, the running sum of those bytes along each row; the predicted bytes)"""
    N = 112 * 112
    counts = [1, 3]
    while sum(counts) + counts[-1] + counts[-2] + 1 <= N // 2:
        counts.append(counts[-1] + counts[-2] + 1)
    left = N - sum(counts)
    n_fill = left // counts[-1]
    assert n_fill >= 1 and len(counts) + n_fill <= 256
    fill = [left // n_fill + (1 if j < left % n_fill else 0) for j in range(n_fill)]
    assert min(fill) >= counts[-1] and max(fill) <= N // 2
    counts = counts + fill
    order = sorted(range(len(counts)), key=lambda s: -counts[s])
    seq = np.repeat(np.array(order, np.uint8), [counts[s] for s in order])
    pred = np.empty(N, np.uint8)                                 # the commonest values on the even places first, then the odd ones
    pred[0::2] = seq[:(N + 1) // 2]
    pred[1::2] = seq[(N + 1) // 2:]
    assert (pred[1:] != pred[:-1]).all()
    img = np.cumsum(pred.reshape(112, 112).astype(np.uint32), 1).astype(np.uint8)
    assert np.array_equal(ref.predict(img).reshape(-1), pred)
    return img, pred


def _cases():
    """name -> the (predicted) bytes of a tile"""
    rng = np.random.default_rng(11)
    out = {"one": b"\x07", "two": b"\x07\x09", "two_equal": b"\x07\x07"}
    for n in ZERO_RUNS:
        out["zeros_%d" % n] = bytes(n)
    out["noise"] = rng.integers(0, 256, 20000, dtype=np.uint8).tobytes()
    out["ramp"] = (np.arange(30000) // 7).astype(np.uint8).tobytes()
    out["runs"] = np.repeat(rng.integers(0, 5, 400), rng.integers(1, 700, 400)).astype(np.uint8).tobytes()
    for k, s in enumerate(_strips()):
        out["strip_%d" % k] = ref.predict(s[:256, :256]).tobytes()
    out["depth_limit"] = depth_limit_tile()[1].tobytes()
    return out


CASES = _cases()


# ---- 1. the specification -------------------------------------------------------------------------------------------------------------
def test_reference_streams_are_zlib_streams():
    for name, x in CASES.items():
        s = ref.encode(x)
        assert s[:2] == b"\x78\x01" and zlib.decompress(s) == x, name
        d = zlib.decompressobj()
        assert d.decompress(s) == x and d.eof and not d.unused_data, name       # one stream, one final block, nothing behind it


def test_the_position_local_rule_is_the_sequential_parse():
    rng = np.random.default_rng(2)
    for n in (1, 2, 3, 4, 5, 259, 260, 261, 262, 517, 518, 519, 520):
        for x in (bytes(n), b"\x01" + bytes(n), bytes(n) + b"\x01", b"\x05" * 3 + bytes(n) + b"\x05" * 4):
            assert ref.tokens_local(x) == ref.tokens(x), n
    assert ref.tokens(bytes(262)) == [("lit", 0), ("match", 258), ("match", 3)]
    assert ref.tokens(bytes(261)) == [("lit", 0), ("match", 258), ("lit", 0), ("lit", 0)]
    assert ref.tokens(bytes(3)) == [("lit", 0)] * 3 and ref.tokens(bytes(4)) == [("lit", 0), ("match", 3)]
    for k in range(300):
        n = int(rng.integers(1, 1500))
        if k % 2:
            x = rng.integers(0, 3, n, dtype=np.uint8).tobytes()
        else:
            x = np.repeat(rng.integers(0, 256, 12), rng.integers(1, 600, 12)).astype(np.uint8).tobytes()
        assert ref.tokens_local(x) == ref.tokens(x)
    for L in range(3, 259):
        s, eb, ev = ref.length_symbol(L)
        assert 257 <= s <= 285 and ref.LEN_BASE[s - 257] + ev == L and 0 <= ev < (1 << eb) + (eb == 0) and eb == ref.LEN_EXTRA[s - 257]


def _heapq_bits(counts):
    """the total bits of an optimal prefix code, by a plain heap"""
    heap = [c for c in counts if c]
    heapq.heapify(heap)
    total = 0
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        total += a + b
        heapq.heappush(heap, a + b)
    return total


def test_code_lengths_are_complete_optimal_and_at_most_15_bits():
    rng = np.random.default_rng(4)
    hists = [ref.histogram(ref.tokens(x)) for x in CASES.values()]
    for k in range(200):
        h = np.zeros(ref.N_SYMS, np.int64)
        used = rng.choice(ref.N_SYMS, int(rng.integers(2, ref.N_SYMS + 1)), replace=False)
        h[used] = rng.integers(1, [4, 100, 100000][k % 3], len(used))
        h[ref.END] = 1
        hists.append([int(v) for v in h])
    hists.append([1] * ref.N_SYMS)
    hists.append([1 if s in (7, ref.END) else 0 for s in range(ref.N_SYMS)])
    limited = 0
    for h in hists:
        lens, halvings = ref.code_lengths(h)
        assert all((k > 0) == (c > 0) for k, c in zip(lens, h))
        assert max(lens) <= ref.MAX_BITS
        assert sum(1 << (ref.MAX_BITS - k) for k in lens if k) == 1 << ref.MAX_BITS          # Kraft: exactly 1
        if ref.unlimited_depth(h) <= ref.MAX_BITS:
            assert halvings == 0 and sum(c * k for c, k in zip(h, lens)) == _heapq_bits(h)
        else:
            limited += 1
            assert halvings >= 1
        codes = ref.canonical_codes(lens)
        assert len({(k, c) for k, c in zip(lens, codes) if k}) == sum(1 for k in lens if k)
    assert limited >= 1
    assert ref.code_lengths([5 if s == 9 else 0 for s in range(ref.N_SYMS)])[0][9] == 1       # one symbol alone: one bit


def test_the_depth_limit_is_hit():
    img, pred = depth_limit_tile()
    toks = ref.tokens(pred.tobytes())
    assert all(kind == "lit" for kind, _v in toks) and len(toks) == 112 * 112               # no matches
    h = ref.histogram(toks)
    assert ref.unlimited_depth(h) == 16
    lens, halvings = ref.code_lengths(h)
    assert halvings >= 1 and max(lens) <= 15 and sum(1 << (15 - k) for k in lens if k) == 1 << 15
    s = ref.tile_streams(img, 112, bgr=False)
    assert len(s) == 1 and s[0] == ref.encode(pred.tobytes()) and zlib.decompress(s[0]) == pred.tobytes()


def test_tiles_are_padded_with_zeros_then_predicted():
    img = _image((37, 50, 3), 5)
    streams = ref.tile_streams(img, 32, bgr=True)
    assert len(streams) == 4
    for t, s in enumerate(streams):
        ty, tx = divmod(t, 2)
        tile = np.zeros((32, 32, 3), np.uint8)
        part = img[ty * 32:(ty + 1) * 32, tx * 32:(tx + 1) * 32, ::-1]
        tile[:part.shape[0], :part.shape[1]] = part
        d = np.frombuffer(zlib.decompress(s), np.uint8).reshape(32, 32, 3)
        assert np.array_equal(np.cumsum(d.astype(np.uint32), 1).astype(np.uint8), tile)      # what libtiff undoes
    assert ref.tile_streams(img[:, :, ::-1], 32, bgr=False) == streams
    for T, ch in ((0, 3), (24, 3), (-16, 1), (32, 2)):
        with pytest.raises(ValueError):
            ref.check_geometry(T, ch)


def test_real_pixels_compress_better_than_the_host_writer_they_replace():
    raw = coded = host = 0
    for s in _strips():
        for y in range(0, s.shape[0] - 255, 256):
            for x in range(0, s.shape[1] - 255, 256):
                tile = np.ascontiguousarray(s[y:y + 256, x:x + 256])
                raw += tile.size
                coded += len(ref.encode(ref.predict(tile).tobytes()))
                host += len(zlib.compress(tile.tobytes(), 1))
    print("real strips, %d tiles of 256 x 256: reference %.4f of the raw bytes, zlib level 1 without predictor %.4f" % (raw // 65536, coded / raw, host / raw))
    assert raw // 65536 == 2 * 10 + 2 * 14
    assert coded / raw < host / raw


# ---- 2. csrc/deflate_core.h under the host sanitizers ---------------------------------------------------------------------------------------
def test_the_core_the_kernels_compile_equals_the_reference(tmp_path):
    src = os.path.join(ROOT, "tools", "deflate_core_host_check.cpp")
    exe = str(tmp_path / "deflate_core_host_check")
    cmd = [os.environ.get("CXX", "c++"), "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan",
           "-static-libubsan", "-I", os.path.join(ROOT, "imagestitch_amd", "csrc"), src, "-o", exe]
    subprocess.run(cmd, check=True, cwd=ROOT, timeout=300)
    args = []
    for name, x in CASES.items():
        with open(str(tmp_path / (name + ".in")), "wb") as f:
            f.write(x)
        args += [str(tmp_path / (name + ".in")), str(tmp_path / (name + ".out"))]
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert not p.stderr.strip(), p.stderr                      # the sanitizers, leak detection included, report nothing
    assert "deflate_core_host_check: %d cases ok" % len(CASES) in p.stdout
    limited = 0
    for name, x in CASES.items():
        o = open(str(tmp_path / (name + ".out")), "rb").read()
        n = struct.unpack_from("<I", o)[0]
        toks = list(struct.unpack_from("<%di" % n, o, 4))
        at = 4 + 4 * n
        lens = list(o[at:at + ref.N_SYMS])
        halvings, unlimited, m = struct.unpack_from("<3I", o, at + ref.N_SYMS)
        stream = o[at + ref.N_SYMS + 12:]
        assert len(stream) == m, name
        want = ref.tokens(x)
        assert toks == [v if kind == "lit" else 256 + v for kind, v in want], name
        h = ref.histogram(want)
        assert (lens, halvings) == ref.code_lengths(h) and unlimited == ref.unlimited_depth(h), name
        assert stream == ref.encode(x), name
        limited += halvings > 0
    assert limited >= 1                                         # the depth-limit tile took the halving path in the header's code too


# ---- 3. the writer --------------------------------------------------------------------------------------------------------------------------
def decode_tile(raw, T, ch):
    d = np.frombuffer(zlib.decompress(raw), np.uint8).reshape(T, T, ch)
    return np.cumsum(d.astype(np.uint32), 1).astype(np.uint8)


def check_file(path, img, levels, T, big=None):
    """the tags and every tile's bytes are the specification's; every page is pyramid_ref's level with the zero padding -> the padded pages"""
    ch = 1 if img.ndim == 2 else 3
    want = ref.file_tiles(img, levels, T)
    lvls = [img] + PR.pyramid_levels(img, levels)
    pages = parse_tiff(path)
    assert len(pages) == levels + 1
    out = []
    for k, pg in enumerate(pages):
        t = pg["tags"]
        h, w = lvls[k].shape[:2]
        assert t[254] == [1 if k else 0] and (t[257][0], t[256][0]) == (h, w) and t[258] == [8] * ch and t[277] == [ch] and t[284] == [1]
        assert t[259] == [8] and t[317] == [2] and t[262] == [2 if ch == 3 else 1] and t[322] == t[323] == [T]
        assert 347 not in t and 530 not in t                    # no JPEGTables, no YCbCr tags
        assert pg["tiles"] == want[k], ("level", k)
        nty, ntx = -(-h // T), -(-w // T)
        padded = np.zeros((nty * T, ntx * T, ch), np.uint8)
        for n, raw in enumerate(pg["tiles"]):
            ty, tx = divmod(n, ntx)
            padded[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = decode_tile(raw, T, ch)
        lv = lvls[k].reshape(h, w, ch)
        assert np.array_equal(padded[:h, :w], lv[:, :, ::-1])
        rest = padded.copy(); rest[:h, :w] = 0
        assert not rest.any(), "edge tiles are padded with zeros"
        if big is not None:
            assert pg["big"] == big
        out.append(padded)
    return out


def check_pillow_reads(path, img, levels):
    from PIL import Image
    lvls = [img] + PR.pyramid_levels(img, levels)
    im = Image.open(path)
    assert im.n_frames == levels + 1
    for k, lv in enumerate(lvls):
        im.seek(k)
        assert im.size == (lv.shape[1], lv.shape[0])
        assert np.array_equal(np.asarray(im), lv[:, :, ::-1] if lv.ndim == 3 else lv), ("page", k)


def stream(writer, img, levels, T, band_rows=64):
    """the bands of `img` as Engine.canvas_encode_pyramid_tiles_deflate hands them over, computed by the specification"""
    rows, cols = img.shape[:2]
    want = ref.file_tiles(img, levels, T)
    for r0 in range(0, rows, band_rows):
        n = min(band_rows, rows - r0)
        payload, index = b"", []
        for k, t in isa.Engine.pyramid_tiles_index(rows, cols, levels, T, r0, n):
            index.append((k, t, len(payload), len(want[k][t])))
            payload += want[k][t]
        writer.tiles(r0, n, np.frombuffer(payload, np.uint8), np.array(index, np.int64).reshape(-1, 4), img.shape)


@pytest.mark.parametrize("shape", [(37, 50), (150, 200), (150, 200, 3)])
def test_writer_files_hold_the_specifications_tiles(tmp_path, shape):
    img = _image(shape, 7)
    for T, levels, band in ((32, 3, 32), (32, 3, 64), (16, 2, 64)):
        for mode, kw in (("classic", {}), ("big", {"force_big": True})):
            path = str(tmp_path / ("p_%d_%d_%s.tif" % (T, band, mode)))
            w = isa.PyramidTiffBandWriter(path, tile=T, levels=levels, compression="deflate-device", **kw)
            assert w.device_tiles and w.tile_codec == "deflate" and w.pyramid_levels(shape) == levels
            stream(w, img, levels, T, band)
            pages = check_file(path, img, levels, T, big=(mode == "big"))
            assert not [n for n in os.listdir(str(tmp_path)) if n.startswith(".")]
            check_pillow_reads(path, img, levels)
            # the file the "deflate" host writer makes from the same bands holds the same pages, padding included
            host = str(tmp_path / ("h_%d_%d_%s.tif" % (T, band, mode)))
            stream_pixels(isa.PyramidTiffBandWriter(host, tile=T, levels=levels, compression="deflate", **kw), img, levels, band)
            theirs = read_tiff(host)
            assert len(theirs) == len(pages)
            for mine, pg in zip(pages, theirs):
                assert pg["tags"][259] == (8,) and 317 not in pg["tags"] and np.array_equal(mine, pg["padded"])


def test_writer_refusals_and_the_writers_that_stay(tmp_path):
    img = _image((100, 70, 3), 2)
    path = str(tmp_path / "sub" / "r.tif")
    host = isa.PyramidTiffBandWriter("x.tif", compression="deflate")
    assert not host.device_tiles and host.tile_codec is None and not isa.PyramidTiffBandWriter("x.tif").device_tiles
    assert isa.PyramidTiffBandWriter("x.tif", compression="jpeg").tile_codec == "jpeg"
    for kw in (dict(tile=24), dict(tile=0), dict(levels=11)):
        with pytest.raises(ValueError):
            isa.PyramidTiffBandWriter(path, compression="deflate-device", **kw)
    isa.PyramidTiffBandWriter(path, compression="deflate-device", tile=32, quality=0, restart_mcus=3)      # quality and restart_mcus play no part
    with pytest.raises(ValueError):
        isa.PyramidTiffBandWriter(path, compression="deflate_device")
    with pytest.raises(ValueError) as e:                        # pixel bands: there is no host encoder behind "deflate-device"
        isa.PyramidTiffBandWriter(path, tile=32, levels=0, compression="deflate-device")(0, img[:20, :30], (20, 30, 3), levels=[])
    assert "deflate-device" in str(e.value)
    with pytest.raises(ValueError):                              # tile streams to the host deflate writer
        isa.PyramidTiffBandWriter(path, tile=32, levels=0, compression="deflate").tiles(0, 20, np.zeros(4, np.uint8), np.array([[0, 0, 0, 4]]), (20, 30, 3))
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="deflate-device")
    with pytest.raises(ValueError):                              # bands out of order
        w.tiles(64, 36, np.zeros(4, np.uint8), np.array([[0, 0, 0, 4]]), img.shape)
    assert not os.path.exists(str(tmp_path / "sub")) or os.listdir(str(tmp_path / "sub")) == []
    with pytest.raises(ValueError):                              # four channels
        isa.PyramidTiffBandWriter(path, tile=32, levels=0, compression="deflate-device").tiles(0, 20, np.zeros(4, np.uint8), np.array([[0, 0, 0, 4]]), (20, 30, 4))


# ---- 4. the Stitcher --------------------------------------------------------------------------------------------------------------------
class DeflateOracleEngine(TileOracleEngine):
    """TileOracleEngine plus canvas_encode_pyramid_tiles_deflate: the payloads of every band computed by the specification"""

    deflate_calls = 0

    def canvas_encode_pyramid_tiles_deflate(self, h, rows, cols, ch, levels, tile, band_rows):
        self.deflate_calls += 1
        if band_rows % tile or band_rows % (1 << levels):
            raise ValueError("band_rows")
        img = self.canvas_download(h, rows, cols, ch)
        want = ref.file_tiles(img, levels, tile)
        for r0 in range(0, rows, band_rows):
            n = min(band_rows, rows - r0)
            payload, index = b"", []
            for k, t in isa.Engine.pyramid_tiles_index(rows, cols, levels, tile, r0, n):
                index.append((k, t, len(payload), len(want[k][t])))
                payload += want[k][t]
            yield r0, n, np.frombuffer(payload, np.uint8), np.array(index, np.int64).reshape(-1, 4)


def test_method_defaults_stay():
    m = isa.Method
    assert (m.outputPyramid, m.pyramidTile, m.pyramidLevels, m.pyramidCompression, m.jpegQuality, m.jpegRestartMcus) == (False, 512, None, "none", 95, 8)
    assert isa.Stitcher()._pyramidOptions() == {"tile": 512, "levels": None, "compression": "none", "quality": 95, "restart_mcus": 8}
    assert set(isa.Stitcher._ROUTES) >= {"device_jpeg", "device_tiles", "pyramid_levels", "plain"}
    assert isa.Stitcher._ROUTES["device_tiles"] == "canvas_encode_pyramid_tiles"


def test_stitcher_writes_one_file_of_the_specifications_tiles(oracle, tmp_path):
    from PIL import Image
    P = _Project(tmp_path)
    eng0, plain = P.run(oracle, "plain", engine=DeflateOracleEngine)
    assert eng0.tile_calls == 0 and eng0.deflate_calls == 0 and eng0.pyramid_calls == 0
    mosaic = np.ascontiguousarray(np.asarray(Image.open(str(plain / "stitching_result_1.tif")))[:, :, ::-1])       # B G R, as the canvas held it
    assert mosaic.shape == (416, 476, 3)
    # jpegQuality and jpegRestartMcus play no part: values "jpeg" would refuse
    for tag, kw, K, T in (("pyr", {"pyramidTile": 32, "pyramidLevels": 3, "jpegRestartMcus": 3}, 3, 32), ("auto", {"pyramidTile": 64, "mosaicBandRows": 128, "jpegQuality": 0}, 3, 64),
                          ("one", {"mosaicBandRows": 4096}, 0, 512)):
        eng, out = P.run(oracle, tag, engine=DeflateOracleEngine, outputPyramid=True, pyramidCompression="deflate-device", **kw)
        assert eng.deflate_calls == 1 and eng.tile_calls == 0 and eng.pyramid_calls == 0
        assert os.listdir(str(out)) == ["stitching_result_1.tif"]
        check_file(str(out / "stitching_result_1.tif"), mosaic, K, T, big=False)
        check_pillow_reads(str(out / "stitching_result_1.tif"), mosaic, K)
    # "deflate" stays the host writer: pixel bands with their levels, no tile call
    eng, out = P.run(oracle, "host", engine=DeflateOracleEngine, outputPyramid=True, pyramidCompression="deflate", pyramidTile=32, pyramidLevels=3)
    assert eng.deflate_calls == 0 and eng.tile_calls == 0 and eng.pyramid_calls == 1
    assert all(317 not in pg["tags"] and pg["tags"][259] == (8,) for pg in read_tiff(str(out / "stitching_result_1.tif")))


def test_stitcher_refusals_come_before_any_decode(oracle, tmp_path):
    P = _Project(tmp_path)
    user_sink = lambda row0, band, full_shape: None
    said = {}
    for tag, exc, kw in (("eng", NotImplementedError, {"engine": TileOracleEngine}), ("sink", ValueError, {"mosaicSink": user_sink}),
                         ("band", ValueError, {"pyramidTile": 64, "mosaicBandRows": 32}), ("tile", ValueError, {"pyramidTile": 24}),
                         ("ext", ValueError, {"ext": "png"}), ("whole", ValueError, {"streamOutput": False}),
                         ("levels", ValueError, {"pyramidTile": 16, "pyramidLevels": 6, "mosaicBandRows": 32})):
        kw.setdefault("engine", DeflateOracleEngine)
        with pytest.raises(exc) as e:
            P.run(oracle, tag, outputPyramid=True, pyramidCompression="deflate-device", **kw)
        said[tag] = str(e.value)
        assert P.decodes == 0, tag
        assert not (tmp_path / tag).exists() or not os.listdir(str(tmp_path / tag)), tag
    assert "canvas_encode_pyramid_tiles_deflate" in said["eng"]
    # the text "jpeg" gets, with this value in it
    with pytest.raises(ValueError) as e:
        P.run(oracle, "sinkj", engine=DeflateOracleEngine, outputPyramid=True, pyramidCompression="jpeg", pyramidTile=32, jpegRestartMcus=2, mosaicSink=user_sink)
    assert said["sink"] == str(e.value).replace("'jpeg'", "'deflate-device'")
