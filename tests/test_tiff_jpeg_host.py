"""CPU tests of JPEG-compressed pyramidal TIFF (Method.pyramidCompression = "jpeg"): the specification tests/tiff_jpeg_ref.py against
tests/jpeg_enc_ref.py's complete files and Pillow's decoder, the library's JPEGTables, PyramidTiffBandWriter fed the specification's payloads
and read back by a parser written here and by Pillow (libtiff), and the Stitcher's wiring through a fake engine."""
import io
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as jref               # noqa: E402
import pyramid_ref as PR                  # noqa: E402
import tiff_jpeg_ref as ref               # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402
from fakes import IngestOracleEngine      # noqa: E402
from test_pyramid_host import PyramidOracleEngine, _Project      # noqa: E402


def _pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def _image(shape, seed):
    rng = np.random.default_rng(seed)
    h, w = shape[:2]
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 8, (h, w))
    img = np.stack([base, 0.7 * base + 30, 255 - base], -1) if len(shape) == 3 else base
    return np.clip(img, 0, 255).astype(np.uint8)


# ---- 1. the specification -------------------------------------------------------------------------------------------------------------
def _from(data, marker):
    return data[data.index(bytes([0xFF, marker])):]


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "colour"])
@pytest.mark.parametrize("T", [16, 32, 64])
def test_rebuilt_tiles_are_the_encoders_files(T, ch):
    for h, w in ((1, 1), (17, 33), (100, 70)):
        level = _image((h, w, 3) if ch == 3 else (h, w), h + w + T)
        n_mcu = (T // (16 if ch == 3 else 8)) ** 2
        for R in (0, 1, 4):
            if n_mcu % (R or n_mcu):
                with pytest.raises(ValueError):
                    ref.level_tiles(level, T, 90, R)
                continue
            tb = ref.tables(ch, 90)
            streams = ref.level_tiles(level, T, 90, R)
            assert len(streams) == -(-h // T) * -(-w // T)
            for t, s in enumerate(streams):
                ty, tx = divmod(t, -(-w // T))
                tile = ref.tile_image(level, ty, tx, T)
                assert tile.shape[:2] == (T, T)
                hh, ww = min(T, h - ty * T), min(T, w - tx * T)
                assert np.array_equal(tile[:hh, :ww], level[ty * T:ty * T + hh, tx * T:tx * T + ww])
                assert (tile[hh:] == tile[hh - 1]).all() and (tile[:, ww:] == tile[:, ww - 1:ww]).all()          # the last row and column repeat
                whole = jref.encode(tile, 90, R)
                full = ref.rebuilt(tb, s)
                assert _from(full, 0xC0)[:len(_from(whole, 0xC0)) - len(_from(whole, 0xC4))] == _from(whole, 0xC0)[:len(_from(whole, 0xC0)) - len(_from(whole, 0xC4))]     # SOF0
                assert _from(full, 0xDD if R else 0xDA) == _from(whole, 0xDD if R else 0xDA)                    # [DRI,] SOS, the scan, EOI
                assert s[:2] == b"\xFF\xD8" and s[2:4] == b"\xFF\xC0" and s[-2:] == b"\xFF\xD9"
                assert b"\xFF\xDB" not in s[:41] and b"\xFF\xC4" not in s[:41] and b"\xFF\xE0" not in s[:41]    # no tables, no APP0
                assert np.array_equal(_pillow(full), _pillow(whole))
                assert s == ref.tile_stream(tile, 90, R)


def test_restart_numbering_starts_at_0_in_every_tile():
    level = _image((40, 70), 3)
    for s in ref.level_tiles(level, 32, 90, 1):                 # 16 intervals a tile: RST0 .. RST7, RST0 .. RST6, none behind the last
        body = s[s.index(b"\xFF\xDA") + 10:-2]
        marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and 0xD0 <= body[i + 1] <= 0xD7]
        assert marks == [0xD0 + (k & 7) for k in range(15)]


def test_geometry_refusals():
    for T, ch, q, R in ((0, 3, 95, 0), (24, 3, 95, 0), (32, 2, 95, 0), (32, 3, 0, 0), (32, 3, 95, 3), (32, 3, 95, 65536), (32, 3, 95, -1),
                        (4112, 3, 95, 0), (2056, 1, 95, 0)):
        with pytest.raises(ValueError):
            ref.geometry(T, ch, q, R)
    assert ref.geometry(512, 3, 95, 8) == (1024, 8) and ref.geometry(512, 1, 95, 0) == (4096, 4096)


def test_the_librarys_tables_are_the_specifications():
    for ch in (1, 3):
        for q in (1, 30, 75, 95, 100):
            assert _lib.tiff_jpeg_tables(ch, q) == ref.tables(ch, q)
    tb = ref.tables(3, 95)
    assert tb[:2] == b"\xFF\xD8" and tb[-2:] == b"\xFF\xD9" and tb.count(b"\xFF\xDB\x00\x43") == 2 and b"\xFF\xC0" not in tb and b"\xFF\xDA" not in tb
    for bad in ((2, 95), (3, 0), (3, 101)):
        with pytest.raises(_lib.VfsmsError):
            _lib.tiff_jpeg_tables(*bad)


# ---- 2. the writer ----------------------------------------------------------------------------------------------------------------------
TYPES = {1: "B", 3: "H", 4: "I", 7: "B", 16: "Q"}


def parse_tiff(path):
    """a minimal reader of tiled TIFF / BigTIFF with JPEG tiles: -> one dict per IFD in chain order with `tags` (tag -> list of values),
    `tiles` (every tile's bytes, row-major) and `big`"""
    data = open(path, "rb").read()
    assert data[:2] == b"II"
    magic = struct.unpack_from("<H", data, 2)[0]
    assert magic in (42, 43)
    big = magic == 43
    ifd = struct.unpack_from("<Q", data, 8)[0] if big else struct.unpack_from("<I", data, 4)[0]
    cfmt, esize, field, ofmt = ("<Q", 20, 8, "<Q") if big else ("<H", 12, 4, "<I")
    pages = []
    while ifd:
        assert ifd % 2 == 0 and len(pages) < 32
        n = struct.unpack_from(cfmt, data, ifd)[0]
        pos = ifd + struct.calcsize(cfmt)
        tags, prev = {}, 0
        for e in range(n):
            tag, ty = struct.unpack_from("<HH", data, pos + e * esize)
            cnt = struct.unpack_from(ofmt, data, pos + e * esize + 4)[0]
            assert tag > prev, "tags ascend"
            prev = tag
            size = struct.calcsize("<" + TYPES[ty]) * cnt
            at = pos + e * esize + 4 + field
            if size > field:
                at = struct.unpack_from(ofmt, data, at)[0]
            tags[tag] = list(struct.unpack_from("<%d%s" % (cnt, TYPES[ty]), data, at))
            if tag == 347:
                assert ty == 7, "JPEGTables is UNDEFINED"
        ifd = struct.unpack_from(ofmt, data, pos + n * esize)[0]
        assert len(tags[324]) == len(tags[325]) == -(-tags[256][0] // tags[322][0]) * -(-tags[257][0] // tags[323][0])
        tiles = [data[o:o + c] for o, c in zip(tags[324], tags[325])]
        assert all(len(t) == c for t, c in zip(tiles, tags[325]))
        pages.append({"tags": tags, "tiles": tiles, "big": big})
    return pages


def check_file(path, img, levels, T, q, R, big=None):
    """the tags and every tile's bytes are the specification's -> the pages"""
    ch = 1 if img.ndim == 2 else 3
    want = ref.file_tiles(img, levels, T, q, R)
    sizes = [img.shape[:2]] + [lv.shape[:2] for lv in PR.pyramid_levels(img, levels)]
    pages = parse_tiff(path)
    assert len(pages) == levels + 1
    for k, pg in enumerate(pages):
        t = pg["tags"]
        assert t[254] == [1 if k else 0] and (t[257][0], t[256][0]) == tuple(sizes[k]) and t[258] == [8] * ch and t[277] == [ch] and t[284] == [1]
        assert t[259] == [7] and t[262] == [6 if ch == 3 else 1] and t[322] == t[323] == [T]
        assert bytes(t[347]) == ref.tables(ch, q)
        assert (t.get(530) == [2, 2]) if ch == 3 else (530 not in t)
        assert pg["tiles"] == want[k], ("level", k)
        if big is not None:
            assert pg["big"] == big
    return pages


def check_pillow_reads(path, img, levels, T, q, R):
    """a reader nobody here wrote: Pillow (libtiff) opens every page, and its pixels are the mosaic of Pillow's own decodes of the rebuilt
    tile streams, cropped"""
    from PIL import Image
    ch = 1 if img.ndim == 2 else 3
    tb = ref.tables(ch, q)
    lvls = [img] + PR.pyramid_levels(img, levels)
    want = ref.file_tiles(img, levels, T, q, R)
    im = Image.open(path)
    assert im.n_frames == levels + 1
    for k, lv in enumerate(lvls):
        im.seek(k)
        h, w = lv.shape[:2]
        assert im.size == (w, h)
        got = np.asarray(im.convert("RGB") if ch == 3 else im)
        nty, ntx = -(-h // T), -(-w // T)
        mosaic = np.zeros((nty * T, ntx * T) + ((3,) if ch == 3 else ()), np.uint8)
        for t, s in enumerate(want[k]):
            ty, tx = divmod(t, ntx)
            mosaic[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T] = _pillow(ref.rebuilt(tb, s))
        assert np.array_equal(got, mosaic[:h, :w]), ("page", k)


def stream(writer, img, levels, T, q, R, band_rows=64):
    """the bands of `img` as Engine.canvas_encode_pyramid_tiles hands them over, computed by the specification"""
    rows, cols = img.shape[:2]
    want = ref.file_tiles(img, levels, T, q, R)
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
    for T, levels, R, band in ((32, 3, 4, 32), (32, 3, 4, 64), (16, 2, 0, 64)):
        for mode, kw in (("classic", {}), ("big", {"force_big": True})):
            path = str(tmp_path / ("p_%d_%d_%s.tif" % (T, band, mode)))
            w = isa.PyramidTiffBandWriter(path, tile=T, levels=levels, compression="jpeg", quality=90, restart_mcus=R, **kw)
            assert w.device_tiles and w.pyramid_levels(shape) == levels
            stream(w, img, levels, T, 90, R, band)
            check_file(path, img, levels, T, 90, R, big=(mode == "big"))
            assert not [n for n in os.listdir(str(tmp_path)) if n.startswith(".")]
            check_pillow_reads(path, img, levels, T, 90, R)
    assert not isa.PyramidTiffBandWriter("x.tif").device_tiles and not isa.PyramidTiffBandWriter("x.tif", compression="deflate").device_tiles


def test_every_band_completes_the_tiles_the_index_helper_names():
    """pyramid_tiles_index over the bands of a walk names every tile of every level once, in order"""
    for rows, cols, levels, T, band in ((150, 200, 3, 32, 32), (150, 200, 3, 32, 64), (1000, 70, 5, 16, 64), (20, 30, 0, 32, 4096)):
        seen = [[] for _ in range(levels + 1)]
        for r0 in range(0, rows, band):
            keys = isa.Engine.pyramid_tiles_index(rows, cols, levels, T, r0, min(band, rows - r0))
            assert keys == sorted(keys)
            for k, t in keys:
                seen[k].append(t)
        for k in range(levels + 1):
            n = -(-PR.level_size(rows, k) // T) * -(-PR.level_size(cols, k) // T)
            assert seen[k] == list(range(n)), (rows, cols, k)


def test_writer_refusals(tmp_path):
    img = _image((100, 70, 3), 2)
    path = str(tmp_path / "sub" / "r.tif")
    for kw in (dict(tile=32, restart_mcus=3), dict(tile=32, restart_mcus=65536), dict(tile=32, quality=0), dict(tile=24), dict(tile=4112, restart_mcus=0)):
        with pytest.raises(ValueError):
            isa.PyramidTiffBandWriter(path, compression="jpeg", **kw)
    with pytest.raises(ValueError):                              # pixel bands: there is no host encoder behind "jpeg"
        isa.PyramidTiffBandWriter(path, tile=32, levels=0, compression="jpeg")(0, img[:20, :30], (20, 30, 3), levels=[])
    with pytest.raises(ValueError):                              # tile streams to a writer of pixels
        isa.PyramidTiffBandWriter(path, tile=32, levels=0).tiles(0, 20, np.zeros(4, np.uint8), np.array([[0, 0, 0, 4]]), (20, 30, 3))
    assert not os.path.exists(str(tmp_path / "sub")) or os.listdir(str(tmp_path / "sub")) == []
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="jpeg", restart_mcus=0)
    with pytest.raises(ValueError):                              # bands out of order
        w.tiles(64, 36, np.zeros(4, np.uint8), np.array([[0, 0, 0, 4]]), img.shape)
    assert os.listdir(str(tmp_path / "sub")) == []


def test_a_writer_that_fails_in_mid_stream_leaves_no_file(tmp_path):
    img = _image((100, 70, 3), 4)
    path = str(tmp_path / "sub" / "broken.tif")
    want = ref.file_tiles(img, 1, 32, 90, 0)
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="jpeg", quality=90, restart_mcus=0)
    first = want[0][0] + want[0][1] + want[0][2]
    index = [[0, 0, 0, len(want[0][0])], [0, 1, len(want[0][0]), len(want[0][1])], [0, 2, len(want[0][0]) + len(want[0][1]), len(want[0][2])]]
    w.tiles(0, 32, np.frombuffer(first, np.uint8), np.array(index), img.shape)
    assert not os.path.exists(path) and len(os.listdir(str(tmp_path / "sub"))) == 1      # the hidden name alone
    with pytest.raises(ValueError):                              # tile 4 of level 0 where tile 3 is due
        w.tiles(32, 32, np.frombuffer(want[0][4], np.uint8), np.array([[0, 4, 0, len(want[0][4])]]), img.shape)
    assert os.listdir(str(tmp_path / "sub")) == []
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="jpeg", quality=90, restart_mcus=0)
    with pytest.raises(ValueError):                              # a record that points beyond the payload
        w.tiles(0, 32, np.frombuffer(first, np.uint8), np.array(index[:2] + [[0, 2, index[2][2], index[2][3] + 1]]), img.shape)
    assert os.listdir(str(tmp_path / "sub")) == []
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="jpeg", quality=90, restart_mcus=0)
    with pytest.raises(AssertionError):                          # the last band arrives, but not every tile did
        w.tiles(0, 100, np.frombuffer(first, np.uint8), np.array(index), img.shape)
    assert os.listdir(str(tmp_path / "sub")) == []
    stream(isa.PyramidTiffBandWriter(path, tile=32, levels=1, compression="jpeg", quality=90, restart_mcus=0), img, 1, 32, 90, 0, 32)
    check_file(path, img, 1, 32, 90, 0)                          # the same name is written whole afterwards


# ---- 3. the Stitcher --------------------------------------------------------------------------------------------------------------------
class TileOracleEngine(PyramidOracleEngine):
    """PyramidOracleEngine plus canvas_encode_pyramid_tiles: the payloads of every band computed by the specification"""

    tile_calls = 0

    def canvas_encode_pyramid_tiles(self, h, rows, cols, ch, levels, tile, quality, restart_mcus, band_rows):
        self.tile_calls += 1
        if band_rows % tile or band_rows % (1 << levels):
            raise ValueError("band_rows")
        img = self.canvas_download(h, rows, cols, ch)
        want = ref.file_tiles(img, levels, tile, quality, restart_mcus)
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
    s = isa.Stitcher()
    assert s._pyramidOptions() == {"tile": 512, "levels": None, "compression": "none", "quality": 95, "restart_mcus": 8}


def test_stitcher_writes_one_file_of_the_specifications_tiles(oracle, tmp_path):
    from PIL import Image
    P = _Project(tmp_path)
    eng0, plain = P.run(oracle, "plain", engine=TileOracleEngine)
    assert eng0.tile_calls == 0 and eng0.pyramid_calls == 0
    mosaic = np.ascontiguousarray(np.asarray(Image.open(str(plain / "stitching_result_1.tif")))[:, :, ::-1])       # B G R, as the canvas held it
    assert mosaic.shape == (416, 476, 3)
    for tag, kw, K, T, R in (("pyr", {"pyramidTile": 32, "pyramidLevels": 3, "jpegRestartMcus": 2}, 3, 32, 2), ("auto", {"pyramidTile": 64, "mosaicBandRows": 128}, 3, 64, 8),
                             ("one", {"jpegRestartMcus": 0, "jpegQuality": 80, "mosaicBandRows": 4096}, 0, 512, 0)):
        eng, out = P.run(oracle, tag, engine=TileOracleEngine, outputPyramid=True, pyramidCompression="jpeg", **kw)
        assert eng.tile_calls == 1 and eng.pyramid_calls == 0    # (also a mosaic that fits one tile: the same call, zero reduced levels)
        assert os.listdir(str(out)) == ["stitching_result_1.tif"]
        q = kw.get("jpegQuality", 95)
        check_file(str(out / "stitching_result_1.tif"), mosaic, K, T, q, R, big=False)
        check_pillow_reads(str(out / "stitching_result_1.tif"), mosaic, K, T, q, R)


def test_stitcher_refusals_come_before_any_decode(oracle, tmp_path):
    P = _Project(tmp_path)
    user_sink = lambda row0, band, full_shape: None
    for tag, exc, kw in (("eng", NotImplementedError, {"engine": PyramidOracleEngine}), ("sink", ValueError, {"mosaicSink": user_sink}),
                         ("band", ValueError, {"pyramidTile": 64, "mosaicBandRows": 32}), ("interval", ValueError, {"pyramidTile": 32, "jpegRestartMcus": 3}),
                         ("quality", ValueError, {"pyramidTile": 32, "jpegQuality": 101}), ("ext", ValueError, {"ext": "jpg"}),
                         ("levels", ValueError, {"pyramidTile": 16, "pyramidLevels": 6, "mosaicBandRows": 32, "jpegRestartMcus": 1})):
        kw.setdefault("engine", TileOracleEngine)
        with pytest.raises(exc):
            P.run(oracle, tag, outputPyramid=True, pyramidCompression="jpeg", **kw)
        assert P.decodes == 0, tag
        assert not (tmp_path / tag).exists() or not os.listdir(str(tmp_path / tag)), tag
    # jpegEncoder is independent of this: "device" with a .tif pyramid goes through the tile path all the same
    eng, out = P.run(oracle, "both", engine=TileOracleEngine, outputPyramid=True, pyramidCompression="jpeg", pyramidTile=32, jpegRestartMcus=2, jpegEncoder="device")
    assert eng.tile_calls == 1 and os.listdir(str(out)) == ["stitching_result_1.tif"]
