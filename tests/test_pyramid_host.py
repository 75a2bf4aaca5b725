"""CPU tests of the pyramidal output (Stitcher.outputPyramid): the specification tests/pyramid_ref.py against an independent float64
formulation, PyramidTiffBandWriter's files read back by a minimal TIFF reader written here (normative: classic and BigTIFF headers, the
IFD chain, the tags the writer sets, raw and zlib tiles) and by Pillow, and the Stitcher's wiring on the CPU test doubles."""
import os
import struct
import zlib

import numpy as np
import pytest

import imagestitch_amd as isa
import pyramid_ref as PR
from fakes import IngestOracleEngine


# ---- 1. the specification ---------------------------------------------------------------------------------------------------------------
def float_levels(img, levels):
    """floor(mean + 0.5) in float64 of the same four clamped samples, sample by index arithmetic on flat coordinates, level by level"""
    out = []
    cur = np.asarray(img)
    for _ in range(levels):
        R, C = cur.shape[:2]
        Rk, Ck = (R + 1) // 2, (C + 1) // 2
        ii, jj = np.meshgrid(np.arange(Rk), np.arange(Ck), indexing="ij")
        x = cur.astype(np.float64)
        acc = np.zeros((Rk, Ck) + cur.shape[2:], np.float64)
        for di in (0, 1):
            for dj in (0, 1):
                acc += x[np.clip(2 * ii + di, None, R - 1), np.clip(2 * jj + dj, None, C - 1)]
        nxt = np.floor(acc / 4.0 + 0.5)
        assert nxt.max() <= 255
        cur = nxt.astype(np.uint8)
        out.append(cur)
    return out


@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (7, 5, 3), (200, 333), (257, 1030, 3)])
def test_reference_equals_the_float_formulation(shape):
    img = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    levels = 10
    got, want = PR.pyramid_levels(img, levels), float_levels(img, levels)
    assert len(got) == levels
    for k, (a, b) in enumerate(zip(got, want), 1):
        assert a.dtype == np.uint8 and a.shape == b.shape == (PR.level_size(shape[0], k), PR.level_size(shape[1], k)) + tuple(shape[2:])
        assert np.array_equal(a, b), k


def test_reference_on_saturated_and_rounding_images():
    full = np.full((37, 50, 3), 255, np.uint8)
    for lv in PR.pyramid_levels(full, 7):
        assert lv.min() == 255 and lv.max() == 255              # (no level may exceed 255: nothing wraps)
    # 2 x 2 blocks whose sums are 1, 2 and 3 mod 4: (s + 2) >> 2 rounds .25 down, .5 up, .75 up
    for block, want in (([[1, 0], [0, 0]], 0), ([[1, 1], [0, 0]], 1), ([[1, 1], [1, 0]], 1), ([[5, 4], [4, 4]], 4), ([[5, 5], [4, 4]], 5), ([[5, 5], [5, 4]], 5)):
        img = np.tile(np.array(block, np.uint8), (6, 9))
        lv = PR.pyramid_levels(img, 1)[0]
        assert lv.shape == (6, 9) and (lv == want).all(), (block, want)
        assert np.array_equal(lv, float_levels(img, 1)[0])


@pytest.mark.parametrize("band,levels", [(256, 8), (128, 7)])
def test_bands_of_levels_concatenate_to_the_whole_image(band, levels):
    R, C = 1000, 777
    img = np.random.default_rng(band).integers(0, 256, (R, C, 3), dtype=np.uint8)
    whole = PR.pyramid_levels(img, levels)
    parts = [[] for _ in range(levels)]
    for r0 in range(0, R, band):
        n = min(band, R - r0)
        for k in range(1, levels + 1):
            first, cnt = PR.band_of_level(r0, n, R, k)
            assert first == r0 >> k and first + cnt == -(-(r0 + n) // (1 << k))
            parts[k - 1].append(whole[k - 1][first:first + cnt])
            # a band's level rows depend on no other band: the band reduced ALONE gives the same rows (its end is the image's, or no
            # level row straddles it)
            alone = PR.pyramid_levels(img[r0:r0 + n], k)[k - 1]
            assert np.array_equal(alone, whole[k - 1][first:first + cnt]), (r0, k)
    for k in range(levels):
        assert np.array_equal(np.concatenate(parts[k], 0), whole[k]), k


def test_default_levels():
    assert PR.default_levels(100, 100, 512) == 0 and PR.default_levels(513, 100, 512) == 1 and PR.default_levels(18647, 16795, 512) == 6
    assert PR.default_levels(1 << 30, 5, 16) == 10
    for R, C, T in ((18647, 16795, 512), (118378, 118378, 256), (37, 50, 16), (1, 1, 16), (5000, 3, 32)):
        K = PR.default_levels(R, C, T)
        assert K == isa.io.default_levels(R, C, T)
        assert K == 10 or max(PR.level_size(R, K), PR.level_size(C, K)) <= T
        assert K == 0 or max(PR.level_size(R, K - 1), PR.level_size(C, K - 1)) > T


# ---- 2. the writer ----------------------------------------------------------------------------------------------------------------------
TYPES = {1: "B", 3: "H", 4: "I", 16: "Q"}


def read_tiff(path):
    """a minimal reader of tiled TIFF / BigTIFF: -> one dict per IFD in chain order with `tags` (tag -> tuple of values), `image` (the level,
    R G B or gray), `padded` (all tiles assembled, edge padding included) and `big`"""
    data = open(path, "rb").read()
    assert data[:2] == b"II"
    magic = struct.unpack_from("<H", data, 2)[0]
    assert magic in (42, 43)
    big = magic == 43
    if big:
        assert struct.unpack_from("<HH", data, 4) == (8, 0)
        ifd = struct.unpack_from("<Q", data, 8)[0]
    else:
        ifd = struct.unpack_from("<I", data, 4)[0]
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
            tags[tag] = struct.unpack_from("<%d%s" % (cnt, TYPES[ty]), data, at)
        ifd = struct.unpack_from(ofmt, data, pos + n * esize)[0]
        cols, rows, ch = tags[256][0], tags[257][0], tags[277][0]
        tw, tl = tags[322][0], tags[323][0]
        assert tags[258] == (8,) * ch and tags[284] == (1,) and tags[262] == ((2,) if ch == 3 else (1,)) and tags[259][0] in (1, 8)
        assert tw % 16 == 0 and tl % 16 == 0
        ntx, nty = -(-cols // tw), -(-rows // tl)
        assert len(tags[324]) == len(tags[325]) == ntx * nty
        padded = np.zeros((nty * tl, ntx * tw, ch), np.uint8)
        for t, (off, cnt) in enumerate(zip(tags[324], tags[325])):
            raw = data[off:off + cnt]
            assert len(raw) == cnt
            if tags[259][0] == 8:
                raw = zlib.decompress(raw)
            assert len(raw) == tw * tl * ch
            ty_, tx_ = divmod(t, ntx)
            padded[ty_ * tl:(ty_ + 1) * tl, tx_ * tw:(tx_ + 1) * tw] = np.frombuffer(raw, np.uint8).reshape(tl, tw, ch)
        img = padded[:rows, :cols]
        pages.append({"tags": tags, "image": img if ch > 1 else img[:, :, 0], "padded": padded, "big": big})
    return pages


def check_file(path, img, levels, tile, big=None, compression=1):
    """every level of the file == the reference of `img` (B G R or gray), the subfile types, the zero padding -> the pages"""
    pages = read_tiff(path)
    want = [img] + PR.pyramid_levels(img, levels)
    assert len(pages) == levels + 1
    for k, (pg, w) in enumerate(zip(pages, want)):
        assert pg["tags"][254] == ((1,) if k else (0,)), k
        assert pg["tags"][322] == pg["tags"][323] == (tile,) and pg["tags"][259] == (compression,)
        assert pg["image"].shape == w.shape, (k, pg["image"].shape, w.shape)
        assert np.array_equal(pg["image"], w[:, :, ::-1] if w.ndim == 3 else w), k
        pad = pg["padded"].copy()
        pad[:w.shape[0], :w.shape[1]] = 0
        assert not pad.any(), "edge tiles are padded with zeros"
        if big is not None:
            assert pg["big"] == big
    return pages


def stream(writer, img, levels, band_rows=64):
    """the bands of `img` with their levels from the reference, as Engine.canvas_download_pyramid_bands hands them over"""
    R = img.shape[0]
    whole = PR.pyramid_levels(img, levels)
    for r0 in range(0, R, band_rows):
        n = min(band_rows, R - r0)
        lv = []
        for k in range(1, levels + 1):
            first, cnt = PR.band_of_level(r0, n, R, k)
            lv.append(whole[k - 1][first:first + cnt])
        writer(r0, img[r0:r0 + n], img.shape, levels=lv)


SHAPES = [(37, 50), (100, 65, 3), (300, 200, 3)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("tile", [16, 32])
def test_writer_files_hold_the_reference_levels(tmp_path, shape, tile):
    from PIL import Image
    img = np.random.default_rng(tile + len(shape)).integers(0, 256, shape, dtype=np.uint8)
    for levels in (2, 3, 4, 5):
        for mode, kw in (("classic", {}), ("big", {"force_big": True}), ("deflate", {"compression": "deflate"})):
            path = str(tmp_path / ("p_%d_%s.tif" % (levels, mode)))
            w = isa.PyramidTiffBandWriter(path, tile=tile, levels=levels, **kw)
            assert w.transient_bands and w.pyramid_levels(shape) == levels
            stream(w, img, levels)
            check_file(path, img, levels, tile, big=(mode == "big"), compression=8 if mode == "deflate" else 1)
            assert not [n for n in os.listdir(str(tmp_path)) if n.startswith(".")]
            if mode == "classic":                               # and a reader nobody here wrote: every frame through Pillow
                im = Image.open(path)
                assert im.n_frames == levels + 1
                want = [img] + PR.pyramid_levels(img, levels)
                for k in range(levels + 1):
                    im.seek(k)
                    assert np.array_equal(np.asarray(im), want[k][:, :, ::-1] if img.ndim == 3 else want[k]), (levels, k)


def test_writer_default_levels_and_refusals(tmp_path):
    img = np.random.default_rng(5).integers(0, 256, (300, 200, 3), dtype=np.uint8)
    w = isa.PyramidTiffBandWriter(str(tmp_path / "d.tif"), tile=32)
    K = w.pyramid_levels(img.shape)
    assert K == PR.default_levels(300, 200, 32) == 4
    stream(w, img, K)
    pages = check_file(str(tmp_path / "d.tif"), img, K, 32, big=False)
    assert pages[-1]["image"].shape[:2] == (19, 13)
    small = img[:20, :30]
    w = isa.PyramidTiffBandWriter(str(tmp_path / "s.tif"), tile=32)              # a mosaic that fits one tile: level 0 alone
    assert w.pyramid_levels(small.shape) == 0
    w(0, small, small.shape, levels=[])
    check_file(str(tmp_path / "s.tif"), small, 0, 32)
    for bad in (0, 8, 24, 100):
        with pytest.raises(ValueError):
            isa.PyramidTiffBandWriter(str(tmp_path / "x.tif"), tile=bad)
    with pytest.raises(ValueError):
        isa.PyramidTiffBandWriter(str(tmp_path / "x.tif"), compression="lzw")
    assert isinstance(isa.band_writer_for("a/b.tif", pyramid={"tile": 64}), isa.PyramidTiffBandWriter)
    assert isinstance(isa.band_writer_for("a/b.tiff", pyramid={}), isa.PyramidTiffBandWriter)
    assert isinstance(isa.band_writer_for("a/b.tif"), isa.TiffBandWriter) and isinstance(isa.band_writer_for("a/b.png"), isa.PngBandWriter)


def test_a_writer_that_fails_in_mid_stream_leaves_no_file(tmp_path):
    img = np.random.default_rng(6).integers(0, 256, (300, 200, 3), dtype=np.uint8)
    path = str(tmp_path / "sub" / "broken.tif")
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=3)
    whole = PR.pyramid_levels(img, 3)
    w(0, img[:64], img.shape, levels=[whole[k][:64 >> (k + 1)] for k in range(3)])
    assert not os.path.exists(path)                              # (nothing under the final name before the last band)
    with pytest.raises(ValueError):
        w(64, img[64:128], img.shape, levels=[whole[0][32:64]])  # two levels short
    assert os.listdir(str(tmp_path / "sub")) == []
    w = isa.PyramidTiffBandWriter(path, tile=32, levels=3, compression="deflate")
    with pytest.raises(Exception):
        w(0, img[:64], img.shape, levels=[whole[0][:32], whole[1][:16], whole[2][:8, :5]])     # a level of the wrong width
    assert os.listdir(str(tmp_path / "sub")) == []
    stream(isa.PyramidTiffBandWriter(path, tile=32, levels=3), img, 3)          # the same name is written whole afterwards
    check_file(path, img, 3, 32)


# ---- 3. the Stitcher ----------------------------------------------------------------------------------------------------------------------
class PyramidOracleEngine(IngestOracleEngine):
    """IngestOracleEngine plus canvas_download_pyramid_bands: bands and levels served from the reference"""

    pyramid_calls = 0

    def canvas_download_pyramid_bands(self, h, rows, cols, ch, levels, band_rows=4096, transient=False):
        self.pyramid_calls += 1
        if band_rows % (1 << levels):
            raise ValueError("band_rows")
        img = self.canvas_download(h, rows, cols, ch)
        whole = PR.pyramid_levels(img, levels)
        for r0 in range(0, rows, band_rows):
            n = min(band_rows, rows - r0)
            lv = []
            for k in range(1, levels + 1):
                first, cnt = PR.band_of_level(r0, n, rows, k)
                lv.append(whole[k - 1][first:first + cnt].copy())
            yield r0, img[r0:r0 + n].copy(), lv


class _Project:
    """four colour tiles of a 2 x 2 synthetic grid as one dataset on disk; every decode is counted"""

    def __init__(self, tmp_path):
        from PIL import Image
        from imagestitch_amd.synthetic import SyntheticGrid
        from test_host_logic import _colour_tiles
        self.root = tmp_path / "proj"
        (self.root / "1").mkdir(parents=True)
        for k, t in enumerate(_colour_tiles(SyntheticGrid(2, 2, 128, overlap=0.25))):
            Image.fromarray(t).save(str(self.root / "1" / ("t%02d.png" % k)))
        self.tmp = tmp_path

    def run(self, oracle, tag, ext="tif", engine=PyramidOracleEngine, **attrs):
        """-> (engine, output directory, decodes)"""
        from imagestitch_amd import stitcher as ST
        eng = engine(oracle, scripted=lambda A, B, job: [1, 96, 0, 9, 10, 10, 9, 0])
        s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.direction = 2
        s.mosaicBandRows = 32
        for k, v in attrs.items():
            setattr(s, k, v)
        out = self.tmp / tag
        counts = {"n": 0}
        real_once, real_imread = ST._decode_once, ST._imread

        def once(path, color):
            counts["n"] += 1
            return real_once(path, color)

        def imread(path, color):
            counts["n"] += 1
            return real_imread(path, color)
        old = (isa.Stitcher.direction, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod)
        ST._decode_once, ST._imread = once, imread
        try:
            isa.Stitcher.direction, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod = 2, True, "surf", "fadeInAndFadeOut"
            try:
                s.imageSetStitchWithMutiple(str(self.root), str(out) + os.sep, 1, s.calculateOffsetForFeatureSearchIncre, fileExtension="png", outputfileExtension=ext)
            finally:
                self.decodes = counts["n"]
        finally:
            ST._decode_once, ST._imread = real_once, real_imread
            isa.Stitcher.direction, isa.Stitcher.isColorMode, isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod = old
        assert not eng.live
        return eng, out


def test_method_defaults():
    m = isa.Method
    assert (m.outputPyramid, m.pyramidTile, m.pyramidLevels, m.pyramidCompression) == (False, 512, None, "none")


def test_stitcher_writes_one_pyramidal_tiff(oracle, tmp_path):
    from PIL import Image
    P = _Project(tmp_path)
    eng0, plain = P.run(oracle, "plain")
    assert eng0.pyramid_calls == 0 and P.decodes > 0           # outputPyramid = False: no pyramid call
    assert os.listdir(str(plain)) == ["stitching_result_1.tif"]
    mosaic = np.asarray(Image.open(str(plain / "stitching_result_1.tif")))       # R G B
    assert mosaic.shape == (416, 476, 3)                      # (the scripted offsets: a staircase of the four tiles, holes beside it)
    for tag, kw, K in (("pyr", {"pyramidTile": 32, "pyramidLevels": 3}, 3), ("auto", {"pyramidTile": 64}, 3),
                       ("z", {"pyramidTile": 16, "pyramidLevels": 5, "pyramidCompression": "deflate"}, 5)):
        eng, out = P.run(oracle, tag, outputPyramid=True, **kw)
        assert eng.pyramid_calls == 1
        assert os.listdir(str(out)) == ["stitching_result_1.tif"]
        assert K == PR.default_levels(416, 476, kw["pyramidTile"]) or "pyramidLevels" in kw
        check_file(str(out / "stitching_result_1.tif"), np.ascontiguousarray(mosaic[:, :, ::-1]), K, kw["pyramidTile"],
                   compression=8 if tag == "z" else 1)
    # a mosaic that fits one tile: level 0 alone, through the ordinary bands
    eng, out = P.run(oracle, "one", outputPyramid=True)
    assert eng.pyramid_calls == 0
    check_file(str(out / "stitching_result_1.tif"), np.ascontiguousarray(mosaic[:, :, ::-1]), 0, 512)


def test_stitcher_refusals_come_before_any_decode(oracle, tmp_path):
    P = _Project(tmp_path)
    for tag, exc, kw in (("ext", ValueError, {"ext": "png"}), ("nostream", ValueError, {"streamOutput": False}),
                         ("band", ValueError, {"pyramidLevels": 3, "mosaicBandRows": 36}), ("eng", NotImplementedError, {"engine": IngestOracleEngine}),
                         ("tile", ValueError, {"pyramidTile": 100})):
        with pytest.raises(exc):
            P.run(oracle, tag, outputPyramid=True, **kw)
        assert P.decodes == 0, tag
        assert not (tmp_path / tag).exists() or not os.listdir(str(tmp_path / tag)), tag
    # pyramidLevels None: the level count follows from the mosaic's size, so the band check comes with the layout -- before anything is
    # fused or written
    with pytest.raises(ValueError):
        P.run(oracle, "late", outputPyramid=True, pyramidTile=32, mosaicBandRows=36)
    assert not [n for n in os.listdir(str(tmp_path / "late")) if n.endswith(".tif")]


def test_a_users_sink_with_pyramid_levels_gets_the_levels(oracle, tmp_path):
    """stitcher.mosaicSink = anything with pyramid_levels: the streaming loop hands every band over with its levels"""
    from imagestitch_amd import stitcher as ST
    from test_host_logic import _write_tiles
    rng = np.random.default_rng(3)
    scene = rng.integers(0, 256, (70, 100)).astype(np.uint8)
    files = _write_tiles(tmp_path, [np.ascontiguousarray(scene[:, x:x + 40]) for x in (0, 30, 60)], "u")
    got = []

    class Sink:
        def pyramid_levels(self, full_shape):
            return 2

        def __call__(self, row0, band, full_shape, levels):
            got.append((row0, band.copy(), [lv.copy() for lv in levels]))
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = False
        for engine, bandrows, exc in ((PyramidOracleEngine, 32, None), (PyramidOracleEngine, 30, ValueError), (IngestOracleEngine, 32, NotImplementedError)):
            s = isa.Stitcher(); s._engine = engine(oracle); s.isPrintLog = False; s.isColorMode = False
            s.fuseMethod = "notFuse"; s.mosaicSink = Sink(); s.mosaicBandRows = bandrows
            del got[:]
            if exc:
                with pytest.raises(exc):
                    s.getStitchByOffset(list(files), [[0, 30], [0, 30]])
                assert not got
                continue
            assert s.getStitchByOffset(list(files), [[0, 30], [0, 30]]) is None
            s2 = isa.Stitcher(); s2._engine = engine(oracle); s2.isPrintLog = False; s2.isColorMode = False; s2.fuseMethod = "notFuse"
            whole = s2.getStitchByOffset(list(files), [[0, 30], [0, 30]])
            assert [g[0] for g in got] == [0, 32, 64] and np.array_equal(np.concatenate([g[1] for g in got], 0), whole)
            for k, w in enumerate(PR.pyramid_levels(whole, 2)):
                assert np.array_equal(np.concatenate([g[2][k] for g in got], 0), w)
    finally:
        isa.Stitcher.isColorMode = old
