"""JPEG tiles for pyramidal TIFF on the device (csrc/jpeg_enc_kernels.hip in tile order; Method.pyramidCompression = "jpeg") against their
specification, tests/tiff_jpeg_ref.py, byte for byte: the operator at the smallest shapes at which each mechanism can go wrong, capacity,
the canvas path with pending rows carried across bands, its contract, the image-order entries it shares kernels with, and the driver."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as jref               # noqa: E402
import tiff_jpeg_ref as ref               # noqa: E402
from test_pyramid_gpu import _canvas      # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402

pytestmark = pytest.mark.gpu


def _image(h, w, ch, seed, noise=False):
    """smooth content with some noise on it (noise: noise alone, the densest stream)"""
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if ch == 3 else (h, w)
    if noise:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 8, (h, w))
    img = np.stack([base, 0.7 * base + 30, 255 - base], -1) if ch == 3 else base
    return np.clip(img, 0, 255).astype(np.uint8)


def _split(payload, offsets):
    payload = bytes(payload)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == len(payload)
    return [payload[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


# (what, h, w, ch, T, quality, R, noise)
OPERATOR = [
    ("one MCU per tile, one pixel", 1, 1, 3, 16, 95, 0, False),
    ("one MCU per tile", 17, 33, 3, 16, 95, 1, False),
    ("MCU columns wholly outside, colour", 65, 65, 3, 64, 90, 4, False),
    ("MCU columns wholly outside, gray", 65, 65, 1, 64, 90, 8, False),
    ("a 256-pixel strip straddles tiles", 40, 300, 3, 32, 95, 2, False),
    ("a 768-pixel strip straddles tiles; waves start in mid-tile", 24, 800, 1, 32, 95, 1, False),
    ("a wave's range exceeds the LDS window", 256, 256, 1, 64, 100, 16, True),
    ("one interval per tile", 70, 100, 3, 32, 95, 0, False),
    ("one interval per tile, gray", 70, 100, 1, 32, 75, 0, False),
]


@pytest.mark.parametrize("case", OPERATOR, ids=[c[0] for c in OPERATOR])
def test_operator_equals_level_0_of_the_specification(engine, case):
    what, h, w, ch, T, q, R, noise = case
    img = _image(h, w, ch, h * 1000 + w, noise)
    want = ref.file_tiles(img, 0, T, q, R)[0]
    payload, offsets = engine.jpeg_encode_tiles_device(img, T, bgr=True, quality=q, restart_mcus=R)
    got = _split(payload, offsets)
    assert len(got) == len(want) == -(-h // T) * -(-w // T)
    for t, (g, x) in enumerate(zip(got, want)):
        assert g == x, (what, "tile", t, len(g), len(x))
    if noise:
        n_int = len(want) * (T // 8) ** 2 // R
        assert n_int <= 64 and len(payload) > 2 * 32768          # one wave, more than two windows
    wide = np.zeros((h, w + 5) + img.shape[2:], np.uint8)
    wide[:, 3:3 + w] = img
    view = wide[:, 3:3 + w]                                     # rows strided, the first pixel at an odd byte
    assert h == 1 or not view.flags.c_contiguous
    p2, o2 = engine.jpeg_encode_tiles_device(view, T, bgr=True, quality=q, restart_mcus=R)
    assert bytes(p2) == bytes(payload) and np.array_equal(o2, offsets), (what, "strided")
    if ch == 3:
        rgb = np.ascontiguousarray(img[:, :, ::-1])
        p3, o3 = engine.jpeg_encode_tiles_device(rgb, T, bgr=False, quality=q, restart_mcus=R)
        assert bytes(p3) == bytes(payload) and np.array_equal(o3, offsets), (what, "rgb")


def test_operator_refusals(engine):
    img = np.zeros((40, 40, 3), np.uint8)
    for what, kw in (("tile no multiple of 16", dict(tile=24)), ("tile 0", dict(tile=0)), ("intervals do not divide the tile", dict(tile=32, restart_mcus=3)),
                     ("restart_mcus too large", dict(tile=32, restart_mcus=65536)), ("quality", dict(tile=32, quality=0)),
                     ("one interval of more than 65535 MCUs", dict(tile=4112, restart_mcus=0))):
        with pytest.raises(_lib.VfsmsError):
            engine.jpeg_encode_tiles_device(img, **kw)
        with pytest.raises(ValueError):
            ref.geometry(kw["tile"], 3, kw.get("quality", 95), kw.get("restart_mcus", 0))
    with pytest.raises(_lib.VfsmsError):
        engine.jpeg_encode_tiles_device(np.zeros((40, 40, 2), np.uint8), 32)


def test_operator_capacity(engine):
    import ctypes as C
    img = _image(70, 100, 3, 5)
    payload, offsets = engine.jpeg_encode_tiles_device(img, 32, quality=95, restart_mcus=2)
    need = len(payload)
    fn = engine.lib.vfsms_jpeg_encode_tiles_device
    offs = np.zeros(offsets.size, np.uint64)

    def call(out):
        n = C.c_size_t()
        rc = fn(engine.ctx, img.ctypes.data_as(C.c_void_p), 70, 100, 3, img.strides[0], 1, 32, 95, 2, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size - 64),
                C.byref(n), offs.ctypes.data_as(C.c_void_p), offs.size)
        return rc, n.value
    small = np.full(need - 1 + 64, 0xAB, np.uint8)              # (64 guard bytes behind the capacity handed over)
    rc, n = call(small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and n == need and (small == 0xAB).all()
    exact = np.full(need + 64, 0xAB, np.uint8)
    rc, n = call(exact)
    assert rc == _lib.VFSMS_OK and n == need and bytes(exact[:need]) == bytes(payload) and (exact[need:] == 0xAB).all()
    assert np.array_equal(offs, offsets)


# ---- the canvas path ------------------------------------------------------------------------------------------------------------------
ROWS, COLS, TILE, LEVELS = 150, 200, 32, 3


@pytest.fixture(scope="module", params=[1, 3], ids=["gray", "colour"])
def canvas(engine, request):
    ch = request.param
    cv = _canvas(engine, ROWS, COLS, ch, 21 + ch)
    img = engine.canvas_download(cv, ROWS, COLS, ch)
    assert (img == 0).any() and img.any()
    yield cv, img, ch, ref.file_tiles(img, LEVELS, TILE, 90, 4)
    engine.canvas_free(cv)


def _walk(engine, cv, ch, band_rows, R=4):
    """-> per level {tile number: stream}, checking the index as it comes"""
    got = [dict() for _ in range(LEVELS + 1)]
    for r0, n, payload, index in engine.canvas_encode_pyramid_tiles(cv, ROWS, COLS, ch, LEVELS, TILE, 90, R, band_rows):
        payload = bytes(payload)
        assert [(int(k), int(t)) for k, t, _o, _c in index] == engine.pyramid_tiles_index(ROWS, COLS, LEVELS, TILE, r0, n)
        pos = 0
        for k, t, off, cnt in index.tolist():                    # file order: back to back, level after level, tiles ascending
            assert off == pos and cnt > 0 and t not in got[k]
            got[k][t] = payload[off:off + cnt]
            pos += cnt
        assert pos == len(payload)
        keys = [(k, t) for k, t, _o, _c in index.tolist()]
        assert keys == sorted(keys)
    return got


@pytest.mark.parametrize("band_rows", [32, 64])
def test_canvas_bands_give_the_files_tiles(engine, canvas, band_rows):
    cv, img, ch, want = canvas
    got = _walk(engine, cv, ch, band_rows)
    for k in range(LEVELS + 1):
        assert sorted(got[k]) == list(range(len(want[k]))), ("level", k)
        for t, x in enumerate(want[k]):
            assert got[k][t] == x, ("level", k, "tile", t, band_rows)
    # levels 1 .. 3 are 75, 38 and 19 rows: with bands of 32 rows level 1 gets 16 rows a band, so a tile row waits for a second band,
    # and the last band flushes short tile rows of every level
    assert [len(w) for w in want] == [5 * 7, 3 * 4, 2 * 2, 1]


def test_canvas_band_contract(engine, canvas):
    cv, img, ch, want = canvas
    out, index = np.empty(1 << 20, np.uint8), np.empty((256, 4), np.int64)

    def call(row0, nrows, levels=LEVELS, tile=TILE, R=4, handle=None, out=out, index=index):
        return engine.canvas_encode_pyramid_tiles_rows(cv if handle is None else handle, row0, nrows, levels, tile, 90, R, out, index)
    for what, kw in (("row0 no multiple of 2^levels", dict(row0=4, nrows=32, tile=16, levels=3)), ("nrows no multiple of 2^levels", dict(row0=0, nrows=16, tile=16, levels=5)),
                     ("row0 no multiple of the tile", dict(row0=16, nrows=32)), ("nrows no multiple of the tile", dict(row0=0, nrows=48)),
                     ("a band out of order", dict(row0=64, nrows=32)), ("levels 11", dict(row0=0, nrows=ROWS, levels=11)),
                     ("rows beyond the canvas", dict(row0=128, nrows=32)), ("intervals do not divide the tile", dict(row0=0, nrows=32, R=3)),
                     ("unknown canvas", dict(row0=0, nrows=32, handle=cv + 12345))):
        with pytest.raises(_lib.VfsmsError) as e:
            call(**kw)
        assert "canvas_encode_pyramid_tiles" in str(e.value), (what, str(e.value))
    # a short buffer consumes nothing: the same band again succeeds, and the walk goes on from it
    rc, need, ni = call(0, 64)
    assert rc == _lib.VFSMS_OK and ni == 2 * 7 + 1 * 4
    small = np.full(need - 1, 0xAB, np.uint8)
    rc, need2, ni2 = call(0, 64, out=small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and (need2, ni2) == (need, ni) and (small == 0xAB).all()
    rc, need2, ni2 = call(0, 64, index=np.empty((ni - 1, 4), np.int64))
    assert rc == _lib.VFSMS_ERR_CAPACITY and (need2, ni2) == (need, ni)
    first = bytes(out[:need])
    rc, need3, _ = call(0, 64)
    assert rc == _lib.VFSMS_OK and bytes(out[:need3]) == first
    with pytest.raises(_lib.VfsmsError):
        call(0 + 32, 32)                                         # the next band is row 64
    rc, need4, ni4 = call(64, 86)                                # .. to the last row, in a band longer than the first: the pending buffer grows
    assert rc == _lib.VFSMS_OK and ni4 == 3 * 7 + 2 * 4 + 2 * 2 + 1
    tiles = {(int(k), int(t)): bytes(out[o:o + c]) for k, t, o, c in index[:ni4].tolist()}
    assert tiles[(0, 34)] == want[0][34] and tiles[(3, 0)] == want[3][0] and tiles[(1, 11)] == want[1][11] and (1, 0) not in tiles


def test_zero_reduced_levels(engine):
    """a mosaic that fits one tile: level 0 alone"""
    cv = _canvas(engine, 20, 30, 3, 4)
    try:
        img = engine.canvas_download(cv, 20, 30, 3)
        bands = list(engine.canvas_encode_pyramid_tiles(cv, 20, 30, 3, 0, 32, 95, 0, 4096))
        assert len(bands) == 1 and bands[0][3].tolist() == [[0, 0, 0, len(bands[0][2])]]
        assert bytes(bands[0][2]) == ref.file_tiles(img, 0, 32, 95, 0)[0][0]
    finally:
        engine.canvas_free(cv)


def test_image_order_entries_still_write_the_encoders_bytes(engine, canvas):
    cv, img, ch, _want = canvas
    assert bytes(engine.jpeg_encode_device(img, bgr=True, quality=90, restart_mcus=3)) == jref.encode(img, 90, 3, True)
    body = b"".join(bytes(p) for _r0, _n, p in engine.canvas_encode_jpeg_bands(cv, ROWS, COLS, ch, 90, 1, 64))
    assert _lib.jpeg_header(ROWS, COLS, ch, 90, 1) + body + b"\xFF\xD9" == jref.encode(img, 90, 1, True)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
def test_stitcher_writes_jpeg_tiles_end_to_end(engine, tmp_path):
    from PIL import Image
    from test_tiff_jpeg_host import parse_tiff, check_pillow_reads
    rng = np.random.default_rng(8)
    proj = tmp_path / "proj"; (proj / "1").mkdir(parents=True)
    yy, xx = np.mgrid[0:192, 0:192]
    for k in range(9):
        base = 128 + 90 * np.sin((xx + 31 * k) / 11.0) * np.cos((yy + 17 * k) / 13.0) + rng.normal(0, 5, (192, 192))
        Image.fromarray(np.clip(np.stack([base, 0.8 * base + 20, 255 - base], -1), 0, 255).astype(np.uint8)).save(str(proj / "1" / ("t%d.png" % k)))
    old = (isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    outs = {}
    try:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = True, "fadeInAndFadeOut"
        for comp in ("none", "jpeg"):
            s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.mosaicBandRows = 64
            s.outputPyramid, s.pyramidTile, s.pyramidCompression = True, 64, comp
            assert s.jpegQuality == 95 and s.jpegRestartMcus == 8
            # a 3 x 3 serpentine arrangement with overlaps and holes
            offsets = iter([[6, 160], [-4, 165], [158, 5], [3, -162], [-5, -160], [161, -3], [4, 163], [-2, 158]])
            out = tmp_path / ("o_" + comp)
            s.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, lambda images: (True, next(offsets)), fileExtension="png", outputfileExtension="tif")
            assert os.listdir(str(out)) == ["stitching_result_1.tif"]
            outs[comp] = str(out / "stitching_result_1.tif")
    finally:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = old
    mosaic = np.ascontiguousarray(np.asarray(Image.open(outs["none"]))[:, :, ::-1])       # B G R, as the canvas held it
    assert mosaic.ndim == 3 and min(mosaic.shape[:2]) > 400 and (mosaic == 0).all(axis=2).any()
    K = isa.io.default_levels(mosaic.shape[0], mosaic.shape[1], 64)
    assert K >= 3
    want = ref.file_tiles(mosaic, K, 64, 95, 8)
    pages = parse_tiff(outs["jpeg"])
    assert len(pages) == K + 1
    for k, page in enumerate(pages):
        assert page["tags"][259] == [7] and page["tags"][347] == list(ref.tables(3, 95)) and page["tiles"] == want[k], ("level", k)
    check_pillow_reads(outs["jpeg"], mosaic, K, 64, 95, 8)
    assert os.path.getsize(outs["jpeg"]) < os.path.getsize(outs["none"]) // 3
