"""The PNG coder on the device (the PNG kernels of csrc/deflate_kernels.hip over csrc/png_core.h; Method.pngEncoder = "device") against its
specification tests/png_ref.py, byte for byte: the bare operator over the shapes, segment sizes and contents at which it can go wrong, the
canvas bands for several band sizes (the row above a band's first row is the canvas's), the band contract and the capacity behaviour, a PNG
band in the middle of a deflate-tile walk, and one stitched dataset end to end."""
import ctypes as C
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_ref as D                   # noqa: E402
import png_ref as ref                     # noqa: E402
import png_cases as K                     # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402
from test_pyramid_gpu import _canvas      # noqa: E402

pytestmark = pytest.mark.gpu


def _bgr(img):
    return np.ascontiguousarray(img[:, :, ::-1]) if img.ndim == 3 else img


@pytest.mark.parametrize("case", K.CASES, ids=[c[0] for c in K.CASES])
def test_operator_equals_the_specification(engine, case):
    what, make, S = case
    img = make()                                                    # R G B
    h, w = img.shape[:2]
    f = ref.filter_rows(img)
    want, adler = ref.device_payload(img, S, filtered=f), ref.band_adler(img, filtered=f)
    payload, got_adler = engine.png_encode_device(img, segment_rows=S, bgr=False)
    assert bytes(payload) == want, (what, len(payload), len(want))
    assert got_adler == adler, what
    wide = np.zeros((h, w + 5) + img.shape[2:], np.uint8)
    wide[:, 3:3 + w] = _bgr(img)
    view = wide[:, 3:3 + w]                                         # rows strided, the first pixel at an odd byte; B G R
    assert h == 1 or not view.flags.c_contiguous
    p2, a2 = engine.png_encode_device(view, segment_rows=S, bgr=True)
    assert bytes(p2) == want and a2 == adler, (what, "strided, bgr")


def test_operator_refusals(engine):
    img = np.zeros((40, 40, 3), np.uint8)
    for what, kw in (("segment_rows 0", dict(segment_rows=0)), ("negative", dict(segment_rows=-16)), ("beyond 4096", dict(segment_rows=4097))):
        with pytest.raises(_lib.VfsmsError) as e:
            engine.png_encode_device(img, **kw)
        assert "png_encode_device" in str(e.value), what
        with pytest.raises(ValueError):
            ref.check_geometry(kw["segment_rows"], 40, 40, 3)
    with pytest.raises(_lib.VfsmsError):
        engine.png_encode_device(np.zeros((40, 40, 2), np.uint8), 16)


def test_operator_capacity(engine):
    img = _bgr(K.real_crop(48, 333))
    payload, adler = engine.png_encode_device(img, 16)
    need = len(payload)
    fn = engine.lib.vfsms_png_encode_device

    def call(out):
        n, a = C.c_size_t(), C.c_uint32()
        rc = fn(engine.ctx, img.ctypes.data_as(C.c_void_p), 48, 333, 1, img.strides[0], 1, 16, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size - 64),
                C.byref(n), C.byref(a))
        return rc, n.value, a.value
    small = np.full(need - 1 + 64, 0xAB, np.uint8)              # (64 guard bytes behind the capacity handed over)
    rc, n, a = call(small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and n == need and a == adler and (small == 0xAB).all()
    exact = np.full(need + 64, 0xAB, np.uint8)
    rc, n, a = call(exact)
    assert rc == _lib.VFSMS_OK and n == need and a == adler and bytes(exact[:need]) == bytes(payload) and (exact[need:] == 0xAB).all()


# ---- the canvas path ------------------------------------------------------------------------------------------------------------------
ROWS, COLS, S = 150, 201, 16


@pytest.fixture(scope="module", params=[1, 3], ids=["gray", "colour"])
def canvas(engine, request):
    ch = request.param
    cv = _canvas(engine, ROWS, COLS, ch, 41 + ch)
    img = engine.canvas_download(cv, ROWS, COLS, ch)                # B G R, holes of zeros
    assert (img == 0).any() and img.any()
    rgb = _bgr(img)
    yield cv, img, ch, rgb, ref.filter_rows(rgb)
    engine.canvas_free(cv)


@pytest.mark.parametrize("band_rows", [16, 32, 64, 4096])
def test_canvas_bands_give_the_files_chunks(engine, canvas, band_rows):
    cv, _img, ch, rgb, f = canvas
    got, adler, rows_in = b"", 1, 0
    for r0, n, payload, a in engine.canvas_encode_png_bands(cv, ROWS, COLS, ch, S, band_rows):
        assert r0 == rows_in and n == min(band_rows, ROWS - r0)
        assert bytes(payload) == ref.device_payload(rgb, S, r0, n, filtered=f), ("band", r0, band_rows)      # the row above r0 is the canvas's
        assert a == ref.band_adler(rgb, r0, n, filtered=f)
        got += bytes(payload)
        adler = ref.adler_combine(adler, a, n * (1 + COLS * ch))
        rows_in += n
    assert rows_in == ROWS and got == ref.device_payload(rgb, S, filtered=f) and adler == ref.band_adler(rgb, filtered=f)
    if band_rows == 4096:
        from PIL import Image
        data = ref.head(ROWS, COLS, ch) + got + ref.tail(adler)
        assert data == ref.encode(rgb, S) and np.array_equal(np.asarray(Image.open(io.BytesIO(data))), rgb)


def test_canvas_band_contract_capacity_and_a_tile_walk_in_progress(engine, canvas):
    cv, img, ch, rgb, f = canvas
    out = np.empty(1 << 20, np.uint8)

    def call(row0, nrows, segment_rows=S, handle=None, out=out):
        return engine.canvas_encode_png_rows(cv if handle is None else handle, row0, nrows, segment_rows, out)
    for what, kw in (("row0 no multiple of segment_rows", dict(row0=8, nrows=16)), ("nrows no multiple of segment_rows", dict(row0=0, nrows=24)),
                     ("rows beyond the canvas", dict(row0=144, nrows=16)), ("no rows", dict(row0=0, nrows=0)), ("segment_rows 0", dict(row0=0, nrows=16, segment_rows=0)),
                     ("segment_rows 4097", dict(row0=0, nrows=ROWS, segment_rows=4097)), ("unknown canvas", dict(row0=0, nrows=16, handle=cv + 12345))):
        with pytest.raises(_lib.VfsmsError) as e:
            call(**kw)
        assert "canvas_encode_png_rows" in str(e.value), (what, str(e.value))
    # any band, in any order, and again: the entry keeps no state
    rc, need, a = call(64, 32)
    assert rc == _lib.VFSMS_OK and bytes(out[:need]) == ref.device_payload(rgb, S, 64, 32, filtered=f) and a == ref.band_adler(rgb, 64, 32, filtered=f)
    first = bytes(out[:need])
    small = np.full(need - 1, 0xAB, np.uint8)
    rc, need2, a2 = call(64, 32, out=small)                         # a short buffer: nothing is written, the size and the Adler-32 are known
    assert rc == _lib.VFSMS_ERR_CAPACITY and (need2, a2) == (need, a) and (small == 0xAB).all()
    rc, need3, a3 = call(144, 6)                                    # the short last segment alone
    assert rc == _lib.VFSMS_OK and bytes(out[:need3]) == ref.device_payload(rgb, S, 144, 6, filtered=f)
    rc, need4, a4 = call(64, 32)
    assert rc == _lib.VFSMS_OK and bytes(out[:need4]) == first and a4 == a
    # a deflate-tile walk in progress is not disturbed: its next band is accepted and its bytes are right
    T = 32
    tiles_out, index = np.empty(1 << 21, np.uint8), np.empty((256, 4), np.int64)
    rc, _need, ni = engine.canvas_encode_pyramid_tiles_deflate_rows(cv, 0, 64, 0, T, tiles_out, index)
    assert rc == _lib.VFSMS_OK and ni == 2 * 7
    rc, need5, _a = call(0, ROWS)
    assert rc == _lib.VFSMS_OK and bytes(out[:need5]) == ref.device_payload(rgb, S, filtered=f)
    rc, _need, ni = engine.canvas_encode_pyramid_tiles_deflate_rows(cv, 64, 86, 0, T, tiles_out, index)
    assert rc == _lib.VFSMS_OK and ni == 3 * 7
    want = D.tile_streams(img, T, True)
    for _k, t, o, c in index[:ni].tolist():
        assert bytes(tiles_out[o:o + c]) == want[t], ("tile", t)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_stitcher_writes_a_device_png_end_to_end(engine, tmp_path, colour):
    from PIL import Image
    rng = np.random.default_rng(8)
    proj = tmp_path / "proj"; (proj / "1").mkdir(parents=True)
    yy, xx = np.mgrid[0:128, 0:128]
    for k in range(9):
        base = 128 + 90 * np.sin((xx + 31 * k) / 11.0) * np.cos((yy + 17 * k) / 13.0) + rng.normal(0, 5, (128, 128))
        tile = np.clip(np.stack([base, 0.8 * base + 20, 255 - base], -1) if colour else base, 0, 255).astype(np.uint8)
        Image.fromarray(tile).save(str(proj / "1" / ("t%d.png" % k)))
    old = (isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    outs = {}
    try:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = colour, "fadeInAndFadeOut"
        for enc in ("host", "device"):
            s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.mosaicBandRows = 64
            s.pngEncoder = enc
            # a 3 x 3 serpentine arrangement with overlaps and holes: the same offsets for both runs
            offsets = iter([[4, 106], [-3, 110], [105, 3], [2, -108], [-3, -106], [107, -2], [3, 108], [-2, 105]])
            out = tmp_path / ("o_" + enc)
            s.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, lambda images: (True, next(offsets)), fileExtension="png", outputfileExtension="png")
            assert os.listdir(str(out)) == ["stitching_result_1.png"]
            outs[enc] = open(str(out / "stitching_result_1.png"), "rb").read()
    finally:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = old
    mosaic = np.asarray(Image.open(io.BytesIO(outs["host"])))       # R G B
    assert min(mosaic.shape[:2]) > 300 and (mosaic == 0).any() and mosaic.ndim == (3 if colour else 2)
    assert outs["device"] == ref.encode(mosaic, 16)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(outs["device"]))), mosaic)
