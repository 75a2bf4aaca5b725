"""The JPEG encoder on the device (csrc/jpeg_enc_kernels.hip; Method.jpegEncoder = "device") against its specification,
tests/jpeg_enc_ref.py, byte for byte: the operator, the canvas bands and their contract, the driver, and one band sized to the hardware."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_cases as cases            # noqa: E402
import jpeg_enc_ref as ref                # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402
from imagestitch_amd.synthetic import SyntheticGrid      # noqa: E402

pytestmark = pytest.mark.gpu

CASES = cases.cases()
IDS = ["%s-%dx%d-%s" % (c, h, w, "gray" if ch == 1 else "colour") for c, h, w, ch in CASES]
_REF = {}


def _encode(img, q, R, bgr=True):
    """the specification's file, computed once per (image, settings)"""
    key = (img.shape, img.tobytes(), q, R, bgr)
    if key not in _REF:
        _REF[key] = ref.encode(img, q, R, bgr)
    return _REF[key]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_operator_equals_the_specification(engine, case):
    img = cases.image(*case)
    h, w = img.shape[:2]
    wide = np.zeros((h, w + 5) + img.shape[2:], np.uint8)
    wide[:, 2:2 + w] = img
    view = wide[:, 2:2 + w]                                    # a column slice of a wider array: rows strided
    assert not view.flags.c_contiguous
    for q in cases.QUALITIES:
        for R in (0, 1, 3, 8):
            want = _encode(img, q, R)
            assert bytes(engine.jpeg_encode_device(img, bgr=True, quality=q, restart_mcus=R)) == want, (q, R)
            assert bytes(engine.jpeg_encode_device(view, bgr=True, quality=q, restart_mcus=R)) == want, (q, R, "strided")
            if img.ndim == 3:
                rgb = np.ascontiguousarray(img[:, :, ::-1])
                assert bytes(engine.jpeg_encode_device(rgb, bgr=False, quality=q, restart_mcus=R)) == want, (q, R, "rgb")
                assert _encode(rgb, q, R, False) == want


def test_operator_refusals(engine):
    with pytest.raises(_lib.VfsmsError):
        engine.jpeg_encode_device(np.zeros((16 * 300, 16 * 300, 3), np.uint8), restart_mcus=0)      # 90000 MCUs in one interval
    with pytest.raises(_lib.VfsmsError):
        engine.jpeg_encode_device(np.zeros((16, 16, 3), np.uint8), restart_mcus=65536)
    with pytest.raises(_lib.VfsmsError):
        engine.jpeg_encode_device(np.zeros((8, 65501), np.uint8), restart_mcus=8)
    with pytest.raises(_lib.VfsmsError):
        engine.jpeg_encode_device(np.zeros((8, 8, 2), np.uint8))
    with pytest.raises(_lib.VfsmsError):
        _lib.jpeg_header(8, 8, 4, 95, 0)


@pytest.fixture(scope="module")
def canvases(engine):
    """an 80 x 100 colour canvas and a 40 x 100 gray one, two pasted tiles each and an empty corner (empty -> 0)"""
    rng = np.random.default_rng(11)
    out = {}
    for name, (rows, cols, ch) in {"colour": (80, 100, 3), "gray": (40, 100, 1)}.items():
        cv = engine.canvas_create(rows, cols, ch)
        shape = lambda h, w: (h, w, ch) if ch > 1 else (h, w)
        engine.canvas_paste(cv, rng.integers(0, 256, shape(rows, 60), dtype=np.uint8), 0, 0)
        engine.canvas_paste(cv, rng.integers(0, 256, shape(rows // 2, 40), dtype=np.uint8), 0, 60)
        img = engine.canvas_download(cv, rows, cols, ch)
        assert not img[rows // 2:, 60:].any() and img[:rows // 2].any()
        out[name] = (cv, img)
    yield out
    for cv, _img in out.values():
        engine.canvas_free(cv)


@pytest.mark.parametrize("name,band_rows,R", [("colour", 32, 1), ("colour", 32, 2), ("colour", 16, 7), ("gray", 16, 13), ("gray", 8, 1)])
def test_canvas_bands_are_the_file(engine, canvases, name, band_rows, R):
    cv, img = canvases[name]
    rows, cols = img.shape[:2]
    ch = 1 if img.ndim == 2 else 3
    body = b"".join(bytes(p) for _r0, _n, p in engine.canvas_encode_jpeg_bands(cv, rows, cols, ch, 95, R, band_rows))
    mcu = 16 if ch == 3 else 8
    bands = [ref.scan(img, 95, R, True, r0 // mcu, -(-min(band_rows, rows - r0) // mcu)) for r0 in range(0, rows, band_rows)]
    assert body == b"".join(bands)
    assert _lib.jpeg_header(rows, cols, ch, 95, R) == ref.header(rows, cols, ch, 95, R)
    assert _lib.jpeg_header(rows, cols, ch, 95, R) + body + b"\xFF\xD9" == ref.encode(img, 95, R)


def test_canvas_band_contract_and_capacity(engine, canvases):
    cv, img = canvases["colour"]                               # 7 MCUs per row, 5 MCU rows
    out = np.empty(1 << 20, np.uint8)
    for row0, nrows, R in [(8, 32, 1), (0, 24, 1), (0, 16, 2), (16, 64, 2), (0, 32, 4), (0, 80, 0 + 65536)]:
        with pytest.raises(_lib.VfsmsError):
            engine.canvas_encode_jpeg_rows(cv, row0, nrows, 95, R, out)
    with pytest.raises(_lib.VfsmsError):
        engine.canvas_encode_jpeg_rows(cv, 0, 96, 95, 1, out)                 # beyond the canvas
    rc, need = engine.canvas_encode_jpeg_rows(cv, 32, 48, 95, 2, out)         # 14 MCUs in front; ends at the last row
    assert rc == _lib.VFSMS_OK and bytes(out[:need]) == ref.scan(img, 95, 2, True, 2, 3)
    small = np.full(need - 1, 0xAB, np.uint8)
    rc, need2 = engine.canvas_encode_jpeg_rows(cv, 32, 48, 95, 2, small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and need2 == need and (small == 0xAB).all()
    exact = np.empty(need, np.uint8)
    rc, need3 = engine.canvas_encode_jpeg_rows(cv, 32, 48, 95, 2, exact)
    assert rc == _lib.VFSMS_OK and need3 == need and bytes(exact) == bytes(out[:need])


def test_noise_at_quality_100_grows_the_buffers_not_past_them(engine):
    """the densest stream there is -- more bytes out than pixels in -- through the band generator, whose ring starts small"""
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (64, 2080, 3), dtype=np.uint8)
    cv = engine.canvas_create(64, 2080, 3)
    try:
        engine.canvas_paste(cv, img, 0, 0)
        engine.__dict__.pop("_jpeg_ring", None)                  # (a ring grown by an earlier test would hide the growth)
        body = b"".join(bytes(p) for _r0, _n, p in engine.canvas_encode_jpeg_bands(cv, 64, 2080, 3, 100, 1, 32))
    finally:
        engine.canvas_free(cv)
    assert body == ref.scan(img, 100, 1, True)
    assert len(body) > 64 * 2080 and len(body) // 2 > 1 << 16        # more than a byte per pixel; a band outgrew the ring's first size


def test_band_sized_to_the_hardware(engine):
    """2056 x 2064 colour, one band, R = 8: 129 x 129 = 16641 MCUs = 2081 intervals -- many workgroups of both kernels, a strip that ends
    inside its workgroup (129 = 8 * 16 + 1 MCUs per row), intervals that wrap MCU rows, three steps of the scan, a last wave that is not
    full, and -- in the noise corner -- waves whose output takes several LDS windows.  (Half the 4096 x 2064 the hardware would ask for:
    the numpy specification needs six seconds for that one; every path named here is taken at this size too.)"""
    rows, cols = 2064, 2056
    yy, xx = np.mgrid[0:rows, 0:cols]
    rng = np.random.default_rng(9)
    base = (128 + 90 * np.sin(xx / 37.0) * np.cos(yy / 53.0)).astype(np.float32)
    img = np.clip(np.stack([base, base * 0.8 + 20, 255 - base], -1) + rng.normal(0, 6, (rows, cols, 3)), 0, 255).astype(np.uint8)
    img[:512, :1024] = rng.integers(0, 256, (512, 1024, 3), dtype=np.uint8)          # a dense corner: long intervals next to short ones
    cv = engine.canvas_create(rows, cols, 3)
    try:
        engine.canvas_paste(cv, img, 0, 0)
        out = np.empty(rows * cols * 3 // 2, np.uint8)
        rc, need = engine.canvas_encode_jpeg_rows(cv, 0, rows, 95, 8, out)
    finally:
        engine.canvas_free(cv)
    assert rc == _lib.VFSMS_OK
    assert bytes(out[:need]) == ref.scan(img, 95, 8, True)


def _pillow(path_or_bytes):
    from PIL import Image
    src = io.BytesIO(path_or_bytes) if isinstance(path_or_bytes, bytes) else path_or_bytes
    return np.asarray(Image.open(src))


def test_driver_writes_the_specifications_file(engine, tmp_path):
    """the 3 x 3 synthetic colour grid through imageSetStitchWithMutiple: jpegEncoder = "device" writes encode() of the mosaic, which decodes
    to the pixels of the default run's file, and leaves nothing under the hidden name"""
    from PIL import Image
    g = SyntheticGrid(3, 3, 768, overlap=0.15)
    proj = tmp_path / "demo"; (proj / "1").mkdir(parents=True)
    for k, t in enumerate(g.tiles(threads=2)):
        f = t.astype(np.float32)
        rgb = np.clip(np.stack([0.6 * f + 30, f, 255 - 0.7 * f], -1), 0, 255).astype(np.uint8)
        Image.fromarray(rgb).save(str(proj / "1" / ("1_%02d.jpg" % k)), quality=92)
    names = ("direction", "directIncre", "roiRatio", "isColorMode", "featureMethod", "fuseMethod", "offsetEvaluate")
    old = {n: getattr(isa.Stitcher, n) for n in names}
    files = {}
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.2, True
        isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate = "surf", "fadeInAndFadeOut", 3
        for tag, encoder, ext in (("host", "host", "jpg"), ("device", "device", "jpg"), ("pixels", "host", "npy")):
            st = isa.Stitcher(); st._engine = engine
            assert st.jpegEncoder == "host" and st.jpegQuality == 95
            st.jpegEncoder = encoder
            isa.Stitcher.direction = 1; st.direction = 1
            st.printAndWrite = lambda c: None
            out = tmp_path / ("out_" + tag)
            st.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                         startNum=1, fileExtension="jpg", outputfileExtension=ext)
            assert sorted(os.listdir(str(out))) == ["stitching_result_1." + ext], os.listdir(str(out))        # nothing under the hidden name
            files[tag] = str(out / ("stitching_result_1." + ext))
            R = int(st.jpegRestartMcus)
    finally:
        for n, v in old.items():
            setattr(isa.Stitcher, n, v)
    mosaic = np.load(files["pixels"])
    assert mosaic.ndim == 3 and mosaic.shape[0] > 2 * 768
    with open(files["device"], "rb") as f:
        device = f.read()
    with open(files["host"], "rb") as f:
        host = f.read()
    assert device == ref.encode(mosaic, 95, R, True)
    assert np.array_equal(_lib.jpeg_decode(device, want_planes=True), _lib.jpeg_decode(host, want_planes=True))
    assert np.array_equal(_pillow(device), _pillow(host))


def test_driver_refuses_band_rows_that_break_intervals(engine, tmp_path):
    st = isa.Stitcher(); st._engine = engine
    st.jpegEncoder, st.mosaicBandRows = "device", 4096 + 16
    with pytest.raises(ValueError):
        st.imageSetStitchWithMutiple(str(tmp_path / "none"), str(tmp_path / "out") + os.sep, 1, st.calculateOffsetForFeatureSearchIncre)
    st.jpegEncoder = "gpu"
    with pytest.raises(ValueError):
        st.imageSetStitch(str(tmp_path / "none"), str(tmp_path / "out") + os.sep, 1, st.calculateOffsetForFeatureSearchIncre)
