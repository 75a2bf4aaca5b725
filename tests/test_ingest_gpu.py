"""csrc/ingest_kernels.hip against tests/ingest_ref.py and Pillow's two decodes, byte for byte: k_ingest_split on planes handed over
directly (the whole Y Cb Cr cube, every tail length, the three source formats) and k_ingest_420 on 4:2:0 files whose content drives
the conversion into its clamps, at the widths where the kernel changes its stores and its column block."""
import io

import numpy as np
import pytest

import ingest_ref as R

pytestmark = pytest.mark.gpu


def _tile_bytes(engine, handle, h, w, ch):
    cv = engine.canvas_create(h, w, ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, h, w, ch)
    finally:
        engine.canvas_free(cv)


def _split(engine, src, h, w, stride, fmt, which="both"):
    """tile_fill_pair of one h x w source -> (gray bytes | None, B G R bytes | None)"""
    hg = engine.tile_reserve(h, w) if which != "color" else 0
    hc = engine.tile_reserve_color(h, w, 3) if which != "gray" else 0
    try:
        engine.tile_fill_pair(hg, hc, src.ctypes.data, stride, fmt)
        return (_tile_bytes(engine, hg, h, w, 1) if hg else None), (_tile_bytes(engine, hc, h, w, 3) if hc else None)
    finally:
        for t in (hg, hc):
            if t:
                engine.tile_free(t)


def test_split_ycc24_on_the_whole_cube(engine):
    """All 2^24 (Y, Cb, Cr) triples as one 4096 x 4096 image in a seeded permutation of cube order (a lane's four pixels then meet every
    value of every byte in every position of the quad): the gray tile is Y, the B G R tile the reference's.  G is the one channel that
    depends on all three bytes, so nothing smaller than the cube covers it."""
    n = 1 << 24
    idx = np.random.default_rng(2024).permutation(n).astype(np.uint32)
    ycc = np.empty((n, 3), np.uint8)
    ycc[:, 0] = idx >> 16; ycc[:, 1] = (idx >> 8) & 255; ycc[:, 2] = idx & 255
    want = np.empty((n, 3), np.uint8)
    for k in range(0, n, 1 << 20):
        want[k:k + (1 << 20)] = R.ycc_to_bgr(ycc[k:k + (1 << 20)])
    assert (want == 0).any(0).all() and (want == 255).any(0).all()
    gray, bgr = _split(engine, ycc, 4096, 4096, 4096 * 3, engine.SRC_YCC24)
    assert np.array_equal(gray.reshape(-1), ycc[:, 0])
    bad = np.flatnonzero((bgr.reshape(-1, 3) != want).any(1))
    assert bad.size == 0, (bad.size, ycc[bad[:4]].tolist(), bgr.reshape(-1, 3)[bad[:4]].tolist(), want[bad[:4]].tolist())


def test_split_yccx32_on_every_chroma_pair(engine):
    """the 4-byte source format: the same conversion, another unpacking.  All 65536 (Cb, Cr) pairs with 16 Y values, permuted, 1024 x 1024;
    the fourth byte is random (Pillow writes 255 there; the kernel must not look at it)"""
    ys = np.array([0, 1, 127, 128, 254, 255, 16, 37, 64, 90, 111, 150, 180, 200, 235, 246], np.uint8)
    rng = np.random.default_rng(7)
    idx = rng.permutation(1 << 20)
    src = np.empty((1 << 20, 4), np.uint8)
    src[:, 0] = ys[idx >> 16]; src[:, 1] = (idx >> 8) & 255; src[:, 2] = idx & 255; src[:, 3] = rng.integers(0, 256, 1 << 20)
    gray, bgr = _split(engine, src, 1024, 1024, 4096, engine.SRC_YCCX32)
    assert np.array_equal(gray.reshape(-1), src[:, 0])
    assert np.array_equal(bgr.reshape(-1, 3), R.ycc_to_bgr(src[:, :3]))


def test_split_gray8_ramp(engine):
    src = np.random.default_rng(8).permutation(np.arange(1024) % 256).astype(np.uint8).reshape(16, 64)
    gray, bgr = _split(engine, src, 16, 64, 64, engine.SRC_GRAY8)
    assert np.array_equal(gray, src)
    assert np.array_equal(bgr, np.repeat(src[:, :, None], 3, 2))
    gray, bgr = _split(engine, src, 16, 64, 64, engine.SRC_GRAY8, "gray")        # a plain copy, no kernel
    assert np.array_equal(gray, src) and bgr is None


TAIL_SHAPES = ((1, 1), (1, 2), (1, 3), (1, 5), (3, 3), (2, 3), (7, 333))


@pytest.mark.parametrize("shape", TAIL_SHAPES, ids=lambda s: "%dx%d" % s)
def test_split_tails_formats_planes_and_strides(engine, shape):
    """image areas with every n % 4 and n < 4 (the byte loop behind the last whole quad), in the three formats, with both tiles, one of
    them, and source rows wider than the image"""
    h, w = shape
    assert {a * b % 4 for a, b in TAIL_SHAPES} == {1, 2, 3} and {a * b for a, b in TAIL_SHAPES} >= {1, 2, 3}     # (n % 4 == 0: the cube)
    rng = np.random.default_rng([h, w])
    for fmt, spx in ((engine.SRC_GRAY8, 1), (engine.SRC_YCC24, 3), (engine.SRC_YCCX32, 4)):
        px = rng.integers(0, 256, (h, w, spx), dtype=np.uint8)
        want_gray = px[:, :, 0]
        want_bgr = R.ycc_to_bgr(px[:, :, :3]) if spx > 1 else np.repeat(px, 3, 2)
        wide = rng.integers(0, 256, (h, w * spx + 7), dtype=np.uint8); wide[:, :w * spx] = px.reshape(h, w * spx)
        for src, stride in ((np.ascontiguousarray(px), w * spx), (wide, w * spx + 7)):
            for which in ("both", "gray", "color"):
                gray, bgr = _split(engine, src, h, w, stride, fmt, which)
                assert gray is None or np.array_equal(gray, want_gray), (shape, fmt, stride, which)
                assert bgr is None or np.array_equal(bgr, want_bgr), (shape, fmt, stride, which)


# ---- k_ingest_420 ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def jpeg_cases(tmp_path_factory):
    """[(name, w, h, bytes, Pillow's grayscale decode, Pillow's B G R decode)] of ingest_ref.jpeg_set(), decoded once for the module"""
    from imagestitch_amd import stitcher as ST
    d = tmp_path_factory.mktemp("jpeg420")
    out = []
    for name, w, h, data in R.jpeg_set():
        p = str(d / (name + ".jpg"))
        with open(p, "wb") as f:
            f.write(data)
        out.append((name, w, h, data, ST._imread(p, False), ST._imread(p, True)))
    return out


def _jpeg_or_skip(engine):
    from PIL import Image
    hg0, hc0 = engine.tile_reserve(8, 8), engine.tile_reserve_color(8, 8, 3)
    probe = io.BytesIO(); Image.fromarray(np.zeros((8, 8, 3), np.uint8)).save(probe, "JPEG")
    ok = engine.tile_fill_jpeg(hg0, hc0, probe.getvalue())
    if not ok:
        engine.tile_fill_pair(hg0, hc0, None, 0, 0)
    engine.tile_free(hg0); engine.tile_free(hc0)
    if not ok:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")


def test_jpeg_reference_reaches_the_clamps(jpeg_cases):
    """a condition on the REFERENCE alone, before any device call: over the set at least a quarter of the pixels have a channel at 0 or
    255, and Cb and Cr each reach <= 8 and >= 247 (measured: 49 %, both 0..255)"""
    for name, w, h, data, gray, bgr in jpeg_cases:
        assert gray.shape == (h, w) and bgr.shape == (h, w, 3), name
    share, lo, hi = R.clamp_statistics([(c[5], R.decode_ycc(c[3])) for c in jpeg_cases])
    print("jpeg set: %d files, saturated share %.3f, Cb %d..%d, Cr %d..%d" % (len(jpeg_cases), share, lo[0], hi[0], lo[1], hi[1]))
    assert share >= 0.25 and (lo <= 8).all() and (hi >= 247).all(), (share, lo, hi)


def test_tile_fill_jpeg_420_equals_the_two_decodes(engine, jpeg_cases):
    """every file of the set through vfsms_tile_fill_jpeg -- both tiles, the gray tile alone, the colour tile alone -- equals Pillow's
    grayscale and colour decodes of the same bytes: widths 4 .. 1028 (dword and byte stores, the second column block, the file of two
    chroma columns that libjpeg replicates), h = 1 and w = 3, a progressive file"""
    test_jpeg_reference_reaches_the_clamps(jpeg_cases)
    _jpeg_or_skip(engine)
    assert sorted({c[1] for c in jpeg_cases[:36]}) == sorted(R.JPEG_WIDTHS) and len(jpeg_cases) == 39
    for name, w, h, data, want_gray, want_bgr in jpeg_cases:
        for which in ("both", "gray", "color"):
            hg = engine.tile_reserve(h, w) if which != "color" else 0
            hc = engine.tile_reserve_color(h, w, 3) if which != "gray" else 0
            try:
                assert engine.tile_fill_jpeg(hg, hc, data), (name, which)
                if hg:
                    assert np.array_equal(_tile_bytes(engine, hg, h, w, 1), want_gray), (name, which, "gray")
                if hc:
                    got = _tile_bytes(engine, hc, h, w, 3)
                    assert np.array_equal(got, want_bgr), (name, which, "colour", int((got != want_bgr).any(-1).sum()))
            finally:
                for t in (hg, hc):
                    if t:
                        engine.tile_free(t)
