"""The reduced levels of a mosaic on the device (csrc/pyramid_kernels.hip) against tests/pyramid_ref.py, byte for byte: whole canvases at odd
sizes and past what one LDS region gives, band by band, the entry point's refusals, and a pyramidal TIFF end to end through the Stitcher.
Canvases are pasted from random tiles with holes between them: never-written pixels are 0 and take part in the means."""
import ctypes as C
import os

import numpy as np
import pytest

import imagestitch_amd as isa
import pyramid_ref as PR

pytestmark = pytest.mark.gpu


def _canvas(engine, rows, cols, ch, seed, fill=None):
    """a canvas with random tiles pasted so that holes remain (fill: one value everywhere instead, no holes) -> handle"""
    rng = np.random.default_rng(seed)
    cv = engine.canvas_create(rows, cols, ch)
    if fill is not None:
        engine.canvas_paste(cv, np.full((rows, cols, ch) if ch > 1 else (rows, cols), fill, np.uint8), 0, 0)
        return cv
    th, tw = max(1, (rows * 2) // 5), max(1, (cols * 2) // 5)
    for fy, fx in ((0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (1.0, 1.0), (0.45, 0.5)):           # the four corners and one in the middle
        y0, x0 = int(fy * (rows - th)), int(fx * (cols - tw))
        engine.canvas_paste(cv, rng.integers(0, 256, (th, tw, ch) if ch > 1 else (th, tw), dtype=np.uint8), y0, x0)
    return cv


def _equal(got, want, what):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want), 1):
        assert g.shape == w.shape and g.dtype == np.uint8, (what, k, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert not len(bad), (what, "level", k, len(bad), "first at", bad[0].tolist(), int(g[tuple(bad[0])]), int(w[tuple(bad[0])]))


@pytest.mark.parametrize("rows,cols,ch,levels,fill", [(200, 333, 1, 8, None), (257, 1030, 3, 5, None), (70, 4099, 1, 3, None),
                                                      (1, 1, 1, 2, None), (3, 2, 1, 2, None), (130, 130, 3, 7, 255)])
def test_canvas_pyramid_equals_the_reference(engine, rows, cols, ch, levels, fill):
    cv = _canvas(engine, rows, cols, ch, rows + cols, fill)
    try:
        img = engine.canvas_download(cv, rows, cols, ch)
        if fill is None and rows > 8:
            assert (img == 0).any() and img.any()                # holes and content
        _equal(engine.canvas_pyramid(cv, rows, cols, ch, levels), PR.pyramid_levels(img, levels), (rows, cols, ch))
        _equal(engine.canvas_pyramid(cv, rows, cols, ch, levels), PR.pyramid_levels(img, levels), "again, from the sized scratch")
    finally:
        engine.canvas_free(cv)


def test_bands_with_their_levels(engine):
    rows, cols, ch, levels, band = 1000, 777, 3, 8, 256
    cv = _canvas(engine, rows, cols, ch, 11)
    try:
        img = engine.canvas_download(cv, rows, cols, ch)
        want = PR.pyramid_levels(img, levels)
        _equal(engine.canvas_pyramid(cv, rows, cols, ch, levels), want, "whole")
        for transient in (False, True):
            bands, parts = [], [[] for _ in range(levels)]
            for r0, b, lv in engine.canvas_download_pyramid_bands(cv, rows, cols, ch, levels, band, transient=transient):
                assert r0 == sum(x.shape[0] for x in bands) and len(lv) == levels
                bands.append(b.copy())
                for k in range(levels):
                    assert lv[k].shape[0] == PR.band_of_level(r0, b.shape[0], rows, k + 1)[1]
                    parts[k].append(lv[k].copy())
            assert np.array_equal(np.concatenate(bands, 0), img), transient
            _equal([np.concatenate(p, 0) for p in parts], want, ("bands", transient))
        with pytest.raises(ValueError):
            next(engine.canvas_download_pyramid_bands(cv, rows, cols, ch, levels, 128))
    finally:
        engine.canvas_free(cv)


def test_the_entry_point_refuses_bad_bands(engine):
    rows, cols, ch = 100, 60, 1
    cv = _canvas(engine, rows, cols, ch, 5)
    try:
        img = engine.canvas_download(cv, rows, cols, ch)
        band, lv = np.empty((rows, cols), np.uint8), np.empty(rows * cols, np.uint8)
        fn = engine.lib.vfsms_canvas_download_rows_pyramid

        def call(handle, row0, nrows, levels, cap=lv.size):
            return fn(engine.ctx, C.c_int64(handle), row0, nrows, levels, band.ctypes.data_as(C.c_void_p), lv.ctypes.data_as(C.c_void_p), C.c_size_t(cap))
        for what, args in (("levels 0", (cv, 0, rows, 0)), ("levels 11", (cv, 0, rows, 11)), ("row0 not a multiple", (cv, 4, 96, 3)),
                           ("nrows not a multiple", (cv, 0, 20, 3)), ("cap too small", (cv, 0, rows, 2, 50 * 30 + 25 * 15 - 1)),
                           ("unknown canvas", (cv + 12345, 0, rows, 2)), ("rows beyond the canvas", (cv, 96, 8, 2))):
            assert call(*args) == isa._lib.VFSMS_ERR_BAD_ARG, what
            buf = C.create_string_buffer(512)
            engine.lib.vfsms_last_error(buf, 512)
            assert b"canvas_download_rows_pyramid" in buf.value, (what, buf.value)
        assert call(cv, 96, 4, 2, 50 * 30 + 25 * 15) == 0        # a valid call afterwards: the last band, not a multiple of 4 rows
        assert np.array_equal(band.reshape(-1)[:4 * cols].reshape(4, cols), img[96:])
        want = PR.pyramid_levels(img, 2)
        assert np.array_equal(lv[:2 * 30].reshape(2, 30), want[0][48:]) and np.array_equal(lv[60:60 + 15].reshape(1, 15), want[1][24:])
    finally:
        engine.canvas_free(cv)


def test_stitcher_writes_a_pyramidal_tiff_end_to_end(engine, tmp_path):
    from PIL import Image
    from test_pyramid_host import check_file
    rng = np.random.default_rng(8)
    proj = tmp_path / "proj"; (proj / "1").mkdir(parents=True)
    for k in range(4):
        Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(str(proj / "1" / ("t%d.png" % k)))
    old = (isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    outs = {}
    try:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = True, "fadeInAndFadeOut"
        for pyramid in (False, True):
            s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.mosaicBandRows = 64
            s.outputPyramid = pyramid; s.pyramidTile = 64
            offsets = iter([[8, 200], [200, -190], [-6, 200]])   # a 2 x 2 arrangement with overlaps and holes
            out = tmp_path / ("o%d" % pyramid)
            s.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, lambda images: (True, next(offsets)), fileExtension="png", outputfileExtension="tif")
            assert os.listdir(str(out)) == ["stitching_result_1.tif"]
            outs[pyramid] = str(out / "stitching_result_1.tif")
    finally:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = old
    mosaic = np.asarray(Image.open(outs[False]))               # R G B
    assert mosaic.ndim == 3 and min(mosaic.shape[:2]) > 400 and (mosaic == 0).all(axis=2).any()
    K = PR.default_levels(mosaic.shape[0], mosaic.shape[1], 64)
    assert K == 3
    check_file(outs[True], np.ascontiguousarray(mosaic[:, :, ::-1]), K, 64, big=False)
