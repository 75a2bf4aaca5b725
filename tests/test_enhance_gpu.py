"""csrc/enhance_kernels.hip against tests/enhance_ref.py (OpenCV 3.3.1's equalizeHist / CLAHE restated in numpy), byte for byte: the
packed single-image entry on the shared case table, the batched path that enhances strided ROI strips of resident tiles inside a fused
SURF batch, and the (mode, clip, grid) argument check of every entry point that takes them."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid
import enhance_ref as R

pytestmark = pytest.mark.gpu

VfsmsError = isa._lib.VfsmsError


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_enhance_equals_the_reference_on_the_table(engine, shape):
    """grids larger than the image, sides of length 1, a side that divides the grid beside one that does not (it still grows by a whole
    grid), rows past one 256-lane block, clip limits that floor to 1 -- 27 cases per shape"""
    for content in R.CONTENTS:
        img = R.image(shape, content)
        assert np.array_equal(engine.enhance(img, 1), R.equalize_hist(img)), (shape, content, "equalizeHist")
        for clip, grid in R.CLAHE_PARAMS:
            got, want = engine.enhance(img, 2, clip, grid), R.clahe(img, clip, grid)
            assert np.array_equal(got, want), (shape, content, clip, grid, int((got != want).sum()))


# ---- the batched, strided path -----------------------------------------------------------------------------------------------------------------
MODES = ((1, 0.0, 0), (2, 20.0, 5))


@pytest.fixture(scope="module")
def strip_batch():
    """the tiles of a 2 x 2 serpentine and ONE batch over its three pairs: the ROI strips of the four directions at ROI ratios 0.2 and 0.4
    (64 x 320, 128 x 320, 320 x 64 and 320 x 128 strips at column origins 0, 192 and 256 of rows 320 bytes apart), and per pair one
    rectangle of odd size at odd row and column origins -> (tiles, [(pair, (ay0, ax0, by0, bx0, h, w))])"""
    g = SyntheticGrid(2, 2, 320)
    tiles = g.tiles(threads=1)
    rects = []
    for k in range(3):
        A, B = tiles[k], tiles[k + 1]
        for d in (1, 2, 3, 4):
            for ratio in (0.2, 0.4):
                ra = isa.roi_rect(A.shape, d, "first", ratio); rb = isa.roi_rect(B.shape, d, "second", ratio)
                assert ra[2:] == rb[2:]
                rects.append((k, (ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])))
        rects.append((k, ((3, 37, 243, 37, 77, 247), (11, 213, 5, 1, 301, 101), (1, 41, 239, 35, 75, 263))[k]))
    assert len({r[4:] for _k, r in rects}) >= 6 and any(r[1] % 2 and r[5] % 4 for _k, r in rects)
    return tiles, rects


def _enhanced(cache, tiles, k, rect, mode):
    """enhance_ref of one rectangle (y0, x0, h, w) of tile k, computed once per module"""
    key = (k, rect, mode)
    if key not in cache:
        y0, x0, h, w = rect
        strip = np.ascontiguousarray(tiles[k][y0:y0 + h, x0:x0 + w])
        cache[key] = R.equalize_hist(strip) if mode[0] == 1 else R.clahe(strip, mode[1], mode[2])
    return cache[key]


@pytest.fixture(scope="module")
def ref_cache():
    return {}


def test_batched_attempts_on_strided_strips_equal_attempts_on_reference_strips(engine, strip_batch, ref_cache):
    """attempt_surf_batch_enhanced enhances every distinct strip where it lies in its tile (stride 320, any origin), all strips of a batch
    in three launches whose grid is cut from the largest strip.  Its rows -- all eight ints, no offset verifier -- must be the rows of
    attempt_surf_batch on tiles that ARE the strips as enhance_ref enhances them."""
    tiles, rects = strip_batch
    engine.set_offset_verifier("none")
    hs = [engine.tile_upload(t) for t in tiles]
    made = []
    try:
        jobs = [(hs[k], hs[k + 1]) + r for k, r in rects]
        plain = engine.attempt_surf_batch(jobs)
        assert (plain[:, 0] == 1).any(), plain[:, :4].tolist()              # the batch holds an accepted row (the true direction of a pair)
        assert (plain[:, 4] > 0).all() and (plain[:, 5] > 0).all()          # ... and no strip without keypoints
        for mode in MODES:
            got = engine.attempt_surf_batch_enhanced(jobs, None, 0.75, 3, mode)
            ref_jobs, up = [], {}
            for k, (ay0, ax0, by0, bx0, h, w) in rects:
                pair = []
                for tk, rect in ((k, (ay0, ax0, h, w)), (k + 1, (by0, bx0, h, w))):
                    if (tk, rect) not in up:
                        up[(tk, rect)] = engine.tile_upload(_enhanced(ref_cache, tiles, tk, rect, mode)); made.append(up[(tk, rect)])
                    pair.append(up[(tk, rect)])
                ref_jobs.append((pair[0], pair[1], 0, 0, 0, 0, h, w))
            want = engine.attempt_surf_batch(ref_jobs)
            assert want.shape == got.shape == (len(rects), 8)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, (mode, [(rects[b], got[b].tolist(), want[b].tolist()) for b in bad[:4]])
            assert (want[:, 0] == 1).any() and not np.array_equal(want, plain)       # the enhancement took part in the result
            for t in made:
                engine.tile_free(t)
            del made[:]
    finally:
        for t in hs + made:
            engine.tile_free(t)


def test_batched_whole_tile_features_equal_features_of_reference_tiles(engine, strip_batch, ref_cache):
    """features_surf_batch with enhancement: the keypoint counts of the four tiles enhanced on the device are the counts of the tiles
    enhance_ref enhanced, and so are the keypoints and descriptors"""
    tiles, _rects = strip_batch
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        for mode in MODES:
            he = [engine.tile_upload(_enhanced(ref_cache, tiles, k, (0, 0) + t.shape, mode)) for k, t in enumerate(tiles)]
            fg, ng = engine.features_surf_batch(hs, None, mode)
            fw, nw = engine.features_surf_batch(he)
            try:
                assert ng == nw and min(nw) > 0, (mode, ng, nw)
                for a, b, n in zip(fg, fw, nw):
                    (ka, da), (kb, db) = engine.features_download(a, n), engine.features_download(b, n)
                    assert np.array_equal(ka, kb) and np.array_equal(da, db), mode
            finally:
                for f in fg + fw:
                    if f:
                        engine.features_free(f)
                for t in he:
                    engine.tile_free(t)
    finally:
        for t in hs:
            engine.tile_free(t)


# ---- arguments -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", (0, -1, 65, 10 ** 6))
def test_clahe_grid_outside_1_to_64_is_refused_by_every_entry_point(engine, grid):
    """a CLAHE grid the library cannot take is VFSMS_ERR_BAD_ARG from the entry point, before any size is computed from it (w % 0 is a
    dead process, grid * grid an int overflow); the engine then goes on as if nothing had happened"""
    img = R.image((64, 80), "uniform")
    tile = R.image((100, 250), "lowcontrast")
    h = engine.tile_upload(tile)
    try:
        job = [(h, h, 0, 0, 50, 0, 50, 250)]
        with pytest.raises(VfsmsError):
            engine.enhance(img, 2, 20.0, grid)
        assert np.array_equal(engine.enhance(img, 2, 20.0, 5), R.clahe(img, 20.0, 5))
        with pytest.raises(VfsmsError):
            engine.attempt_surf_batch_enhanced(job, None, 0.75, 3, (2, 20.0, grid))
        with pytest.raises(VfsmsError):
            engine.features_surf_batch([h], None, (2, 20.0, grid))
        with pytest.raises(VfsmsError):
            engine.features_surf(h, (0, 0, 100, 250), None, (2, 20.0, grid))
        assert np.array_equal(engine.enhance(tile, 2, 3.5, 7), R.clahe(tile, 3.5, 7))
        # equalizeHist does not look at the grid: the Stitcher passes (1, 0, 0)
        assert np.array_equal(engine.enhance(img, 1, 0.0, grid), R.equalize_hist(img))
        row = engine.attempt_surf_batch_enhanced(job, None, 0.75, 3, (1, 0.0, grid))
        assert row.shape == (1, 8)
        feats, counts = engine.features_surf_batch([h], None, (1, 0.0, grid))
        for f in feats:
            if f:
                engine.features_free(f)
    finally:
        engine.tile_free(h)
