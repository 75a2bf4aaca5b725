"""Method.exposureCompensation on the device against tests/exposure_ref.py, exactly (np.array_equal): the overlap statistic at ragged
shapes, every kind of offset and three bands, sums beyond 32 bits, wrapped strided tiles, the in-place apply, the refusals of the C ABI,
and the compensation through Stitcher.getStitchByOffset alone, behind the shading correction and behind a global adjustment."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import imagestitch_amd as isa

import exposure_ref as ER
import shading_ref as SH
from test_exposure_host import SERPENTINE, exposure_grid
from test_shading_gpu import _free, _stitch, _tile_bytes, _upload

pytestmark = pytest.mark.gpu

BANDS = [(0, 255), (1, 254), (100, 100)]


# ---- the statistic -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stat_tiles():
    """(5, 7), (33, 130, 3) -- rows of 390 bytes -- and (70, 257), each as random bytes and as a {0, 17, 255} ties tile, and a second
    colour shape (20, 141, 3); shared: do not write to the arrays"""
    rng = np.random.default_rng(41)
    tiles = []
    for shape in ((5, 7), (33, 130, 3), (70, 257)):
        tiles.append(rng.integers(0, 256, shape).astype(np.uint8))
        tiles.append(rng.choice(np.array([0, 17, 255], np.uint8), shape))
    tiles.append(rng.integers(0, 256, (20, 141, 3)).astype(np.uint8))
    tiles[2][4:9, 10:60] = 100                               # something for the band (100, 100) to find: the rows meet at dx = 0 ...
    tiles[6][4:9, 30:90] = 100                               # ... and at small shifts
    tiles[4][10:30, 100:200] = 100
    for t in tiles:
        t.setflags(write=False)
    return tiles


def stat_jobs():
    """(a, b, dx, dy) over indices into stat_tiles(): 70 jobs"""
    jobs = []
    for a, b in ((0, 1), (2, 3), (4, 5)):
        h, w = stat_tiles()[a].shape[:2]
        for dx, dy in ((0, 0), (2, 3), (2, -3), (-2, 3), (-2, -3), (0, 3), (0, -3), (2, 0), (-2, 0),      # every sign combination
                       (h - 1, 0), (1 - h, 1), (0, w - 1), (-1, 1 - w), (h - 1, w - 1), (1 - h, 1 - w),    # one row, one column, one pixel
                       (h, 0), (0, -w), (-h, w),                                                         # empty
                       (1000000, -1000000), (2147483647, -2147483648)):                                  # far outside
            jobs.append((a, b, dx, dy))
    jobs += [(2, 6, 0, 0), (6, 2, 0, 0), (2, 6, 5, -20), (6, 2, -5, 20), (2, 6, -3, 11), (6, 2, 19, 129), (2, 6, 32, -140)]   # two shapes
    jobs += [(4, 4, 3, -4), (4, 4, 0, 0), (0, 0, 0, 0)]                                                   # A is B
    return jobs


@pytest.mark.parametrize("band", BANDS)
def test_statistics_equal_the_reference(engine, band):
    tiles, jobs = stat_tiles(), stat_jobs()
    want = np.array([ER.stats(tiles[a], tiles[b], dx, dy, *band) for a, b, dx, dy in jobs], np.int64)
    assert len(jobs) >= 60 and (want[:, 0] > 0).sum() >= (40 if band != (100, 100) else 5) and (want[:, 0] == 0).sum() >= 15
    handles = _upload(engine, tiles)
    try:
        got = engine.overlap_stats_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in jobs], *band)
        assert got.dtype == np.int64 and got.shape == want.shape
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert np.array_equal(got, want), [(jobs[k], got[k].tolist(), want[k].tolist()) for k in bad[:5]]
        one = engine.overlap_stats_batch([(handles[4], handles[5], 2, -3)], *band)                        # a batch of one
        assert np.array_equal(one[0], want[jobs.index((4, 5, 2, -3))])
        assert engine.overlap_stats_batch([], *band).shape == (0, 3)                                      # n = 0 is fine
    finally:
        _free(engine, handles)


def test_the_sums_leave_32_bits(engine):
    """all-255 tiles of 2400 x 2400 x 3 at (0, 0): Sa = Sb = 4 406 400 000 > 2^32; a lane of the kernel still sums in 32 bits"""
    t = np.full((2400, 2400, 3), 255, np.uint8)
    handles = _upload(engine, [t, t])
    try:
        got = engine.overlap_stats_batch([(handles[0], handles[1], 0, 0), (handles[0], handles[1], -1, 2)], 0, 255)
    finally:
        _free(engine, handles)
    assert got[0].tolist() == [17280000, 4406400000, 4406400000] and 4406400000 > 2 ** 32
    n = 2399 * 2398 * 3
    assert got[1].tolist() == [n, 255 * n, 255 * n]


def _hip():
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    return C.CDLL(loaded[0] if loaded else "libamdhip64.so")            # the HIP runtime the library itself runs on


def test_wrapped_strided_tiles(engine):
    """device rows 41 bytes apart for w = 37, behind an odd base address (the recipe of test_shading_gpu.py::test_profile_of_strided_tiles):
    the statistic reads them where they are; the apply refuses them and leaves the memory alone"""
    rng = np.random.default_rng(11)
    h, w, stride = 12, 37, 41
    tiles = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(5)]
    padded = rng.integers(0, 256, (5, h, stride)).astype(np.uint8)       # the padding is not zero: it must stay out of the sums
    for k, t in enumerate(tiles):
        padded[k, :, :w] = t
    jobs = [(0, 1, 0, 0), (1, 2, 3, -5), (2, 3, -4, 6), (3, 4, 11, 36), (4, 0, -11, -36), (0, 4, 0, 21), (2, 2, 1, 1), (1, 3, 12, 0)]
    hip = _hip()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(padded.size + 1)) == 0
    handles = []
    try:
        assert hip.hipMemcpy(C.c_void_p(buf.value + 1), padded.ctypes.data_as(C.c_void_p), C.c_size_t(padded.size), 1) == 0
        handles = [engine.tile_wrap(buf.value + 1 + k * h * stride, h, w, stride) for k in range(5)]
        own = engine.tile_upload(tiles[0])
        handles.append(own)
        for band in BANDS[:2]:
            want = np.array([ER.stats(tiles[a], tiles[b], dx, dy, *band) for a, b, dx, dy in jobs], np.int64)
            got = engine.overlap_stats_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in jobs], *band)
            assert np.array_equal(got, want), band
        with pytest.raises(isa.VfsmsError):
            engine.exposure_apply([own, handles[1]], [5000, 5000])
        back = np.empty_like(padded)
        engine.sync()
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(buf.value + 1), C.c_size_t(padded.size), 2) == 0
        assert np.array_equal(back, padded) and np.array_equal(_tile_bytes(engine, own, (h, w)), tiles[0])
    finally:
        _free(engine, handles)
        engine.sync()
        hip.hipFree(buf)


# ---- the apply -----------------------------------------------------------------------------------------------------------------------------
GAINS = [0, 1, 4095, 4096, 4097, 9000, 65535]


def test_apply_in_place(engine):
    """seven gains on each of the three shapes, all 21 tiles in ONE call"""
    rng = np.random.default_rng(17)
    tiles, gains = [], []
    for shape in ((5, 7), (33, 130, 3), (70, 257)):
        for q in GAINS:
            tiles.append(rng.integers(0, 256, shape).astype(np.uint8)); gains.append(q)
    want = [ER.apply(t, q) for t, q in zip(tiles, gains)]
    assert (want[6] == 255).any() and not want[0].any()      # a gain of 65535 saturates, a gain of 0 clears
    handles = _upload(engine, tiles)
    try:
        engine.profile_enable(True); engine.profile_read(reset=True)
        engine.exposure_apply(handles, gains)
        engine.overlap_stats_batch([(handles[0], handles[1], 0, 0)], 0, 255)
        stages = engine.profile_read(reset=True)
        engine.profile_enable(False)
        assert stages["exposure"][1] == 2, stages            # both kernels run under the profiler stage "exposure"
        for k, h in enumerate(handles):
            got = _tile_bytes(engine, h, tiles[k].shape)
            assert np.array_equal(got, want[k]), (tiles[k].shape, gains[k], int(np.count_nonzero(got != want[k])))
            if gains[k] == 4096:
                assert np.array_equal(got, tiles[k])
        # (the call, what the library says): one fault each, then two at once -- an unknown handle is reported before a tile named twice
        for bad, says in ((lambda: engine.exposure_apply([handles[0], handles[1], handles[0]], [5000, 5000, 5000]), "exposure_apply: a tile is named twice (it would be corrected twice)"),
                          (lambda: engine.exposure_apply([handles[0], 987654321], [5000, 5000]), "exposure_apply: unknown tile handle"),
                          (lambda: engine.exposure_apply([], []), "exposure_apply: 1..4096 tiles and a gain for each"),          # n = 0
                          (lambda: engine.exposure_apply([handles[0], handles[0], 987654321], [5000, 5000, 5000]), "exposure_apply: unknown tile handle")):
            with pytest.raises(isa.VfsmsError, match=re.escape(says)):
                bad()
        with pytest.raises(ValueError):
            engine.exposure_apply(handles[:2], [5000])
        for k in (0, 8, 20):                                  # the refusals changed nothing
            assert np.array_equal(_tile_bytes(engine, handles[k], tiles[k].shape), want[k])
    finally:
        engine.profile_enable(False)
        _free(engine, handles)


def test_abi_refusals(engine):
    rng = np.random.default_rng(2)
    gray = rng.integers(0, 256, (16, 24)).astype(np.uint8)
    colour = rng.integers(0, 256, (16, 24, 3)).astype(np.uint8)
    hg, hc = engine.tile_upload(gray), engine.tile_upload_color(colour)
    try:
        for bad in (lambda: engine.overlap_stats_batch([(hg, hg, 0, 0)], 101, 100),        # lo > hi
                    lambda: engine.overlap_stats_batch([(hg, hg, 0, 0)], 0, 256),
                    lambda: engine.overlap_stats_batch([(hg, hg, 0, 0)], -1, 255),
                    lambda: engine.overlap_stats_batch([(hg, 987654321, 0, 0)], 0, 255),   # an unknown handle
                    lambda: engine.overlap_stats_batch([(987654321, hg, 0, 0)], 0, 255),
                    lambda: engine.overlap_stats_batch([(hg, hc, 0, 0)], 0, 255),          # gray against colour
                    lambda: engine.overlap_stats_batch([(hg, hg, 0, 0), (hc, hg, 0, 0)], 0, 255)):
            with pytest.raises(isa.VfsmsError):
                bad()
        assert engine.overlap_stats_batch([(hc, hc, 0, 0)], 0, 255)[0].tolist() == list(ER.stats(colour, colour, 0, 0, 0, 255))
    finally:
        _free(engine, [hg, hc])


# ---- through Stitcher ------------------------------------------------------------------------------------------------------------------------
LOG = "  exposure compensation: "


@pytest.mark.parametrize("color", [False, True])
def test_stitcher_compensates_the_mosaic(engine, tmp_path, color):
    """"gain" over the 3 x 3 grid == "none" over the same tiles corrected beforehand by the reference"""
    tiles, _ = exposure_grid(color)
    got, msgs = _stitch(engine, tmp_path, tiles, SERPENTINE, color, "gain", exposureCompensation="gain", exposureMinPixels=256)
    want, _ = _stitch(engine, tmp_path, ER.correct(tiles, SERPENTINE, 1, 254, 256, 2.0), SERPENTINE, color, "ref")
    none, none_msgs = _stitch(engine, tmp_path, tiles, SERPENTINE, color, "none", exposureCompensation="none")
    raw, raw_msgs = _stitch(engine, tmp_path, tiles, SERPENTINE, color, "raw")
    assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert np.array_equal(none, raw) and len(none_msgs) == len(raw_msgs) and not np.array_equal(got, raw)
    g = ER.gains(tiles, SERPENTINE, 1, 254, 256, 2.0)[1]
    assert [m for m in msgs if m.startswith(LOG)] == [LOG + "20 edges, gains %.4f .. %.4f" % (g.min(), g.max())]
    assert not [m for m in raw_msgs + none_msgs if "exposure" in m]
    with pytest.raises(ValueError):
        _stitch(engine, tmp_path, tiles, SERPENTINE, color, "bad", exposureCompensation="histogram")


def test_shading_first_then_exposure(engine, tmp_path):
    tiles, _ = exposure_grid(False)
    got, msgs = _stitch(engine, tmp_path, tiles, SERPENTINE, False, "both", shadingCorrection="estimate", shadingMinTiles=2,
                        exposureCompensation="gain", exposureMinPixels=256)
    shaded = SH.correct(tiles, 50, 32)
    want, _ = _stitch(engine, tmp_path, ER.correct(shaded, SERPENTINE, 1, 254, 256, 2.0), SERPENTINE, False, "bref")
    other = SH.correct(ER.correct(tiles, SERPENTINE, 1, 254, 256, 2.0), 50, 32)              # the other order gives other bytes
    assert any(not np.array_equal(a, b) for a, b in zip(other, ER.correct(shaded, SERPENTINE, 1, 254, 256, 2.0)))
    assert np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert len([m for m in msgs if m.startswith(LOG)]) == 1


def test_exposure_uses_the_adjusted_offsets(engine, tmp_path):
    """flowStitch with one vote 2 px wrong, globalAdjust = "ncc" and "gain": the mosaic of the TRUE offsets over tiles the reference
    compensated under the true offsets (the correlation does not see a gain, so the adjustment recovers the truth as it does without)"""
    from PIL import Image
    import adjust_cases as AC
    from test_adjust_gpu import ScriptedStitcher
    from test_exposure_host import TRUTH
    plain, true = AC.grid("g7")
    tiles = [np.clip(np.rint(t.astype(np.float64) * g), 0, 255).astype(np.uint8) for t, g in zip(plain, TRUTH)]
    wrong = AC.perturbed(true, {4: (2, 0)})
    q_true = ER.gains(tiles, true, 1, 254, AC.MIN_PIXELS, 2.0)[0]
    assert not np.array_equal(q_true, ER.gains(tiles, wrong, 1, 254, AC.MIN_PIXELS, 2.0)[0])      # a condition on the case: the offsets matter

    def mosaic(images, offsets, tag, **settings):
        files = []
        for k, t in enumerate(images):
            files.append(os.path.join(str(tmp_path), "%s%02d.png" % (tag, k)))
            Image.fromarray(t).save(files[-1])
        st = ScriptedStitcher(offsets)
        st._engine = engine
        st.fuseMethod = "fadeInAndFadeOut"
        st.adjustMinPixels = st.exposureMinPixels = AC.MIN_PIXELS
        for k, v in settings.items():
            setattr(st, k, v)
        (status, _end), img = st.flowStitch(files, st.scripted)
        assert status
        return st, np.asarray(img)
    st, got = mosaic(tiles, wrong, "w", globalAdjust="ncc", exposureCompensation="gain")
    _, want = mosaic([ER.apply(t, q) for t, q in zip(tiles, q_true)], true, "t")
    assert "  The adjusted offsetList is " + str(true) in st.lines
    assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert st.exposureReport["edges"] == len(ER.overlap_edges([t.shape for t in tiles], true, AC.MIN_PIXELS))
