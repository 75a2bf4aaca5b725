"""Method.shadingCorrection on the device against tests/shading_ref.py, exactly (np.array_equal at every stage): the profile at every
tile count where the selection kernel changes path, the smoothed field and the gain at radii beyond the tile, the in-place apply, the
refusals of the C ABI, and the correction through Stitcher.getStitchByOffset and behind an untouched registration."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imagestitch_amd as isa

import shading_ref as SH

pytestmark = pytest.mark.gpu

# the selection kernel stages up to this many tiles in LDS and re-reads the stack from global memory above (SHADE_LDS_MAX_N in
# csrc/shading_kernels.hip, DESIGN.md "Shading correction"): one N on each side
LDS_MAX_N = 320


def _upload(engine, tiles):
    return [engine.tile_upload_color(t) if t.ndim == 3 else engine.tile_upload(t) for t in tiles]


def _free(engine, handles):
    for h in handles:
        engine.tile_free(h)


def _squeeze(shape):
    return shape[:2] if shape[2] == 1 else shape


def _stack(rng, kind, n, shape):
    shape = _squeeze(shape)
    if kind == "random":
        return [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(n)]
    if kind == "ties":
        return [rng.choice(np.array([0, 17, 255], np.uint8), shape) for _ in range(n)]
    one = rng.integers(0, 256, shape).astype(np.uint8)
    return [one.copy() for _ in range(n)]


def _check_profiles(engine, tiles, counts, tag):
    handles = _upload(engine, tiles)
    try:
        for n in counts:
            for pct in (0, 37, 50, 100):
                f = engine.shading_estimate(handles[:n], pct, 1)
                try:
                    _g, _q, prof = engine.shading_download(f, with_profile=True)
                finally:
                    engine.shading_free(f)
                want = SH.profile(tiles[:n], pct)
                assert prof.dtype == np.uint8 and prof.shape == want.shape, (tag, n, pct)
                assert np.array_equal(prof, want), (tag, n, pct, int(np.count_nonzero(prof != want)))
    finally:
        _free(engine, handles)


@pytest.mark.parametrize("kind", ["random", "ties", "equal"])
@pytest.mark.parametrize("shape", [(5, 7, 1), (33, 130, 3), (70, 257, 1)])
def test_profile(engine, shape, kind):
    """(33, 130, 3): rows of 390 bytes, no multiple of 4; (70, 257, 1): several waves and a ragged last dword"""
    rng = np.random.default_rng(sum(shape) + len(kind))
    _check_profiles(engine, _stack(rng, kind, 90, shape), (1, 2, 3, 4, 9, 90), (shape, kind))


def test_profile_on_both_sides_of_the_lds_bound(engine):
    rng = np.random.default_rng(5)
    _check_profiles(engine, _stack(rng, "random", LDS_MAX_N + 1, (5, 7, 1)), (LDS_MAX_N, LDS_MAX_N + 1), "bound")
    _check_profiles(engine, _stack(rng, "ties", LDS_MAX_N + 1, (9, 13, 3)), (LDS_MAX_N, LDS_MAX_N + 1), "bound, ties")
    _check_profiles(engine, _stack(rng, "random", 200, (64, 80, 1)), (200,), "N = 200")


def test_profile_of_strided_tiles(engine):
    """tile_upload packs the rows it is given (vfsms_tile_upload copies w bytes per row into a dense buffer), so a non-contiguous view
    arrives with stride w: checked first.  Row strides other than w reach the kernel only through tile_wrap: device rows 41 bytes apart
    for w = 37, behind an odd base address, so neither the stride nor the alignment of the dense path holds"""
    rng = np.random.default_rng(11)
    big = [rng.integers(0, 256, (12, 80)).astype(np.uint8) for _ in range(5)]
    views = [b[:, 3:40] for b in big]
    _check_profiles(engine, views, (5,), "views")
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")            # the HIP runtime the library itself runs on
    h, w, stride = 12, 37, 41
    tiles = [np.ascontiguousarray(v) for v in views]
    padded = np.zeros((5, h, stride), np.uint8)
    for k, t in enumerate(tiles):
        padded[k, :, :w] = t
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(padded.size + 1)) == 0
    handles = []
    try:
        assert hip.hipMemcpy(C.c_void_p(buf.value + 1), padded.ctypes.data_as(C.c_void_p), C.c_size_t(padded.size), 1) == 0
        handles = [engine.tile_wrap(buf.value + 1 + k * h * stride, h, w, stride) for k in range(5)]
        for pct in (0, 37, 50, 100):
            f = engine.shading_estimate(handles, pct, 2)
            try:
                got = engine.shading_download(f, with_profile=True)
            finally:
                engine.shading_free(f)
            want = SH.estimate(tiles, pct, 2)
            for a, b in zip(got, want):
                assert np.array_equal(a, b), pct
    finally:
        _free(engine, handles)
        engine.sync()
        hip.hipFree(buf)


# ---- smooth and gain ---------------------------------------------------------------------------------------------------------------
def _check_field(engine, tiles, R, pct=50):
    handles = _upload(engine, tiles)
    try:
        f = engine.shading_estimate(handles, pct, R)
        try:
            gain, q8, prof = engine.shading_download(f, with_profile=True)
            only = engine.shading_download(f)
        finally:
            engine.shading_free(f)
    finally:
        _free(engine, handles)
    wg, wq, wp = SH.estimate(tiles, pct, R)
    assert np.array_equal(prof, wp), R
    assert q8.dtype == np.uint16 and np.array_equal(q8, wq), (R, int(np.count_nonzero(q8 != wq)))
    assert gain.dtype == np.uint16 and np.array_equal(gain, wg), (R, int(np.count_nonzero(gain != wg)))
    assert np.array_equal(only, gain)
    return gain, q8


@pytest.mark.parametrize("R", [1, 3, 40, 127])
@pytest.mark.parametrize("shape", [(33, 130, 3), (64, 64, 1)])
def test_smooth_and_gain(engine, shape, R):
    """R = 40 and 127 exceed the 33 rows, and both dimensions of 64 x 64; 1300 px wide with R = 3 crosses a row segment of the
    horizontal pass (1024 samples) inside a pixel of the 3-channel row"""
    rng = np.random.default_rng(R + shape[0])
    tiles = _stack(rng, "random", 5, shape)
    _check_field(engine, tiles, R)
    if R == 3:
        wide = _stack(rng, "random", 3, (37, 1300, shape[2]))
        _check_field(engine, wide, R, 37)


@pytest.mark.parametrize("R", [1, 3])
def test_gain_is_one_where_the_field_is_zero(engine, R):
    """a zero region 4R + 1 wide keeps Q == 0 at its centre through both passes: G = 4096 there"""
    rng = np.random.default_rng(R)
    tiles = _stack(rng, "random", 4, (33, 130, 3))
    for t in tiles:
        t[8:8 + 4 * R + 1, 20:20 + 4 * R + 1] = 0
    gain, q8 = _check_field(engine, tiles, R)
    zero = q8 == 0
    assert zero.any() and (gain[zero] == 4096).all() and zero[8 + 2 * R, 20 + 2 * R].all()


def test_gain_saturates(engine):
    """a profile of 255 except a 5 x 5 block of ones, R = 1: M / Q > 16 at the block's centre, the gain stops at 65535"""
    for shape in ((64, 64), (33, 130, 3)):
        t = np.full(shape, 255, np.uint8); t[10:15, 10:15] = 1
        gain, q8 = _check_field(engine, [t, t.copy(), t.copy()], 1)
        assert gain.max() == 65535 and (gain[12, 12] == 65535).all() and (q8[12, 12] == 256).all()


# ---- apply ---------------------------------------------------------------------------------------------------------------------------
def _tile_bytes(engine, handle, shape):
    ch = shape[2] if len(shape) == 3 else 1
    cv = engine.canvas_create(shape[0], shape[1], ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, shape[0], shape[1], ch)
    finally:
        engine.canvas_free(cv)


@pytest.mark.parametrize("shape", [(33, 130, 3), (70, 257, 1), (5, 7, 1)])
def test_apply_in_place(engine, shape):
    rng = np.random.default_rng(shape[1])
    tiles = _stack(rng, "random", 9, shape)
    for t in tiles[:-1]:
        t[:3] = np.minimum(t[:3], 60)                         # a dark band in the profile: gains above one there ...
    tiles[-1][:3] = 255                                       # ... and one tile that is bright in it: its pixels saturate
    want_gain = SH.estimate(tiles, 50, 3)[0]
    want = [SH.apply(t, want_gain) for t in tiles]
    assert ((tiles[-1].astype(np.int64) * want_gain + 2048) >> 12).max() > 255 and (want[-1][:3] == 255).any()
    for source in ("estimate", "from_gain"):
        handles = _upload(engine, tiles)
        try:
            f = engine.shading_estimate(handles, 50, 3) if source == "estimate" else engine.shading_from_gain(want_gain)
            try:
                if source == "from_gain":
                    g, q, p = engine.shading_download(f, with_profile=True)
                    assert np.array_equal(g, want_gain) and not q.any() and not p.any()
                engine.shading_apply(f, handles)
            finally:
                engine.shading_free(f)
            for k, h in enumerate(handles):
                got = _tile_bytes(engine, h, tiles[k].shape)
                assert np.array_equal(got, want[k]), (source, k, int(np.count_nonzero(got != want[k])))
        finally:
            _free(engine, handles)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_tiles_unchanged(engine):
    rng = np.random.default_rng(2)
    tiles = _stack(rng, "random", 3, (16, 24, 1))
    other = rng.integers(0, 256, (16, 25)).astype(np.uint8)
    colour = rng.integers(0, 256, (16, 24, 3)).astype(np.uint8)
    handles = _upload(engine, tiles)
    ho, hc = engine.tile_upload(other), engine.tile_upload_color(colour)
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(16 * 24)) == 0
    assert hip.hipMemcpy(buf, tiles[0].ctypes.data_as(C.c_void_p), C.c_size_t(16 * 24), 1) == 0
    hw = engine.tile_wrap(buf.value, 16, 24, 24)
    f = engine.shading_estimate(handles, 50, 2)
    f25 = engine.shading_estimate([ho], 50, 2)
    try:
        # (the call, what the library says): one fault each, then two at once -- an unknown handle is reported before a handle named twice
        for bad, says in ((lambda: engine.shading_estimate(handles + [ho], 50, 2), "shading_estimate: tile 3 is 16 x 25 x 1, tile 0 is 16 x 24 x 1"),   # mixed shapes
                          (lambda: engine.shading_estimate(handles + [hc], 50, 2), "shading_estimate: tile 3 is 16 x 24 x 3, tile 0 is 16 x 24 x 1"),   # mixed channel counts
                          (lambda: engine.shading_estimate(handles, 101, 2), "shading_estimate: percentile 101 / radius 2 (0..100; 1..127)"),
                          (lambda: engine.shading_estimate(handles, -1, 2), "shading_estimate: percentile -1 / radius 2 (0..100; 1..127)"),
                          (lambda: engine.shading_estimate(handles, 50, 0), "shading_estimate: percentile 50 / radius 0 (0..100; 1..127)"),
                          (lambda: engine.shading_estimate(handles, 50, 128), "shading_estimate: percentile 50 / radius 128 (0..100; 1..127)"),
                          (lambda: engine.shading_estimate([], 50, 2), "shading_estimate: 1..4096 tiles"),                        # n = 0
                          (lambda: engine.shading_estimate(handles + [987654321], 50, 2), "shading_estimate: unknown tile handle"),
                          (lambda: engine.shading_apply(f, handles + [ho]), "shading_apply: tile 3 is 16 x 25 x 1, tile 0 is 16 x 24 x 1"),   # mixed shapes
                          (lambda: engine.shading_apply(f25, handles), "shading_apply: the tiles are 16 x 24 x 1, the field is 16 x 25 x 1"),
                          (lambda: engine.shading_apply(f, [handles[0], hw]), "shading_apply: tile 1 comes from vfsms_tile_wrap: the library does not own its memory"),
                          (lambda: engine.shading_apply(f, [handles[0], handles[1], handles[0]]), "shading_apply: a tile is named twice (it would be corrected twice)"),
                          (lambda: engine.shading_apply(f, []), "shading_apply: 1..4096 tiles"),                                  # n = 0
                          (lambda: engine.shading_apply(987654321, handles), "shading_apply: unknown handle"),                    # unknown field
                          (lambda: engine.shading_free(987654321), "shading_free: unknown handle"),
                          (lambda: engine.shading_apply(f, [handles[0], handles[0], 987654321]), "shading_apply: unknown tile handle")):
            with pytest.raises(isa.VfsmsError, match=re.escape(says)):
                bad()
        fw = engine.shading_estimate([hw], 50, 2)                                      # a wrapped tile may be READ
        try:
            assert np.array_equal(engine.shading_download(fw), SH.estimate(tiles[:1], 50, 2)[0])
        finally:
            engine.shading_free(fw)
        for k, h in enumerate(handles):
            assert np.array_equal(_tile_bytes(engine, h, tiles[k].shape), tiles[k]), k
        back = np.empty((16, 24), np.uint8)
        engine.sync()
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), buf, C.c_size_t(16 * 24), 2) == 0
        assert np.array_equal(back, tiles[0])
    finally:
        engine.shading_free(f); engine.shading_free(f25)
        _free(engine, handles + [ho, hc, hw])
        engine.sync()
        hip.hipFree(buf)


# ---- through Stitcher ------------------------------------------------------------------------------------------------------------------
def _vignetted_row(n, color):
    """n tiles of 96 x 128 cut from one scene 100 px apart (two rows up or down in turn) under one vignette -> (tiles, offsets)"""
    from test_shading_host import vignette
    rng = np.random.default_rng(21)
    scene = np.clip(rng.normal(150, 30, (110, 128 + 100 * n)), 0, 255)
    V = vignette(96, 128)
    tiles, offs, y = [], [], 4
    for k in range(n):
        t = np.clip(np.rint(V * scene[y:y + 96, 100 * k:100 * k + 128]), 0, 255).astype(np.uint8)
        if color:
            t = np.ascontiguousarray(np.stack([t, 255 - t, (t.astype(np.int32) * 7 + 31 & 255).astype(np.uint8)], -1))
        tiles.append(t)
        dy = 2 if k % 2 == 0 else -2
        if k < n - 1:
            offs.append([dy, 100]); y += dy
    return tiles, offs


def _stitch(engine, tmp_path, tiles, offs, color, tag, **settings):
    from test_host_logic import _write_tiles
    files = _write_tiles(tmp_path, tiles, tag)
    s = isa.Stitcher(); s._engine = engine; s.isColorMode = color; s.fuseMethod = "fadeInAndFadeOut"
    msgs = []
    s.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
    for k, v in settings.items():
        setattr(s, k, v)
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = color
        return s.getStitchByOffset(files, [list(o) for o in offs]), msgs
    finally:
        isa.Stitcher.isColorMode = old


@pytest.mark.parametrize("color", [False, True])
def test_stitcher_corrects_the_mosaic(engine, tmp_path, color):
    """"estimate" over 9 tiles == "none" over the same tiles corrected beforehand by the reference"""
    tiles, offs = _vignetted_row(9, color)
    got, _ = _stitch(engine, tmp_path, tiles, offs, color, "est", shadingCorrection="estimate")
    want, _ = _stitch(engine, tmp_path, SH.correct(tiles, 50, 32), offs, color, "ref")
    raw, _ = _stitch(engine, tmp_path, tiles, offs, color, "raw", shadingCorrection="none")
    assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert not np.array_equal(got, raw)
    got5, _ = _stitch(engine, tmp_path, tiles, offs, color, "est5", shadingCorrection="estimate", shadingPercentile=20, shadingRadius=5)
    want5, _ = _stitch(engine, tmp_path, SH.correct(tiles, 20, 5), offs, color, "ref5")
    assert np.array_equal(got5, want5) and not np.array_equal(got5, got)


def test_stitcher_leaves_small_mosaics_alone_and_takes_a_given_gain(engine, tmp_path):
    tiles, offs = _vignetted_row(7, False)
    got, msgs = _stitch(engine, tmp_path, tiles, offs, False, "s7", shadingCorrection="estimate")
    raw, raw_msgs = _stitch(engine, tmp_path, tiles, offs, False, "r7")
    assert np.array_equal(got, raw)
    assert [m for m in msgs if "shading" in m] == ["  shading correction skipped: 7 tiles, shadingMinTiles is 8"]
    assert not [m for m in raw_msgs if "shading" in m]
    gain = SH.estimate(tiles, 50, 8)[0]                       # "measured elsewhere": any Q12 array of the tile shape
    got2, msgs2 = _stitch(engine, tmp_path, tiles[:2], offs[:1], False, "g2", shadingCorrection="estimate", shadingGain=gain)
    want2, _ = _stitch(engine, tmp_path, [SH.apply(t, gain) for t in tiles[:2]], offs[:1], False, "w2")
    raw2, _ = _stitch(engine, tmp_path, tiles[:2], offs[:1], False, "r2")
    assert np.array_equal(got2, want2) and not np.array_equal(got2, raw2) and not [m for m in msgs2 if "skipped" in m]
    with pytest.raises(ValueError):
        _stitch(engine, tmp_path, tiles[:2], offs[:1], False, "g3", shadingCorrection="estimate", shadingGain=gain[:, :100])
    with pytest.raises(ValueError):
        _stitch(engine, tmp_path, tiles[:2], offs[:1], False, "g4", shadingCorrection="estimate", shadingGain=gain.astype(np.float32))
    nine, offs9 = _vignetted_row(9, False)
    ragged = nine[:8] + [np.ascontiguousarray(nine[8][:, :120])]                      # tiles of different shapes: before a canvas exists
    with pytest.raises(ValueError):
        _stitch(engine, tmp_path, ragged, offs9, False, "rg", shadingCorrection="estimate")


def test_registration_is_untouched(engine, tmp_path):
    """flowStitch over a line scan: the offsets the registrar hands to getStitchByOffset are the same with "estimate" as with "none"
    (the correction runs behind the registration, on tiles nothing else reads), and only the mosaic differs"""
    from PIL import Image
    from imagestitch_amd.synthetic import line_scan
    tiles, truth = line_scan()
    files = []
    for k, t in enumerate(tiles):
        f = os.path.join(str(tmp_path), "scan_%02d.png" % k)
        Image.fromarray(t).save(f); files.append(f)
    names = ("direction", "directIncre", "featureMethod", "offsetEvaluate", "isEnhance", "isClahe", "isColorMode", "fuseMethod")
    old = [getattr(isa.Stitcher, n) for n in names]
    try:
        for n, v in zip(names, (4, 0, "surf", 3, False, False, False, "fadeInAndFadeOut")):
            setattr(isa.Stitcher, n, v)
        runs = {}
        for corr in ("none", "estimate"):
            st = isa.Stitcher(); st._engine = engine; st.isPrintLog = False
            st.shadingCorrection = corr; st.shadingMinTiles = 2; st.shadingRadius = 16
            seen = []
            inner = st.getStitchByOffset
            st.getStitchByOffset = lambda fl, offs, seen=seen, inner=inner: (seen.append([list(o) for o in offs]), inner(fl, offs))[1]
            (status, end), mosaic = st.flowStitch(list(files), st.calculateOffsetForFeatureSearch)
            runs[corr] = (status, end, seen[0], mosaic)
        assert runs["none"][0] and runs["none"][1] == 3 and len(runs["none"][2]) == 3
        assert runs["estimate"][:3] == runs["none"][:3]
        for o, t in zip(runs["none"][2], truth):
            assert abs(o[0] - t[0]) <= 1 and abs(o[1] - t[1]) <= 1
        assert runs["estimate"][3].shape == runs["none"][3].shape and not np.array_equal(runs["estimate"][3], runs["none"][3])
    finally:
        for n, v in zip(names, old):
            setattr(isa.Stitcher, n, v)
        isa.Stitcher.tempImageFeature.isBreak = True
