"""Method.lensCorrection on the device against tests/lens_ref.py, exactly (np.array_equal): the block displacement field at every radius
and block size the kernel distinguishes, gray and colour, wrapped strided tiles, empty and one-block lattices; the resampling in place
and from host arrays at ragged shapes, extreme coefficients and centres; the refusals of the C ABI; and the correction through
Stitcher.getStitchByOffset alone, behind the shading correction, in front of the exposure compensation and with given coefficients."""
import ctypes as C
import functools
import re

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import lens
from imagestitch_amd._lib import NccJob
from imagestitch_amd.adjust import neighbour_edges
from imagestitch_amd.synthetic import texture_window

import exposure_ref as ER
import lens_cases as LC
import lens_ref as LR
import shading_ref as SH
from test_exposure_gpu import _hip
from test_shading_gpu import _free, _tile_bytes, _upload

pytestmark = pytest.mark.gpu


# ---- the block displacement field ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def field_tiles(h, w, color):
    """four overlapping crops of one noisy scene at the origins ORIGINS (scaled to the shape), a tile with a flat quarter and a flat
    tile; shared: do not write to the arrays"""
    rng = np.random.default_rng(h + w + int(color))
    scene = 128.0 + 45.0 * texture_window(300, 500, 2 * h, 2 * w, seed=h).astype(np.float64)
    tiles = []
    for oy, ox in origins(h, w):
        v = scene[oy:oy + h, ox:ox + w]
        if color:
            v = np.stack([0.8 * v + 20.0, v, 1.1 * v - 10.0], axis=-1)
        tiles.append(np.clip(np.rint(v + rng.normal(0.0, 3.0, v.shape)), 0, 255).astype(np.uint8))
    part = tiles[1].copy(); part[:h // 2, :w // 2] = 200         # flat blocks in B (and in A, when it is the first of a job)
    tiles += [part, np.full_like(tiles[0], 93)]
    for t in tiles:
        t.setflags(write=False)
    return tiles


def origins(h, w):
    return [(0, 0), (h * 5 // 12, 3), (2, w // 2 + 1), (h // 2, w // 2)]


def _check_field(engine, tiles, handles, jobs, block, radius):
    """one call over `jobs` (indices into tiles / handles) against the reference, job by job"""
    shape = tiles[0].shape[:2]
    first = lens.block_first(shape, [(dx, dy) for _a, _b, dx, dy in jobs], block, radius)
    wfirst, wbest, wsurf = LR.block_ncc_batch(tiles, jobs, block, radius)
    assert np.array_equal(first, wfirst)
    best, surf = engine.block_ncc_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in jobs], first, block, radius, want_surface=True)
    assert best.dtype == np.int32 and best.shape == wbest.shape and surf.shape == wsurf.shape
    bad = np.nonzero((best != wbest).any(axis=1) | (surf != wsurf).any(axis=(1, 2)))[0]
    assert np.array_equal(best, wbest) and np.array_equal(surf, wsurf), (block, radius, bad[:5].tolist(), best[bad[:3]].tolist(), wbest[bad[:3]].tolist())
    only = engine.block_ncc_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in jobs], first, block, radius)
    assert np.array_equal(only, wbest)                        # without the surfaces
    return first, wbest


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("radius", [1, 3, 16])
def test_block_field_equals_the_reference(engine, color, radius):
    """96 x 128 tiles, block 16: offsets of every sign, perturbed ones, a lattice of exactly one block, lattices of none (alone in a call
    and between jobs that have blocks), flat blocks, jobs that share tiles"""
    h, w, block = 96, 128, 16
    tiles = field_tiles(h, w, color)
    o = origins(h, w)
    d = lambda a, b: (o[b][0] - o[a][0], o[b][1] - o[a][1])        # noqa: E731
    one = (h - block - 2 * radius, w - block - 2 * radius)         # an overlap of (block + 2 R)^2: exactly one block
    jobs = [(0, 1) + d(0, 1), (1, 0) + d(1, 0), (0, 2) + d(0, 2), (2, 0) + d(2, 0), (1, 3) + d(1, 3), (0, 3) + d(0, 3), (3, 0) + d(3, 0),
            (0, 1, d(0, 1)[0] + 1, d(0, 1)[1] - 1), (2, 3, d(2, 3)[0] - 1, d(2, 3)[1] + 1),
            (0, 3, h - 8, 0), (0, 3) + one, (3, 0, -one[0], -one[1]), (0, 1, h, w), (1, 2, one[0] + 1, one[1]),
            (0, 4) + d(0, 1), (4, 0) + d(1, 0), (5, 1) + d(0, 1), (0, 0, 0, 0), (2, 2, 3, -5)]
    handles = _upload(engine, tiles)
    try:
        engine.profile_enable(True); engine.profile_read(reset=True)
        first, wbest = _check_field(engine, tiles, handles, jobs, block, radius)
        stages = engine.profile_read(reset=True)
        engine.profile_enable(False)
        assert stages["lens_blocks"][1] == 2, stages
        counts = np.diff(first)
        assert counts[10] == 1 and counts[11] == 1 and counts[9] == 0 and counts[12] == 0 and counts[13] == 0 and (counts > 1).sum() >= (4 if radius == 16 else 9)
        assert (wbest[first[16]:first[17]] == [0, 0, 0, block * block]).all() and counts[16] > 0     # a flat A: every block scores 0 at (0, 0)
        flat_b = wbest[first[14]:first[15]]
        assert radius == 16 or ((flat_b[:, 2] == 0).any() and (flat_b[:, 2] > 0).any())              # tile 4 as B: its flat quarter
        # a lattice without blocks, alone: nothing to do, nothing returned
        none = engine.block_ncc_batch([(handles[0], handles[1], h, w)], [0, 0], block, radius, want_surface=True)
        assert none[0].shape == (0, 4) and none[1].shape == (0, 2 * radius + 1, 2 * radius + 1)
        assert engine.block_ncc_batch([], [0], block, radius).shape == (0, 4)
    finally:
        engine.profile_enable(False)
        _free(engine, handles)


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("block", [8, 64])
def test_block_sizes(engine, color, block):
    """160 x 192 tiles, radius 2: the smallest block, and one whose rows are cut into slices"""
    h, w = 160, 192
    tiles = field_tiles(h, w, color)
    o = origins(h, w)
    o = o + [o[1]]                                           # tile 4 is tile 1 with a flat quarter
    jobs = [(a, b, o[b][0] - o[a][0] + e, o[b][1] - o[a][1] - e) for a, b, e in ((0, 1, 0), (1, 0, 1), (0, 2, -1), (3, 1, 0), (0, 3, 1), (4, 0, 0))]
    handles = _upload(engine, tiles)
    try:
        first, _ = _check_field(engine, tiles, handles, jobs, block, 2)
        assert first[-1] >= (6 if block == 64 else 400)
    finally:
        _free(engine, handles)


def test_largest_block_and_radius(engine):
    """block 128 with radius 16 on 200 x 330 tiles: the largest LDS image the kernel asks for"""
    h, w = 200, 330
    tiles = field_tiles(h, w, False)
    handles = _upload(engine, tiles[:2])
    try:
        first, _ = _check_field(engine, tiles[:2], handles, [(0, 1, 20, 3), (1, 0, -20, -3)], 128, 16)
        assert first.tolist() == [0, 2, 4]
    finally:
        _free(engine, handles)


def test_wrapped_strided_tiles(engine):
    """device rows 141 bytes apart for w = 128, behind an odd base address: the field reads them where they are; lens_apply refuses them
    and leaves the memory alone"""
    h, w, stride = 96, 128, 141
    tiles = field_tiles(h, w, False)[:4]
    rng = np.random.default_rng(11)
    padded = rng.integers(0, 256, (4, h, stride)).astype(np.uint8)       # the padding is not zero: it must stay out of the sums
    for k, t in enumerate(tiles):
        padded[k, :, :w] = t
    o = origins(h, w)
    jobs = [(a, b, o[b][0] - o[a][0], o[b][1] - o[a][1]) for a, b in ((0, 1), (1, 0), (0, 2), (3, 2), (0, 3))]
    hip = _hip()
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(padded.size + 1)) == 0
    handles = []
    try:
        assert hip.hipMemcpy(C.c_void_p(buf.value + 1), padded.ctypes.data_as(C.c_void_p), C.c_size_t(padded.size), 1) == 0
        handles = [engine.tile_wrap(buf.value + 1 + k * h * stride, h, w, stride) for k in range(4)]
        _check_field(engine, tiles, handles, jobs, 16, 3)
        own = engine.tile_upload(tiles[0])
        handles.append(own)
        with pytest.raises(isa.VfsmsError):
            engine.lens_apply([own, handles[1]], 1 << 24, 0)
        back = np.empty_like(padded)
        engine.sync()
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(buf.value + 1), C.c_size_t(padded.size), 2) == 0
        assert np.array_equal(back, padded) and np.array_equal(_tile_bytes(engine, own, (h, w)), tiles[0])
    finally:
        _free(engine, handles)
        engine.sync()
        hip.hipFree(buf)


def test_block_field_refusals(engine):
    """every refusal leaves best4 and surface as they were"""
    tiles = field_tiles(96, 128, False)
    rng = np.random.default_rng(3)
    extra = [rng.integers(0, 256, (96, 129)).astype(np.uint8), field_tiles(96, 128, True)[0], rng.integers(0, 256, (96, 128, 4)).astype(np.uint8)]
    handles = _upload(engine, list(tiles[:2]) + extra)
    g0, g1, wide, col, four = handles
    first = lens.block_first((96, 128), [(40, 3)], 16, 3)
    best = np.full((int(first[-1]), 4), -7, np.int32)
    surf = np.full((int(first[-1]), 7, 7), -7, np.int32)

    def call(jobs, f, block=16, radius=3):
        arr = (NccJob * len(jobs))(*[NccJob(*j) for j in jobs])
        f = np.ascontiguousarray(f, np.int64)
        return engine.lib.vfsms_block_ncc_batch(engine.ctx, arr, len(jobs), block, radius, f.ctypes.data_as(C.c_void_p),
                                                best.ctypes.data_as(C.c_void_p), surf.ctypes.data_as(C.c_void_p))
    try:
        for rc in (call([(g0, 987654321, 40, 3)], first),                      # an unknown handle
                   call([(g0, wide, 40, 3)], first),                            # two shapes in a job
                   call([(g0, col, 40, 3)], first),                             # two channel counts in a job
                   call([(four, four, 40, 3)], first),                          # four channels
                   call([(g0, g1, 40, 3)], first + [0, 1]),                     # a first that does not match the lattice
                   call([(g0, g1, 40, 3)], [1, 1 + int(first[-1])]),
                   call([(g0, g1, 40, 3)], first, block=12), call([(g0, g1, 40, 3)], first, block=136), call([(g0, g1, 40, 3)], first, block=0),
                   call([(g0, g1, 40, 3)], first, radius=0), call([(g0, g1, 40, 3)], first, radius=17)):
            assert rc != 0
        assert (best == -7).all() and (surf == -7).all()
        with pytest.raises(isa.VfsmsError):
            engine.block_ncc_batch([(g0, col, 40, 3)], first, 16, 3)
        with pytest.raises(ValueError):
            engine.block_ncc_batch([(g0, g1, 40, 3)], [0], 16, 3)
        assert call([(g0, g1, 40, 3)], first) == 0                              # the same call with nothing wrong
        wbest, wsurf = LR.block_ncc(tiles[0], tiles[1], 40, 3, 16, 3)
        assert np.array_equal(best, wbest) and np.array_equal(surf, wsurf)
    finally:
        _free(engine, handles)


# ---- the resampling ----------------------------------------------------------------------------------------------------------------------
SHAPES = [(1, 1), (1, 9), (5, 7), (33, 130, 3), (70, 257), (96, 128)]
COEFFICIENTS = [(0, 0), (1 << 28, -(1 << 27)), (-(1 << 28), 1 << 27)]
INTERP = ["bilinear", "cubic"]


@functools.lru_cache(maxsize=None)
def remap_tiles():
    rng = np.random.default_rng(23)
    tiles = [rng.integers(0, 256, s).astype(np.uint8) for s in SHAPES]
    for t in tiles:
        t.setflags(write=False)
    return tiles


def _centres(shape):
    """the default centre and both ends of its allowed range, on either axis"""
    h, w = shape[:2]
    return [(-1, -1), ((h - 1) - (h - 1) // 2, (w - 1) + (w - 1) // 2), ((h - 1) + (h - 1) // 2, (w - 1) - (w - 1) // 2)]


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("coef", COEFFICIENTS)
def test_remap_equals_the_reference(engine, coef, interp):
    """lens_remap on host arrays, one of them strided, and lens_apply on the same tiles resident, shape by shape and centre by centre"""
    for t in remap_tiles():
        for cy2, cx2 in _centres(t.shape):
            want = LR.remap(t, coef[0], coef[1], cy2, cx2, interp)
            got = engine.lens_remap(t, coef[0], coef[1], (cy2, cx2), INTERP[interp])
            assert got.dtype == np.uint8 and np.array_equal(got, want), (t.shape, coef, (cy2, cx2), interp, int(np.count_nonzero(got != want)))
            if coef == (0, 0):
                assert np.array_equal(got, t)
            h = _upload(engine, [t])
            try:
                engine.lens_apply(h, coef[0], coef[1], (cy2, cx2), INTERP[interp])
                assert np.array_equal(_tile_bytes(engine, h[0], t.shape), want), (t.shape, coef, (cy2, cx2), interp)
            finally:
                _free(engine, h)
    wide = np.random.default_rng(5).integers(0, 256, (70, 300)).astype(np.uint8)
    for src in (wide[:, 3:260], wide[::2, 1:258], np.random.default_rng(6).integers(0, 256, (33, 150, 3)).astype(np.uint8)[:, 7:137]):
        assert not src.flags["C_CONTIGUOUS"]
        assert np.array_equal(engine.lens_remap(src, coef[0], coef[1], (-1, -1), INTERP[interp]), LR.remap(np.ascontiguousarray(src), coef[0], coef[1], None, None, interp))


@pytest.mark.parametrize("interp", [0, 1])
def test_apply_a_batch_of_shapes_in_one_call(engine, interp):
    tiles = remap_tiles()
    a1, a2 = COEFFICIENTS[1]
    handles = _upload(engine, tiles)
    try:
        engine.profile_enable(True); engine.profile_read(reset=True)
        engine.lens_apply(handles, a1, a2, (-1, -1), INTERP[interp])
        stages = engine.profile_read(reset=True)
        engine.profile_enable(False)
        assert stages["lens_apply"][1] == 1, stages
        for k, t in enumerate(tiles):
            want = LR.remap(t, a1, a2, None, None, interp)
            assert np.array_equal(_tile_bytes(engine, handles[k], t.shape), want), t.shape
        # an explicit centre that every tile of the call accepts: two tiles of one shape
        pair = _upload(engine, [tiles[5], tiles[5][::-1].copy()])
        try:
            engine.lens_apply(pair, -a1, -a2, (95 + 47, 127 - 63), INTERP[interp])
            assert np.array_equal(_tile_bytes(engine, pair[1], (96, 128)), LR.remap(tiles[5][::-1], -a1, -a2, 95 + 47, 127 - 63, interp))
            assert np.array_equal(_tile_bytes(engine, pair[0], (96, 128)), LR.remap(tiles[5], -a1, -a2, 95 + 47, 127 - 63, interp))
        finally:
            _free(engine, pair)
    finally:
        engine.profile_enable(False)
        _free(engine, handles)


def test_resampling_refusals(engine):
    """every refusal leaves the tiles and the output as they were"""
    tiles = [remap_tiles()[5], remap_tiles()[3], remap_tiles()[1]]
    handles = _upload(engine, tiles)
    try:
        # (the call, what the library says): one fault each, then two at once -- an unknown handle is reported before a tile named twice
        for bad, says in ((lambda: engine.lens_apply([handles[0], handles[1], handles[0]], 1 << 20, 0), "lens_apply: a tile is named twice (it would be corrected twice)"),
                          (lambda: engine.lens_apply([handles[0], 987654321], 1 << 20, 0), "lens_apply: unknown tile handle"),
                          (lambda: engine.lens_apply([], 1 << 20, 0), "lens_apply: 1..4096 tiles"),
                          (lambda: engine.lens_apply(handles[:2], (1 << 28) + 1, 0), "lens_apply: coefficients 268435457, 0 outside +-2^28 (Q30)"),
                          (lambda: engine.lens_apply(handles[:2], 0, -(1 << 28) - 1), "lens_apply: coefficients 0, -268435457 outside +-2^28 (Q30)"),
                          (lambda: engine.lens_apply(handles[:1], 1 << 20, 0, (95 + 48, 127)),                    # the centre outside the middle half
                           "lens_apply: the centre (143, 127) / 2 lies outside the middle half of a 96 x 128 image"),
                          (lambda: engine.lens_apply(handles[:1], 1 << 20, 0, (95, 127 - 64)), "lens_apply: the centre (95, 63) / 2 lies outside the middle half of a 96 x 128 image"),
                          (lambda: engine.lens_apply([handles[0], handles[2]], 1 << 20, 0, (95, 127)),            # ... of the second tile (1 x 9)
                           "lens_apply: the centre (95, 127) / 2 lies outside the middle half of a 1 x 9 image"),
                          (lambda: engine.lens_apply(handles[:2], 1 << 20, 0, (-1, -1), 2), "lens_apply: interp 2 (0 bilinear or 1 cubic)"),
                          (lambda: engine.lens_apply(handles[:2], 1 << 20, 0, (-1, -1), -1), "lens_apply: interp -1 (0 bilinear or 1 cubic)"),
                          (lambda: engine.lens_apply([handles[0], handles[0], 987654321], 1 << 20, 0), "lens_apply: unknown tile handle")):
            with pytest.raises(isa.VfsmsError, match=re.escape(says)):
                bad()
        with pytest.raises(ValueError):
            engine.lens_apply(handles[:1], 1 << 20, 0, (-1, -1), "lanczos")
        for k, t in enumerate(tiles):
            assert np.array_equal(_tile_bytes(engine, handles[k], t.shape), t)
        src = np.ascontiguousarray(tiles[0])
        dst = np.full(src.shape, 7, np.uint8)
        p = lambda a: a.ctypes.data_as(C.c_void_p)                # noqa: E731
        lib, ctx = engine.lib, engine.ctx
        for rc in (lib.vfsms_lens_remap_u8(ctx, p(src), 96, 128, 1, 128, (1 << 28) + 1, 0, -1, -1, 1, p(dst)),
                   lib.vfsms_lens_remap_u8(ctx, p(src), 96, 128, 1, 128, 0, 0, 95 - 48, 127, 1, p(dst)),
                   lib.vfsms_lens_remap_u8(ctx, p(src), 96, 128, 1, 128, 0, 0, -1, -1, 2, p(dst)),
                   lib.vfsms_lens_remap_u8(ctx, p(src), 96, 128, 1, 127, 0, 0, -1, -1, 1, p(dst)),
                   lib.vfsms_lens_remap_u8(ctx, p(src), 96, 128, 5, 640, 0, 0, -1, -1, 1, p(dst)),
                   lib.vfsms_lens_remap_u8(ctx, None, 96, 128, 1, 128, 0, 0, -1, -1, 1, p(dst))):
            assert rc != 0
        assert (dst == 7).all()
        with pytest.raises(ValueError):
            engine.lens_remap(src.astype(np.float32), 0, 0)
    finally:
        _free(engine, handles)


def test_undistort_operator(engine):
    img = remap_tiles()[3]
    got = isa.undistort(img, (0.03, 0.0027), centre=(15.5, 70.0), interpolation="bilinear", engine=engine)
    q = LR.coefficients_q30(0.03, 0.0027)
    assert np.array_equal(got, LR.remap(img, q[0], q[1], 31, 140, 0))


# ---- through Stitcher ------------------------------------------------------------------------------------------------------------------------
LOG = "  lens correction"
SETTINGS = dict(lensBlock=LC.BLOCK, lensRadius=LC.RADIUS, lensMinBlocks=8)


def _stitch(engine, tmp_path, tiles, offs, color, tag, **settings):
    """test_shading_gpu._stitch, returning the Stitcher too"""
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
        return s.getStitchByOffset(files, [list(o) for o in offs]), msgs, s
    finally:
        isa.Stitcher.isColorMode = old


def _reference_chain(tiles, offs, given=None):
    edges = neighbour_edges([t.shape for t in tiles], np.asarray(offs), LC.RADIUS)
    return LR.chain(tiles, edges.tolist(), offs, LC.BLOCK, LC.RADIUS, 0.5, 8, 0.25, 1, lens.fit_radial, given)


@pytest.mark.parametrize("color", [False, True])
def test_stitcher_corrects_the_mosaic(engine, tmp_path, color):
    """"estimate" on the 2 x 2 case with two path offsets off by a pixel or two == "none" over tiles the reference corrected, at the
    offsets the reference measured again; the report is that of the reference chain, float for float; "given" with the fitted pair gives
    the same mosaic"""
    tiles, true = LC.grid("s+", color)
    offs = [[true[0][0] + 1, true[0][1] - 2], list(true[1]), [true[2][0] - 1, true[2][1] + 1]]
    fixed, want_offs, want_rep = _reference_chain(tiles, offs)
    assert want_rep["apply"] and want_offs == [list(o) for o in true]
    got, msgs, s = _stitch(engine, tmp_path, tiles, offs, color, "est", lensCorrection="estimate", **SETTINGS)
    want, _, _ = _stitch(engine, tmp_path, fixed, want_offs, color, "ref")
    none, none_msgs, _ = _stitch(engine, tmp_path, tiles, offs, color, "none", lensCorrection="none")
    raw, raw_msgs, _ = _stitch(engine, tmp_path, tiles, offs, color, "raw")
    assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert np.array_equal(none, raw) and [m.replace("none_", "raw_") for m in none_msgs] == raw_msgs          # every log line but for the file names
    assert not np.array_equal(got, raw) and not [m for m in raw_msgs if "lens" in m]
    rep = s.lensReport
    for key, value in want_rep.items():
        assert rep[key] == value, key                           # b1, a1, a2, corner_px, spread_before included: equal as floats
    assert s.lensCoefficients == (want_rep["a1"], want_rep["a2"]) and rep["moved"] == 2 and rep["spread_after"] <= rep["spread_before"] / 2
    assert len([m for m in msgs if m.startswith(LOG)]) == 1
    given, gmsgs, s2 = _stitch(engine, tmp_path, tiles, offs, color, "giv", lensCorrection="given", lensCoefficients=s.lensCoefficients, **SETTINGS)
    assert np.array_equal(given, got) and s2.lensReport["spread_after"] == rep["spread_after"]
    with pytest.raises(ValueError):
        _stitch(engine, tmp_path, tiles, offs, color, "bad", lensCorrection="brown", **SETTINGS)


def test_undistorted_tiles_go_through_untouched(engine, tmp_path):
    tiles, true = LC.grid("s0")
    got, msgs, s = _stitch(engine, tmp_path, tiles, true, False, "s0", lensCorrection="estimate", **SETTINGS)
    raw, _, _ = _stitch(engine, tmp_path, tiles, true, False, "s0r")
    assert np.array_equal(got, raw) and s.lensCoefficients is None and not s.lensReport["apply"]
    assert [m for m in msgs if m.startswith(LOG)] == [LOG + " skipped: " + s.lensReport["reason"]]


def test_shading_first_then_lens_then_exposure(engine, tmp_path):
    tiles, true = LC.grid("m-")
    offs = [list(true[0]), [true[1][0] + 2, true[1][1] - 1], list(true[2])]
    shaded = SH.correct(tiles, 50, 32)
    fixed, want_offs, want_rep = _reference_chain(shaded, offs)
    assert want_rep["apply"] and want_offs != offs
    got, msgs, s = _stitch(engine, tmp_path, tiles, offs, False, "all", shadingCorrection="estimate", shadingMinTiles=2, lensCorrection="estimate",
                           exposureCompensation="gain", exposureMinPixels=256, **SETTINGS)
    want, _, _ = _stitch(engine, tmp_path, ER.correct(fixed, want_offs, 1, 254, 256, 2.0), want_offs, False, "allref")
    assert got.shape == want.shape and np.array_equal(got, want), int(np.count_nonzero(got != want))
    assert s.lensReport["a1"] == want_rep["a1"] and s.exposureReport["edges"] == len(ER.overlap_edges([t.shape for t in tiles], want_offs, 256))
    lines = [m for m in msgs if m.startswith(LOG) or m.startswith("  exposure compensation")]
    assert len(lines) == 2 and lines[0].startswith(LOG)
