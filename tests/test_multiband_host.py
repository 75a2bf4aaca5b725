"""CPU tests of fuseMethod "multiBandBlending": tests/multiband_ref.py (the specification the HIP kernels are checked against) pinned
against an independent scalar restatement, its invariants, the seam against the fade's weights, and the host routing of Stitcher /
ImageFusion on the CPU test double."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from fakes import OracleEngine

import multiband_ref as MB

F = np.float32
SIZES = ((1, 1), (1, 5), (2, 3), (3, 3), (4, 5), (7, 6))


# ---- an independent scalar restatement: plain Python loops over np.float32 scalars ------------------------------------------------
def _refl(i, n):
    if n == 1:
        return 0
    while i < 0 or i >= n:
        if i < 0:
            i = -i
        else:
            i = 2 * n - 2 - i
    return i


def _down_loop(S):
    n, m = S.shape
    dn, dm = (n + 1) // 2, (m + 1) // 2
    R = [[None] * dm for _ in range(n)]
    for y in range(n):
        for x in range(dm):
            t = [S[y, _refl(2 * x + d, m)] for d in (-2, -1, 0, 1, 2)]
            R[y][x] = F(F(F(F(t[2] * F(6)) + F(F(t[1] + t[3]) * F(4))) + t[0]) + t[4])
    D = np.empty((dn, dm), F)
    for y in range(dn):
        for x in range(dm):
            t = [R[_refl(2 * y + d, n)][x] for d in (-2, -1, 0, 1, 2)]
            D[y, x] = F(F(F(F(F(t[2] * F(6)) + F(F(t[1] + t[3]) * F(4))) + t[0]) + t[4]) * F(1.0 / 256))
    return D


def _up_loop(S, oh, ow):
    h, w = S.shape

    def nb(i, n):                                   # neighbour index: -1 reflects, n replicates
        if i < 0:
            return 1 if n > 1 else 0
        return min(i, n - 1)
    R = np.empty((h, 2 * w), F)
    for y in range(h):
        for x in range(w):
            R[y, 2 * x] = F(F(S[y, nb(x - 1, w)] + F(S[y, x] * F(6))) + S[y, nb(x + 1, w)])
            R[y, 2 * x + 1] = F(F(S[y, x] + S[y, nb(x + 1, w)]) * F(4))
    U = np.empty((2 * h, ow), F)
    for y in range(h):
        for x in range(ow):
            U[2 * y, x] = F(F(F(R[nb(y - 1, h), x] + F(R[y, x] * F(6))) + R[nb(y + 1, h), x]) * F(1.0 / 64))
            U[2 * y + 1, x] = F(F(F(R[y, x] + R[nb(y + 1, h), x]) * F(4)) * F(1.0 / 64))
    return U[:oh]


@pytest.mark.parametrize("shape", SIZES)
def test_pyr_down_matches_the_scalar_restatement(shape):
    S = np.random.default_rng(shape[0] * 10 + shape[1]).uniform(-40, 300, shape).astype(F)
    want = _down_loop(S)
    got = MB.pyr_down(S)
    assert got.dtype == F and got.shape == ((shape[0] + 1) // 2, (shape[1] + 1) // 2)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # channels are independent
    S3 = np.stack([S, S * F(0.5), S + F(3)], -1)
    got3 = MB.pyr_down(S3)
    for k in range(3):
        assert np.array_equal(got3[..., k].view(np.uint32), _down_loop(np.ascontiguousarray(S3[..., k])).view(np.uint32))


@pytest.mark.parametrize("shape", SIZES)
def test_pyr_up_matches_the_scalar_restatement(shape):
    S = np.random.default_rng(7 + shape[0] * 10 + shape[1]).uniform(-40, 300, shape).astype(F)
    h, w = shape
    for oh in sorted({2 * h - 1, 2 * h}):
        for ow in sorted({2 * w - 1, 2 * w}):
            want = _up_loop(S, oh, ow)
            got = MB.pyr_up(S, oh, ow)
            assert got.shape == (oh, ow)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (shape, oh, ow)


def test_reflect101_border_cases():
    assert [MB.reflect101(i, 5) for i in (-2, -1, 0, 4, 5, 6)] == [2, 1, 0, 4, 3, 2]
    assert [MB.reflect101(i, 2) for i in (-2, -1, 2, 3)] == [0, 1, 0, 1]
    assert [MB.reflect101(i, 1) for i in (-2, -1, 0, 1, 2)] == [0] * 5


def test_level_size_chains():
    assert MB.level_sizes(1, 4) == [1, 1, 1, 1, 1]
    assert MB.level_sizes(2, 3) == [2, 1, 1, 1]
    assert MB.level_sizes(3, 3) == [3, 2, 1, 1]
    assert MB.level_sizes(5, 4) == [5, 3, 2, 1, 1]
    assert MB.level_sizes(2047, 6) == [2047, 1024, 512, 256, 128, 64, 32]


def test_constant_planes_stay_constant():
    for shape in ((1, 1), (5, 7), (33, 20), (6, 4, 3)):
        for v in (0.0, 1.0, 77.0, 255.0):
            S = np.full(shape, v, F)
            d = MB.pyr_down(S)
            assert np.all(d == F(v))
            u = MB.pyr_up(d, shape[0], shape[1])
            assert np.all(u == F(v))


def _no_corner(A):
    raise AssertionError("strip geometry expected")


@pytest.mark.parametrize("levels", range(1, 7))
def test_identical_inputs_give_the_input_back(oracle, levels):
    rng = np.random.default_rng(levels)
    for shape in ((1, 1), (3, 8), (37, 53), (24, 30, 3), (65, 17, 3)):
        A = rng.integers(0, 256, shape).astype(np.int64)
        out = MB.multiband(A, A.copy(), 3, -2, levels, oracle.corner_ramps)
        assert out.dtype == np.uint8 and np.array_equal(out, A.astype(np.uint8)), (shape, levels)


def _strip_weights_loop(A, dx, dy):
    """orc_fuse_fade's strip loops (oracle/vfsms_oracle.c), one index at a time"""
    r, c = A.shape[:2]
    wAr = [F(1)] * r; wBr = [F(1)] * r; wAc = [F(1)] * c; wBc = [F(1)] * c
    if c <= r:
        for i in range(c):
            f = F(i) if dy >= 0 else F(c - i)
            wAc[c - i - 1] = F(F(F(wAc[c - i - 1] * f) * F(1)) / F(c))
            wBc[i] = F(F(F(wBc[i] * f) * F(1)) / F(c))
    else:
        for i in range(r):
            f = F(i) if dx <= 0 else F(r - i)
            wAr[i] = F(F(F(wAr[i] * f) * F(1)) / F(r))
            wBr[r - i - 1] = F(F(F(wBr[r - i - 1] * f) * F(1)) / F(r))
    wA = np.array([[F(wAr[i] * wAc[j]) for j in range(c)] for i in range(r)], F)
    wB = np.array([[F(wBr[i] * wBc[j]) for j in range(c)] for i in range(r)], F)
    return wA, wB


def test_seam_is_where_the_fade_weights_tie(oracle, golden_dir):
    """M0 = wA >= wB: corner fixtures against OracleEngine.fuse_ramps_i64 (getWeightsMatrix), strip fixtures against the fade's strip
    loops restated index by index"""
    eng = OracleEngine(oracle)
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    n_strip = n_corner = 0
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        A = g["f%d_A" % i]
        M = MB.seam_mask(A, int(dx), int(dy), oracle.corner_ramps)
        assert M.dtype == F and M.shape == A.shape[:2] and set(np.unique(M)) <= {F(0), F(1)}
        if np.count_nonzero(A > -1) / A.size > 0.65:
            wA, wB = _strip_weights_loop(A, int(dx), int(dy))
            n_strip += 1
        else:
            (_wAr, wBr, _wAc, wBc), _info = eng.fuse_ramps_i64(A, dx, dy, force_corner=True)
            wB = wBr[:, None] * wBc[None, :]
            wA = F(1) - wB
            n_corner += 1
        assert np.array_equal(M, (wA >= wB).astype(F)), i
    assert n_strip > 20 and n_corner > 20, (n_strip, n_corner)


def test_fill_rules():
    A = np.array([[-1, 5, -1, 7]], np.int64); B = np.array([[3, -1, -1, 9]], np.int64)
    A1, B1 = MB.fill(A, B)
    assert A1.tolist() == [[3, 5, 0, 7]] and B1.tolist() == [[3, 5, 0, 9]]


def test_levels_out_of_range_are_refused(oracle):
    A = np.zeros((4, 4), np.int64)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            MB.multiband(A, A, 0, 0, bad, oracle.corner_ramps)


# ---- host routing -----------------------------------------------------------------------------------------------------------------
class MultibandOracleEngine(OracleEngine):
    """the CPU double with the new operator: the numpy reference, recording what reached it"""
    def __init__(self, oracle):
        super().__init__(oracle)
        self.mb_calls = []

    def fuse_multiband_i64(self, A, B, dx, dy, levels=4, return_info=False):
        self.mb_calls.append((np.array(A, copy=True), np.array(B, copy=True), dx, dy, levels))
        return MB.multiband(A, B, dx, dy, levels, self.O.corner_ramps)


def test_fuse_image_routes_raw_regions_and_levels(oracle):
    eng = MultibandOracleEngine(oracle)
    s = isa.Stitcher(); s._engine = eng; s.isColorMode = False
    s.fuseMethod = "multiBandBlending"; s.multiBandLevels = 3
    rng = np.random.default_rng(2)
    A = rng.integers(0, 256, (12, 40)).astype(np.int64); A[:, :9] = -1
    B = rng.integers(0, 256, (12, 40)).astype(np.int64)
    A0 = A.copy()
    out = s.fuseImage([A, B], 4, -3)
    (gA, gB, dx, dy, levels), = eng.mb_calls
    assert np.array_equal(gA, A0) and (gA == -1).any()          # raw -1 regions, not zero-filled
    assert (dx, dy, levels) == (4, -3, 3)
    assert np.array_equal(out, MB.multiband(A0, B, 4, -3, 3, oracle.corner_ramps))
    assert np.array_equal(A, np.where(A0 < 0, B, A0))             # A's holes filled in place, as the fade does
    assert isa.Method.multiBandLevels == 4 and isa.ImageFusion.multiBandLevels == 4


def test_image_fusion_one_argument_call(oracle):
    f = isa.ImageFusion(); f._engine = MultibandOracleEngine(oracle)
    A = np.full((6, 8), 40, np.int64); B = np.full((6, 8), 40, np.int64)
    out = f.fuseByMultiBandBlending([A, B])
    assert out.dtype == np.uint8 and np.all(out == 40)
    assert f._engine.mb_calls[0][2:] == (0, 0, 4)


def test_optimal_seam_line_still_raises(oracle):
    s = isa.Stitcher(); s._engine = MultibandOracleEngine(oracle); s.isColorMode = False
    s.fuseMethod = "optimalSeamLine"
    with pytest.raises(NotImplementedError):
        s.fuseImage([np.zeros((2, 2), np.int64), np.zeros((2, 2), np.int64)], 0, 0)


@pytest.mark.parametrize("color", [False, True])
def test_get_stitch_by_offset_with_multiband_on_the_cpu_double(oracle, tmp_path, color):
    """getStitchByOffset with an engine that has no canvas multi-band entry point: the int64 / -1 walk, every overlap through
    fuseImage -> the engine's fuse_multiband_i64 with multiBandLevels; the mosaic equals the reference's walk restated here"""
    from test_host_logic import _write_tiles
    from imagestitch_amd.synthetic import SyntheticGrid
    from imagestitch_amd.stitcher import _imread
    g = SyntheticGrid(2, 2, 96, blobs=True)
    tiles = g.tiles(threads=1)
    if color:
        tiles = [np.stack([t, 255 - t, t // 2], -1).astype(np.uint8) for t in tiles]
    offs = [list(map(int, o)) for o in g.true_offsets()]
    files = _write_tiles(tmp_path, tiles, "mbh%d" % int(color))
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = color
        eng = MultibandOracleEngine(oracle)
        s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.isColorMode = color
        s.fuseMethod = "multiBandBlending"; s.multiBandLevels = 2
        got = s.getStitchByOffset(files, [list(o) for o in offs])
        # the reference's walk (Stitcher.py:434-486) with the numpy blend
        ims = [_imread(f, color).astype(np.int64) for f in files]
        origin = [[0, 0]] + offs
        offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout([im.shape for im in ims], origin)
        canvas = np.full((rows, cols, 3) if color else (rows, cols), -1, np.int64)
        for i, im in enumerate(ims):
            oy, ox = offsetList[i]
            if i == 0:
                canvas[oy:oy + im.shape[0], ox:ox + im.shape[1]] = im
                continue
            y0, x0 = max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0])
            y1, x1 = min(oy + im.shape[0], rangeX[i - 1][1]), min(ox + im.shape[1], rangeY[i - 1][1])
            A = canvas[y0:y1, x0:x1].copy()
            canvas[oy:oy + im.shape[0], ox:ox + im.shape[1]] = im
            B = canvas[y0:y1, x0:x1].copy()
            canvas[y0:y1, x0:x1] = MB.multiband(A, B, origin[i][0], origin[i][1], 2, oracle.corner_ramps)
        canvas[canvas == -1] = 0
        assert np.array_equal(got, canvas.astype(np.uint8))
        assert len(eng.mb_calls) == 3 and all(c[4] == 2 for c in eng.mb_calls)
        assert any((c[0] == -1).any() for c in eng.mb_calls)           # the raw -1 regions reached the engine
    finally:
        isa.Stitcher.isColorMode = old
