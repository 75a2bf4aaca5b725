"""CPU tests of fuseMethod "optimalSeamLine": tests/seam_ref.py (the specification the HIP kernels are checked against) pinned against an
exhaustive search over all connected seams and a scalar restatement of the energy, its properties, corner mode on the fade fixtures,
and the host routing of Stitcher / ImageFusion on a CPU test double."""
import itertools
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from fakes import OracleEngine

import multiband_ref as MB
import seam_ref as SR


def _no_corner(A):
    raise AssertionError("strip geometry expected")


# ---- independent restatements ---------------------------------------------------------------------------------------------------------
def _energy_loop(A, B):
    """the docstring's energy, one pixel at a time"""
    A = np.asarray(A, np.int64); B = np.asarray(B, np.int64)
    if A.ndim == 2:
        A = A[:, :, None]; B = B[:, :, None]
    r, c, ch = A.shape

    def valid(X, i, j):
        return X[i, j, 0] != -1 if ch == 1 else int(X[i, j].sum()) != -3

    def d(i, j, k):
        a, b = int(A[i, j, k]), int(B[i, j, k])
        a1 = a if a >= 0 else b
        b1 = b if b >= 0 else a1
        return max(a1, 0) - max(b1, 0)
    E = np.zeros((r, c), np.int64)
    for i in range(r):
        for j in range(c):
            if not (valid(A, i, j) and valid(B, i, j)):
                continue
            jm, jp, im, ip = max(j - 1, 0), min(j + 1, c - 1), max(i - 1, 0), min(i + 1, r - 1)
            E[i, j] = sum(abs(d(i, j, k)) + abs(d(i, jp, k) - d(i, jm, k)) + abs(d(ip, j, k) - d(im, j, k)) for k in range(ch))
    return E


def _brute_seam(E):
    """every connected seam of an L x W plane; the minimum, ties broken as the forward pass breaks them: the lowest end position, then the
    lowest predecessor at every step back (= the lexicographic minimum of the seam read from its last step)"""
    L, W = E.shape
    best = None
    for p0 in range(W):
        for moves in itertools.product((-1, 0, 1), repeat=L - 1):
            s = [p0]
            for m in moves:
                s.append(s[-1] + m)
            if min(s) < 0 or max(s) >= W:
                continue
            key = (sum(int(E[t, s[t]]) for t in range(L)), tuple(reversed(s)))
            if best is None or key < best:
                best = key
    return np.array(list(reversed(best[1])), np.int64), best[0]


def _region(rng, r, c, ch, levels, holes):
    shape = (r, c) if ch == 1 else (r, c, ch)
    A = rng.integers(0, levels, shape).astype(np.int64); B = rng.integers(0, levels, shape).astype(np.int64)
    if holes and r * c >= 6:
        A[rng.integers(0, r), rng.integers(0, c)] = -1
        B[rng.integers(0, r), rng.integers(0, c)] = -1
    return A, B


def test_energy_matches_the_scalar_restatement():
    rng = np.random.default_rng(3)
    for (r, c) in ((1, 1), (1, 4), (3, 1), (4, 5), (6, 3)):
        for ch in (1, 3):
            for holes in (False, True):
                A, B = _region(rng, r, c, ch, 256, holes)
                assert np.array_equal(SR.energy(A, B), _energy_loop(A, B)), (r, c, ch, holes)
    A = np.array([[-1, -1, -1], [9, 9, 9]], np.int64).reshape(1, 2, 3)       # a colour pixel that is all -1 is empty, a partly -1 one is not
    B = np.full((1, 2, 3), 50, np.int64)
    E = SR.energy(A, B)
    assert E[0, 0] == 0 and E[0, 1] > 0
    assert SR.energy(np.full((3, 3), 255, np.int64), np.zeros((3, 3), np.int64)).max() == 255      # a constant difference has no gradient
    X = np.zeros((3, 3, 4), np.int64); X[1, 1] = 255; X[0, 1] = 255; X[1, 0] = 255
    assert SR.energy(X, np.zeros((3, 3, 4), np.int64)).max() <= SR.E_MAX


def test_the_seam_is_the_exhaustive_minimum():
    """every region up to 6 x 5 of a seeded random set: gray and colour, both strip orientations, both signs of dy / dx, holes, and
    energies from so few grey levels that ties are the rule"""
    rng = np.random.default_rng(17)
    n = n_tied = 0
    for r in range(1, 7):
        for c in range(1, 6):
            for ch in (1, 3):
                for levels in (2, 3, 256):
                    for holes in (False, True):
                        for sgn in (1, -1):
                            A, B = _region(rng, r, c, ch, levels, holes)
                            if np.count_nonzero(A > -1) / A.size <= 0.65:
                                continue
                            dx, dy = 3 * sgn, 2 * sgn
                            sv, sh, label, cost = SR.seams(A, B, dx, dy, _no_corner)
                            E = _energy_loop(A, B)
                            if c <= r:
                                assert sh is None
                                want, total = _brute_seam(E)
                                assert np.array_equal(sv, want) and cost[0] == total, (r, c, ch, levels, holes, sgn)
                                j = np.arange(c)[None, :]
                                side = j < want[:, None] if dy >= 0 else j > want[:, None]
                            else:
                                assert sv is None
                                want, total = _brute_seam(E.T)
                                assert np.array_equal(sh, want) and cost[1] == total, (r, c, ch, levels, holes, sgn)
                                i = np.arange(r)[:, None]
                                side = i > want[None, :] if dx <= 0 else i < want[None, :]
                            assert np.array_equal(label, side & SR.pixel_valid(A))
                            n += 1
                            n_tied += len({int(x) for x in np.unique(E)}) < E.size
    assert n > 600 and n_tied > 300, (n, n_tied)


def test_ties_made_on_purpose():
    E = np.zeros((4, 5), np.int64)
    s, total = SR.strip_seam(E)
    assert total == 0 and s.tolist() == [0, 0, 0, 0]                      # lowest end, lowest predecessor
    E = np.array([[5, 1, 5, 1, 5], [5, 5, 1, 5, 5], [5, 1, 5, 1, 5]], np.int64)
    s, total = SR.strip_seam(E)
    want, wtotal = _brute_seam(E)
    assert total == wtotal == 3 and s.tolist() == want.tolist() == [1, 2, 1]
    E = np.array([[0, 9, 0], [9, 9, 9], [9, 0, 9]], np.int64)
    s, _ = SR.strip_seam(E)
    assert s.tolist() == _brute_seam(E)[0].tolist() == [0, 0, 1]
    with pytest.raises(ValueError):
        SR.strip_seam(np.zeros((2 ** 31 // 5100 + 1, 1), np.int64))


# ---- properties -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("blend", ["none", "multiBandBlending"])
def test_identical_inputs_give_the_input_back(blend):
    rng = np.random.default_rng(4)
    for shape in ((1, 1), (3, 8), (37, 23), (24, 30, 3), (40, 17, 3)):
        A = rng.integers(0, 256, shape).astype(np.int64)
        for dx, dy in ((3, -2), (-3, 2)):
            out = SR.seam_fuse(A, A.copy(), dx, dy, blend, 3, _no_corner)
            assert out.dtype == np.uint8 and np.array_equal(out, A.astype(np.uint8)), (shape, blend)


@pytest.mark.parametrize("tall", [True, False])
def test_planted_corridor_is_found(tall):
    """A and B agree on a 3-wide band around a wandering path and differ by a constant elsewhere: the path's cells have zero energy
    (their four neighbours lie in the band or carry the same difference), so the seam costs 0 and runs inside the band"""
    rng = np.random.default_rng(8)
    L, W = 60, 31
    path = [15]
    for _ in range(L - 1):
        path.append(int(np.clip(path[-1] + rng.integers(-1, 2), 2, W - 3)))
    path = np.array(path)
    A = rng.integers(60, 200, (L, W)).astype(np.int64)
    band = np.abs(np.arange(W)[None, :] - path[:, None]) <= 1
    B = np.where(band, A, A + 40)
    if not tall:
        A, B, band = A.T.copy(), B.T.copy(), band.T
    sv, sh, _label, cost = SR.seams(A, B, 1, 1, _no_corner)
    s, total = (sv, cost[0]) if tall else (sh, cost[1])
    assert total == 0
    on_band = band[np.arange(L), s] if tall else band[s, np.arange(L)]
    assert on_band.all()


def _straight_seam_cost(A, B, dx, dy):
    """the cost of the straight seam where the fade's weights tie: the first B position next to A's side of M0"""
    M = MB.seam_mask(A, dx, dy, _no_corner)
    E = SR.energy(A, B)
    r, c = M.shape
    if c <= r:
        b_cols = np.flatnonzero(M[0] == 0)
        col = int(b_cols[0] if dy >= 0 else b_cols[-1]) if len(b_cols) else (c - 1 if dy >= 0 else 0)
        return int(E[:, col].sum())
    b_rows = np.flatnonzero(M[:, 0] == 0)
    row = int(b_rows[-1] if dx <= 0 else b_rows[0]) if len(b_rows) else (0 if dx <= 0 else r - 1)
    return int(E[row, :].sum())


def test_never_worse_than_the_straight_seam_and_never_mixes(oracle):
    rng = np.random.default_rng(21)
    mixed = 0
    for shape in ((40, 12), (12, 40), (33, 33), (30, 9, 3), (9, 30, 3)):
        for dx, dy in ((4, 6), (-4, -6)):
            A = rng.integers(0, 256, shape).astype(np.int64); B = rng.integers(0, 256, shape).astype(np.int64)
            A[0, 0] = -1
            _sv, _sh, _label, cost = SR.seams(A, B, dx, dy, _no_corner)
            total = cost[0] if cost[0] is not None else cost[1]
            assert total <= _straight_seam_cost(A, B, dx, dy), (shape, dx, dy)
            out = SR.seam_fuse(A, B, dx, dy, "none", 4, _no_corner)
            A1, B1 = MB.fill(A, B)
            assert np.all((out == A1) | (out == B1)), shape                  # every output pixel is a pixel of one input
            assert (out == A1).any() and (out == B1).any()
            fade = oracle.fuse_fade(A.copy(), B, dx, dy)
            mixed += int(np.count_nonzero((fade != A1) & (fade != B1)))      # ... which the fade is not
    assert mixed > 1000


# ---- corner mode ------------------------------------------------------------------------------------------------------------------------
def _corner_fixtures(golden_dir):
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        A, B = g["f%d_A" % i], g["f%d_B" % i]
        if np.count_nonzero(A > -1) / A.size <= 0.65:
            yield i, A, B, int(dx), int(dy)


def test_corner_mode_on_the_fade_fixtures(oracle, golden_dir):
    """L-shaped validity patterns (the fade's corner fixtures), all four `index` values: each arm's seam is the strip solver's on that
    arm's cells of the region's energy, the arm contains every index the fade's ramp touches, A's side is toward the edge where the ramp
    gives B weight 0, and a pixel is A iff it is A-valid and on A's side of either seam; geometries the fade refuses are refused"""
    seen, refused = set(), 0
    for i, A, B, dx, dy in _corner_fixtures(golden_dir):
        try:
            wr, wc, info = oracle.corner_ramps(A)
        except IndexError:
            with pytest.raises(IndexError):
                SR.seam_fuse(A, B, dx, dy, "none", 4, oracle.corner_ramps)
            with pytest.raises(IndexError):
                oracle.fuse_fade(A.copy(), B, dx, dy)
            refused += 1
            continue
        index, rowIndex, colIndex = int(info[1]), int(info[2]), int(info[3])
        r, c = A.shape[:2]
        sv, sh, label, _cost = SR.seams(A, B, dx, dy, oracle.corner_ramps)
        E = _energy_loop(A, B) if r * c <= 4000 else SR.energy(A, B)
        side = np.zeros((r, c), bool)
        for n, at, up, ramp, s, is_h in ((r, rowIndex, index in (2, 1), wr, sh, True), (c, colIndex, index in (2, 3), wc, sv, False)):
            arm = ((0, at) if at >= 1 else None) if up else (max(at, 0), n - 1)
            touched = np.flatnonzero(np.asarray(ramp) != 1)
            if arm is None:
                assert s is None and len(touched) == 0, i
                continue
            lo, hi = arm
            assert len(touched) == 0 or (lo <= touched.min() and touched.max() <= hi), i
            assert ramp[lo if up else hi] == 0 or hi == lo, i                 # the arm's edge on A's side is where B's weight is 0
            sub = E[lo:hi + 1, :].T if is_h else E[:, lo:hi + 1]
            want, _total = SR.strip_seam(sub)
            assert np.array_equal(s, want + lo), i
            if sub.shape[0] <= 6 and sub.shape[1] <= 5:
                assert np.array_equal(want, _brute_seam(sub)[0]), i
            if is_h:
                ii = np.arange(r)[:, None]
                side |= (ii < s[None, :]) if up else (ii > s[None, :])
            else:
                jj = np.arange(c)[None, :]
                side |= (jj < s[:, None]) if up else (jj > s[:, None])
        assert np.array_equal(label, side & SR.pixel_valid(A)), i
        out, seam = SR.seam_fuse(A, B, dx, dy, "none", 4, oracle.corner_ramps, return_seam=True)
        A1, B1 = MB.fill(A, B)
        lab = label if A.ndim == 2 else label[:, :, None]
        assert np.array_equal(out, np.where(lab, A1, B1).astype(np.uint8)), i
        assert seam.dtype == np.int32 and seam.shape == (r + c,)
        assert np.array_equal(seam[:r], sv if sv is not None else np.full(r, -1)) and np.array_equal(seam[r:], sh if sh is not None else np.full(c, -1))
        seen.add(index)
    assert seen == {0, 1, 2, 3}, (seen, refused)


def test_refused_geometry_and_bad_arguments(oracle):
    A = np.full((2, 2), -1, np.int64); A[0, 0] = 9
    B = np.full((2, 2), 50, np.int64)
    with pytest.raises(IndexError):
        SR.seam_fuse(A, B, 1, 1, "none", 4, oracle.corner_ramps)
    rng = np.random.default_rng(12)
    refused = accepted = 0
    for _ in range(300):                                     # small L-shaped patterns: refused exactly where the fade refuses
        r, c = int(rng.integers(2, 7)), int(rng.integers(2, 7))
        A = np.full((r, c), -1, np.int64)
        a, b = int(rng.integers(0, r)), int(rng.integers(0, c))
        quad = int(rng.integers(0, 4))
        A[(slice(0, a + 1), slice(a, r))[quad & 1], :] = 7
        A[:, (slice(0, b + 1), slice(b, c))[quad >> 1]] = 7
        A[(slice(a + 1, r), slice(0, a))[quad & 1], (slice(b + 1, c), slice(0, b))[quad >> 1]] = -1
        if np.count_nonzero(A > -1) / A.size > 0.65:
            continue
        B = np.full((r, c), 50, np.int64)
        try:
            oracle.fuse_fade(A.copy(), B, 1, 1)
        except IndexError:
            refused += 1
            with pytest.raises(IndexError):
                SR.seam_fuse(A, B, 1, 1, "none", 4, oracle.corner_ramps)
            continue
        accepted += 1
        SR.seam_fuse(A, B, 1, 1, "none", 4, oracle.corner_ramps)
    assert refused > 0 and accepted > 10, (refused, accepted)
    Z = np.zeros((4, 4), np.int64)
    with pytest.raises(ValueError):
        SR.seam_fuse(Z, Z, 0, 0, "average", 4, oracle.corner_ramps)
    for bad in (0, 9):
        with pytest.raises(ValueError):
            SR.seam_fuse(Z, Z, 0, 0, "multiBandBlending", bad, oracle.corner_ramps)


def test_multiband_blend_takes_the_label_plane(oracle):
    rng = np.random.default_rng(6)
    A = rng.integers(0, 256, (40, 14)).astype(np.int64); B = rng.integers(0, 256, (40, 14)).astype(np.int64)
    _sv, _sh, label, _ = SR.seams(A, B, 2, 5, oracle.corner_ramps)
    want = np.clip(np.rint(MB.blend_planes(A.astype(MB.F), B.astype(MB.F), label.astype(MB.F), 3)), 0, 255).astype(np.uint8)
    got = SR.seam_fuse(A, B, 2, 5, "multiBandBlending", 3, oracle.corner_ramps)
    assert np.array_equal(got, want)
    assert not np.array_equal(got, MB.multiband(A, B, 2, 5, 3, oracle.corner_ramps))          # the fade-tie mask gives other bytes


# ---- host routing -----------------------------------------------------------------------------------------------------------------------
class SeamOracleEngine(OracleEngine):
    """the CPU double with the new operator: the numpy reference, recording what reached it"""
    def __init__(self, oracle):
        super().__init__(oracle)
        self.seam_calls = []

    def fuse_seam_i64(self, A, B, dx, dy, blend="none", levels=4, return_info=False, return_seam=False):
        self.seam_calls.append((np.array(A, copy=True), np.array(B, copy=True), dx, dy, blend, levels))
        return SR.seam_fuse(A, B, dx, dy, blend, levels, self.O.corner_ramps, return_seam=return_seam)


@pytest.mark.parametrize("blend", ["none", "multiBandBlending"])
def test_fuse_image_routes_raw_regions_blend_and_levels(oracle, blend):
    eng = SeamOracleEngine(oracle)
    s = isa.Stitcher(); s._engine = eng; s.isColorMode = False
    s.fuseMethod = "optimalSeamLine"; s.seamLineBlend = blend; s.multiBandLevels = 3
    rng = np.random.default_rng(2)
    A = rng.integers(0, 256, (12, 40)).astype(np.int64); A[:, :9] = -1
    B = rng.integers(0, 256, (12, 40)).astype(np.int64)
    A0 = A.copy()
    out = s.fuseImage([A, B], 4, -3)
    (gA, gB, dx, dy, gblend, levels), = eng.seam_calls
    assert np.array_equal(gA, A0) and (gA == -1).any() and np.array_equal(gB, B)          # raw -1 regions, not zero-filled
    assert (dx, dy, gblend, levels) == (4, -3, blend, 3)
    assert np.array_equal(out, SR.seam_fuse(A0, B, 4, -3, blend, 3, oracle.corner_ramps))
    assert np.array_equal(A, np.where(A0 < 0, B, A0))                                       # A's holes filled in place, as the fade does
    assert isa.Method.seamLineBlend == "none" and isa.ImageFusion.seamLineBlend == "none"


def test_image_fusion_one_argument_call(oracle):
    f = isa.ImageFusion(); f._engine = SeamOracleEngine(oracle)
    A = np.full((6, 8), 40, np.int64); B = np.full((6, 8), 40, np.int64)
    out = f.fuseByOptimalSeamLine([A, B])
    assert out.dtype == np.uint8 and np.all(out == 40)
    assert f._engine.seam_calls[0][2:] == (0, 0, "none", 4)


def test_engines_without_the_operator_cannot_run_the_method(oracle):
    s = isa.Stitcher(); s._engine = OracleEngine(oracle); s.isColorMode = False
    s.fuseMethod = "optimalSeamLine"
    A = np.array([[-1, 0, 7]], np.int64); B = np.array([[5, 6, 0]], np.int64)
    with pytest.raises(NotImplementedError):
        s.fuseImage([A, B], 0, 0)
    assert A.tolist() == [[-1, 0, 7]]                                 # nothing was touched
    f = isa.ImageFusion(); f._engine = OracleEngine(oracle)
    with pytest.raises(NotImplementedError):
        f.fuseByOptimalSeamLine([A, B], 0, 0)
    assert hasattr(isa.Engine, "fuse_seam_i64") and hasattr(isa.Engine, "canvas_set_seam_blend")


@pytest.mark.parametrize("color", [False, True])
def test_get_stitch_by_offset_with_the_seam_on_the_cpu_double(oracle, tmp_path, color):
    """getStitchByOffset with an engine that has no canvas seam entry point: the int64 / -1 walk, every overlap through fuseImage -> the
    engine's fuse_seam_i64; the mosaic equals the reference's walk restated here with seam_ref"""
    from test_host_logic import _write_tiles
    from imagestitch_amd.synthetic import SyntheticGrid
    from imagestitch_amd.stitcher import _imread
    g = SyntheticGrid(2, 2, 96, blobs=True)
    tiles = g.tiles(threads=1)
    if color:
        tiles = [np.stack([t, 255 - t, t // 2], -1).astype(np.uint8) for t in tiles]
    offs = [list(map(int, o)) for o in g.true_offsets()]
    files = _write_tiles(tmp_path, tiles, "smh%d" % int(color))
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = color
        eng = SeamOracleEngine(oracle)
        s = isa.Stitcher(); s._engine = eng; s.isPrintLog = False; s.isColorMode = color
        s.fuseMethod = "optimalSeamLine"
        got = s.getStitchByOffset(files, [list(o) for o in offs])
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
            canvas[y0:y1, x0:x1] = SR.seam_fuse(A, B, origin[i][0], origin[i][1], "none", 4, oracle.corner_ramps)
        canvas[canvas == -1] = 0
        assert np.array_equal(got, canvas.astype(np.uint8))
        assert len(eng.seam_calls) == 3 and all(c[4] == "none" for c in eng.seam_calls)
        assert any((c[0] == -1).any() for c in eng.seam_calls)           # the raw -1 regions reached the engine
    finally:
        isa.Stitcher.isColorMode = old
