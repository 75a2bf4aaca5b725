"""Cases and accounting shared by test_phase_cases_host.py and test_phase_transforms_gpu.py: every length the LDS phase transforms of
csrc/phase_kernels.hip can run at, peaks placed on the border of the surface, degenerate strips, batches whose jobs differ, the workgroup
geometries, one-row / one-column strips.  Everything is deterministic (fixed seeds).

make_sched / own_shape below restate the host side of phase_kernels.hip (make_sched, phase_own_shape).  They CHOOSE and COUNT cases (which
lengths exist, which radix runs where, which geometry settings the host clamps back); no value is ever checked against them: the values
come from tests/phase_numpy.py (pocketfft) and oracle/vfsms_oracle.c (own mixed-radix transform).

THE TIGHT BOUND.  The project's bound on a phase result (1e-6 px relative to max(1, |offset|), 1e-9 in the response) lets a transform pass
that is wrong by a small constant.  The two references share no transform code; over exactly the planted pairs of the length sweep below
they disagree by REF_DISAGREE_PX / REF_DISAGREE_RESPONSE at the most (test_phase_cases_host.py measures it and fails if the constants
understate it).  The device differs from either in pass order, FMA use and twiddles formed by up to four products -- all O(eps log N),
like the references' own differences -- so 100 times their disagreement is the bound it is held to.
The position is a quotient, sum(x v) / sum(v) over the 5 x 5 window, and response = sum(v) / (M N): where the window sum is next to zero
the quotient magnifies any rounding by 1 / |response|.  One planted pair of the sweep is like that -- (3, 4): the window covers the whole
3 x 4 surface, whose sum is the DC bin x / (x^2 + eps) of the cross power, response 3e-7, offsets in the millions of pixels, and the
references themselves 5.3e-10 apart -- so the disagreement is measured, and the tight bound applied, as deviation x min(1, |response|)
(the reference's response).  For every other case of the sweep that factor is between 0.014 and 1."""
import functools

import numpy as np

from phase_numpy import optimal_dft_size, phase_correlate as np_phase
import phase_resolve_ref as PR

# Largest disagreement of phase_numpy.phase_correlate and the oracle over the 354 planted pairs of the sweep, measured by
# test_phase_cases_host.py::test_reference_disagreement_fixes_the_tight_bound: 4.94e-14 px relative to max(1, |offset|), times
# min(1, |response|), at (625, 640); 1.55e-15 in the response, at (3, 50).  (Unweighted, the px figure is 5.33e-10, at (3, 4) alone;
# the next is 5.06e-14.)  The constants round that up.
REF_DISAGREE_PX = 5e-14
REF_DISAGREE_RESPONSE = 1.6e-15
TIGHT_PX = 100 * REF_DISAGREE_PX                  # 5e-12 px, relative to max(1, |offset|), divided by min(1, |response|)
TIGHT_RESPONSE = 100 * REF_DISAGREE_RESPONSE      # 1.6e-13
OUTER_PX, OUTER_RESPONSE = 1e-6, 1e-9             # the project's bound: the outer limit

PEAKS = 4                                          # K of the unrelated pairs
RESOLVE_THRESHOLD, RESOLVE_MIN_PIXELS = 0.5, 64
MAX_DROPPED = 0.05                                 # of the unrelated pairs, by peak_gap_ok on the reference


def rand_img(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


# ---- the host side of phase_kernels.hip, restated for choosing and counting ---------------------------------------------------------
PHASE_LDS_MAX = 162816
RADICES = (16, 9, 8, 6, 10, 4, 3, 5, 2)


def five_smooth(lo, hi):
    return sorted(n for n in range(lo, hi + 1) if optimal_dft_size(n) == n)


def fft_lp(L):
    return L + (L >> 4) + 1


def make_sched(L):
    """-> [(R, Ls)]: the radix of every pass and the length done before it (Ls == 1: a first pass, without twiddles)"""
    a = b = c = 0
    rest = L
    while rest % 2 == 0:
        a += 1; rest //= 2
    while rest % 3 == 0:
        b += 1; rest //= 3
    while rest % 5 == 0:
        c += 1; rest //= 5
    assert rest == 1, L
    rs = []
    while a >= 4:
        rs.append(16); a -= 4
    if a == 3:
        rs.append(8)
    if a == 2:
        rs.append(4)
    if a == 1:
        if b >= 1:
            rs.append(6); b -= 1
        elif c >= 1:
            rs.append(10); c -= 1
        else:
            rs.append(2)
    while b >= 2:
        rs.append(9); b -= 2
    if b:
        rs.append(3)
    rs += [5] * c
    out, Ls = [], 1
    for R in rs:
        out.append((R, Ls)); Ls *= R
    assert Ls == L
    return out


def _round64(x):
    return min(512, max(64, (x + 63) // 64 * 64))


PLAN_KEYS = ("lds_transforms", "transposed", "M", "N", "columns_per_workgroup", "rows_per_workgroup", "row_threads", "column_threads")


def own_shape(h, w, rowpts=2048, tdiv=8, C=4, tcol=None):
    """what engine.phase_plan(h, w) answers under VFSMS_PHASE_ROWPTS / _TDIV / _C / _TCOL (defaults: unset)"""
    Mo, No = optimal_dft_size(h), optimal_dft_size(w)
    tr = int(Mo > No)
    for _attempt in range(2):
        M, N = (No, Mo) if tr else (Mo, No)
        tr_now, tr = tr, 1 - tr
        if N % 2 or N < 4 or M < 2:
            continue
        H = N // 2
        if H > 4096:
            continue
        RPW = max(1, min(16, max(1, rowpts) // H))
        td = max(1, tdiv)
        Trow = _round64((RPW * H + td - 1) // td)
        if RPW * H > 8 * Trow or 16 * RPW * fft_lp(H) > PHASE_LDS_MAX:
            continue
        c = C
        while c >= 2 and (16 * 2 * c * fft_lp(M) > PHASE_LDS_MAX or 2 * c * M > 4096):
            c >>= 1
        if c < 2:
            continue
        c = 1 << (c.bit_length() - 1)
        Tcol = _round64(tcol if tcol is not None else (2 * c * M + td - 1) // td)
        if 2 * c * M > 8 * Tcol:
            Tcol = _round64((2 * c * M + 7) // 8)
        return dict(zip(PLAN_KEYS, (1, tr_now, M, N, c, RPW, Trow, Tcol)))
    return dict(zip(PLAN_KEYS, (0, 0, Mo, No, 0, 0, 0, 0)))


# ---- 1. the length sweep -------------------------------------------------------------------------------------------------------------
ROW_HALF_LENGTHS = five_smooth(2, 4096)            # 136: every H = N / 2 of a packed real row
COL_LENGTHS = five_smooth(2, 1024)                 # 86: every column length M (2 C M <= 4096 with C >= 2)
ROW_GROUPS, COL_GROUPS = 9, 3                      # about 30 shapes per test item; dealt round-robin, so that every item has short and long ones


@functools.lru_cache(maxsize=None)
def row_shapes():
    """(3, 2 H) for every H, and (3, 2 H - 1) where that still pads to 2 H (the last real sample of a row is the padding's)"""
    out = []
    for H in ROW_HALF_LENGTHS:
        out.append((3, 2 * H))
        if optimal_dft_size(2 * H - 1) == 2 * H:
            out.append((3, 2 * H - 1))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def col_shapes():
    """(M, M) for an even M >= 4; else (M, w), w the smallest even five-smooth length >= max(M, 4): the row axis stays the long one"""
    out = []
    for M in COL_LENGTHS:
        if M % 2 == 0 and M >= 4:
            out.append((M, M))
        else:
            w = max(M, 4)
            while w % 2 or optimal_dft_size(w) != w:
                w += 1
            out.append((M, w))
    return tuple(out)


def sweep_shapes():
    return row_shapes() + col_shapes()


def sweep_groups():
    """-> [(name, shapes)]"""
    return ([("rows%d" % g, row_shapes()[g::ROW_GROUPS]) for g in range(ROW_GROUPS)] +
            [("cols%d" % g, col_shapes()[g::COL_GROUPS]) for g in range(COL_GROUPS)])


def _seed(shape):
    return sweep_shapes().index(shape)


def planted_shift(shape):
    return min(5, shape[0] // 3), -min(9, shape[1] // 3)


def planted(seed, shape, shift=None):
    """a random strip and its circular shift plus noise >> 3: one dominant peak, a well-conditioned centroid"""
    a = rand_img(300000 + seed, shape)
    dy, dx = planted_shift(shape) if shift is None else shift
    b = np.roll(np.roll(a, dy, 0), dx, 1)
    b = (b.astype(np.int32) + (rand_img(400000 + seed, shape) >> 3)).clip(0, 255).astype(np.uint8)
    return a, b


def planted_pair(shape):
    return planted(_seed(shape), shape)


def unrelated_pair(shape):
    k = _seed(shape)
    return rand_img(500000 + k, shape), rand_img(600000 + k, shape)


_refs = {}


def refs(key, a, b, oracle):
    """(x, y, response) of both references for the pair (a, b), computed once per key -> (numpy's, the oracle's, numpy's peak position)"""
    if key not in _refs:
        (nx, ny), nr, pos = np_phase(a, b)
        (ox, oy), orr = oracle.phase_correlate(np.ascontiguousarray(a), np.ascontiguousarray(b))
        _refs[key] = ((nx, ny, nr), (ox, oy, orr), pos)
    return _refs[key]


def planted_refs(shape, oracle):
    return refs(("planted", shape), *planted_pair(shape), oracle)


@functools.lru_cache(maxsize=None)
def unrelated_ref(shape):
    """-> (the K peak positions of the reference surface, does the list stand clear of the transform's rounding)"""
    R = PR.surface(*unrelated_pair(shape))
    return PR.peaks(R, PEAKS)[0], PR.peak_gap_ok(R, PEAKS)


def deviation(got, want):
    """(x, y, response) against a reference's -> (px relative to max(1, |offset|), response), as the bounds are stated"""
    return (max(abs(got[0] - want[0]) / max(1.0, abs(want[0])), abs(got[1] - want[1]) / max(1.0, abs(want[1]))), abs(got[2] - want[2]))


def conditioning(want):
    """the factor the tight bound's px figure is taken with: min(1, |response|) of the reference (see the module's docstring)"""
    return min(1.0, abs(want[2]))


worst = {"px": 0.0, "px x conditioning": 0.0, "response": 0.0}      # the largest device deviation seen in this process: for information only


def hold(got, numpy_ref, oracle_ref, what):
    """the bounds of item 1(a): both references, the outer and the tight bound, truncated offsets equal (what Stitcher.py:231-232 keeps)"""
    for name, want in (("numpy", numpy_ref), ("oracle", oracle_ref)):
        px, rs = deviation(got, want)
        tight = px * conditioning(want)
        worst["px"] = max(worst["px"], px); worst["px x conditioning"] = max(worst["px x conditioning"], tight); worst["response"] = max(worst["response"], rs)
        assert px < OUTER_PX and rs < OUTER_RESPONSE, (what, name, got, want)
        assert tight < TIGHT_PX and rs < TIGHT_RESPONSE, (what, name, px, tight, rs, got, want)
        for g, o in zip(got[:2], want[:2]):
            if abs(o - round(o)) > 1e-9:
                assert int(g) == int(o), (what, name, got, want)


# ---- 2. peaks placed at the border ---------------------------------------------------------------------------------------------------
BORDER_SHAPES = [(16, 32), (32, 16), (45, 60), (60, 45), (25, 27), (48, 625), (625, 48)]      # h = M, w = N: the correlation is circular


def unshift2(ys, xs, M, N):
    """phasecorr.cpp's fftShift as a map shifted -> source (its own inverse): the quadrants of (M >> 1) x (N >> 1) swap diagonally, an odd
    last row or column stays where it is along both axes"""
    ym, xm = M >> 1, N >> 1
    if ys < 2 * ym and xs < 2 * xm:
        return (ys + ym if ys < ym else ys - ym), (xs + xm if xs < xm else xs - xm)
    return ys, xs


def border_targets(M, N):
    """positions on the SHIFTED surface: corners, edge midpoints, 1 and 2 elements inside each edge, the centre"""
    my, mx = M // 2, N // 2
    return ([(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1)] +
            [(0, mx), (M - 1, mx), (my, 0), (my, N - 1)] +
            [(1, mx), (2, mx), (M - 2, mx), (M - 3, mx), (my, 1), (my, 2), (my, N - 2), (my, N - 3)] +
            [(my, mx)])


@functools.lru_cache(maxsize=None)
def border_cases(shape):
    """-> [(target (py, px), a, b)]: b = a rolled so that the one near-delta of the surface lands on the target"""
    M, N = shape
    assert (optimal_dft_size(M), optimal_dft_size(N)) == (M, N)
    out = []
    for k, (ty, tx) in enumerate(border_targets(M, N)):
        uy, ux = unshift2(ty, tx, M, N)                     # R peaks at (-sy mod M, -sx mod N) for b = roll(a, (sy, sx))
        a = rand_img(700000 + 100 * BORDER_SHAPES.index(shape) + k, shape)
        out.append(((ty, tx), a, np.roll(np.roll(a, -uy, 0), -ux, 1)))
    return out


def border_refs(shape, k, oracle):
    _t, a, b = border_cases(shape)[k]
    return refs(("border", shape, k), a, b, oracle)


# ---- 3. degenerate strips ------------------------------------------------------------------------------------------------------------
DEGENERATE_SHAPES = [(16, 32), (15, 20), (409, 2048), (2048, 409)]
CONSTANT_SHAPES = [(16, 32), (15, 20)]


def degenerate_pairs(shape):
    """zeros against zeros and against content, either way round: the surface is exactly zero -> ((N / 2, M / 2), 0.0) exactly"""
    z, r = np.zeros(shape, np.uint8), rand_img(800000 + DEGENERATE_SHAPES.index(shape), shape)
    return [("zeros, zeros", z, z), ("zeros, content", z, r), ("content, zeros", r, z)]


def degenerate_result(shape):
    return (optimal_dft_size(shape[1]) / 2.0, optimal_dft_size(shape[0]) / 2.0, 0.0)


# ---- 4. batches whose jobs differ ----------------------------------------------------------------------------------------------------
BATCH_SHAPES = [(24, 80), (80, 24)]                # one per orientation: the second is correlated as its transpose
BATCH_SHIFTS = [(5, -9), (-3, 20), (0, 0), (11, 33), (-7, -1), (2, 40), (9, -25)]
BATCH_K = 2
CHUNKS = (None, "1", "2", "3")
MANY = 70                                          # jobs of (80, 24): chunks of 32 + 32 + 6


@functools.lru_cache(maxsize=None)
def batch_strips(shape, n=len(BATCH_SHIFTS)):
    """n DISTINCT planted pairs of one shape, every one with its own content and its own shift -> [(name, a, b)]"""
    h, w = shape
    out = []
    for k in range(n):
        s, lap = BATCH_SHIFTS[k % len(BATCH_SHIFTS)], k // len(BATCH_SHIFTS)
        sh = (s[0] + 2 * lap, s[1] - 3 * lap)
        if h > w:
            sh = (sh[1], sh[0])
        out.append(("%dx%d #%d" % (h, w, k),) + planted(900000 + 1000 * BATCH_SHAPES.index(shape) + k, shape, sh))
    return out


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """the seven pairs of each shape, interleaved"""
    return [s for pair in zip(batch_strips(BATCH_SHAPES[0]), batch_strips(BATCH_SHAPES[1])) for s in pair]


@functools.lru_cache(maxsize=None)
def mixed_batch_resolved():
    """phase_resolve_ref.resolve of every job of the mixed batch -> [(dict, peak_gap_ok of its surface)]"""
    out = []
    for _n, a, b in mixed_batch():
        R = PR.surface(a, b)
        out.append((PR.resolve(a, b, BATCH_K, RESOLVE_THRESHOLD, RESOLVE_MIN_PIXELS, R=R), PR.peak_gap_ok(R, BATCH_K)))
    return out


def resident(engine, strips, pad=(3, 7)):
    """every strip inside a tile of its own, at an odd corner and with a row stride that is no multiple of 16: the sums kernel's head /
    body / tail split and the funnel shift see every alignment -> (handles, jobs)"""
    handles, jobs = [], []
    for k, (_n, A, B) in enumerate(strips):
        h, w = A.shape
        oy, ox = (pad[0] + k % 2, pad[1] + k % 5)
        ta = np.full((h + oy + 2, w + ox + 5), 9, np.uint8); tb = np.full((h + 3, w + 11 + k % 3), 200, np.uint8)
        ta[oy:oy + h, ox:ox + w] = A; tb[1:1 + h, 2 + k % 3:2 + k % 3 + w] = B
        ha, hb = engine.tile_upload(ta), engine.tile_upload(tb)
        handles += [ha, hb]
        jobs.append((ha, hb, oy, ox, 1, 2 + k % 3, h, w))
    return handles, jobs


# ---- 5. workgroup geometry -----------------------------------------------------------------------------------------------------------
GEOMETRY_SHAPES = [(3, 4), (3, 90), (3, 864), (3, 2048), (3, 2499), (3, 3000), (3, 8192),            # H = 2, 45, 432, 1024, 1250, 1500, 4096
                   (2, 4), (6, 6), (81, 90), (250, 250), (432, 432), (625, 640), (1024, 1024),      # M = 2, 6, 81, 250, 432, 625, 1024
                   (409, 2048), (2048, 409)]                                                        # the production strips, both orientations
GEOMETRY_SETTINGS = [("VFSMS_PHASE_C", "2"), ("VFSMS_PHASE_C", "8"), ("VFSMS_PHASE_ROWPTS", "1"), ("VFSMS_PHASE_ROWPTS", "4096"),
                     ("VFSMS_PHASE_TDIV", "4"), ("VFSMS_PHASE_TDIV", "16"), ("VFSMS_PHASE_TCOL", "64")]
GEOMETRY_KEYS = ("columns_per_workgroup", "rows_per_workgroup", "row_threads", "column_threads")
_KNOB_ARG = {"VFSMS_PHASE_C": "C", "VFSMS_PHASE_ROWPTS": "rowpts", "VFSMS_PHASE_TDIV": "tdiv", "VFSMS_PHASE_TCOL": "tcol"}


def geometry_takes(plan, default):
    """does a plan under a setting run the LDS transforms of the default plan's problem with another workgroup geometry?  (The host clamps
    a setting back -- or, where the rows of a workgroup no longer fit its threads, leaves the LDS path: both are skipped and counted.)"""
    return bool(plan["lds_transforms"] == 1 and [plan[k] for k in PLAN_KEYS[:4]] == [default[k] for k in PLAN_KEYS[:4]] and
                any(plan[k] != default[k] for k in GEOMETRY_KEYS))


def geometry_restated(shape, knob, value):
    return own_shape(*shape, **{_KNOB_ARG[knob]: int(value)})


def geometry_pair(shape):
    return planted(950000 + GEOMETRY_SHAPES.index(shape), shape)


# ---- 6. one-row and one-column strips ------------------------------------------------------------------------------------------------
VECTOR_SHAPES = [s for n in (2, 3, 8, 9, 15, 16) for s in ((1, n), (n, 1))]


def vector_pair(shape):
    k = VECTOR_SHAPES.index(shape)
    n = max(shape)
    a = rand_img(980000 + k, shape)
    b = np.roll(a, n // 3, int(shape[1] > 1))
    if n >= 8:
        b = (b.astype(np.int32) + (rand_img(990000 + k, shape) >> 3)).clip(0, 255).astype(np.uint8)
    return a, b


def vector_refs(shape, oracle):
    return refs(("vector", shape), *vector_pair(shape), oracle)
