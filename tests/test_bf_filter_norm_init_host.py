"""CPU check of the fp16 candidate filter of the 64-d 2-NN search in its trimmed form (csrc/match_kernels.hip: k_bf_split16,
k_bf_mfma16_d64): |t|^2 is the INITIAL VALUE of the float32 accumulator instead of a k-slot of its own, and pass 0 takes its bound
from every BFM_P0_STRIDE-th 32-train tile of a chunk plus the chunk's last tile.

The scores are emulated in numpy the way the sweeps form them: descriptors rounded to float16 (queries scaled by -2 first), the
accumulator starts at k_bf_split16's float32 sum of squares, and the 64 products (exact in float32) are added k-step by k-step --
k-step s holds dims 8s..8s+7 and 32+8s..32+8s+7, the lane halves' fragments -- with one float32 rounding per product, the most
roundings any summation order inside the matrix instruction can make (the derivation in the source counts one per slot).

  - |score - (|t|^2 - 2 q.t in float64)| <= BFM_F16_ERR (read from the source), and the derivation of the source comment, recomputed
    here term by term, stays under that constant;
  - window: with thr(q) = the second smallest of pass 0's values -- one minimum per (visited tile, lane half), rows 4h + (i & 3) +
    8 (i >> 2) of a tile belong to lane half h -- + 2 BFM_F16_ERR + BFM_MARGIN, both trains of the reference's 2-NN
    (oracle.bf_l2_knn2) score <= thr(q), for strides 1, 2, 4 and the committed BFM_P0_STRIDE, one chunk and eight;
  - the lists stay usable on the production strip: at most BFM_CAPL trains score <= thr(q) per (query, chunk, lane half), and at
    most BFV_HITS score within the verifier's cut (second smallest score + window) for >= 99 % of the queries.  These are conditions,
    asserted for the emulated scores and, so that they are seen to be a property of the inputs, for the float64 scores too; the
    stress rows (dozens of exact ties by construction) are not asked to meet them -- a list that overflows sends its query to the
    exhaustive scan, which tests/test_bf_fp16_gpu.py covers.

Inputs: the oracle's descriptors of one production strip pair, the stress rows of tests/test_bf_fp16_host.py (subnormal elements,
float16 ties, norms of exactly 1) and two more sets: duplicated rows, and squared norms at the 1.0001 limit.  No GPU."""
import re

import numpy as np
import pytest

from test_bf_fp16_host import ETA, NORM2_MAX, SRC, U, _constant, _exact, _stress_rows, _unit

STRIDES = (1, 2, 4)
KSTEP_DIMS = [list(range(8 * s, 8 * s + 8)) + list(range(32 + 8 * s, 32 + 8 * s + 8)) for s in range(4)]


def _int_constant(name):
    m = re.search(r"^#define\s+%s\s+([0-9]+)\b" % name, open(SRC).read(), re.M)
    assert m, name
    return int(m.group(1))


def _scores(q, t):
    """float32 scores as the sweeps form them: accumulator = float32 |t|^2, then 4 k-steps of 16 fp16 products each"""
    q16 = (np.float32(-2.0) * q).astype(np.float16).astype(np.float32)
    t16 = t.astype(np.float16).astype(np.float32)
    tot = np.zeros(len(t), np.float32)
    for d in range(64):                                           # k_bf_split16's sequential float32 sum (halves met at the end)
        tot += t[:, d] * t[:, d]
    acc = np.repeat(tot[None, :], len(q), axis=0)
    for dims in KSTEP_DIMS:
        for d in dims:
            acc += q16[:, d:d + 1] * t16[None, :, d]              # float32 x float32 of two fp16 values: exact; the add rounds once
    assert acc.dtype == np.float32
    return acc


def _visited_tiles(ntiles, nsplit, stride):
    """the tiles pass 0 sweeps: per chunk tile0, tile0 + stride, ... and the chunk's last"""
    tchunk = (ntiles + nsplit - 1) // nsplit
    out = []
    for sp in range(nsplit):
        tile0, tile1 = sp * tchunk, min(ntiles, (sp + 1) * tchunk)
        if tile1 <= tile0:
            continue
        nvis = (tile1 - tile0 - 1 + stride - 1) // stride + 1
        vis = [min(tile0 + k * stride, tile1 - 1) for k in range(nvis)]
        assert len(set(vis)) == len(vis) and vis[-1] == tile1 - 1 and (tile1 - tile0 > 2 or len(vis) == tile1 - tile0)
        out += vis
    return out


def _lane_half(nt):
    return (np.arange(nt) % 32 >> 2) & 1


def _pass0_m2(s, nsplit, stride):
    """second smallest of pass 0's values per query: one minimum per (visited tile, lane half); inf with fewer than two values"""
    nt = s.shape[1]
    half = _lane_half(nt)
    mins = []
    for tl in _visited_tiles((nt + 31) // 32, nsplit, stride):
        rows = np.arange(tl * 32, min(tl * 32 + 32, nt))
        for h in (0, 1):
            r = rows[half[rows] == h]
            if len(r):
                mins.append(s[:, r].min(1))
    if len(mins) < 2:
        return np.full(s.shape[0], np.inf)
    return np.partition(np.stack(mins, 1), 1, axis=1)[:, 1]


def _check(q, t, oracle, err, window):
    assert float((q.astype(np.float64) ** 2).sum(1).max()) <= NORM2_MAX and float((t.astype(np.float64) ** 2).sum(1).max()) <= NORM2_MAX
    s = _scores(q, t).astype(np.float64)
    dev = float(np.abs(s - _exact(q, t)).max())
    assert dev <= err, dev
    if len(t) >= 2:
        i1, _d1, i2, _d2 = oracle.bf_l2_knn2(q, t)
        rows = np.arange(len(q))
        s2 = np.partition(s, 1, axis=1)[:, 1]
        for stride in sorted(set(STRIDES + (_int_constant("BFM_P0_STRIDE"),))):
            for nsplit in (1, 8):
                m2 = _pass0_m2(s, nsplit, stride)
                assert (m2 >= s2).all(), (stride, nsplit)                 # a bound over a subset of the trains
                assert (s[rows, i1] <= m2 + window).all() and (s[rows, i2] <= m2 + window).all(), (stride, nsplit)
    return dev


def test_committed_stride_is_one_the_kernel_takes():
    assert _int_constant("BFM_P0_STRIDE") in STRIDES


def test_derivation_stays_under_the_constant():
    err = _constant("BFM_F16_ERR")
    relative = 2.0 * ((1.0 + U) ** 2 - 1.0) * NORM2_MAX           # sum |2 q_i t_i| <= 2 |q||t|
    absolute = 64 * 3 * ETA                                       # eta (|t'_i| + |2 q_i|) <= 3 eta per term
    accumulate = 64 * 2.0 ** -23 * 3.01                           # one rounding per product slot on partial sums <= 2 |q||t| + |t|^2
    initial = 64 * 2.0 ** -24 * NORM2_MAX                         # float32 sum of squares, entered as it is
    assert relative + absolute + accumulate + initial <= err


@pytest.fixture(scope="module")
def strip_descriptors(oracle):
    """oracle descriptors of the facing ROI strips of tiles 0 and 1 of the bench grid (roiRatio 0.2, direction 1)"""
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid
    A, B = SyntheticGrid(10, 9, 2048).tiles(range(2))
    ra = isa.roi_rect(A.shape, 1, "first", 0.2); rb = isa.roi_rect(B.shape, 1, "second", 0.2)
    _ka, da = oracle.surf_detect_describe(np.ascontiguousarray(A[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]]))
    _kb, db = oracle.surf_detect_describe(np.ascontiguousarray(B[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]]))
    assert len(da) > 4000 and len(db) > 4000 and da.shape[1] == 64
    return da, db


def test_production_strip(strip_descriptors, oracle):
    da, db = strip_descriptors
    err, window = _constant("BFM_F16_ERR"), 2 * _constant("BFM_F16_ERR") + _constant("BFM_MARGIN")
    dev = _check(da[::4], db, oracle, err, window)                # every fourth query against all trains
    print("production strip: max |fp16 score - exact| = %.3e (bound %.3e)" % (dev, err))


def _list_counts(s, m2, cut_window, nsplit):
    """(largest number of trains <= m2 + cut_window over (query, chunk, lane half), per-query number within cut_window of the
    second smallest score)"""
    nt = s.shape[1]
    half = _lane_half(nt)
    tchunk = ((nt + 31) // 32 + nsplit - 1) // nsplit
    chunk = np.arange(nt) // 32 // tchunk
    listed = s <= (m2 + cut_window)[:, None]
    worst = max(int(listed[:, (chunk == c) & (half == h)].sum(1).max()) for c in range(nsplit) for h in (0, 1))
    s2 = np.partition(s, 1, axis=1)[:, 1]
    return worst, (s <= (s2 + cut_window)[:, None]).sum(1)


def test_lists_stay_usable_on_the_production_strip(strip_descriptors):
    da, db = strip_descriptors
    q = da[::4]
    err, window = _constant("BFM_F16_ERR"), 2 * _constant("BFM_F16_ERR") + _constant("BFM_MARGIN")
    capl, hits = _int_constant("BFM_CAPL"), _int_constant("BFV_HITS")
    exact, s = _exact(q, db), _scores(q, db).astype(np.float64)
    for stride in sorted(set(STRIDES + (_int_constant("BFM_P0_STRIDE"),))):
        for nsplit in (1, 8):                                     # one chunk: the longest lists; eight: the headline batch's split
            # the inputs themselves: the same counts from float64 scores
            worst, within = _list_counts(exact, _pass0_m2(exact, nsplit, stride), window, nsplit)
            assert worst <= capl and (within <= hits).mean() >= 0.99, ("inputs", stride, nsplit, worst, float((within <= hits).mean()))
            worst, within = _list_counts(s, _pass0_m2(s, nsplit, stride), window, nsplit)
            print("stride %d, %d chunk(s): longest list %d (BFM_CAPL %d), %.2f trains inside the cut per query, %.4f of the queries <= BFV_HITS %d"
                  % (stride, nsplit, worst, capl, within.mean(), (within <= hits).mean(), hits))
            assert worst <= capl, (stride, nsplit, worst)
            assert (within <= hits).mean() >= 0.99, (stride, nsplit)


def _more_stress_rows():
    """what the shared stress rows lack: trains that occur twice or more, and squared norms at the 1.0001 that bf_l2_host admits"""
    rng = np.random.default_rng(11)
    base = _unit(rng.normal(size=(40, 64)))
    dup = base[rng.integers(0, 40, 96)]                           # 96 rows out of 40: every tile holds exact duplicates
    lim = _unit(rng.normal(size=(96, 64))).astype(np.float64) * np.sqrt(1.0001) * (1 - 2.0 ** -22)
    lim = lim.astype(np.float32)
    n2 = (lim.astype(np.float64) ** 2).sum(1)
    assert len(np.unique(dup, axis=0)) <= 40 and n2.max() <= NORM2_MAX and n2.min() > 1.00009
    return {"duplicated": dup, "norm_limit": lim}


def test_stress_rows(oracle):
    err, window = _constant("BFM_F16_ERR"), 2 * _constant("BFM_F16_ERR") + _constant("BFM_MARGIN")
    sets = _stress_rows()
    sets.update(_more_stress_rows())
    every = np.concatenate(list(sets.values()))
    worst = 0.0
    for name, rows in sets.items():
        dev = max(_check(rows, rows, oracle, err, window), _check(rows, every, oracle, err, window), _check(every, rows, oracle, err, window))
        print("%-16s max |fp16 score - exact| = %.3e" % (name, dev))
        worst = max(worst, dev)
    assert worst >= 0.9 * 2 * ((1 + U) ** 2 - 1) * 63 / 64         # the rows do reach the relative term (63 of 64 elements at full roundoff)
    sub = sets["subnormal"]
    assert (np.abs(sub) < 6.1e-5).sum() > 64 * 32 and ((np.abs(sub) < 6.1e-5) & (sub != 0)).sum() > 64 * 16
