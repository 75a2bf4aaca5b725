"""CPU check of the error bound of the fp16 candidate filter of the 64-d 2-NN search (csrc/match_kernels.hip: k_bf_split16,
k_bf_mfma16_d64).  The filter's scores are emulated in numpy the way the kernels form them: descriptors rounded to float16 (queries
scaled by -2 first), products accumulated in float32, |t|^2 summed in float32 and entered as a two-term float16 sum hi + lo.

  - |score - (|t|^2 - 2 q.t in float64)| <= BFM_F16_ERR, the constant the kernels use (read from the source), and the derivation of
    the source comment, recomputed here term by term, stays under that constant;
  - the reference's two nearest trains of every query (oracle.bf_l2_knn2, float arithmetic) score at most
    second smallest fp16 score + 2 BFM_F16_ERR + BFM_MARGIN: they are on the list that pass 1 writes and inside the verifier's cut.

Inputs: the oracle's descriptors of one production strip pair (409 x 2048 ROIs of the 10 x 9 grid of 2048^2 tiles) and unit-norm rows
built to stress the bound.  No GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "imagestitch_amd", "csrc", "match_kernels.hip")
U = 2.0 ** -11                      # unit roundoff of float16 (11 significand bits, round to nearest even)
ETA = 2.0 ** -25                    # half the float16 subnormal spacing: the absolute error below the normal range (|x| < 2^-14)
NORM2_MAX = 1.0001                  # what bf_l2_host admits to the filtered search


def _constant(name):
    m = re.search(r"#define\s+%s\s+([0-9.eE+-]+)f\b" % name, open(SRC).read())
    assert m, name
    return float(np.float32(float(m.group(1))))


def _scores(q, t):
    """float32 scores as the sweeps form them: 64 fp16 products + the norm slot's hi * 1 + lo * 1, float32 accumulation"""
    q16 = (np.float32(-2.0) * q).astype(np.float16)
    t16 = t.astype(np.float16)
    tot = np.zeros(len(t), np.float32)
    for d in range(64):                                           # k_bf_split16's sequential float32 sum (halves met at the end)
        tot += t[:, d] * t[:, d]
    hi = tot.astype(np.float16)
    lo = (tot - hi.astype(np.float32)).astype(np.float16)
    s = q16.astype(np.float32) @ t16.astype(np.float32).T          # products of two float16 values are exact in float32
    s = s + hi.astype(np.float32)[None, :]
    return s + lo.astype(np.float32)[None, :]


def _exact(q, t):
    q64, t64 = q.astype(np.float64), t.astype(np.float64)
    return (t64 * t64).sum(1)[None, :] - 2.0 * (q64 @ t64.T)


def _check(q, t, oracle, err, window):
    assert float((q.astype(np.float64) ** 2).sum(1).max()) <= NORM2_MAX and float((t.astype(np.float64) ** 2).sum(1).max()) <= NORM2_MAX
    s = _scores(q, t).astype(np.float64)
    dev = float(np.abs(s - _exact(q, t)).max())
    assert dev <= err, dev
    if len(t) >= 2:
        i1, _d1, i2, _d2 = oracle.bf_l2_knn2(q, t)
        s2 = np.partition(s, 1, axis=1)[:, 1]
        rows = np.arange(len(q))
        assert (s[rows, i1] <= s2 + window).all() and (s[rows, i2] <= s2 + window).all()
    return dev


def test_derivation_stays_under_the_constant():
    err = _constant("BFM_F16_ERR")
    relative = 2.0 * ((1.0 + U) ** 2 - 1.0) * NORM2_MAX           # sum |2 q_i t_i| <= 2 |q||t|
    absolute = 64 * 3 * ETA                                       # eta (|t'_i| + |2 q_i|) <= 3 eta per term
    accumulate = 65 * 2.0 ** -23 * 3.01                           # one rounding per k-slot on partial sums <= 2 |q||t| + |t|^2
    norm_slot = 64 * 2.0 ** -24 * NORM2_MAX + 2.0 ** -22          # float32 sum of squares + the rounding of lo
    assert relative + absolute + accumulate + norm_slot <= err


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


def _unit(a):
    a = a.astype(np.float64)
    n = np.linalg.norm(a, axis=1, keepdims=True); n[n == 0] = 1
    a = (a / n).astype(np.float32)
    return a


def _stress_rows():
    rng = np.random.default_rng(5)
    sets = {}
    signs = rng.choice([-1.0, 1.0], size=(96, 64))
    eq = (0.125 * signs).astype(np.float32)                       # all magnitudes 1/8: norm exactly 1, exact in float16
    eq[0] = 0.125; eq[1] = -0.125
    eq[2] = 0.125 * (-1.0) ** np.arange(64)                       # sign-alternating
    sets["equal_eighths"] = eq
    one = np.zeros((64, 64), np.float32)                          # one element at +-1
    one[np.arange(64), np.arange(64)] = (-1.0) ** np.arange(64)
    sets["one_hot"] = one
    # elements below float16's normal range (6.1e-5): subnormals and zeros beside a few large elements
    tiny = rng.uniform(-6.0e-5, 6.0e-5, size=(96, 64))
    tiny[:, ::3] = 0
    tiny[:32, :4] = rng.normal(size=(32, 4)); tiny[32:64, 60:] = rng.normal(size=(32, 4)); tiny[64:, 30:34] = rng.normal(size=(32, 4))
    t = _unit(tiny)
    big = np.abs(t) > 1e-3
    t[~big] = tiny[~big].astype(np.float32)                       # keep the small elements in the subnormal range after normalising
    t[0, 4:] = 2.0 ** -24 * 0.49; t[1, 4:] = 2.0 ** -25            # below half the smallest subnormal; an exact tie to even (zero)
    sets["subnormal"] = t
    # worst relative rounding: every non-zero element an exact float16 tie 1/8 (1 + 2^-11), which rounds to even = 1/8, off by
    # u / (1 + u) relative, the same way on both sides so that the 63 product errors add up; one zero keeps the norm under 1
    tie = np.full((64, 64), 0.125 * (1.0 + U), np.float32)
    tie[np.arange(64), np.arange(64)] = 0
    tie[32:] *= np.float32(-1)
    tie[::2] *= ((-1.0) ** np.arange(64)).astype(np.float32)      # sign-alternating copies: q.t of either sign
    sets["ties_to_even"] = tie
    up = np.where(tie == 0, tie, np.nextafter(tie, np.where(tie < 0, -np.inf, np.inf).astype(np.float32)))      # just past the tie: rounds away
    sets["just_past_ties"] = up
    sets["random_unit"] = _unit(rng.normal(size=(128, 64)))
    return sets


def test_stress_rows(oracle):
    err, window = _constant("BFM_F16_ERR"), 2 * _constant("BFM_F16_ERR") + _constant("BFM_MARGIN")
    sets = _stress_rows()
    every = np.concatenate(list(sets.values()))
    worst = 0.0
    for name, rows in sets.items():
        dev = max(_check(rows, rows, oracle, err, window), _check(rows, every, oracle, err, window), _check(every, rows, oracle, err, window))
        print("%-16s max |fp16 score - exact| = %.3e" % (name, dev))
        worst = max(worst, dev)
    assert worst >= 0.9 * 2 * ((1 + U) ** 2 - 1) * 63 / 64         # the rows do reach the relative term (63 of 64 elements at full roundoff)
    sub = sets["subnormal"]
    assert (np.abs(sub) < 6.1e-5).sum() > 64 * 32 and ((np.abs(sub) < 6.1e-5) & (sub != 0)).sum() > 64 * 16
