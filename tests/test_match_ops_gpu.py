"""The matcher operators behind a user's own matchDescriptors / getOffsetByMode -- vfsms_bf_l2_knn2, vfsms_bf_l2_knn2_ratio,
vfsms_bf_hamming_nn, vfsms_mode_offset, vfsms_consensus_offset -- each one job of a match run (csrc/api.hip), held to the numpy-facing
CPU oracle for exact equality at the shapes where the wiring of that job, not a kernel, can go wrong: one row, one more than a tile,
more queries than trains, both plans of the L2 search, more pairs than one pass of the vote; and the two properties of the wiring
itself: the context's vote settings do not reach the operators, and no state leaks from one plan into the next call.

Dim 32: the oracle's L2 search is generic in the row length and accepts a (65, 130) dim-32 input, so dim 32 is tested at (65, 130)."""
import numpy as np
import pytest

import imagestitch_amd as isa

pytestmark = pytest.mark.gpu

L2_SHAPES_64 = [(1, 1), (1, 65), (65, 1), (64, 64), (257, 31)]
HAMMING_SHAPES = [(1, 1), (63, 65), (300, 7)]


def _unit_rows(rng, n, dim):
    a = rng.normal(size=(n, dim)).astype(np.float32)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _l2_case(seed, nq, nt, dim, scale=1):
    rng = np.random.default_rng(seed)
    return _unit_rows(rng, nq, dim) * np.float32(scale), _unit_rows(rng, nt, dim) * np.float32(scale)


def _hamming_case(seed, nq, nt):
    rng = np.random.default_rng(seed)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8); t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    if nt > 1:
        t[nt - 1] = t[0]; q[0] = t[0] ^ np.uint8(1)                     # a duplicated train row: query 0 ties between trains 0 and nt - 1
    return q, t


def _pairs_case(seed, m):
    """m matches between 2 m + 3 keypoints a side whose votes pile up on (40, -7) with noise around it"""
    rng = np.random.default_rng(seed)
    n = 2 * m + 3
    kB = rng.integers(0, 2000, (n, 2)).astype(np.float32)
    kA = kB + np.float32([-7, 40]) + (rng.random((n, 1)) < 0.4) * rng.integers(-30, 30, (n, 2)).astype(np.float32)
    idx = rng.permutation(n)[:m].astype(np.int32)
    return kA.astype(np.float32), kB, np.stack([idx, idx], 1)              # (trainIdx, queryIdx)


def _check_l2(engine, oracle, q, t, what):
    i1, d1, d2 = engine.bf_l2_knn2(q, t)
    oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
    assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2), what
    assert np.array_equal(engine.bf_l2_ratio_matches(q, t, 0.75), oracle.bf_l2_ratio_matches(q, t, 0.75)), what


@pytest.mark.parametrize("nq,nt", L2_SHAPES_64)
def test_l2_dim64_both_plans(engine, oracle, nq, nt):
    """unit-norm rows take the filtered plan, the same rows times 3 the exhaustive one"""
    for scale in (1, 3):
        q, t = _l2_case(100 + nq + nt, nq, nt, 64, scale)
        _check_l2(engine, oracle, q, t, (nq, nt, scale))


@pytest.mark.parametrize("dim", [128, 32])
def test_l2_other_dims(engine, oracle, dim):
    q, t = _l2_case(200 + dim, 65, 130, dim)
    _check_l2(engine, oracle, q, t, dim)


@pytest.mark.parametrize("nq,nt", HAMMING_SHAPES)
def test_hamming(engine, oracle, nq, nt):
    q, t = _hamming_case(300 + nq, nq, nt)
    for max_dist in (-1, 64):
        want, _dist = oracle.bf_hamming_matches(q, t, max_dist)
        assert np.array_equal(engine.bf_hamming_matches(q, t, max_dist), want), (nq, nt, max_dist)


@pytest.mark.parametrize("m", [1, 1025])
def test_given_pairs(engine, oracle, m):
    kA, kB, pairs = _pairs_case(400 + m, m)
    for ev in (1, 3):
        want = oracle.mode_offset(kA, kB, pairs, ev)
        assert engine.mode_offset(kA, kB, pairs, ev) == want, (m, ev)
        assert engine.consensus_offset(kA, kB, pairs, 0, ev) == want, (m, ev)


def _fresh(call):
    eng = isa.Engine(0)
    try:
        return call(eng)
    finally:
        eng.close()


def _same(a, b):
    if isinstance(a, tuple):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(a, b) if isinstance(a, np.ndarray) else a == b


def test_context_vote_settings_do_not_reach_the_operators(engine):
    """with the consensus estimator and the NCC verifier in force the operators launch neither: the estimator is the one the call names,
    and a job without strips never meets the verifier"""
    q, t = _l2_case(500, 257, 31, 64)
    hq, ht = _hamming_case(501, 63, 65)
    kA, kB, pairs = _pairs_case(502, 1025)
    calls = [lambda e: e.bf_l2_ratio_matches(q, t, 0.75), lambda e: e.bf_l2_knn2(q, t), lambda e: e.bf_hamming_matches(hq, ht, 64),
             lambda e: e.mode_offset(kA, kB, pairs, 3)]
    want = _fresh(lambda e: [c(e) for c in calls])
    try:
        engine.set_offset_estimator("consensus", 3)
        engine.set_offset_verifier("ncc", 0.5, 16)
        got = [c(engine) for c in calls]
    finally:
        engine.set_offset_estimator()
        engine.set_offset_verifier()
    for k, (g, w) in enumerate(zip(got, want)):
        assert _same(g, w), k


def test_no_state_leaks_from_one_plan_to_the_next(engine):
    q, t = _l2_case(600, 257, 31, 64)
    q3, t3 = _l2_case(601, 64, 64, 64, 3)
    hq, ht = _hamming_case(602, 300, 7)
    kA, kB, pairs = _pairs_case(603, 1025)
    calls = [lambda e: (e.bf_l2_knn2(q, t), e.bf_l2_ratio_matches(q, t, 0.75)),            # filtered
             lambda e: (e.bf_l2_knn2(q3, t3), e.bf_l2_ratio_matches(q3, t3, 0.75)),        # exhaustive
             lambda e: e.bf_hamming_matches(hq, ht, -1),
             lambda e: e.mode_offset(kA, kB, pairs, 3),
             lambda e: (e.bf_l2_knn2(q, t), e.bf_l2_ratio_matches(q, t, 0.75))]            # filtered again
    got = [c(engine) for c in calls]
    for k, c in enumerate(calls):
        assert _same(got[k], _fresh(c)), k
