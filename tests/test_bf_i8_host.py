"""CPU tests of what holds the integer 128-d 2-NN search (tests/test_bf_i8_gpu.py): the seeded cases of tests/bf_i8_cases.py contain what
they are built for -- asserted from the reference alone -- and the integer reference tests/bf_i8_ref.py equals two independent float
references bit for bit: the CPU oracle (normL2Sqr_ order) on every case, and the float32 emulation of k_bf_l2_gen<128> with a sequential
knn_update scan on a subset."""
import numpy as np
import pytest

import bf_i8_cases as K
import bf_i8_ref as R


def _sorted_dsq(kind, nq, nt):
    q, t = K.case(kind, nq, nt)
    s = R.dsq(q, t)
    return s, np.sort(s, axis=1)


def test_shapes_reach_every_edge_of_the_split_rule():
    assert len(K.SHAPES) == 120 and len(K.KINDS) == 7
    empty = partial_only = 0
    for nt in K.NT:
        per = K.split_trains(nt, 8)
        for sp in range(8):
            lo, hi = sp * per, min(nt, (sp + 1) * per)
            empty += hi <= lo
            partial_only += 0 < hi - lo < 16
    assert empty > 0 and partial_only > 0
    assert K.split_trains(129, 8) == 32 and K.split_trains(129, 2) == 80 and K.split_trains(17, 8) == 16


@pytest.mark.parametrize("kind", K.KINDS)
def test_every_case_is_u8_and_below_2_24(kind):
    for nq, nt in K.SHAPES:
        q, t = K.case(kind, nq, nt)
        assert q.dtype == np.uint8 and t.dtype == np.uint8 and q.shape == (nq, 128) and t.shape == (nt, 128)
        assert int(R.dsq(q, t).max()) < 2 ** 24                                # R.dsq asserts it as well
    assert K.case(kind, 17, 33)[0] is K.case(kind, 17, 33)[0]                   # one build per process
    a = K._BUILD[kind](K._rng(kind, 17, 33), 17, 33)
    assert np.array_equal(a[0], K.case(kind, 17, 33)[0]) and np.array_equal(a[1], K.case(kind, 17, 33)[1])      # seeded


def test_far_cases_hold_sqrt_collisions():
    """two integer squared distances with one sqrtf: the first index of the sqrt minimum differs from the integer argmin, and d1 == d2
    although the two smallest dsq differ"""
    moved = tied = 0
    for nq, nt in K.SHAPES:
        if nt < 2:
            continue
        s, so = _sorted_dsq("far", nq, nt)
        assert 7_282_800 <= int(s.min()) and int(s.max()) <= 7_282_800 + 16 * 9
        i1, d1, d2 = K.reference("far", nq, nt)
        moved += int((i1 != np.argmin(s, axis=1)).sum())
        tied += int(((d1 == d2) & (so[:, 0] != so[:, 1])).sum())
    print("far: queries whose sqrt-domain first minimum is not the integer argmin: %d; d1 == d2 with differing dsq: %d" % (moved, tied))
    assert moved >= 5 and tied >= 10


def test_extremes_reach_the_largest_distance():
    top = 0
    for nq, nt in K.SHAPES:
        q, t = K.case("extremes", nq, nt)
        assert set(np.unique(q)) <= {0, 255} and set(np.unique(t)) <= {0, 255}
        top = max(top, int(R.dsq(q, t).max()))
    assert top == 128 * 255 * 255


def test_duplicates_tie_at_every_placement():
    """per placement: queries whose smallest distance is attained by both copies of a placed pair, at distance 0 and at an equal
    non-zero distance; the reference names the lower copy"""
    zero = {k: 0 for k in K.duplicate_pairs(129)}
    nonzero = dict(zero)
    for nq, nt in K.SHAPES:
        q, t = K.case("duplicates", nq, nt)
        if nt >= 2:
            _u, cnt = np.unique(t, axis=0, return_counts=True)
            assert cnt.min() >= 2                                               # every train row occurs several times
        s = R.dsq(q, t)
        i1, d1, d2 = K.reference("duplicates", nq, nt)
        if nt >= 2:
            assert np.array_equal(d1, d2)
        for name, pairs in K.duplicate_pairs(nt).items():
            for a, b in pairs:
                assert np.array_equal(t[a], t[b]) and a < b
                if name == "within_lane":
                    assert b - a == 1 and K.lane_group(a) == K.lane_group(b) and a >> 4 == b >> 4
                elif name == "cross_lane":
                    assert a >> 4 == b >> 4 and K.lane_group(a) < K.lane_group(b)
                elif name == "cross_lane_up":
                    assert a >> 4 < b >> 4 and K.lane_group(a) > K.lane_group(b)
                elif name == "cross_tile":
                    assert b - a == 16
                else:
                    assert all(a // K.split_trains(nt, ns) < b // K.split_trains(nt, ns) for ns in (2, 3, 8))
                hit = (i1 == a) & (s[:, a] == s.min(axis=1)) & (s[:, b] == s[:, a])
                zero[name] += int((hit & (s[:, a] == 0)).sum())
                nonzero[name] += int((hit & (s[:, a] > 0)).sum())
    print("duplicates: ties at distance 0", zero, "at a non-zero distance", nonzero)
    assert min(zero.values()) >= 20 and min(nonzero.values()) >= 20


def test_near_ties_differ_by_exactly_one():
    n = 0
    for nq, nt in K.SHAPES:
        if nt < 8:
            continue
        _s, so = _sorted_dsq("near_ties", nq, nt)
        assert np.array_equal(so[:, 0], np.full(nq, 3)) and np.array_equal(so[:, 1], np.full(nq, 4))
        n += nq
    assert n > 1000


def test_pad_bait_holds_the_all_128_queries_and_zero_rows_the_zero_rows():
    for nq, nt in K.SHAPES:
        q, t = K.case("pad_bait", nq, nt)
        assert (q == 128).all(axis=1).sum() == (nq + 2) // 3
        assert int(np.abs(t.astype(np.int32) - 128).min()) >= 87
        q, t = K.case("zero_rows", nq, nt)
        assert (q == 0).all(axis=1).any() and (t == 0).all(axis=1).any()
    assert sum(nt % 16 != 0 for nt in K.NT) == 9


@pytest.mark.parametrize("kind", K.KINDS)
def test_reference_equals_the_oracle_on_every_case(oracle, kind):
    """float arithmetic in normL2Sqr_ order, sqrtf, K-insertion with strict <: the reference matcher's own form"""
    for nq, nt in K.SHAPES:
        q, t = K.case(kind, nq, nt)
        i1, d1, _i2, d2 = oracle.bf_l2_knn2(q.astype(np.float32), t.astype(np.float32))
        ri, r1, r2 = K.reference(kind, nq, nt)
        assert np.array_equal(i1, ri) and np.array_equal(d1, r1) and np.array_equal(d2, r2), (kind, nq, nt)


def _scan_f32(q, t):
    """k_bf_l2_gen<128> in float32 (the emulation of tests/test_sift_batch_host.py) and knn_update over ascending train indices"""
    from test_sift_batch_host import _gen_order_f32
    inf = np.float32(np.inf)
    i1 = np.empty(len(q), np.int32); d1 = np.empty(len(q), np.float32); d2 = np.empty(len(q), np.float32)
    for i in range(len(q)):
        b1 = b2 = b1s = b2s = inf; best = -1
        for j in range(len(t)):
            dsq = _gen_order_f32(q[i].astype(np.int64), t[j].astype(np.int64))
            if dsq < b2s:
                d = np.sqrt(dsq)
                assert d.dtype == np.float32
                if d < b1:
                    b2, b2s, b1, b1s, best = b1, b1s, d, dsq, j
                elif d < b2:
                    b2, b2s = d, dsq
        i1[i], d1[i], d2[i] = best, b1, b2
    return i1, d1, d2


@pytest.mark.parametrize("kind", K.KINDS)
def test_reference_equals_the_float32_emulation_of_the_valu_kernel(kind):
    for nq, nt in ((1, 1), (15, 17), (16, 33)):
        q, t = K.case(kind, nq, nt)
        i1, d1, d2 = _scan_f32(q, t)
        ri, r1, r2 = K.reference(kind, nq, nt)
        assert np.array_equal(i1, ri) and np.array_equal(d1, r1) and np.array_equal(d2, r2), (kind, nq, nt)
