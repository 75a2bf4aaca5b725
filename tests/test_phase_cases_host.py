"""CPU side of tests/phase_cases.py: every condition of the phase-transform tests that concerns the references alone -- the generators are
deterministic, the sweep covers every length and every radix in both positions, the two references agree as closely as the tight bound
says, the peak lists of the unrelated pairs stand clear of rounding, the border peaks land where they are meant to, zeros give exact zeros,
the batch jobs differ and the two references agree on vector surfaces.  test_phase_transforms_gpu.py runs the same cases on the device."""
import numpy as np
import pytest

import phase_cases as C
import phase_resolve_ref as PR
from phase_numpy import optimal_dft_size, phase_correlate as np_phase


def test_generators_are_deterministic():
    for make, shape in ((C.planted_pair, (3, 90)), (C.unrelated_pair, (81, 90)), (C.geometry_pair, (6, 6)), (C.vector_pair, (1, 9))):
        a, b = make(shape); a2, b2 = make(shape)
        assert a.dtype == np.uint8 and a.shape == shape and np.array_equal(a, a2) and np.array_equal(b, b2) and not np.array_equal(a, b)
    assert rand_sum() == 127750
    t0, a0, b0 = C.border_cases((16, 32))[3]
    assert t0 == (15, 31) and np.array_equal(b0, np.roll(np.roll(a0, -7, 0), -15, 1))
    assert C.sweep_groups() == C.sweep_groups() and [n for n, _s in C.sweep_groups()][::4] == ["rows0", "rows4", "rows8"]


def rand_sum():
    return int(C.rand_img(1, (32, 32)).sum())


def test_sweep_covers_every_length_and_every_radix_in_both_positions():
    assert len(C.ROW_HALF_LENGTHS) == 136 and len(C.COL_LENGTHS) == 86
    assert (C.ROW_HALF_LENGTHS[0], C.ROW_HALF_LENGTHS[-1], C.COL_LENGTHS[0], C.COL_LENGTHS[-1]) == (2, 4096, 2, 1024)
    # the restated phase_own_shape accepts nothing longer: H = 4096 and M = 1024 are the last
    assert C.own_shape(3, 2 * 4100)["lds_transforms"] == 0 and C.own_shape(1025, 2048)["lds_transforms"] == 0
    rows = [C.own_shape(*s) for s in C.row_shapes()]
    cols = [C.own_shape(*s) for s in C.col_shapes()]
    assert all(p["lds_transforms"] == 1 and p["transposed"] == 0 for p in rows + cols)
    assert sorted({p["N"] // 2 for p in rows}) == C.ROW_HALF_LENGTHS
    assert sorted({p["M"] for p in cols}) == C.COL_LENGTHS
    assert sum((3, 2 * H) in C.row_shapes() for H in C.ROW_HALF_LENGTHS) == 136 and len(C.row_shapes()) == 268      # 132 with an odd width too
    assert all(s[1] % 2 == 1 and optimal_dft_size(s[1]) == s[1] + 1 for s in C.row_shapes() if (3, s[1]) != (3, 2 * (s[1] // 2)))
    assert len(C.col_shapes()) == 86 and all(M == s[0] and s[1] % 2 == 0 and s[1] >= M for M, s in zip(C.COL_LENGTHS, C.col_shapes()))
    groups = C.sweep_groups()
    assert sorted(s for _n, g in groups for s in g) == sorted(C.sweep_shapes()) and all(28 <= len(g) <= 30 for _n, g in groups)
    for lengths in (C.ROW_HALF_LENGTHS, C.COL_LENGTHS):
        first, later = set(), set()
        for L in lengths:
            sched = C.make_sched(L)
            assert int(np.prod([R for R, _l in sched])) == L and sched[0][1] == 1
            for R, Ls in sched:
                (first if Ls == 1 else later).add(R)
        assert first == set(C.RADICES) and later == set(C.RADICES), (first, later)


def test_reference_disagreement_fixes_the_tight_bound(oracle):
    """the largest disagreement of the two references over exactly the planted pairs of the sweep; the constants of phase_cases.py must not
    understate it (nor overstate it by more than a rounding-up), and the tight bound is 100 times it"""
    wpx = wrs = wraw = 0.0
    at = [None, None]
    low = []
    for s in sorted(set(C.sweep_shapes())):
        n, o, _pos = C.planted_refs(s, oracle)
        px, rs = C.deviation(n, o)
        assert px < C.OUTER_PX and rs < C.OUTER_RESPONSE, (s, n, o)
        assert [int(v) for v in n[:2]] == [int(v) for v in o[:2]], (s, n, o)
        if C.conditioning(n) < 0.01:
            low.append(s)
        wraw = max(wraw, px)
        if px * C.conditioning(n) > wpx:
            wpx, at[0] = px * C.conditioning(n), s
        if rs > wrs:
            wrs, at[1] = rs, s
    print("reference disagreement over the planted sweep: %.3g px x conditioning at %r, %.3g response at %r; %.3g px unweighted; ill-conditioned: %r"
          % (wpx, at[0], wrs, at[1], wraw, low))
    assert low == [(3, 4)]                                       # the one pair whose window sum is next to zero
    assert wpx <= C.REF_DISAGREE_PX <= 2 * wpx and wrs <= C.REF_DISAGREE_RESPONSE <= 2 * wrs
    assert C.TIGHT_PX == 100 * C.REF_DISAGREE_PX and C.TIGHT_RESPONSE == 100 * C.REF_DISAGREE_RESPONSE
    assert C.TIGHT_PX < 1e-9 and C.TIGHT_PX < C.OUTER_PX and C.TIGHT_RESPONSE < C.OUTER_RESPONSE


def test_unrelated_pairs_keep_their_peak_lists_clear_of_rounding():
    shapes = sorted(set(C.sweep_shapes()))
    dropped = [s for s in shapes if not C.unrelated_ref(s)[1]]
    print("unrelated pairs excluded by peak_gap_ok: %d of %d %r" % (len(dropped), len(shapes), dropped))
    assert len(dropped) <= C.MAX_DROPPED * len(shapes)
    assert all(len(C.unrelated_ref(s)[0]) == C.PEAKS for s in shapes)


@pytest.mark.parametrize("shape", C.BORDER_SHAPES)
def test_border_peaks_land_where_intended(oracle, shape):
    M, N = shape
    targets = [t for t, _a, _b in C.border_cases(shape)]
    assert len(targets) == 17 and len(set(targets)) == 17
    assert {(0, 0), (0, N - 1), (M - 1, 0), (M - 1, N - 1), (M // 2, N // 2), (0, N // 2), (M // 2, N - 1), (1, N // 2), (M // 2, N - 3)} <= set(targets)
    for k, (t, a, b) in enumerate(C.border_cases(shape)):
        n, o, pos = C.border_refs(shape, k, oracle)
        assert pos == t, (shape, t, pos)                          # phase_numpy's own peak position
        px, rs = C.deviation(n, o)
        assert px * C.conditioning(n) <= C.REF_DISAGREE_PX * 10 and rs <= C.REF_DISAGREE_RESPONSE * 10 and n[2] > 0.9, (shape, t, n, o)
        # the window is clamped exactly where the target is within two elements of an edge
        assert (min(t[0], M - 1 - t[0]) < 2 or min(t[1], N - 1 - t[1]) < 2) == (k < 8 or k in (8, 10, 12, 14))
    plans = {s: (C.own_shape(*s)["lds_transforms"], C.own_shape(*s)["transposed"]) for s in C.BORDER_SHAPES}
    assert plans == {(16, 32): (1, 0), (32, 16): (1, 1), (45, 60): (1, 0), (60, 45): (1, 1), (25, 27): (0, 0), (48, 625): (1, 1), (625, 48): (1, 0)}


@pytest.mark.parametrize("shape", C.DEGENERATE_SHAPES)
def test_zero_strips_give_an_exactly_zero_surface(oracle, shape):
    want = C.degenerate_result(shape)
    for name, a, b in C.degenerate_pairs(shape):
        assert not PR.surface(a, b).any(), (shape, name)
        if shape[0] * shape[1] > 1 << 16 and name != "zeros, content":
            continue                                             # the large shapes once: the surface above is what matters
        (nx, ny), nr, pos = np_phase(a, b)
        (ox, oy), orr = oracle.phase_correlate(a, b)
        assert (nx, ny, nr) == want and (ox, oy, orr) == want and pos == (0, 0), (shape, name)


def test_constant_strips_are_not_a_defined_input(oracle):
    """why test_phase_transforms_gpu.py asks only for finite numbers on constant non-zero strips: the references differ by whole pixels"""
    a = np.full((15, 20), 255, np.uint8)
    (nx, _ny), _nr, _pos = np_phase(a, a)
    (ox, _oy), _orr = oracle.phase_correlate(a, a)
    assert abs(nx - ox) > 1.0


def test_batch_jobs_differ_and_suit_both_references(oracle):
    assert [C.own_shape(*s)["transposed"] for s in C.BATCH_SHAPES] == [0, 1]
    jobs = C.mixed_batch()
    assert len(jobs) == 14 and [a.shape for _n, a, _b in jobs] == C.BATCH_SHAPES * 7
    res = C.mixed_batch_resolved()
    assert all(ok for _r, ok in res)
    assert len({tuple(r["peaks"][0]) for r, _ok in res}) >= 12 and len({a.tobytes() for _n, a, _b in jobs}) == 14
    many = C.batch_strips(C.BATCH_SHAPES[1], C.MANY)
    assert len(many) == 70 and len({a.tobytes() for _n, a, _b in many}) == 70
    found = set()
    for name, a, b in jobs + many:
        n, o, pos = C.refs(("batch", name), a, b, oracle)
        px, rs = C.deviation(n, o)
        assert px * C.conditioning(n) <= C.REF_DISAGREE_PX * 10 and rs <= C.REF_DISAGREE_RESPONSE * 10 and n[2] > 0.5, (name, n, o)
        found.add((a.shape, pos))
    assert len(found) >= 60                                      # the jobs of a batch have answers of their own


def test_geometry_shapes_and_settings():
    sweep = set(C.sweep_shapes())
    assert all(s in sweep for s in C.GEOMETRY_SHAPES[:-2]) and C.GEOMETRY_SHAPES[-2:] == [(409, 2048), (2048, 409)]
    plans = [C.own_shape(*s) for s in C.GEOMETRY_SHAPES]
    assert {2, 1024, 4096} <= {p["N"] // 2 for p in plans[:7]} and {2, 432, 625, 1024} <= {p["M"] for p in plans[7:14]}
    assert len(C.GEOMETRY_SHAPES) == 16 and all(p["lds_transforms"] == 1 for p in plans)
    takes = {}
    for knob, value in C.GEOMETRY_SETTINGS:
        takes[knob, value] = sum(C.geometry_takes(C.geometry_restated(s, knob, value), p) for s, p in zip(C.GEOMETRY_SHAPES, plans))
    print("shapes on which each geometry setting takes, of 16:", takes)
    # by the restated host rule TDIV = 16 and TCOL = 64 are always clamped back (a workgroup's points must fit 8 per thread)
    assert all(takes[k] >= 9 for k in list(takes)[:5]) and takes["VFSMS_PHASE_TDIV", "16"] == 0 and takes["VFSMS_PHASE_TCOL", "64"] == 0


def test_references_agree_on_vector_surfaces(oracle):
    """phase_numpy with phasecorr.cpp's rule for a 1 x n or n x 1 surface (its two halves swap) against the oracle's; 2-D results are untouched"""
    for s in C.VECTOR_SHAPES:
        n, o, pos = C.vector_refs(s, oracle)
        px, rs = C.deviation(n, o)
        assert px < C.OUTER_PX and px * C.conditioning(n) <= C.REF_DISAGREE_PX and rs <= C.REF_DISAGREE_RESPONSE, (s, n, o)
        assert [int(v) for v in n[:2]] == [int(v) for v in o[:2]]
    R = np.arange(7.0).reshape(1, 7)
    mid = 3
    assert np.concatenate([R[0, mid:2 * mid], R[0, :mid], R[0, 2 * mid:]]).tolist() == [3, 4, 5, 0, 1, 2, 6]
