"""CPU tests of the global placement (Method.globalAdjust = "ncc"): the specification of the window search (tests/ncc_search_ref.py), the
neighbour discovery, the least-squares solve and adjust_offsets over an engine whose search IS the specification.  No GPU."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import adjust as ADJ
import adjust_cases as AC
import ncc_search_ref as S
import verify_ref as V


def test_flat_pair_returns_the_centre_and_empty_overlaps_score_zero():
    A = np.full((40, 48), 90, np.uint8)
    i, j, fx, surface = S.search(A, A.copy(), 3, -2, 4, 0)
    assert (i, j, fx) == (0, 0, 0) and not surface.any()              # every candidate ties at 0: the smallest i^2 + j^2 wins
    rng = np.random.default_rng(1)
    A = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    B = rng.integers(0, 256, (40, 48), dtype=np.uint8)
    # centred 2 rows outside the tile: candidates with dx + i >= 40 share no pixel and score exactly 0, the others a 1- or 2-row strip
    i, j, fx, surface = S.search(A, B, 42, 0, 3, 0)
    for ii in range(-3, 4):
        for jj in range(-3, 4):
            n = S.shared_pixels(A.shape, 42 + ii, jj)
            assert (n == 0) == (ii >= -2)
            if n == 0:
                assert surface[ii + 3, jj + 3] == 0
            else:
                assert surface[ii + 3, jj + 3] == V.fixed(V.score(V.sums(A, B, 42 + ii, jj), 0))
    # min_pixels above every candidate's share: all 0 again, the centre wins
    assert S.search(A, B, 42, 0, 3, 97)[:3] == (0, 0, 0)


def test_ties_go_to_the_smallest_distance_then_i_then_j():
    """Tiles that are their own mirror images in both axes, centred on (0, 0): the candidates (+-i, +-j) pair the same pixels, so their
    six integers -- hence their double scores -- are equal.  The winner must be the one with the smallest i, then the smallest j."""
    rng = np.random.default_rng(0)

    def symmetric():
        q = rng.integers(0, 256, (12, 14), dtype=np.uint8)
        top = np.concatenate([q, q[:, ::-1]], axis=1)
        return np.concatenate([top, top[::-1]], axis=0)
    A, B = symmetric(), symmetric()
    R = 3
    i, j, fx, surface = S.search(A, B, 0, 0, R, 0)
    scores = {(a, b): V.score(V.sums(A, B, a, b), 0) for a in range(-R, R + 1) for b in range(-R, R + 1)}
    top = max(scores.values())
    tied = sorted(k for k, v in scores.items() if v == top)
    assert len(tied) == 4 and i != 0 and j != 0                        # a real four-way tie, off both axes
    assert np.array_equal(surface, surface[::-1, ::-1])
    assert (i, j) == min(tied, key=lambda k: (k[0] * k[0] + k[1] * k[1], k[0], k[1])) == (-abs(i), -abs(j))
    assert fx == V.fixed(top)


def test_neighbour_edges_of_the_3x3_serpentine():
    tiles, true = AC.grid("g7")
    E = ADJ.neighbour_edges([t.shape for t in tiles], true, AC.RADIUS)
    assert [tuple(e[:2]) for e in E.tolist()] == AC.EDGES_3X3
    P = ADJ.path_positions(true)
    assert all([dx, dy] == (P[b] - P[a]).tolist() for a, b, dx, dy in E.tolist())
    # a path whose consecutive tiles do not even touch keeps its path pairs; tiles of two sizes are refused
    far = ADJ.neighbour_edges([(64, 64)] * 3, [[500, 0], [0, 500]], 4)
    assert [tuple(e[:2]) for e in far.tolist()] == [(0, 1), (1, 2)]
    with pytest.raises(ValueError):
        ADJ.neighbour_edges([(64, 64), (64, 65)], [[50, 0]], 4)


def test_neighbour_edges_is_vectorised_enough_for_1024_tiles():
    g = isa.synthetic.SyntheticGrid(32, 32, 512, overlap=0.1, jitter=8, seed=2)
    E = ADJ.neighbour_edges([(512, 512)] * g.n_tiles, g.true_offsets(), 4)
    assert len(E) == 2 * 32 * 31                                      # every side-by-side pair of the grid, none diagonal


def _incidence(n, edges):
    M = np.zeros((len(edges), n - 1))
    for k, (a, b, _dx, _dy) in enumerate(edges):
        if a:
            M[k, a - 1] = -1.0
        if b:
            M[k, b - 1] = 1.0
    return M


def test_solve_positions_is_the_least_squares_fit():
    rng = np.random.default_rng(3)
    _tiles, true = AC.grid("g7")
    P = ADJ.path_positions(true)
    edges = [(a, b, P[b][0] - P[a][0] + int(rng.integers(-3, 4)), P[b][1] - P[a][1] + int(rng.integers(-3, 4))) for a, b in AC.EDGES_3X3]
    got = ADJ.solve_positions(9, edges)
    want, *_ = np.linalg.lstsq(_incidence(9, edges), np.array([e[2:] for e in edges], np.float64), rcond=None)
    assert got.dtype == np.float64 and got.shape == (9, 2) and not got[0].any()
    assert np.abs(got[1:] - want).max() < 1e-9
    consistent = [(a, b, P[b][0] - P[a][0], P[b][1] - P[a][1]) for a, b in AC.EDGES_3X3]
    assert np.array_equal(ADJ.solve_positions(9, consistent), P.astype(np.float64))


@pytest.mark.parametrize("name", sorted(AC.GRIDS))
def test_adjust_offsets_recovers_the_true_offsets(name):
    """What the specification gives on these grids at min_pixels = 256: all 12 edges peak exactly at the truth,
    score >= 0.9968 and margin to the runner-up >= 0.03 at the precision they are stated with (measured: 0.99677 and 0.02992 at the
    lowest).  The path offsets are wrong on three pairs by up to 3 px; the adjusted ones must be the truth."""
    tiles, true = AC.grid(name)
    shapes = [t.shape for t in tiles]
    eng = AC.SpecEngine(name)
    for a, b, dx, dy in ADJ.neighbour_edges(shapes, true, AC.RADIUS).tolist():
        best, surface = eng.ncc_search_batch([(a, b, dx, dy)], AC.RADIUS, AC.MIN_PIXELS, True)
        sc = surface[0] / float(V.FIXED_ONE)
        others = sc.copy(); others[AC.RADIUS, AC.RADIUS] = -2.0
        assert best[0, :2].tolist() == [0, 0]
        assert round(float(sc[AC.RADIUS, AC.RADIUS]), 4) >= 0.9968 and round(float(sc[AC.RADIUS, AC.RADIUS] - others.max()), 2) >= 0.03
    calls = eng.calls
    got, report = ADJ.adjust_offsets(eng, list(range(9)), shapes, AC.perturbed(true), AC.RADIUS, 0.5, AC.MIN_PIXELS)
    assert eng.calls == calls + 1                                      # ONE search batch over all edges
    assert got == true
    assert report["edges"] == 12 and report["measured"] == 12 and report["dropped"] == 0 and report["kept_votes"] == 0
    assert report["residual_after"]["max"] == 0.0 and report["residual_before"]["max"] > 0.0


class ScriptedSearch:
    """ncc_search_batch answered from a table {(a, b): (i, j, score)}; handles are tile indices"""

    def __init__(self, table):
        self.table = table

    def ncc_search_batch(self, jobs, radius, min_pixels, want_surface=False):
        rows = [self.table[(int(a), int(b))] for a, b, _dx, _dy in jobs]
        return np.array([[i, j, V.fixed(sc), 10000] for i, j, sc in rows], np.int32)


def test_unmeasured_edges_drop_out_or_keep_their_vote():
    """A 2 x 2 serpentine 0 1 / 3 2 (tile 3 beside tile 0).  Pair (0, 1) is measured one row off its vote; pair (1, 2) scores below the
    threshold and pair (2, 3) peaks on the border of the window: both keep their votes; the cross edge (0, 3) scores below the threshold
    and is dropped."""
    shapes = [(100, 100)] * 4
    votes = [[80, 1], [2, 80], [-80, -1]]
    R = 4
    assert [tuple(e[:2]) for e in ADJ.neighbour_edges(shapes, votes, R).tolist()] == [(0, 1), (0, 3), (1, 2), (2, 3)]
    eng = ScriptedSearch({(0, 1): (1, 0, 0.9), (0, 3): (0, 2, 0.49), (1, 2): (2, 2, 0.2), (2, 3): (R, 0, 0.95)})
    got, report = ADJ.adjust_offsets(eng, [0, 1, 2, 3], shapes, votes, R, 0.5, 0)
    assert got == [[81, 1], [2, 80], [-80, -1]]
    assert (report["edges"], report["measured"], report["dropped"], report["kept_votes"]) == (4, 1, 1, 2)
    # the same cross edge measured: it enters the fit and pulls the loop closed (the 2-px disagreement in dy is spread over the loop)
    eng.table[(0, 3)] = (0, 2, 0.8)
    got2, report2 = ADJ.adjust_offsets(eng, [0, 1, 2, 3], shapes, votes, R, 0.5, 0)
    assert report2["measured"] == 2 and report2["dropped"] == 0
    P = np.floor(ADJ.solve_positions(4, [(0, 1, 81, 1), (0, 3, 2, 82), (1, 2, 2, 80), (2, 3, -80, -1)]) + 0.5)
    assert got2 == (P[1:] - P[:-1]).astype(int).tolist() and got2 != got
    # a peak on the border in j counts as unmeasured as well; exactly at the threshold counts as measured
    eng.table[(0, 1)] = (0, -R, 0.99)
    eng.table[(0, 3)] = (0, 0, 0.5)
    _got3, report3 = ADJ.adjust_offsets(eng, [0, 1, 2, 3], shapes, votes, R, 0.5, 0)
    assert (report3["measured"], report3["kept_votes"]) == (1, 3)


def test_method_attributes_and_the_short_segment():
    m = isa.Method()
    assert (m.globalAdjust, m.adjustRadius, m.adjustThreshold, m.adjustMinPixels) == ("none", 4, 0.5, 4096)
    st = isa.Stitcher()
    st.globalAdjust = "ncc"
    st.isPrintLog = False
    assert st._globalAdjust(["a", "b"], [[5, 6]]) == [[5, 6]]           # two tiles: nothing to adjust, no engine, no file is opened
    st.globalAdjust = "bogus"
    with pytest.raises(ValueError):
        st._globalAdjust(["a", "b", "c"], [[5, 6], [7, 8]])
