"""Method.exposureCompensation on the host: the edges, the solver of imagestitch_amd/exposure.py against tests/exposure_ref.py, what the
reference solve recovers of a known truth, the defaults and the refusals.  No GPU: the engine is a small numpy double defined here."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import exposure as EX

import exposure_ref as ER

# ---- the 3 x 3 grid of the tests: tiles of 96 x 128 with 24 px overlaps along a serpentine path ------------------------------------
TH, TW, OV = 96, 128, 24
SERPENTINE = [[0, TW - OV], [0, TW - OV], [TH - OV, 0], [0, OV - TW], [0, OV - TW], [TH - OV, 0], [0, TW - OV], [0, TW - OV]]
TRUTH = [1.0, 0.85, 1.2, 0.9, 1.1, 0.8, 1.25, 0.95, 1.05]       # the exposure of the tile at grid position (row, col), row-major


def grid_positions():
    return ER.positions(SERPENTINE)


def exposure_grid(color=False):
    """-> (tiles along the path, truth per tile): tiles cut from the smooth scene 100 + 40 sin(y / 17) cos(x / 23) + N(0, 6) (seed 3),
    each multiplied by its exposure and rounded; no sample saturates"""
    rng = np.random.default_rng(3)
    H, W = TH + 2 * (TH - OV), TW + 2 * (TW - OV)
    y, x = np.mgrid[0:H, 0:W]
    scene = 100.0 + 40.0 * np.sin(y / 17.0) * np.cos(x / 23.0) + rng.normal(0.0, 6.0, (H, W))
    tiles, truth = [], []
    for py, px in grid_positions().tolist():
        g = TRUTH[(py // (TH - OV)) * 3 + px // (TW - OV)]
        t = np.rint(scene[py:py + TH, px:px + TW] * g)
        assert t.min() >= 1 and t.max() <= 254
        t = t.astype(np.uint8)
        if color:                                             # three channels of different brightness, the same exposure
            t = np.ascontiguousarray(np.stack([t, (t * 0.5 + 0.5).astype(np.uint8), (t * 0.75 + 0.5).astype(np.uint8)], -1))
        tiles.append(t); truth.append(g)
    return tiles, np.array(truth)


# ---- 1. edges ------------------------------------------------------------------------------------------------------------------------
def test_edges_of_a_serpentine():
    shapes = [(TH, TW)] * 9
    for fn in (EX.overlap_edges, ER.overlap_edges):
        e = fn(shapes, SERPENTINE, 256)
        assert e.dtype == np.int64 and e.shape == (20, 4)
        assert [tuple(r) for r in e[:, :2].tolist()] == sorted(tuple(r) for r in e[:, :2].tolist()) and (e[:, 0] < e[:, 1]).all()
        corner = (e[:, 2] != 0) & (e[:, 3] != 0)
        assert corner.sum() == 8 and (~corner).sum() == 12
        side = fn(shapes, SERPENTINE, OV * OV + 1)            # a corner overlap is 24 x 24 = 576
        assert np.array_equal(side, e[~corner]) and len(fn(shapes, SERPENTINE, OV * OV)) == 20
    assert np.array_equal(EX.overlap_edges(shapes, SERPENTINE, 256), ER.overlap_edges(shapes, SERPENTINE, 256))
    P = grid_positions()
    e = EX.overlap_edges(shapes, SERPENTINE, 256)
    assert np.array_equal(e[:, 2:], P[e[:, 1]] - P[e[:, 0]])


def test_edges_of_tiles_of_different_sizes():
    shapes = [(40, 60), (30, 100, 3), (10, 10)]
    offs = [[25, -20], [-100, 5]]
    for mp in (0, 1, 900, 901):
        assert np.array_equal(EX.overlap_edges(shapes, offs, mp), ER.overlap_edges(shapes, offs, mp)), mp
    assert EX.overlap_edges(shapes, offs, 0).tolist() == [[0, 1, 25, -20]]                # 15 rows x 60 columns; empty overlaps are no edges
    assert len(EX.overlap_edges(shapes, offs, 901)) == 0
    with pytest.raises(ValueError):
        EX.overlap_edges(shapes, offs[:1], 0)


# ---- 2. the solver against the reference ------------------------------------------------------------------------------------------------
def _random_problem(seed, n, E):
    rng = np.random.default_rng(seed)
    pairs = sorted({tuple(sorted(rng.choice(n, 2, replace=False).tolist())) for _ in range(E)})
    edges = np.array([(a, b, 0, 0) for a, b in pairs], np.int64)
    N = rng.integers(200, 9000, len(edges))
    Sa = (N * rng.uniform(60, 180, len(edges))).astype(np.int64)
    Sb = (N * rng.uniform(60, 180, len(edges))).astype(np.int64)
    return edges, np.stack([N, Sa, Sb], 1).astype(np.int64)


def _check_against_reference(n, edges, stats, min_samples, max_gain):
    g_ref, q_ref = ER.solve_gains(n, edges, stats, min_samples, max_gain)
    frac = g_ref * 4096.0 - np.floor(g_ref * 4096.0)
    assert (np.abs(frac - 0.5) > 1e-6).all(), "the seed puts a reference gain on a rounding boundary"     # a condition on the seed
    g, q = EX.solve_gains(n, edges, stats, min_samples, max_gain)
    assert g.dtype == np.float64 and q.dtype == np.uint16
    assert np.abs(g / g_ref - 1.0).max() <= 1e-12, float(np.abs(g / g_ref - 1.0).max())
    assert np.array_equal(q, q_ref)
    return g, q


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_solver_equals_the_reference(seed):
    edges, stats = _random_problem(seed, 12, 30)
    _check_against_reference(12, edges, stats, 1000, 2.0)     # min_samples 1000 leaves edges unmeasured: several components
    _check_against_reference(12, edges, stats, 0, 1.1)        # ... and a bound that clips
    tiles, _ = exposure_grid()
    _q, _g, e9, s9 = ER.gains(tiles, SERPENTINE, 1, 254, 256, 2.0)
    _check_against_reference(9, e9, s9, 256, 2.0)


# ---- 3. what the fit recovers ---------------------------------------------------------------------------------------------------------------
# measured with the reference alone on exposure_grid(): G_k * g_k constant within 8e-5 of its geometric mean; the largest edge
# |log(Sa / Sb)| 0.405 before, 3.5e-4 after.  Asserted within 5 x the two figures.
FLATNESS, RESIDUAL = 8e-5, 3.5e-4


def test_the_fit_recovers_known_exposures():
    tiles, truth = exposure_grid()
    Q, g, edges, stats = ER.gains(tiles, SERPENTINE, 1, 254, 256, 2.0)
    assert len(edges) == 20 and ER.measured(stats, 256).all()
    prod = g * truth
    flat = float(np.abs(prod / np.exp(np.log(prod).mean()) - 1.0).max())
    before, after = ER.residual(edges, stats, np.ones(9), 256), ER.residual(edges, stats, g, 256)
    print("flatness %.3e, residual %.4f -> %.3e" % (flat, before, after))
    assert flat <= 5 * FLATNESS and after <= 5 * RESIDUAL and 0.40 < before < 0.41
    gp, qp = EX.solve_gains(9, edges, stats, 256, 2.0)        # the product: equal to the reference, which is the yardstick
    assert np.abs(gp / g - 1.0).max() <= 1e-12 and np.array_equal(qp, Q)
    assert abs(EX.edge_residual(edges, stats, g, 256) - after) < 1e-12


# ---- 4. components, isolated tiles, unmeasured edges, the bound ----------------------------------------------------------------------------
def test_components_isolated_tiles_and_the_bound():
    edges = np.array([(0, 1, 0, 0), (1, 2, 0, 0), (3, 4, 0, 0)], np.int64)
    stats = np.array([(5000, 500000, 600000), (4000, 440000, 400000), (3000, 300000, 390000)], np.int64)
    for fn in (EX.solve_gains, ER.solve_gains):
        g, q = fn(6, edges, stats, 1000, 2.0)
        lg = np.log(g)
        assert abs(lg[:3].mean()) < 1e-12 and abs(lg[3:5].mean()) < 1e-12 and (np.abs(lg[:5]) > 0.001).all()
        assert abs(lg[3] - lg[4] - np.log(1.3)) < 1e-12       # a single edge is met exactly
        assert g[5] == 1.0 and q[5] == 4096                   # no edge at all
        # Sa == 0, Sb == 0 or too few samples: unmeasured, and nothing else to go by
        dead = np.array([(5000, 0, 600000), (5000, 600000, 0), (999, 90000, 120000)], np.int64)
        g, q = fn(6, edges, dead, 1000, 2.0)
        assert (g == 1.0).all() and (q == 4096).all()
        # a ratio of 10 on one edge: sqrt(10) and its inverse, held at the bound
        g, q = fn(2, edges[:1], np.array([(5000, 100000, 1000000)], np.int64), 1000, 2.0)
        assert g.tolist() == [2.0, 0.5] and q.tolist() == [8192, 2048]
        with pytest.raises(ValueError):
            fn(2, edges[:1], stats[:1], 1000, 16.0)
    _check_against_reference(6, edges, stats, 1000, 2.0)


# ---- 5. defaults, the engine double, refusals -------------------------------------------------------------------------------------------------
def test_method_defaults():
    m = isa.Method
    assert (m.exposureCompensation, m.exposureBand, m.exposureMinPixels, m.exposureMaxGain) == ("none", (1, 254), 4096, 2.0)
    assert m.exposureMinPixels == m.adjustMinPixels


class NumpyEngine:
    """the two exposure calls over host arrays, through the reference: handle k is tiles[k]"""

    def __init__(self, tiles):
        self.tiles = {k: t.copy() for k, t in enumerate(tiles)}
        self.applied = []

    def overlap_stats_batch(self, jobs, lo, hi):
        return np.array([ER.stats(self.tiles[a], self.tiles[b], dx, dy, lo, hi) for a, b, dx, dy in jobs], np.int64).reshape(-1, 3)

    def exposure_apply(self, handles, gains):
        assert len(set(handles)) == len(handles) == len(gains)
        self.applied.append(list(handles))
        for h, q in zip(handles, gains):
            self.tiles[h] = ER.apply(self.tiles[h], int(q))


class BareEngine:
    """an engine without the exposure calls (and without anything else: the mosaic's tiles stay on the host)"""


def _stitcher(engine, **settings):
    s = isa.Stitcher(); s._engine = engine; s.isColorMode = False; s.fuseMethod = "fadeInAndFadeOut"
    msgs = []
    s.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
    for k, v in settings.items():
        setattr(s, k, v)
    return s, msgs


def test_compensate_on_the_numpy_double():
    tiles, _ = exposure_grid()
    eng = NumpyEngine(tiles)
    s, msgs = _stitcher(eng, exposureCompensation="gain", exposureMinPixels=256)
    s._compensateExposure(list(range(9)), [t.shape for t in tiles], [[0, 0]] + SERPENTINE)
    Q, g, edges, stats = ER.gains(tiles, SERPENTINE, 1, 254, 256, 2.0)
    want = ER.correct(tiles, SERPENTINE, 1, 254, 256, 2.0)
    assert all(np.array_equal(eng.tiles[k], want[k]) for k in range(9)) and eng.applied == [list(range(9))]
    r = s.exposureReport
    assert msgs == ["  exposure compensation: 20 edges, gains %.4f .. %.4f" % (r["gain_min"], r["gain_max"])]
    assert (r["edges"], r["measured"], r["components"]) == (20, 20, 1) and 0.40 < r["residual_before"] < 0.41
    assert abs(r["gain_min"] / g.min() - 1) <= 1e-12 and abs(r["gain_max"] / g.max() - 1) <= 1e-12
    # the tiles were multiplied by the Q12 gains: two roundings of at most 0.5 / 4096 on gains of at least 0.8 add less than 2 / 4096
    assert r["residual_after"] <= 5 * RESIDUAL + 2.0 / 4096
    # the default exposureMinPixels leaves no edge of these small tiles: nothing is measured, nothing changes
    eng = NumpyEngine(tiles)
    s, msgs = _stitcher(eng, exposureCompensation="gain")
    s._compensateExposure(list(range(9)), [t.shape for t in tiles], [[0, 0]] + SERPENTINE)
    assert all(np.array_equal(eng.tiles[k], tiles[k]) for k in range(9))
    assert msgs == ["  exposure compensation: 0 edges, gains 1.0000 .. 1.0000"] and s.exposureReport["components"] == 9


def test_a_tile_listed_twice_is_corrected_once():
    tiles, _ = exposure_grid()
    eng = NumpyEngine(tiles[:2])
    q, report = EX.compensate(eng, [0, 1, 0], [tiles[0].shape, tiles[1].shape, tiles[0].shape], [SERPENTINE[0], [500, 500]],
                              band=(1, 254), min_pixels=256, max_gain=2.0)
    Q = ER.gains(tiles[:2], SERPENTINE[:1], 1, 254, 256, 2.0)[0]
    assert q.tolist() == [Q[0], Q[1], Q[0]] and eng.applied == [[0, 1]] and report["edges"] == 1
    assert np.array_equal(eng.tiles[0], ER.apply(tiles[0], Q[0])) and np.array_equal(eng.tiles[1], ER.apply(tiles[1], Q[1]))
    with pytest.raises(ValueError):
        EX.compensate(eng, [0, 1], [tiles[0].shape], [SERPENTINE[0]])


def test_refusals_through_the_stitcher(tmp_path):
    from test_host_logic import _write_tiles
    tiles, _ = exposure_grid()
    files = _write_tiles(tmp_path, tiles[:3], "x")
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = False
        for engine, setting, error in ((BareEngine(), "gain", NotImplementedError),        # no entry points
                                       (NumpyEngine(tiles[:3]), "gain", NotImplementedError),   # the calls, but no resident tiles
                                       (BareEngine(), "reinhard", ValueError), (NumpyEngine(tiles[:3]), "Gain", ValueError)):
            s, _ = _stitcher(engine, exposureCompensation=setting, exposureMinPixels=256)
            with pytest.raises(error):
                s.getStitchByOffset(files, [list(o) for o in SERPENTINE[:2]])
    finally:
        isa.Stitcher.isColorMode = old
