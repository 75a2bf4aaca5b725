"""GPU tests of offsetCaculate = "ransac" (csrc/consensus_kernels.hip): vfsms_consensus_offset and the consensus vote tail of the fused
paths equal the numpy specification tests/consensus_ref.py bit for bit, equal the mode at t = 0, and register real and synthetic
paths through the Stitcher and GridRegistrar."""
import json
import os

import numpy as np
import pytest

import consensus_ref as R
import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

pytestmark = pytest.mark.gpu

TOLS = (0, 1, 3, 64)


def _cluster_votes(rng, nv):
    """nv non-(0, 0) votes: a true offset split over neighbouring tuples, a second weaker cluster, duplicated outliers, uniform noise"""
    if nv == 0:
        return np.zeros((0, 2), np.int64)
    parts = [rng.integers(0, 2, (nv // 3 + 1, 2)) + [731, -212],
             rng.integers(-2, 3, (nv // 5 + 1, 2)) + [-1400, 388],
             np.repeat(rng.integers(-3000, 3000, (nv // 50 + 1, 2)), 4, axis=0),
             rng.integers(-4000, 4000, (nv, 2))]
    V = np.concatenate(parts)[:nv]
    V = V[rng.permutation(len(V))]
    V[(V[:, 0] == 0) & (V[:, 1] == 0)] = [1, 1]
    return V


def _with_zero_votes(rng, V):
    """(0, 0) votes sprinkled in: the matches count them, the estimator drops them"""
    n0 = max(1, len(V) // 20)
    Z = np.zeros((len(V) + n0, 2), np.int64)
    keep = np.sort(rng.choice(len(Z), len(V), replace=False))
    Z[keep] = V
    return Z


def _vote_sets():
    rng = np.random.default_rng(17)
    sets = [("nv%d" % nv, _with_zero_votes(rng, _cluster_votes(rng, nv))) for nv in (0, 1, 2, 1023, 1024, 1025, 5600, 5601, 9000, 20000)]
    sets.append(("all_equal", np.tile([[37, -5]], (3000, 1))))
    g = np.stack(np.meshgrid(np.arange(-20, 20), np.arange(-20, 20)), -1).reshape(-1, 2) * 3
    sets.append(("lattice_ties", np.tile(g[(g[:, 0] != 0) | (g[:, 1] != 0)], (3, 1))))               # every tuple three times
    sets.append(("lattice_dense", np.tile(g // 3, (2, 1))))                                           # spacing 1: windows overlap everywhere
    e = np.array([[8191, -8191], [-8191, 8191], [8191, 8191], [-8191, -8191], [8190, -8191], [-8191, 8190]])
    sets.append(("extremes", np.concatenate([np.tile(e, (300, 1)), rng.integers(-8191, 8192, (1500, 2))])))
    dup = np.repeat(rng.integers(-600, 600, (40, 2)), rng.integers(1, 200, 40), axis=0)
    sets.append(("heavy_duplication", dup[rng.permutation(len(dup))]))
    return sets


@pytest.fixture(scope="module")
def vote_sets():
    return [(name, V, *R.keypoints_for_votes(V, seed=k)) for k, (name, V) in enumerate(_vote_sets())]


def test_consensus_offset_equals_the_specification(engine, vote_sets):
    for name, V, kA, kB, m in vote_sets:
        for t in TOLS:
            want = R.consensus_from_votes(V, t, 3)
            got = engine.consensus_offset(kA, kB, m, t, 3)
            assert got == want, (name, t, got, want)
            assert engine.consensus_offset(kA, kB, m, t, 10**6) == (False, want[1], want[2]), (name, t)
    assert engine.consensus_offset(np.zeros((3, 2), np.float32), np.zeros((3, 2), np.float32), np.zeros((0, 2), np.int32), 3) == (False, [0, 0], 0)
    kA, kB, m = R.keypoints_for_votes([(4, 4)] * 5)
    for bad in (-1, 65):
        with pytest.raises(isa.VfsmsError):
            engine.consensus_offset(kA, kB, m, bad)
    for bad in ((2, 3), (1, -1), (1, 65)):
        with pytest.raises(isa.VfsmsError):
            engine.set_offset_estimator(*bad)


def test_consensus_at_zero_tolerance_is_the_mode(engine, vote_sets):
    for name, V, kA, kB, m in vote_sets:
        for ev in (1, 3, 50):
            assert engine.consensus_offset(kA, kB, m, 0, ev) == engine.mode_offset(kA, kB, m, ev), (name, ev)


# ---- the fused paths -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_tiles():
    g = SyntheticGrid(2, 2, 640)
    return g, g.tiles(threads=1)


def _jobs(tiles, handles):
    """ROI pairs of the 2 x 2 grid in all four directions and two ROI growths -> [(job, roiA, roiB)]"""
    out = []
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        for d in (1, 2, 3, 4):
            for i in (1, 2):
                ra = isa.roi_rect(tiles[a].shape, d, "first", 0.2 * i)
                rb = isa.roi_rect(tiles[b].shape, d, "second", 0.2 * i)
                job = (handles[a], handles[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])
                out.append((job, tiles[a][ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]], tiles[b][rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]]))
    return out


def _check_rows(rows, mode_rows, per_op, t, ev=3):
    for k, (row, mrow, (kA, kB, pairs)) in enumerate(zip(rows, mode_rows, per_op)):
        assert list(row[4:7]) == list(mrow[4:7]), (k, row, mrow)
        assert int(row[6]) == len(pairs), (k, row)
        st, off, c = R.consensus_offset(kA, kB, pairs, t, ev)
        assert [int(row[0]), int(row[1]), int(row[2]), int(row[3])] == [int(st), off[0], off[1], c], (k, t, row, (st, off, c))
        if t == 0:
            assert list(row) == list(mrow), (k, row, mrow)


def _run(engine, fn, t):
    engine.set_offset_estimator("ransac", t)
    try:
        return fn()
    finally:
        engine.set_offset_estimator("mode")


def test_fused_surf_and_orb_batches_under_the_consensus(engine, grid_tiles):
    _g, tiles = grid_tiles
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        jobs = _jobs(tiles, hs)
        J = [j for j, _a, _b in jobs]
        surf_ops, orb_ops = [], []
        for _j, a, b in jobs:
            ka, da = engine.surf_detect_describe(np.ascontiguousarray(a)); kb, db = engine.surf_detect_describe(np.ascontiguousarray(b))
            surf_ops.append((ka, kb, engine.bf_l2_ratio_matches(da, db, 0.75) if len(ka) and len(kb) else np.zeros((0, 2), np.int32)))
            ka, da = engine.orb_detect_describe(np.ascontiguousarray(a)); kb, db = engine.orb_detect_describe(np.ascontiguousarray(b))
            orb_ops.append((ka, kb, engine.bf_hamming_matches(da, db, -1) if len(ka) and len(kb) else np.zeros((0, 2), np.int32)))
        surf_mode = engine.attempt_surf_batch(J)
        orb_mode = engine.attempt_orb_batch(J)
        assert (surf_mode[:, 6] > 20).sum() > 8 and (orb_mode[:, 6] > 20).sum() > 8
        for t in TOLS:
            _check_rows(_run(engine, lambda: engine.attempt_surf_batch(J), t), surf_mode, surf_ops, t)
            _check_rows(_run(engine, lambda: engine.attempt_surf_batch_enhanced(J), t), surf_mode, surf_ops, t)
            _check_rows(_run(engine, lambda: engine.attempt_orb_batch(J), t), orb_mode, orb_ops, t)
        assert np.array_equal(engine.attempt_surf_batch(J), surf_mode)                  # mode again
    finally:
        for h in hs:
            engine.tile_free(h)


def test_features_match_offset_batch_under_the_consensus(engine, grid_tiles):
    _g, tiles = grid_tiles
    hs = [engine.tile_upload(t) for t in tiles]
    feats, _n = engine.features_surf_batch(hs)
    try:
        fa, fb = [feats[0], feats[0], feats[1], feats[2]], [feats[1], feats[2], feats[3], feats[3]]
        per_op = []
        for a, b in zip(fa, fb):
            ia, ib = feats.index(a), feats.index(b)
            ka, da = engine.surf_detect_describe(tiles[ia]); kb, db = engine.surf_detect_describe(tiles[ib])
            per_op.append((ka, kb, engine.bf_l2_ratio_matches(da, db, 0.75)))
        mode_rows = engine.features_match_offset_batch(fa, fb)
        for t in TOLS:
            _check_rows(_run(engine, lambda: engine.features_match_offset_batch(fa, fb), t), mode_rows, per_op, t)
            one = _run(engine, lambda: engine.features_match_offset(fa[1], fb[1]), t)
            st, off, c = R.consensus_offset(*per_op[1], t, 3)
            assert [int(v) for v in one[:4]] == [int(st), off[0], off[1], c]
    finally:
        for f in feats:
            engine.features_free(f)
        for h in hs:
            engine.tile_free(h)


# ---- whole paths -------------------------------------------------------------------------------------------------------------------
def test_synthetic_grid_through_the_stitcher_with_ransac(engine):
    grid = SyntheticGrid(3, 3, 1024)
    tiles = grid.tiles(threads=4)
    truth = grid.true_offsets()
    hs = [engine.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    J = [(hs[0], hs[1], *isa.roi_rect(shapes[0], 1, "first", 0.2)[:2], *isa.roi_rect(shapes[1], 1, "second", 0.2)[:2],
          *isa.roi_rect(shapes[0], 1, "first", 0.2)[2:])]
    before = engine.attempt_surf_batch(J)
    try:
        st = isa.Stitcher(); st._engine = engine
        st.isPrintLog = False; st.featureMethod = "surf"; st.roiRatio = 0.2; st.offsetCaculate = "ransac"; st.direction = 1
        regs = []
        for native in (True, False):
            reg = st._makeRegistrar("surf", len(tiles))
            reg.native = native
            regs.append(reg.register(hs, shapes, 1))
        assert np.array_equal(regs[0][0], regs[1][0]) and regs[0][1] == regs[1][1]
        table = regs[0][0]
        for k, row in enumerate(table):
            assert row[0] == 1 and abs(int(row[1]) - truth[k][0]) <= 1 and abs(int(row[2]) - truth[k][1]) <= 1, (k, row, truth[k])
        # pair by pair through the reference's call surface, direction threaded: the same rows
        st.direction = 1
        for k, row in enumerate(table):
            assert st.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]]) == (True, [int(row[1]), int(row[2])]), k
            assert st.direction == int(row[3])
        st.releaseTiles()
        assert np.array_equal(engine.attempt_surf_batch(J), before)                    # the registrar restored mode
    finally:
        for h in hs:
            engine.tile_free(h)


def test_real_dendritic_pairs_surf_ransac(engine, golden_dir):
    """the 25 real dendriticCrystal pairs of tests/golden/real_path_strips (five neighbourhoods around the turns of the path), pair by pair
    through the Stitcher with SURF and offsetCaculate "ransac", the direction threaded: every pair within 1 px of Stitcher.py:87"""
    from test_oracle_golden import _rebuild_frames
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    rows = []
    for nb in meta:
        frames = _rebuild_frames(nb, g)
        st = isa.Stitcher(); st._engine = engine
        st.featureMethod = "surf"; st.roiRatio = 0.2; st.offsetEvaluate = 3; st.isPrintLog = False; st.offsetCaculate = "ransac"
        st.direction = nb["incoming_direction"]
        for k, e in enumerate(nb["expected"]):
            ok, off = st.calculateOffsetForFeatureSearchIncre([frames[k], frames[k + 1]])
            good = ok and abs(off[0] - e["gold"][0]) <= 1 and abs(off[1] - e["gold"][1]) <= 1
            rows.append({"turn": nb["turn"], "ok": bool(ok), "offset": list(off), "direction": st.direction, "gold": e["gold"],
                         "mode_offset": e["offset"], "within_1px": bool(good)})
        st.releaseTiles()
    print(json.dumps(rows))
    assert len(rows) == 25 and all(r["within_1px"] for r in rows), [r for r in rows if not r["within_1px"]]
