"""GPU tests (-m gpu) of featureMethod "orb" (csrc/orb_kernels.hip): the device equals the independent numpy reference tests/orb_ref.py
field for field and byte for byte -- at production strip and tile shapes, at the shape boundaries of the 64 x 16 FAST / NMS tiles, on
adversarial inputs (ties that overflow the default keypoint capacities, FAST threshold clipping, exact axis angles, keypoints at the
border distance) and over the parameter space -- and passes the float64 checks of tests/orb_f64.py.  The fused attempt
(vfsms_attempt_orb_batch) equals the chain reference -> Hamming 1-NN -> the oracle's mode vote."""
import ctypes as C

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd._lib import VFSMS_ERR_BAD_ARG, VFSMS_ERR_UNSUPPORTED
import orb_cases as OC
import orb_f64 as F
import orb_ref as R

pytestmark = pytest.mark.gpu
FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def _params(p):
    return isa.Engine.orb_params(p["nfeatures"], p["scale_factor"], p["nlevels"], p["edge_threshold"], p["first_level"], 2, 0,
                                 p["patch_size"], p["fast_threshold"])


def _device(engine, img, p):
    kxy, desc, k = engine.orb_detect_describe(img, _params(p), full=True)
    assert np.array_equal(kxy[:, 0], k["x"]) and np.array_equal(kxy[:, 1], k["y"])
    return k, desc


def _assert_same(name, got, want):
    (kg, dg), (kw, dw) = got, want
    assert len(kg) == len(kw), (name, len(kg), len(kw))
    for f in FIELDS:
        bad = np.nonzero(kg[f] != kw[f])[0]
        assert bad.size == 0, (name, f, int(bad[0]), kg[bad[0]], kw[bad[0]])
    bad = np.nonzero((dg != dw).any(1))[0]
    assert bad.size == 0, (name, "descriptor", int(bad[0]), kg[bad[0]])


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_device_equals_reference(engine, name):
    """production shapes, real strips, adversarial inputs (the lattices of period 8 and 12 hold more tied keypoints than the default
    capacities: every one comes back), parameter variants and the small edge thresholds whose reads leave the level"""
    k, d, st = OC.reference(name)
    got = _device(engine, OC.image(name), OC.CASES[name][1])
    _assert_same(name, got, (k, d))
    p = OC.CASES[name][1]
    F.check_all(got[0], got[1], st, p["scale_factor"], p["patch_size"])


# heights / widths at the FAST + NMS tile boundaries (64 x 16 tiles, 4 px halo) and at the border rule (2 x 31 + 1)
EDGE_DIMS = [1, 2, 31, 62, 63, 64, 65, 95, 97]
TILE_W = [127, 129, 191, 193]
TILE_H = [47, 49, 79, 81]


def _shape_cases():
    out = [(d, 2048) for d in EDGE_DIMS] + [(2048, d) for d in EDGE_DIMS]
    out += [(409, w) for w in TILE_W] + [(h, 640) for h in TILE_H]
    return out


@pytest.mark.parametrize("shape", _shape_cases(), ids=lambda s: "%dx%d" % s)
def test_shape_boundaries(engine, shape):
    """a level of 0 rows or columns (upstream's resize asserts) gives 0 keypoints, as the reference does, never a fault"""
    img = OC.texture(*shape, seed=shape[0] * 7 + shape[1])
    _assert_same(shape, _device(engine, img, OC.DEFAULT), R.detect_describe(img))


def test_zero_row_levels_at_scale_two(engine):
    """scale 2, 8 levels: 63 rows leave the top level with 0 rows -> no keypoints although level 0 has corners"""
    p = OC.params(scale_factor=2.0)
    img = OC.texture(63, 2048, 9)
    assert R.level_sizes(63, 2048, 2.0, 8)[-1][0] == 0
    k, d = _device(engine, img, p)
    assert len(k) == 0 and len(R.detect_describe(img, **p)[0]) == 0
    assert len(R.detect_describe(img, **OC.params(scale_factor=2.0, nlevels=6))[0]) > 0


def test_tile_2048_and_strided_views(engine):
    big = OC.texture(2048, 2048, 21)
    _assert_same("2048^2", _device(engine, big, OC.DEFAULT), R.detect_describe(big))
    host = OC.texture(600, 2200, 22)
    for view in (host[17:17 + 409, 33:33 + 2048], host[:2048 // 5, 100:2100].T.copy().T):
        want = R.detect_describe(np.ascontiguousarray(view))
        _assert_same("view", _device(engine, view, OC.DEFAULT), want)


def test_capacity_retry_reports_every_tied_keypoint(engine):
    """a caller's cap below the count is an error that reports the count; cap=None runs once more with it"""
    img = OC.image("lattice8")
    k, _, _ = OC.reference("lattice8")
    kxy, desc = engine.orb_detect_describe(img)
    assert len(kxy) == len(k) > 12048
    with pytest.raises(isa.VfsmsError):
        engine.orb_detect_describe(img, cap=100)


@pytest.mark.parametrize("change", [dict(first_level=1), dict(wta_k=3), dict(wta_k=4), dict(score_type=1), dict(patch_size=32),
                                    dict(patch_size=31, edge_threshold=15), dict(patch_size=2, edge_threshold=1), dict(n_levels=0),
                                    dict(n_levels=9), dict(scale_factor=1.0), dict(scale_factor=0.9)],
                         ids=lambda c: ",".join("%s=%s" % kv for kv in c.items()))
def test_refusals(engine, change):
    p = isa.Engine.orb_params()
    for k, v in change.items():
        setattr(p, k, v)
    img = OC.texture(128, 128, 1)
    kxy = np.zeros((16, 2), np.float32); desc = np.zeros((16, 32), np.uint8); n = C.c_int(-7)
    rc = engine.lib.vfsms_orb_detect_describe(engine.ctx, img.ctypes.data_as(C.c_void_p), 128, 128, 128, C.byref(p),
                                              kxy.ctypes.data_as(C.c_void_p), desc.ctypes.data_as(C.c_void_p), None, 16, C.byref(n))
    assert rc in (VFSMS_ERR_UNSUPPORTED, VFSMS_ERR_BAD_ARG), (change, rc)
    assert n.value == -7


# ---- fused attempts ---------------------------------------------------------------------------------------------------------------------
def _chain(oracle, ref, A, B, max_dist, offset_evaluate):
    """reference keypoints of both strips -> Hamming 1-NN (lowest train index on ties) -> the oracle's mode vote -> the first 7 ints of
    an attempt row"""
    (ka, da), (kb, db) = ref(A), ref(B)
    pairs, _ = R.hamming_1nn(da, db, max_dist)
    st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, offset_evaluate)
    return [int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs)]


def test_attempt_batch_equals_the_reference_chain(engine, oracle):
    from imagestitch_amd.synthetic import SyntheticGrid
    tiles = list(SyntheticGrid(2, 2, 640).tiles(threads=1)) + [OC.lattice(640, 2048, 12, 3), OC.lattice(640, 2048, 12, 5)]
    hs = [engine.tile_upload(t) for t in tiles]
    shapes = [t.shape for t in tiles]
    try:
        jobs = []
        for a, b, d in [(0, 1, 1), (1, 2, 2), (2, 3, 3), (0, 2, 4), (0, 1, 2)]:
            ra = isa.roi_rect(shapes[a], d, "first", 0.2); rb = isa.roi_rect(shapes[b], d, "second", 0.2)
            jobs.append((hs[a], hs[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]))
        jobs.append((hs[4], hs[5], 0, 0, 100, 0, 409, 2048))          # tied lattice keypoints beyond the default capacities
        p = OC.DEFAULT
        memo = {}

        def ref(strip):
            key = strip.tobytes() + bytes(str(strip.shape), "ascii")
            if key not in memo:
                memo[key] = R.detect_describe(strip, **p)
            return memo[key]

        for max_dist in (-1, 30):
            for oe in (3, 10):
                rows = engine.attempt_orb_batch(jobs, _params(p), max_dist, oe)
                for j, row in zip(jobs, rows):
                    ta, tb = hs.index(j[0]), hs.index(j[1])
                    A = tiles[ta][j[2]:j[2] + j[6], j[3]:j[3] + j[7]]; B = tiles[tb][j[4]:j[4] + j[6], j[5]:j[5] + j[7]]
                    assert list(row[:7]) == _chain(oracle, ref, A, B, max_dist, oe), (j[2:], max_dist, oe, row[:7])
        assert rows[-1][4] > 2 * 1086 + 1024                           # above the default quota-cut capacity of level 0
    finally:
        for h in hs:
            engine.tile_free(h)


def test_batch_retry_with_overflowing_strips_of_two_shapes(engine, oracle):
    """nfeatures = 100: capacities cap1 = 2136, cap2 = 1068, cap = 2248.  The 256 x 1024 lattice (2937 keypoints, 2880 on level 0) exceeds
    all of them, the 640 x 256 one (1784, 1728 on level 0) the level-0 capacity cap2 alone, the 256 x 768 one of period 12 (1041, 944) none:
    the batch runs once more with capacities grown over BOTH overflowing shapes, and the single image takes the same retry"""
    p = OC.params(nfeatures=100)
    tiles = [OC.lattice(256, 1024, 8, 3), OC.lattice(256, 1024, 8, 5), OC.lattice(640, 256, 8, 3), OC.lattice(640, 256, 8, 5),
             OC.lattice(256, 768, 12, 3), OC.lattice(256, 768, 12, 5)]
    refs = [R.detect_describe(t, **p) for t in tiles]
    assert [len(refs[i][0]) for i in (0, 2, 4)] == [2937, 1784, 1041]
    assert [int((refs[i][0]["octave"] == 0).sum()) for i in (0, 2, 4)] == [2880, 1728, 944]

    def ref(tile):
        return refs[next(i for i, t in enumerate(tiles) if t is tile)]

    hs = [engine.tile_upload(t) for t in tiles]
    try:
        pairs = [(0, 1), (4, 5), (2, 3), (0, 1)]                      # mixed shapes; the first overflowing strip is named by two jobs
        jobs = [(hs[a], hs[b], 0, 0, 0, 0) + tiles[a].shape for a, b in pairs]
        for max_dist, oe in ((-1, 3), (30, 10)):
            rows = engine.attempt_orb_batch(jobs, _params(p), max_dist, oe)
            for (a, b), row in zip(pairs, rows):
                assert list(row[:7]) == _chain(oracle, ref, tiles[a], tiles[b], max_dist, oe), (a, b, max_dist, oe, row[:7])
            assert [int(rows[k][4]) for k in (0, 2, 3)] == [2937, 1784, 2937]
    finally:
        for h in hs:
            engine.tile_free(h)
    _assert_same("lattice 256x1024", _device(engine, tiles[0], p), refs[0])
    with pytest.raises(isa.VfsmsError):
        engine.orb_detect_describe(tiles[0], _params(p), cap=100)


# ---- Hamming 1-NN (vfsms_bf_hamming_nn): one job of the batched matcher, trains in up to eight ascending ranges ------------------------------
def _hamming_sets(nq, nt, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, 256, (nq, 32), dtype=np.uint8), rng.integers(0, 256, (nt, 32), dtype=np.uint8)


def test_hamming_ties_across_train_splits_keep_the_lowest_train(engine, oracle):
    """300 queries against 70 trains: eight splits of nine trains.  Trains 35.. repeat trains 0..34, so EVERY query's minimum is tied
    between two splits; trains 5, 23, 33 (hence 40, 58, 68) are one row and so are 8 | 9 on either side of a split boundary.  The pair
    list is the oracle's, and the tied blocks name the lowest train whatever the oracle says"""
    q, t = _hamming_sets(300, 70, 11)
    t[9] = t[8]
    t[23] = t[33] = t[5]
    t[35:] = t[:35]
    assert all(np.array_equal(t[5], t[j]) for j in (23, 68)) and np.array_equal(t[8], t[9])
    assert -(-70 // 8) == 9                                           # the split's train range: 8 | 9 is a boundary
    q[100:140] = t[5]
    q[200:220] = t[8]
    for max_dist in (-1, 30):
        got = engine.bf_hamming_matches(q, t, max_dist)
        assert np.array_equal(got, oracle.bf_hamming_matches(q, t, max_dist)[0]), max_dist
        train_of = dict((int(qi), int(ti)) for ti, qi in got)
        assert all(train_of[i] == 5 for i in range(100, 140)) and all(train_of[i] == 8 for i in range(200, 220))
        assert len(got) == (300 if max_dist < 0 else 60) and got[:, 0].max() < 35


@pytest.mark.parametrize("nq,nt", [(1, 1), (1, 3), (257, 3), (64, 8)])
def test_hamming_edge_shapes(engine, oracle, nq, nt):
    """fewer trains than splits leave splits empty; 257 queries leave one lane of a second workgroup"""
    q, t = _hamming_sets(nq, nt, 100 * nq + nt)
    q[nq - 1] = t[nt - 1]                                             # one exact match survives max_dist = 30
    for max_dist in (-1, 30):
        got = engine.bf_hamming_matches(q, t, max_dist)
        assert np.array_equal(got, oracle.bf_hamming_matches(q, t, max_dist)[0]), max_dist
        assert len(got) >= 1 and tuple(got[-1]) == (np.nonzero((t == t[nt - 1]).all(1))[0][0], nq - 1)
