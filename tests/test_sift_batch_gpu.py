"""GPU tests (-m gpu) of the fused SIFT attempt batch (vfsms_attempt_sift_batch): rows equal the chain numpy specification ->
oracle matcher -> oracle vote; the integer matrix-core 2-NN equals the exhaustive VALU kernel at production scale (VFSMS_BF_EXACT=1 in a
child process, and the operators called one by one); rows do not depend on how the jobs are batched, ordered, deduplicated or grouped;
GridRegistrar(method="sift") equals the per-pair walk.  Every comparison is == on integer rows.

Run as a script (`python tests/test_sift_batch_gpu.py <job set> <out.json>`) this file is the child process: it prints nothing and
writes the rows of a named job set, computed under whatever VFSMS_* switches its environment carries."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 600                                 # seconds, per child process


# ---- job sets (deterministic: parent and child build the same) ---------------------------------------------------------------------
def _roi_job(hs, shapes, a, b, d, ratio=0.2):
    ra = isa.roi_rect(shapes[a], d, "first", ratio); rb = isa.roi_rect(shapes[b], d, "second", ratio)
    assert ra[2:] == rb[2:]
    return (hs[a], hs[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])


def mixed_set():
    """strips of a 2 x 2 grid of 640 px tiles in all four directions (two shapes), one job with A and B from the same tile, one against a
    constant tile (no keypoints), one strip used by several jobs, one job twice -> (tiles, jobs as (tile a, tile b, ay0, ...))"""
    tiles = list(SyntheticGrid(2, 2, 640).tiles(threads=1)) + [np.full((640, 640), 93, np.uint8)]
    shapes = [t.shape for t in tiles]
    idx = list(range(len(tiles)))
    jobs = [_roi_job(idx, shapes, a, b, d) for a, b, d in [(0, 1, 1), (1, 2, 2), (2, 3, 3), (0, 2, 4), (0, 1, 2), (1, 1, 1), (0, 4, 1),
                                                           (4, 3, 2), (0, 1, 1)]]
    return tiles, jobs


def _tie_tile(strip):
    """a tile whose right half repeats its left half: every keypoint well inside a half has a twin with the same descriptor"""
    t = strip.copy()
    w = t.shape[1] // 2
    t[:, w:2 * w] = t[:, :w]
    return t


def scale_set():
    """the production strip pair (409 x 2048 of a 2 x 1 grid of 2048 px tiles), the three real strip pairs of tests/golden/real_strips.npz
    (whole arrays as tiles) and a constructed tie case: the production A strip against a B strip made of two copies of one half"""
    A, B = SyntheticGrid(2, 1, 2048).tiles(threads=2)
    g = np.load(os.path.join(GOLDEN, "real_strips.npz"))
    tiles = [A, B]
    jobs = [_roi_job([0, 1], [A.shape, B.shape], 0, 1, 1)]
    for n in range(3):
        a, b = np.ascontiguousarray(g["r%d_roiA" % n]), np.ascontiguousarray(g["r%d_roiB" % n])
        tiles += [a, b]
        jobs.append((len(tiles) - 2, len(tiles) - 1, 0, 0, 0, 0, a.shape[0], a.shape[1]))
    sa = np.ascontiguousarray(A[-409:]); tie = _tie_tile(np.ascontiguousarray(B[:409]))
    tiles += [sa, tie]
    jobs.append((len(tiles) - 2, len(tiles) - 1, 0, 0, 0, 0, 409, 2048))
    return tiles, jobs


SETS = {"mixed": mixed_set, "scale": scale_set}


def _strips(tiles, job):
    a, b, ay0, ax0, by0, bx0, h, w = job
    return (np.ascontiguousarray(tiles[a][ay0:ay0 + h, ax0:ax0 + w]), np.ascontiguousarray(tiles[b][by0:by0 + h, bx0:bx0 + w]))


def run_set(engine, name, ratio=0.75, oe=3, order=None, one_by_one=False):
    """rows of a job set through attempt_sift_batch (optionally permuted, or one call per job), in the set's own order"""
    tiles, jobs = SETS[name]()
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        real = [(hs[j[0]], hs[j[1]]) + tuple(j[2:]) for j in jobs]
        order = list(range(len(real))) if order is None else list(order)
        if one_by_one:
            got = [engine.attempt_sift_batch([real[k]], None, ratio, oe)[0] for k in order]
        else:
            got = engine.attempt_sift_batch([real[k] for k in order], None, ratio, oe)
        rows = [None] * len(real)
        for k, r in zip(order, got):
            rows[k] = [int(v) for v in r[:7]]
        return rows
    finally:
        for h in hs:
            engine.tile_free(h)


def child_rows(name, env):
    """the rows of a job set from a fresh process with `env` added to the environment (the switches are read once per process)"""
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "rows.json")
        e = dict(os.environ, **env)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), name, out], env=e, cwd=ROOT, timeout=CHILD_TIMEOUT,
                           capture_output=True, text=True)
        assert p.returncode == 0, (env, p.returncode, p.stderr[-2000:])
        return json.load(open(out))


# ---- 1. the batch equals the chain computed outside the product ---------------------------------------------------------------------
def test_batch_equals_the_reference_chain(engine, oracle):
    import sift_ref as S
    tiles, jobs = mixed_set()
    memo = {}

    def ref(strip):
        key = strip.tobytes() + bytes(str(strip.shape), "ascii")
        if key not in memo:
            memo[key] = S.sift_detect_describe(strip, None)[:2]
        return memo[key]

    def chain(A, B, ratio, oe):
        (ka, da), (kb, db) = ref(A), ref(B)
        pairs = oracle.bf_l2_ratio_matches(da, db, ratio) if len(da) and len(db) else np.zeros((0, 2), np.int32)
        st, off, votes = oracle.mode_offset(ka, kb, pairs, oe) if len(pairs) else (False, [0, 0], 0)
        return [int(st), int(off[0]), int(off[1]), int(votes), len(ka), len(kb), len(pairs)]

    shapes = {tuple(j[6:]) for j in jobs}
    assert len(shapes) == 2
    for ratio in (0.75, 0.6):
        for oe in (3, 10):
            rows = run_set(engine, "mixed", ratio, oe)
            for j, row in zip(jobs, rows):
                A, B = _strips(tiles, j)
                assert row == chain(A, B, ratio, oe), (j, ratio, oe, row)
    assert rows[6][5] == 0 and rows[7][4] == 0                # the constant strips have no keypoints
    assert rows[0][4] > 100 and rows[0] == rows[8]


# ---- 2. both matchers agree at scale ------------------------------------------------------------------------------------------------
def _operator_chain(engine, A, B, ratio, oe):
    ka, da = engine.sift_detect_describe(A); kb, db = engine.sift_detect_describe(B)
    pairs = engine.bf_l2_ratio_matches(da, db, ratio) if len(da) and len(db) else np.zeros((0, 2), np.int32)
    st, off, votes = engine.mode_offset(ka, kb, pairs, oe) if len(pairs) else (False, [0, 0], 0)
    return [int(st), int(off[0]), int(off[1]), int(votes), len(ka), len(kb), len(pairs)]


def test_integer_matcher_equals_the_valu_kernel_at_scale(engine):
    tiles, jobs = scale_set()
    rows = run_set(engine, "scale")
    print("rows (integer matcher):", rows)
    exact = child_rows("scale", {"VFSMS_BF_EXACT": "1"})
    print("rows (VFSMS_BF_EXACT=1):", exact)
    assert rows == exact
    for j, row in zip(jobs, rows):
        A, B = _strips(tiles, j)
        assert row == _operator_chain(engine, A, B, 0.75, 3), (j, row)
    assert min(r[4] for r in rows[:4]) > 500 and rows[0][4] > 5000
    # the tie case: B's descriptors come in identical pairs; the lower index wins and the ratio test drops the match
    A, B = _strips(tiles, jobs[-1])
    _ka, da = engine.sift_detect_describe(A); _kb, db = engine.sift_detect_describe(B)
    i1, d1, d2 = engine.bf_l2_knn2(da, db)
    _u, first, inv, cnt = np.unique(db, axis=0, return_index=True, return_inverse=True, return_counts=True)
    twins = cnt[inv.ravel()[i1]] > 1
    assert twins.sum() > 100, int(twins.sum())
    assert np.array_equal(d1[twins], d2[twins])
    lowest = np.array([np.nonzero((db == db[i]).all(1))[0][0] for i in i1[twins][:200]])
    assert np.array_equal(i1[twins][:200], lowest)
    assert rows[-1][6] < (~twins).sum() + 1 and rows[-1][6] <= len(da) - int(twins.sum())


# ---- 3. independence from batching --------------------------------------------------------------------------------------------------
def test_rows_do_not_depend_on_batching(engine):
    base = run_set(engine, "mixed")
    assert run_set(engine, "mixed", one_by_one=True) == base
    perm = list(np.random.default_rng(4).permutation(len(base)))
    assert run_set(engine, "mixed", order=perm) == base
    assert run_set(engine, "mixed", order=list(range(len(base)))[::-1]) == base
    assert child_rows("mixed", {"VFSMS_STRIP_DEDUP": "0"}) == base
    assert child_rows("mixed", {"VFSMS_SIFT_GROUP_BYTES": "1"}) == base          # one strip per group
    assert child_rows("mixed", {"VFSMS_SIFT_GROUP_BYTES": "1", "VFSMS_STRIP_DEDUP": "0", "VFSMS_BF_EXACT": "1"}) == base


# ---- 4. registrar and Stitcher ------------------------------------------------------------------------------------------------------
class GenericOnly:
    """the engine without its fused SIFT batch: the Stitcher falls back to the per-pair operator path"""

    def __init__(self, base):
        self.base = base

    def __getattr__(self, name):
        if name == "attempt_sift_batch":
            raise AttributeError(name)
        return getattr(self.base, name)


@pytest.fixture(scope="module")
def serpentine(engine):
    """the 3 x 3 serpentine of 1024-px tiles, resident on the engine, and the per-pair SIFT walk over it (computed once)
    -> (tiles, handles, shapes, truth, walk rows, end direction of the walk, the walking Stitcher)"""
    g = SyntheticGrid(3, 3, 1024)
    tiles = g.tiles(threads=4)
    st = isa.Stitcher(); st._engine = GenericOnly(engine)
    st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = 1
    assert not st._usesStockOperators()
    walk = []
    for k in range(len(tiles) - 1):
        ok, off = st.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        assert ok, k
        walk.append([1, int(off[0]), int(off[1]), st.direction])
    hs = [engine.tile_upload(t) for t in tiles]
    yield tiles, hs, [t.shape for t in tiles], g.true_offsets(), walk, st.direction, st
    for h in hs:
        engine.tile_free(h)


def _sift_registrar(engine, st):
    from imagestitch_amd.grid import GridRegistrar
    return GridRegistrar(engine, method="sift", roiRatio=0.2, searchRatio=st.searchRatio, offsetEvaluate=st.offsetEvaluate,
                         directIncre=st.directIncre, siftParams=st._siftParams())


def test_registrar_equals_the_per_pair_walk(engine, serpentine):
    _tiles, hs, shapes, truth, walk, d_walk, st = serpentine
    reg = _sift_registrar(engine, st)
    table, d = reg.register(hs, shapes, 1)
    again, _d = reg.register(hs, shapes, 1)                # with the path memory of the first run
    assert [list(r[:4]) for r in table.tolist()] == walk and d == d_walk
    assert np.array_equal(table, again)
    for k, r in enumerate(table.tolist()):
        assert abs(r[1] - truth[k][0]) <= 1 and abs(r[2] - truth[k][1]) <= 1, (k, r, truth[k])


def test_both_routes_of_the_registrar_run_one_machine(engine, serpentine):
    """GridRegistrar.native selects the evaluator, never the machine: device-evaluated chains (vfsms_pairs_offsets) and the library's
    machine over the engine's fused batches (vfsms_pairs_offsets_eval over GridRegistrar._attempts) give the same table, the same end
    direction and the same attempt and batch counts for SURF, ORB and phase correlation, cold and with the path memory of the first run;
    SIFT, which has the evaluator route only, gives the per-pair walk."""
    from imagestitch_amd.grid import GridRegistrar
    _tiles, hs, shapes, _truth, walk, d_walk, st = serpentine
    for method in ("surf", "orb", "phase"):
        got = []
        for native in (True, False):
            reg = GridRegistrar(engine, method=method, roiRatio=0.2, directIncre=1, window=8)
            reg.native = native
            runs = [reg.register(hs, shapes, 1) for _ in range(2)]
            got.append(([t.tolist() for t, _d in runs], [int(d) for _t, d in runs], reg.stats["attempts"], reg.stats["batches"]))
        print("%s: %d of %d pairs registered, %d attempts in %d batches over two runs" % (method, sum(r[0] for r in got[0][0][0]), len(hs) - 1, got[0][2], got[0][3]))
        assert got[0] == got[1], (method, got)
    reg = _sift_registrar(engine, st)
    assert not reg.native
    table, d = reg.register(hs, shapes, 1)
    assert [list(r[:4]) for r in table.tolist()] == walk and d == d_walk


def test_dendritic_pairs_through_the_fused_attempt(engine, golden_dir):
    """the 25 real pairs of tests/golden/real_path_strips through the Stitcher, whose "sift" attempts now run attempt_sift_batch: the rows
    of the generic operator path, and 25 of 25 within 1 px of Stitcher.py:87"""
    from test_oracle_golden import _rebuild_frames
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    within, total = 0, 0
    for nb in meta:
        frames = _rebuild_frames(nb, g)
        got = []
        for eng in (engine, GenericOnly(engine)):
            st = isa.Stitcher(); st._engine = eng
            st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = nb["incoming_direction"]
            assert st._usesStockOperators() == (eng is engine)
            out = []
            for k in range(len(nb["expected"])):
                ok, off = st.calculateOffsetForFeatureSearchIncre([frames[k], frames[k + 1]])
                out.append((bool(ok), list(off), st.direction))
            got.append(out)
        assert got[0] == got[1]
        for e, (ok, off, _d) in zip(nb["expected"], got[0]):
            total += 1
            within += bool(ok and abs(off[0] - e["gold"][0]) <= 1 and abs(off[1] - e["gold"][1]) <= 1)
    print("sift dendritic pairs within 1 px through the fused attempt: %d / %d" % (within, total))
    assert total == 25 and within == 25


# ---- 5. capacity --------------------------------------------------------------------------------------------------------------------
def test_a_small_keypoint_capacity_truncates_nothing(engine):
    """the batch sizes every array from counts it reads back (two syncs per group), so no capacity applies to it: with the SURF paths'
    keypoint capacity forced far below a strip's keypoints the rows are complete, and later calls are unaffected"""
    base = run_set(engine, "mixed")
    engine.set_keypoint_capacity(16)
    try:
        small = run_set(engine, "mixed")
    finally:
        engine.set_keypoint_capacity(0)
    assert small == base and max(r[4] for r in base) > 16
    assert run_set(engine, "mixed") == base


def test_bad_arguments_and_refusals(engine):
    assert engine.attempt_sift_batch([]).shape == (0, isa._lib.ATTEMPT_INTS)
    h = engine.tile_upload(np.zeros((64, 64), np.uint8))
    try:
        with pytest.raises(isa.VfsmsError):
            engine.attempt_sift_batch([(h, h, 0, 0, 0, 0, 32, 64)], engine.sift_params(n_features=100))
        with pytest.raises(isa.VfsmsError):
            engine.attempt_sift_batch([(h, h, 0, 0, 0, 0, 32, 64)], engine.sift_params(n_octave_layers=9))
        with pytest.raises(isa.VfsmsError):
            engine.attempt_sift_batch([(h, h, 40, 0, 0, 0, 32, 64)])
        assert list(engine.attempt_sift_batch([(h, h, 0, 0, 0, 0, 32, 64)])[0][:7]) == [0, 0, 0, 0, 0, 0, 0]
    finally:
        engine.tile_free(h)


if __name__ == "__main__":
    name, out_path = sys.argv[1], sys.argv[2]
    eng = isa.Engine(0)
    try:
        rows = run_set(eng, name)
    finally:
        eng.close()
    with open(out_path, "w") as f:
        json.dump(rows, f)
