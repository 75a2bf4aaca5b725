"""The SURF candidate path at its list and capacity limits (-m gpu).

What the rest of the suite never reaches: k_nms's direct-append branch (a workgroup with more than NMS_LOCAL = 192 candidates), a ROI whose
candidate count meets or exceeds RoiDev::cap -- on the operator and inside a fused batch, where every kernel behind k_nms still runs to the
end on min(count, cap) --, the choice between k_rank_sort and k_bucket_sort at capacity 1023 / 1024, and the capacity retry of the native
chain (csrc/grid.hip device_eval) and of GridRegistrar._surf_batch.

Every comparison is exact: array_equal against the CPU oracle, or equality of rows against the same call at a generous capacity.  The
inputs and the figures they are chosen by (candidates per workgroup, candidate counts) are asserted from the oracle alone in
tests/test_surf_limits_host.py."""
import functools

import numpy as np
import pytest

import imagestitch_amd as isa
import surf_limit_cases as S
from chain_ref import ChainRef
from imagestitch_amd._lib import VFSMS_ERR_CAPACITY
from imagestitch_amd.grid import GridRegistrar

pytestmark = pytest.mark.gpu


def _kp_fields(k):
    return np.stack([k["x"], k["y"], k["size"], k["response"], k["octave"].astype(np.float32), k["class_id"].astype(np.float32)], 1)


@functools.lru_cache(maxsize=None)
def _oracle_describe(name):
    from oracle import oracle as O
    return O.surf_detect_describe(np.ascontiguousarray(S.case_image(name)))


def _detect_equals_oracle(engine, name):
    a, b = engine.surf_detect(S.case_image(name)), S.oracle_detect(name)
    assert len(a) == len(b) and len(b) > 0, (name, len(a), len(b))
    assert np.array_equal(_kp_fields(a), _kp_fields(b)), name
    return a


def _describe_equals_oracle(engine, name):
    kxy, desc, kfull = engine.surf_detect_describe(S.case_image(name), full=True)
    ko, do = _oracle_describe(name)
    assert len(kfull) == len(ko) and desc.shape == do.shape, (name, len(kfull), len(ko))
    assert np.array_equal(_kp_fields(kfull), _kp_fields(ko)) and np.array_equal(kfull["angle"], ko["angle"]), name
    assert np.array_equal(kxy, np.stack([ko["x"], ko["y"]], 1)) and np.array_equal(desc, do), name


# ---- a. the direct-append branch --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,cap", [(n, 0) for n in S.LATTICE_CASES] + [("lattice_small", S.SORT_BUCKETS - 1), ("lattice_small", S.SORT_BUCKETS)])
def test_direct_append_equals_oracle(engine, oracle, name, cap):
    """Lattice images put 409 .. 546 candidates into one k_nms workgroup: more than half of them take the direct append.  Capacity 0 is the
    operator's default (>= 1024: bucket sort); the small image also runs at 1023 (rank sort) and 1024.  Twice each: candidates arrive in
    the list in whatever order the atomics grant, and the result must not depend on it."""
    engine.set_keypoint_capacity(cap)
    try:
        for _ in range(2):
            _detect_equals_oracle(engine, name)
            _describe_equals_oracle(engine, name)
    finally:
        engine.set_keypoint_capacity(0)


# ---- b. the capacity edge on the operator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["noise", "lattice"])
def test_capacity_edge_on_the_operator(engine, oracle, name):
    """C candidates fit capacity C exactly; capacity C - 1 is VFSMS_ERR_CAPACITY naming C - 1; the call after it is right again"""
    C = len(S.oracle_detect(name))
    try:
        engine.set_keypoint_capacity(C)
        _detect_equals_oracle(engine, name)
        _describe_equals_oracle(engine, name)
        engine.set_keypoint_capacity(C - 1)
        for call in (engine.surf_detect, engine.surf_detect_describe):
            with pytest.raises(isa.VfsmsError) as e:
                call(S.case_image(name))
            assert e.value.code == VFSMS_ERR_CAPACITY and "exceeded %d keypoint candidates" % (C - 1) in str(e.value), str(e.value)
        engine.set_keypoint_capacity(0)
        _detect_equals_oracle(engine, name)
        _describe_equals_oracle(engine, name)
    finally:
        engine.set_keypoint_capacity(0)


# ---- c. the sort boundary ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["periodic", "lattice_small"])
def test_sort_boundary_1023_1024(engine, oracle, name):
    """capacity 1023 ranks by k_rank_sort, 1024 by k_bucket_sort + k_bucket_rank (which keeps its 1024 bucket bounds in keep_pos / order):
    the same keypoints in the same order, exact response ties included"""
    got = []
    try:
        for cap in (S.SORT_BUCKETS - 1, S.SORT_BUCKETS):
            engine.set_keypoint_capacity(cap)
            got.append(_detect_equals_oracle(engine, name))
            _describe_equals_oracle(engine, name)
    finally:
        engine.set_keypoint_capacity(0)
    assert got[0].tobytes() == got[1].tobytes()


# ---- d. overflow inside a fused batch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extended", [False, True])
def test_overflow_inside_a_fused_batch(engine, oracle, extended):
    tiles, jobs = S.batch_tiles(), S.batch_jobs()
    strips = S.strip_table(jobs)
    C = [len(oracle.surf_detect(S.strip_pixels(tiles, s))) for s in strips]
    dense = int(np.argmax(C))
    Cmax = C[dense]
    params = engine.surf_params(extended=extended)
    want = [S.oracle_row(oracle, S.strip_pixels(tiles, (j[0],) + j[2:4] + j[6:8]), S.strip_pixels(tiles, (j[1],) + j[4:8]), extended) for j in jobs]
    rng = np.random.default_rng(3)
    q = rng.normal(size=(300, 64)).astype(np.float32); t = rng.normal(size=(700, 64)).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True); t /= np.linalg.norm(t, axis=1, keepdims=True)
    handles = [engine.tile_upload(x) for x in tiles]
    try:
        hj = [(handles[j[0]], handles[j[1]]) + j[2:] for j in jobs]
        default = engine.attempt_surf_batch(hj, params)
        assert [list(r[:7]) for r in default.tolist()] == want
        engine.set_keypoint_capacity(Cmax)
        assert np.array_equal(engine.attempt_surf_batch(hj, params), default)
        engine.set_keypoint_capacity(Cmax - 1)
        with pytest.raises(isa.VfsmsError) as e:
            engine.attempt_surf_batch(hj, params)
        msg = "strip %d of %d (%d x %d) exceeded %d keypoint candidates" % (dense, len(strips), strips[dense][3], strips[dense][4], Cmax - 1)
        assert e.value.code == VFSMS_ERR_CAPACITY and msg in str(e.value), str(e.value)
        engine.set_keypoint_capacity(0)
        assert np.array_equal(engine.attempt_surf_batch(hj, params), default)            # right after: the same engine, the same rows
        i1, d1, d2 = engine.bf_l2_knn2(q, t)                                              # ... and an operator that has nothing to do with it
        oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
        assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2)
    finally:
        engine.set_keypoint_capacity(0)
        for h in handles:
            engine.tile_free(h)


# ---- e. the retry, native and Python ---------------------------------------------------------------------------------------------------------------
def test_capacity_retry_native_and_python(engine, oracle):
    """Pair 0 teaches the chain a capacity of 1.5 x 139 + 1024; the strips of pairs 1 and 2 hold 3533 .. 3595 candidates.  The batch that
    meets them overflows, is repeated at the library default and the table is the one of a run that never adapted, and the
    specification's over oracle attempts."""
    tiles = S.retry_tiles()
    shapes = [x.shape for x in tiles]
    ref, d_ref = ChainRef(S.retry_attempts(oracle, tiles), shapes, 0.2, 1, 16).chain(0, 3, 1)
    handles = [engine.tile_upload(x) for x in tiles]

    def override_is_off():
        """The context's capacity override is 0 again: 8349 candidates fit the operator's default (h w / 24 + 4096 = 9096) and nothing a
        chain can have learnt (at most 1.5 x 3595 + 1024).  Called DIRECTLY behind a chain, with no set_keypoint_capacity in between."""
        a, b = engine.surf_detect(S.case_image("lattice_large")), S.oracle_detect("lattice_large")
        assert len(a) == len(b) and np.array_equal(_kp_fields(a), _kp_fields(b))

    try:
        gp = engine.grid_params(method="surf", roiRatio=0.2, window=16)
        # native: the chain whose last batch is the retried one ...
        table, d, st = engine.pairs_offsets(handles, shapes, gp, 0, 3, 1)
        override_is_off()
        assert st[2] >= 1 and st[:2] == (3, 2), st                                       # capacity retries of device_eval
        assert np.array_equal(table, ref) and d == d_ref, (table.tolist(), ref.tolist())
        # ... and the one over the dense pairs alone: pair 1 at the default teaches about 6300, pair 2 -- the LAST batch -- runs under it
        # and fits, so only device_eval's own restore takes the override back
        table12, d12, st12 = engine.pairs_offsets(handles, shapes, gp, 1, 3, 1)
        override_is_off()
        assert st12[:3] == (2, 2, 0), st12
        assert np.array_equal(table12, ref[1:]) and d12 == d_ref
        engine.set_keypoint_capacity(8192)                                               # a user's capacity switches the adaptive rule off
        generous, d_g, st_g = engine.pairs_offsets(handles, shapes, gp, 0, 3, 1)
        engine.set_keypoint_capacity(0)
        assert st_g[:3] == (3, 2, 0), st_g
        assert np.array_equal(table, generous) and d == d_g
        # Python: the library's machine over _attempts -> _surf_batch, the same two chains
        reg = GridRegistrar(engine, roiRatio=0.2, window=16)
        reg.native = False
        res, d_py = reg.register(handles, shapes, 1)
        override_is_off()
        assert reg.capacity_retries >= 1 and (reg.stats["attempts"], reg.stats["batches"]) == (3, 2)
        assert np.array_equal(res, generous) and np.array_equal(res, ref) and d_py == d_ref
        reg = GridRegistrar(engine, roiRatio=0.2, window=16)
        res12, d_py = reg.chain(handles, shapes, 1, 3, 1)
        override_is_off()
        assert getattr(reg, "capacity_retries", 0) == 0 and (reg.stats["attempts"], reg.stats["batches"]) == (2, 2) and reg._kp_cap > 3595
        assert np.array_equal(res12, ref[1:]) and d_py == d_ref
    finally:
        engine.set_keypoint_capacity(0)
        for h in handles:
            engine.tile_free(h)
