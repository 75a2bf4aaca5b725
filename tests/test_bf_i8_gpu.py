"""GPU tests (-m gpu) of the integer 128-d 2-NN search behind every fused SIFT attempt -- k_pack_i8_d128 + k_bf_i8_d128 + k_merge_ratio
(csrc/match_kernels.hip) -- through the operator entry vfsms_bf_l2_knn2_u8d128 (Engine.bf_l2_knn2_u8d128), which packs and searches host
descriptors exactly as the batch does.  Every comparison is np.array_equal on (i1, d1, d2): against the integer reference
tests/bf_i8_ref.py (held to two float references by tests/test_bf_i8_host.py) and against the exhaustive VALU kernel k_bf_l2_gen<128>
(Engine.bf_l2_knn2) in the same process.

Count run: the full product, 7 kinds x 120 shapes x 5 split counts (0 = the batch's own rule, 1, 2, 3, 8) = 4200 calls of the entry and
840 of the VALU operator, none larger than 257 x 129; one test per kind."""
import ctypes

import numpy as np
import pytest

import imagestitch_amd as isa
import bf_i8_cases as K
import bf_i8_ref as R

pytestmark = pytest.mark.gpu
ENTRY = "bf_l2_knn2_u8d128"


def _same(got, want):
    return all(g.dtype == w.dtype and np.array_equal(g, w) for g, w in zip(got, want))


def _where(got, want):
    """the first differing query of the first differing array, for the failure message"""
    for name, g, w in zip(("i1", "d1", "d2"), got, want):
        bad = np.nonzero(~((g == w) | ((g != g) & (w != w))))[0]
        if len(bad):
            return "%s differs at %d of %d queries, first q=%d: got %r, want %r" % (name, len(bad), len(g), bad[0], g[bad[0]], w[bad[0]])
    return "dtype"


# ---- 1. every kind, every shape, every split count ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", K.KINDS)
def test_entry_equals_the_reference_and_the_valu_kernel(engine, kind):
    failed = []
    for nq, nt in K.SHAPES:
        q, t = K.case(kind, nq, nt)
        want = K.reference(kind, nq, nt)
        qf, tf = q.astype(np.float32), t.astype(np.float32)
        valu = engine.bf_l2_knn2(qf, tf)
        if not _same(valu, want):
            failed.append((kind, nq, nt, "valu", _where(valu, want)))
        for ns in K.NSPLITS:
            got = engine.bf_l2_knn2_u8d128(qf, tf, ns)
            if not _same(got, want):
                failed.append((kind, nq, nt, "nsplit %d" % ns, _where(got, want)))
    print("%s: %d of %d calls differ" % (kind, len(failed), len(K.SHAPES) * (len(K.NSPLITS) + 1)))
    for f in failed[:40]:
        print("  ", f)
    assert not failed, (len(failed), failed[:5])


# ---- 2. no state leaks from one call into the next ----------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before(engine):
    """pad rows and norms live in the arena, which the next call reuses: a large pad_bait call, then 1 x 1, then 17 x 17, then the first
    again, on one engine; each must equal what a fresh engine gives"""
    rng = np.random.default_rng(K.SEED)
    calls = [K.case("pad_bait", 257, 129), (rng.integers(0, 256, (1, 128)), rng.integers(0, 256, (1, 128))),
             K.case("pad_bait", 17, 17), K.case("pad_bait", 257, 129)]
    for ns in (0, 8):
        fresh = []
        for q, t in calls:
            eng = isa.Engine(0)
            try:
                fresh.append(eng.bf_l2_knn2_u8d128(q, t, ns))
            finally:
                eng.close()
        for n, (q, t) in enumerate(calls):
            got = engine.bf_l2_knn2_u8d128(q, t, ns)
            assert _same(got, fresh[n]), (ns, n, _where(got, fresh[n]))
            assert _same(got, R.knn2(np.asarray(q), np.asarray(t))), (ns, n)


# ---- 3. the entry is the fused batch's search -----------------------------------------------------------------------------------------
def test_entry_counts_the_matches_of_the_fused_batch(engine):
    """descriptors of two jobs of the fused batch's mixed set (two strip shapes) through the entry with the batch's own split rule: the
    reference, the VALU operator, and the ratio count equal to column 6 of the job's attempt row"""
    from test_sift_batch_gpu import _strips, mixed_set, run_set
    tiles, jobs = mixed_set()
    rows = run_set(engine, "mixed")
    for k in (0, 1):
        assert jobs[k][6:] != jobs[1 - k][6:]
        A, B = _strips(tiles, jobs[k])
        _ka, da = engine.sift_detect_describe(A); _kb, db = engine.sift_detect_describe(B)
        assert len(da) == rows[k][4] > 0 and len(db) == rows[k][5] > 0
        assert np.array_equal(da, np.rint(da)) and da.min() >= 0 and da.max() <= 255
        got = engine.bf_l2_knn2_u8d128(da, db, 0)
        want = R.knn2(da.astype(np.int64), db.astype(np.int64))
        assert _same(got, want), _where(got, want)
        valu = engine.bf_l2_knn2(da, db)
        assert _same(got, valu), _where(got, valu)
        _i1, d1, d2 = got
        count = int((d1.astype(np.float64) < d2.astype(np.float64) * 0.75).sum()) if len(db) >= 2 else 0
        print("job %d: %d x %d descriptors, %d ratio matches" % (k, len(da), len(db), count))
        assert count == rows[k][6]
    assert rows[0][4] > 100 and rows[0][6] > 0


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def _last_error(engine):
    buf = ctypes.create_string_buffer(512)
    engine.lib.vfsms_last_error(buf, 512)
    return buf.value.decode(errors="replace")


def test_bad_arguments_are_refused_by_name(engine):
    q, t = K.case("sift_like", 17, 33)
    qf, tf = q.astype(np.float32), t.astype(np.float32)
    want = K.reference("sift_like", 17, 33)
    bad_values = (0.5, -1.0, 256.0, np.nan, np.inf, 254.99998)
    for v in bad_values:
        for side in (0, 1):
            a, b = qf.copy(), tf.copy()
            (a, b)[side][-1, -1] = v
            with pytest.raises(isa.VfsmsError) as e:
                engine.bf_l2_knn2_u8d128(a, b, 1)
            assert "error %d:" % isa._lib.VFSMS_ERR_BAD_ARG in str(e.value) and ENTRY in str(e.value), (v, side, str(e.value))
    for ns in (-1, 9, 64):
        with pytest.raises(isa.VfsmsError) as e:
            engine.bf_l2_knn2_u8d128(qf, tf, ns)
        assert "error %d:" % isa._lib.VFSMS_ERR_BAD_ARG in str(e.value) and ENTRY in str(e.value), (ns, str(e.value))
    i1 = np.empty(17, np.int32); d1 = np.empty(17, np.float32); d2 = np.empty(17, np.float32)
    P = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    f = engine.lib.vfsms_bf_l2_knn2_u8d128
    for args in ((None, 17, P(tf), 33), (P(qf), 17, None, 33), (P(qf), -1, P(tf), 33), (P(qf), 17, P(tf), -1)):
        assert f(engine.ctx, *args, 0, P(i1), P(d1), P(d2)) == isa._lib.VFSMS_ERR_BAD_ARG, args[1::2]
        assert ENTRY in _last_error(engine)
    # empty sets are no error: nothing written without queries, (-1, inf, inf) without trains
    none = np.zeros((0, 128), np.float32)
    assert [len(a) for a in engine.bf_l2_knn2_u8d128(none, tf)] == [0, 0, 0]
    e1, e2, e3 = engine.bf_l2_knn2_u8d128(qf, none)
    assert (e1 == -1).all() and np.isinf(e2).all() and np.isinf(e3).all()
    assert f(engine.ctx, None, 0, None, 0, 0, None, None, None) == 0
    # a valid call afterwards succeeds
    for ns in K.NSPLITS:
        assert _same(engine.bf_l2_knn2_u8d128(qf, tf, ns), want)
