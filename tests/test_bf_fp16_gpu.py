"""GPU tests (-m gpu) of the fp16 candidate filter of the 64-d 2-NN search (csrc/match_kernels.hip: k_bf_split16, k_bf_mfma16_d64<0/1>,
k_bf_verify_d64) through the engine's entry point vfsms_bf_l2_knn2: at train and query counts on the edges of the 32-train tile and
the 64-query wave, on descriptor sets built against the filter (exact duplicates, near-ties far inside the fp16 error, elements in
fp16's subnormal range, norms of exactly 1, all-zero rows), (i1, d1, d2) must equal the exhaustive exact kernel's, bit for bit.  That
kernel is selected by VFSMS_BF_EXACT=1, which is read once per process: the reference runs in ONE child process over the same seeded
cases.  A fused batch of two production strip pairs must give the rows of the pairs alone."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                  # run as a child process: python tests/test_bf_fp16_gpu.py out.npz
    sys.path.insert(0, ROOT)

import imagestitch_amd as isa                             # noqa: E402
from imagestitch_amd.synthetic import SyntheticGrid       # noqa: E402

pytestmark = pytest.mark.gpu
NT = (1, 2, 31, 32, 33, 64, 65)
NQ = (1, 63, 64, 65, 129)
KINDS = ("duplicates", "near_ties", "subnormal", "norm_one", "zero_row")


def _unit(a):
    a = np.asarray(a, np.float64)
    n = np.linalg.norm(a, axis=1, keepdims=True); n[n == 0] = 1
    return (a / n).astype(np.float32)


def _case(kind, nq, nt):
    """seeded (q, t): float32 rows of norm <= 1 (the filtered search), the same in the parent and the child"""
    rng = np.random.default_rng(1000 * KINDS.index(kind) + 10 * nq + nt)
    if kind == "duplicates":                              # every train row occurs twice or more: ties keep the lower index
        base = _unit(rng.normal(size=(max(1, (nt + 2) // 3), 64)))
        t = base[rng.integers(0, len(base), nt)]
        q = t[rng.integers(0, nt, nq)].copy()             # distance 0 to several trains
        q[::3] = _unit(rng.normal(size=(len(q[::3]), 64)))
    elif kind == "near_ties":                             # trains 1e-4 around one centre: squared distances differ by ~1e-7, the fp16 error is
        c = rng.normal(size=(1, 64))                      # 2e-3 and BFM_MARGIN 1e-3 -- every train is a candidate (lists of 64 trains overflow)
        t = _unit(c + 1e-4 * rng.normal(size=(nt, 64)))
        q = _unit(c + 1e-4 * rng.normal(size=(nq, 64)))
        q[::5] = _unit(rng.normal(size=(len(q[::5]), 64)))
    elif kind == "subnormal":                             # a few large elements, the rest below 6.1e-5 (fp16 subnormals) or zero
        def rows(n):
            a = rng.uniform(-6.0e-5, 6.0e-5, size=(n, 64)); a[:, ::3] = 0
            big = rng.normal(size=(n, 4)); big /= np.linalg.norm(big, axis=1, keepdims=True)
            c0 = rng.integers(0, 16, n) * 4
            for k in range(n):
                a[k, c0[k]:c0[k] + 4] = big[k] * 0.9999
            return a.astype(np.float32)
        q, t = rows(nq), rows(nt)
    elif kind == "norm_one":                              # norm exactly 1: all magnitudes 1/8, or a single element at +-1
        q = (0.125 * rng.choice([-1.0, 1.0], size=(nq, 64))).astype(np.float32)
        t = (0.125 * rng.choice([-1.0, 1.0], size=(nt, 64))).astype(np.float32)
        t[::4] = 0; t[np.arange(0, nt, 4), rng.integers(0, 64, len(t[::4]))] = 1.0
        q[::7] = 0; q[np.arange(0, nq, 7), rng.integers(0, 64, len(q[::7]))] = -1.0
    else:                                                 # one all-zero train and one all-zero query among unit rows
        q, t = _unit(rng.normal(size=(nq, 64))), _unit(rng.normal(size=(nt, 64)))
        t[nt // 2] = 0; q[nq // 2] = 0
    return np.ascontiguousarray(q, np.float32), np.ascontiguousarray(t, np.float32)


def _all_cases():
    return [(kind, nq, nt) for kind in KINDS for nq in NQ for nt in NT]


def _run_all(engine):
    out = {}
    for kind, nq, nt in _all_cases():
        i1, d1, d2 = engine.bf_l2_knn2(*_case(kind, nq, nt))
        out["%s_%d_%d_i1" % (kind, nq, nt)] = i1; out["%s_%d_%d_d1" % (kind, nq, nt)] = d1; out["%s_%d_%d_d2" % (kind, nq, nt)] = d2
    return out


@pytest.fixture(scope="module")
def exact_results(tmp_path_factory):
    """(i1, d1, d2) of every case from the exhaustive kernel: a fresh child process with VFSMS_BF_EXACT=1"""
    path = str(tmp_path_factory.mktemp("bf_fp16") / "exact.npz")
    p = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, VFSMS_BF_EXACT="1"), capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return dict(np.load(path))


@pytest.fixture(scope="module")
def filtered_results(engine):
    return _run_all(engine)


@pytest.mark.parametrize("kind", KINDS)
def test_filtered_equals_exhaustive(filtered_results, exact_results, kind):
    assert sorted(filtered_results) == sorted(exact_results)
    for k, nq, nt in _all_cases():
        if k != kind:
            continue
        for f in ("i1", "d1", "d2"):
            key = "%s_%d_%d_%s" % (kind, nq, nt, f)
            assert np.array_equal(filtered_results[key], exact_results[key]), key
        assert len(filtered_results["%s_%d_%d_i1" % (kind, nq, nt)]) == nq


def test_two_cases_against_the_oracle(engine, oracle):
    for kind, nq, nt in (("near_ties", 129, 65), ("duplicates", 65, 33)):
        q, t = _case(kind, nq, nt)
        i1, d1, d2 = engine.bf_l2_knn2(q, t)
        oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
        assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2), (kind, nq, nt)
        assert np.array_equal(engine.bf_l2_ratio_matches(q, t, 0.75), oracle.bf_l2_ratio_matches(q, t, 0.75)), (kind, nq, nt)


def test_fused_batch_of_two_production_strip_pairs(engine):
    """two pairs of 409 x 2048 ROI strips (the bench grid's tiles 0-1 and 1-2) in one vfsms_attempt_surf_batch against each pair alone"""
    tiles = SyntheticGrid(10, 9, 2048).tiles(range(3))
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        ra = isa.roi_rect(tiles[0].shape, 1, "first", 0.2); rb = isa.roi_rect(tiles[0].shape, 1, "second", 0.2)
        jobs = [(hs[k], hs[k + 1], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]) for k in range(2)]
        rows = engine.attempt_surf_batch(jobs).tolist()
        alone = [engine.attempt_surf_batch([j])[0].tolist() for j in jobs]
        assert rows == alone
        assert all(r[0] == 1 and r[4] > 4000 and r[5] > 4000 and r[6] > 100 for r in rows), rows
    finally:
        for h in hs:
            engine.tile_free(h)


if __name__ == "__main__":
    eng = isa.Engine(0)
    np.savez(sys.argv[1], **_run_all(eng))
    eng.close()
