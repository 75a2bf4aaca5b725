"""GPU tests of offsetVerify = "ncc" (csrc/verify_kernels.hip): vfsms_verify_ncc and the verifier behind the vote tail of the fused
batches equal tests/verify_ref.py bit for bit; the registrars with the verifier on take every decision of the oracle's chain with
verify_ref in its acceptance."""
import json
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar
from imagestitch_amd.synthetic import SyntheticGrid
import verify_ref as V

pytestmark = pytest.mark.gpu

THR, MINPX = isa.Method.verifyThreshold, isa.Method.verifyMinPixels


def _expect(a, b, dx, dy, min_pixels):
    s = V.sums(a, b, dx, dy)
    sc = V.score(s, min_pixels)
    return s, sc, V.fixed(sc)


def _same(got, exp):
    """six sums equal, score equal as BITS, fixed-point equal"""
    return got[0] == exp[0] and np.float64(got[1]).tobytes() == np.float64(exp[1]).tobytes() and got[2] == exp[2]


# ---- the per-operator entry ----------------------------------------------------------------------------------------------------------
def test_verify_ncc_equals_the_specification(engine):
    rng = np.random.default_rng(11)
    cases = []
    for h, w in ((1, 1), (3, 5), (17, 33), (31, 47), (64, 64), (129, 255), (200, 1001)):
        A = rng.integers(0, 256, (h, w), dtype=np.uint8)
        B = (A.astype(np.int32) // 2 + rng.integers(0, 128, (h, w))).astype(np.uint8)
        for dx, dy in ((0, 0), (1, 0), (-1, 0), (0, 1), (0, -1), (h // 2, -(w // 3)), (-(h // 3), w // 2), (h - 1, w - 1), (1 - h, 1 - w), (h, 0), (0, -w), (3, 17), (-5, -15), (2, 16)):
            cases.append((A, B, dx, dy, 0))
    big = rng.integers(0, 256, (300, 700), dtype=np.uint8)
    cases.append((big[3:290:2, 5:650], big[7:294:2, 9:654], 4, -3, 0))                       # strided views (rows 2 apart)
    cases.append((big[::3, 1::2], big[1::3, ::2], -2, 5, 0))                                  # columns 2 apart: made contiguous by the binding
    flat = np.full((40, 50), 9, np.uint8)
    cases += [(flat, big[:40, :50], 2, 3, 0), (big[:40, :50], flat, 0, 0, 0), (big[:40, :50], big[:40, :50], 10, 10, 1201), (big[:40, :50], big[:40, :50], 10, 10, 1200)]
    for A, B, dx, dy, mp in cases:
        got = engine.verify_ncc(A, B, dx, dy, mp)
        assert _same(got, _expect(A, B, dx, dy, mp)), (A.shape, dx, dy, mp, got, _expect(A, B, dx, dy, mp))
    with pytest.raises(isa.VfsmsError):
        engine.verify_ncc(big, big, 0, 0, -1)


def test_verify_ncc_at_production_sizes(engine):
    rng = np.random.default_rng(12)
    for (h, w), votes in (((409, 2048), ((-201, 3), (188, -2), (0, 0), (-370, 1000))), ((819, 4096), ((-402, 7), (5, -4090)))):
        scene = rng.integers(0, 256, (2 * h, w + 64), dtype=np.uint8)
        A = scene[:h, :w]; B = scene[201:201 + h, 3:3 + w]                                   # B(r, c) = A(r + 201, c + 3) where both exist
        for dx, dy in votes + ((201, 3),):
            got = engine.verify_ncc(A, B, dx, dy, MINPX)
            assert _same(got, _expect(A, B, dx, dy, MINPX)), (h, w, dx, dy)
        assert engine.verify_ncc(A, B, 201, 3, MINPX)[1] > 1 - 1e-12
    # a whole 4096 x 4096 tile at offset (0, 0): Sab ~ 2^40, N * Sab would not fit int64
    T = rng.integers(0, 256, (4096, 4096), dtype=np.uint8)
    U = np.maximum(T, 200)
    got = engine.verify_ncc(T, U, 0, 0, MINPX)
    assert _same(got, _expect(T, U, 0, 0, MINPX)) and got[0][0] == 1 << 24
    W = np.full((4096, 4096), 255, np.uint8)
    got = engine.verify_ncc(W, W, 0, 0, 0)
    assert got[0] == (1 << 24, 255 << 24, 255 << 24, 65025 << 24, 65025 << 24, 65025 << 24) and got[1] == 0.0


def test_set_offset_verifier_arguments(engine):
    for bad in (("ncc", 1.5, 0), ("ncc", -1.01, 0), ("ncc", float("nan"), 0), ("ncc", 0.5, -1), (2, 0.5, 0), (-1, 0.0, 0)):
        with pytest.raises(isa.VfsmsError):
            engine.set_offset_verifier(*bad)
    engine.set_offset_verifier("ncc", 0.5, 100)
    engine.set_offset_verifier("none")


# ---- the fused batches ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def grid_tiles():
    g = SyntheticGrid(2, 2, 640)
    return g.tiles(threads=1) + [np.full((640, 640), 31, np.uint8)]                           # the last tile is flat: no keypoints


def _jobs(tiles, handles):
    out = []
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3), (0, 4), (4, 1)):
        for d in (1, 2, 3, 4):
            for i in (1, 2):
                ra = isa.roi_rect(tiles[a].shape, d, "first", 0.2 * i)
                rb = isa.roi_rect(tiles[b].shape, d, "second", 0.2 * i)
                out.append(((handles[a], handles[b], ra[0], ra[1], rb[0], rb[1], ra[2], ra[3]),
                            tiles[a][ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]], tiles[b][rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]]))
    return out


def _verified(engine, fn, thr, minpx):
    engine.set_offset_verifier("ncc", thr, minpx)
    try:
        return fn()
    finally:
        engine.set_offset_verifier("none")


def test_fused_batches_with_the_verifier_equal_the_specification(engine, grid_tiles):
    """SURF, enhanced SURF, ORB and SIFT batches under both estimators: a row with the verifier on is the row without it (which the
    parity suites hold equal to the oracle's attempt row) behind verify_ref.verify_row on the RAW strips -- status, int 7, everything
    else untouched.  Every batch mixes accepted, rejected and no-keypoint jobs."""
    tiles = grid_tiles
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        jobs = _jobs(tiles, hs)
        J = [j for j, _a, _b in jobs]
        batches = {"surf": lambda: engine.attempt_surf_batch(J), "enhanced": lambda: engine.attempt_surf_batch_enhanced(J, None, 0.75, 3, (2, 20.0, 5)),
                   "orb": lambda: engine.attempt_orb_batch(J), "sift": lambda: engine.attempt_sift_batch(J)}
        for est in (("mode", 3), ("ransac", 3)):
            engine.set_offset_estimator(*est)
            try:
                for name, fn in batches.items():
                    off = fn()
                    assert not off[:, 7].any()
                    on = _verified(engine, fn, THR, MINPX)
                    exp = np.array([V.verify_row(r, a, b, THR, MINPX) for r, (_j, a, b) in zip(off, jobs)], np.int32)
                    assert np.array_equal(on, exp), (name, est, np.nonzero((on != exp).any(1))[0], on[(on != exp).any(1)], exp[(on != exp).any(1)])
                    kept, rejected, empty = int(on[:, 0].sum()), int((off[:, 0] == 1).sum() - on[:, 0].sum()), int(((off[:, 4] == 0) | (off[:, 5] == 0)).sum())
                    print(name, est, "accepted", kept, "rejected", rejected, "no keypoints", empty)
                    assert kept >= 1 and empty >= 1, (name, kept, rejected, empty)       # "mixed": at least one job of each kind
                    if name == "orb":
                        assert rejected >= 1, (name, est)                     # three equal random votes: what the check is for
                    assert np.array_equal(fn(), off)                          # and off again: rows byte-equal to before
                    # a threshold nothing reaches rejects every accepted row and keeps its offset and counts
                    none = _verified(engine, fn, 1.0, MINPX)
                    hard = np.array([V.verify_row(r, a, b, 1.0, MINPX) for r, (_j, a, b) in zip(off, jobs)], np.int32)
                    assert np.array_equal(none, hard) and np.array_equal(none[:, 1:7], off[:, 1:7])
            finally:
                engine.set_offset_estimator("mode")
    finally:
        for h in hs:
            engine.tile_free(h)


def test_feature_sets_refuse_the_verifier(engine, grid_tiles):
    tiles = grid_tiles
    hs = [engine.tile_upload(t) for t in tiles[:2]]
    feats, _counts = engine.features_surf_batch(hs, None, (0, 0.0, 0))
    try:
        row = engine.features_match_offset(feats[0], feats[1], 0.75, 3)
        engine.set_offset_verifier("ncc", THR, MINPX)
        for call in (lambda: engine.features_match_offset(feats[0], feats[1], 0.75, 3), lambda: engine.features_match_offset_batch(feats[:1], feats[1:], 0.75, 3)):
            with pytest.raises(isa.VfsmsError, match="-6"):
                call()
        engine.set_offset_verifier("none")
        assert np.array_equal(engine.features_match_offset(feats[0], feats[1], 0.75, 3), row)
    finally:
        engine.set_offset_verifier("none")
        for f in feats:
            engine.features_free(f)
        for h in hs:
            engine.tile_free(h)


# ---- the registrars --------------------------------------------------------------------------------------------------------------------
def verified_orb_attempt(oracle, A, B, thr=THR, minpx=MINPX, roiRatio=0.2):
    """the oracle's ORB attempt with verify_ref in its acceptance: the reference chain of the tests below"""
    from test_oracle_golden import oracle_orb_attempt
    raw = oracle_orb_attempt(oracle, A, B, roiRatio)

    def attempt(d, i):
        st, off, votes = raw(d, i)
        if st:
            ra = isa.roi_rect(A.shape, d, "first", i * roiRatio); rb = isa.roi_rect(B.shape, d, "second", i * roiRatio)
            st = V.verify(A[ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]], B[rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]], int(off[0]), int(off[1]), thr, minpx)[0]
        return st, off, votes
    return attempt


def _reference_chain(oracle, tiles, memo=None):
    from test_oracle_golden import _chain_search
    direction, exp = 1, []
    for k in range(len(tiles) - 1):
        raw = verified_orb_attempt(oracle, tiles[k], tiles[k + 1])

        def attempt(d, i, k=k, raw=raw):
            if memo is None:
                return raw(d, i)
            if (k, d, i) not in memo:
                memo[(k, d, i)] = raw(d, i)
            return memo[(k, d, i)]
        st, off, d, i, log = _chain_search(attempt, tiles[k].shape, tiles[k + 1].shape, direction)
        exp.append([int(st), off[0], off[1], d if st else direction, i, log[-1][5] if st else 0])
        if st:
            direction = d
    return exp


def _compare(table, exp):
    got = [[int(v) for v in row[:6]] for row in table]
    assert len(got) == len(exp)
    for k, (a, b) in enumerate(zip(got, exp)):
        if b[0]:
            assert a == b, (k, a, b)
        else:
            assert a[0] == 0, (k, a, b)


def _off_truth(rows, truth):
    return [k for k, r in enumerate(rows) if not (r[0] and [r[1], r[2]] == [int(truth[k][0]), int(truth[k][1])])]


def test_orb_grid_3x3_with_the_verifier_equals_the_reference_chain(engine, oracle):
    """configs[2]'s geometry (2048^2 tiles, 10 % overlap, ORB at offsetEvaluate 3) on a 3 x 3 serpentine, verifier on: the native registrar
    (vfsms_pairs_offsets) AND GridRegistrar.chain take every decision of the oracle chain with verify_ref in its acceptance"""
    g = SyntheticGrid(3, 3, 2048, overlap=0.10)
    tiles = g.tiles(threads=4)
    exp = _reference_chain(oracle, tiles)
    hs = [engine.tile_upload(t) for t in tiles]
    try:
        for native in (True, False):
            reg = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1, offsetVerify="ncc", verifyThreshold=THR, verifyMinPixels=MINPX)
            reg.native = native
            table, _d = reg.register(hs, [t.shape for t in tiles], 1)
            _compare(table, exp)
        off = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1)
        plain, _d = off.register(hs, [t.shape for t in tiles], 1)
    finally:
        for h in hs:
            engine.tile_free(h)
    truth = g.true_offsets()
    print("3 x 3 ORB grid: pairs off truth %s with the verifier, %s without" % (_off_truth(exp, truth), _off_truth([[int(v) for v in r[:6]] for r in plain], truth)))
    assert _off_truth([[int(v) for v in r[:6]] for r in table], truth) == _off_truth(exp, truth)


@pytest.mark.timeout(1200)
def test_config2_full_orb_grid_with_the_verifier_equals_the_reference_chain(engine, oracle):
    """The synthetic 10 x 9 grid of 2048^2 tiles (89 pairs), ORB at the reference's offsetEvaluate = 3, verifier on at the default
    threshold: the table equals the oracle chain with verify_ref in its acceptance, and so does the count of pairs off the synthetic
    truth, which is printed (18 without the verifier).  Measured: the reference chain leaves 2, pairs 6 and 63 -- no false accepts but
    votes of 416 and 398 for an offset one pixel from the synthetic truth (NCC 0.962 / 0.963), counted because ORB is asked for the exact
    truth; every wrong-direction 3-vote candidate scores below 0.05 under verify_ref and is rejected."""
    from concurrent.futures import ThreadPoolExecutor
    from test_oracle_golden import pool_size
    g = SyntheticGrid(10, 9, 2048, overlap=0.10)
    tiles = g.tiles(threads=8)
    P = len(tiles) - 1
    hs = [engine.tile_upload(t) for t in tiles]
    reg = GridRegistrar(engine, method="orb", roiRatio=0.2, offsetEvaluate=3, directIncre=1, surfParams=engine.orb_params(),
                        offsetVerify="ncc", verifyThreshold=THR, verifyMinPixels=MINPX)
    table, _d = reg.register(hs, [t.shape for t in tiles], 1)
    for h in hs:
        engine.tile_free(h)
    memo = {}
    jobs = [(k, d, 1) for k in range(P) for d in (1, 2, 3, 4)]              # every pair's first ring ahead, in parallel; the walk decides alone
    with ThreadPoolExecutor(max_workers=pool_size()) as ex:
        for key, r in zip(jobs, ex.map(lambda kd: verified_orb_attempt(oracle, tiles[kd[0]], tiles[kd[0] + 1])(kd[1], kd[2]), jobs)):
            memo[key] = r
    exp = _reference_chain(oracle, tiles, memo)
    _compare(table, exp)
    truth = g.true_offsets()
    ref_off, got_off = _off_truth(exp, truth), _off_truth([[int(v) for v in r[:6]] for r in table], truth)
    print("configs[2] with the verifier: %d of %d pairs off truth in the reference chain %s; attempts %d" % (len(ref_off), P, ref_off, reg.stats["attempts"]))
    assert got_off == ref_off


def test_real_dendritic_pairs_with_the_verifier(engine, golden_dir):
    """the 25 real pairs (frames rebuilt around the committed strips), SURF and ORB, verifier on.  SURF rows are unchanged.  ORB's rows
    follow the reference chain: on these frames -- zero outside the 640-px crops, so most shared pixels are 0 on both sides -- verify_ref
    scores every stored accept above 0.9, the three thin-overlap 3-4-vote rows (tiles 14, 61, 74) included, so the chain is the stored
    one; on the crops' own pixels those three score 0.004 .. 0.022 (tests/test_verify_host.py)."""
    from test_oracle_golden import _rebuild_frames
    from test_verify_host import _raw
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    n = 0
    for nb in meta:
        frames = _rebuild_frames(nb, g)
        hs = [engine.tile_upload(f) for f in frames]
        try:
            for method, key in (("surf", "expected"), ("orb", "expected_orb")):
                for k, e in enumerate(nb[key]):                      # the reference: the stored accept passes verify_ref, the failed candidates before it stay failed
                    ra = isa.roi_rect(frames[k].shape, e["direction"], "first", 0.2 * e["i"]); rb = isa.roi_rect(frames[k + 1].shape, e["direction"], "second", 0.2 * e["i"])
                    r = _raw(e["offset"], e["direction"], e["i"], frames[k].shape)
                    ok, sc, _fx, _s = V.verify(frames[k][ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]], frames[k + 1][rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]], r[0], r[1], THR, MINPX)
                    assert ok, (method, e["a"], sc)
                reg = GridRegistrar(engine, method=method, roiRatio=0.2, offsetEvaluate=3, directIncre=1, offsetVerify="ncc", verifyThreshold=THR, verifyMinPixels=MINPX)
                table, _d = reg.register(hs, [f.shape for f in frames], nb["incoming_direction"])
                for row, e in zip(table, nb[key]):
                    assert [int(v) for v in row[:6]] == [1] + e["offset"] + [e["direction"], e["i"], e["votes"]], (method, nb["turn"], e, row)
                    n += 1
        finally:
            for h in hs:
                engine.tile_free(h)
    assert n == 50
