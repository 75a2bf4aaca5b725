"""CPU tests of the fused SIFT attempt batch's host layers: GridRegistrar(method="sift") against a sequential walk of the reference's
candidate order, the consensus estimator set around the batch and restored after it, the Stitcher's routing of featureMethod "sift"
to Engine.attempt_sift_batch, and the arithmetic claim behind the integer matcher (csrc/match_kernels.hip: k_bf_i8_d128)."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar
from scripted import ScriptedAttemptEngine, random_truth, serpentine_truth

SHAPE = (1000, 1400)
SIFT_PARAMS = ("sift-params", 3, 0.04, 10.0, 1.6)          # an opaque record: the registrar hands it through untouched


class ScriptedSiftEngine(ScriptedAttemptEngine):
    """answers attempt_sift_batch from the truth table and has no other fused entry point; records the arguments and the estimator
    setting of every call"""

    def __init__(self, *a, fail=False, **k):
        super().__init__(*a, **k)
        self.calls, self.estimator, self.seen, self.fail = [], ("mode", 3), [], fail

    def attempt_surf_batch(self, *a, **k):
        raise AssertionError("the SIFT registrar must not call the SURF batch")

    def set_offset_estimator(self, kind="mode", tol=3):
        self.estimator = (kind, tol)

    def attempt_sift_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        self.calls.append((len(jobs), params, ratio, offset_evaluate))
        self.seen.append(self.estimator)
        if self.fail:
            raise RuntimeError("batch failed")
        return ScriptedAttemptEngine.attempt_surf_batch(self, jobs, params, ratio, offset_evaluate)


def _rotate(d, incre):
    d += incre
    return 1 if d == 5 else 4 if d == 0 else d


def plain_walk(accept, roiRatio, incre, d0):
    """Stitcher.py:306-367 written out: for i in 1 .. maxI - 1, directions from the inherited one round to it again; the first accepted
    candidate gives the row and the direction the next pair inherits; the axis correction of Stitcher.py:352-360"""
    H, W = SHAPE
    maxI = int(np.floor(0.5 / roiRatio) + 1) + 1
    rows, d_in = [], d0
    for acc in accept:
        hit = None
        for i in range(1, maxI):
            d = d_in
            while True:
                if (d, i) in acc:
                    hit = (d, i)
                    break
                d = _rotate(d, incre)
                if d == d_in:
                    break
            if hit:
                break
        if not hit:
            rows.append([0, 0, 0, d_in])
            continue
        d, i = hit
        dx, dy = acc[hit]
        if d == 1:
            dx += H - int(i * roiRatio * H)
        elif d == 2:
            dy += W - int(i * roiRatio * W)
        elif d == 3:
            dx -= H - int(i * roiRatio * H)
        else:
            dy -= W - int(i * roiRatio * W)
        rows.append([1, dx, dy, d])
        d_in = d
    return rows, d_in


@pytest.mark.parametrize("seed", range(8))
def test_sift_registrar_equals_a_sequential_walk(seed):
    rng = np.random.default_rng(100 + seed)
    roiRatio = float(rng.choice([0.1, 0.2]))
    incre = int(rng.choice([-1, 1]))
    d0 = int(rng.integers(1, 5))
    P = int(rng.integers(1, 40))
    accept = random_truth(rng, P, roiRatio) if seed else serpentine_truth(6, 4, roiRatio)
    P = len(accept)
    want, d_end = plain_walk(accept, roiRatio, incre, d0)
    for window in (1, 16):
        eng = ScriptedSiftEngine(SHAPE, roiRatio, accept)
        reg = GridRegistrar(eng, method="sift", roiRatio=roiRatio, searchRatio=0.6, offsetEvaluate=7, directIncre=incre, window=window,
                            siftParams=SIFT_PARAMS)
        res, d = reg.register(list(range(P + 1)), [SHAPE] * (P + 1), d0)
        assert [list(r[:4]) for r in res.tolist()] == want, (seed, window)
        assert d == d_end
        assert eng.calls and all(c[1] is SIFT_PARAMS and c[2] == 0.6 and c[3] == 7 for c in eng.calls)
        assert sum(c[0] for c in eng.calls) == len(eng.log) == reg.stats["attempts"]
        assert set(eng.seen) == {("mode", 3)}


def test_sift_registrar_sets_the_consensus_around_the_batch_and_restores_mode():
    accept = serpentine_truth(4, 3, 0.2)
    P = len(accept)
    eng = ScriptedSiftEngine(SHAPE, 0.2, accept)
    reg = GridRegistrar(eng, method="sift", roiRatio=0.2, offsetCaculate="ransac", ransacThreshold=6)
    assert reg.offsetCaculate == "ransac"
    res, _d = reg.register(list(range(P + 1)), [SHAPE] * (P + 1), 1)
    assert [list(r[:4]) for r in res.tolist()] == plain_walk(accept, 0.2, 1, 1)[0]
    assert eng.seen and set(eng.seen) == {("ransac", 6)} and eng.estimator[0] == "mode"
    bad = ScriptedSiftEngine(SHAPE, 0.2, accept, fail=True)
    reg = GridRegistrar(bad, method="sift", roiRatio=0.2, offsetCaculate="ransac", ransacThreshold=6)
    with pytest.raises(RuntimeError):
        reg.register(list(range(P + 1)), [SHAPE] * (P + 1), 1)
    assert bad.seen == [("ransac", 6)] and bad.estimator[0] == "mode"


# ---- Stitcher ----------------------------------------------------------------------------------------------------------------------
class RoutingEngine:
    """an engine with tiles and the fused SIFT batch only; `row` is what every attempt answers"""

    def __init__(self, row):
        self.row, self.jobs, self.args, self.generic = row, [], [], []

    def tile_upload(self, img):
        return 41 + len(self.jobs)

    def tile_free(self, h):
        pass

    @staticmethod
    def sift_params(*a):
        return ("params",) + a

    def attempt_sift_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        self.jobs += [tuple(int(v) for v in j) for j in jobs]
        self.args.append((params, ratio, offset_evaluate))
        return np.tile(np.array(self.row, np.int32), (len(jobs), 1))

    # the generic per-pair operators
    def sift_detect_describe(self, img, params=None, cap=None, full=False):
        self.generic.append(np.asarray(img).shape)
        return np.zeros((0, 2), np.float32), np.zeros((0, 128), np.float32)


class NoBatchEngine(RoutingEngine):
    def __getattribute__(self, name):
        if name == "attempt_sift_batch":
            raise AttributeError(name)
        return super().__getattribute__(name)


def _stitcher(cls, eng):
    st = cls(); st._engine = eng
    st.isPrintLog = False; st.featureMethod = "sift"; st.roiRatio = 0.2; st.searchRatio = 0.7; st.offsetEvaluate = 4; st.direction = 1
    return st


def test_stitcher_routes_sift_to_the_fused_batch():
    A = np.zeros((100, 120), np.uint8); B = np.zeros((100, 120), np.uint8)
    eng = RoutingEngine([1, 7, 9, 5, 10, 10, 6, 0])
    st = _stitcher(isa.Stitcher, eng)
    assert st._usesStockOperators()
    assert st._batchedMethod(st.calculateOffsetForFeatureSearchIncre, 4) == "sift"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearch, 4) is None          # the whole-tile scan has no SIFT form
    ok, off = st.calculateOffsetForFeatureSearchIncre([A, B])
    assert ok and off == [7 + 100 - 20, 9]
    ra = isa.roi_rect(A.shape, 1, "first", 0.2); rb = isa.roi_rect(B.shape, 1, "second", 0.2)
    assert len(eng.jobs) == 1 and eng.jobs[0][2:] == (ra[0], ra[1], rb[0], rb[1], ra[2], ra[3])
    p, ratio, oe = eng.args[0]
    assert ratio == 0.7 and oe == 4 and p == st._siftParams()
    assert not eng.generic
    reg = st._makeRegistrar("sift", 4)
    assert reg.method == "sift" and reg.params == st._siftParams() and not reg.native
    st.isEnhance = True
    assert not st._usesStockOperators()                                              # SIFT with isEnhance stays on the generic path


def test_a_row_without_keypoints_is_no_features():
    A = np.zeros((100, 120), np.uint8)
    eng = RoutingEngine([1, 7, 9, 5, 0, 10, 0, 0])
    st = _stitcher(isa.Stitcher, eng)
    ok, _msg = st.calculateOffsetForFeatureSearchIncre([A, A])
    assert ok is False and st.direction == 1                                           # status 1 in the row, but featuresA is None
    assert len(eng.jobs) == 4 * (st._maxI() - 1)                                       # every candidate was tried, none counted


def test_sift_takes_the_generic_path_without_the_batch_or_with_user_operators():
    A = np.zeros((100, 120), np.uint8)
    eng = NoBatchEngine([1, 7, 9, 5, 10, 10, 6, 0])
    st = _stitcher(isa.Stitcher, eng)
    assert not st._usesStockOperators()
    assert st._batchedMethod(st.calculateOffsetForFeatureSearchIncre, 4) is None
    ok, _off = st.calculateOffsetForFeatureSearchIncre([A, A])
    assert not ok and eng.generic and not eng.jobs

    class OwnMatcher(isa.Stitcher):
        def matchDescriptors(self, featuresA, featuresB):
            return []
    eng = RoutingEngine([1, 7, 9, 5, 10, 10, 6, 0])
    st = _stitcher(OwnMatcher, eng)
    assert not st._usesStockOperators()
    ok, _off = st.calculateOffsetForFeatureSearchIncre([A, A])
    assert not ok and eng.generic and not eng.jobs


def test_a_wrapper_with_its_own_detector_takes_the_generic_path():
    """an engine wrapper that hands attempt_sift_batch through but detects with its own sift_detect_describe (tests/test_sift_host.py's
    SpecEngine does) is served by its detector, not by the wrapped engine's fused batch"""
    class OwnDetector:
        def __init__(self, base):
            self.base, self.own = base, []

        def __getattr__(self, name):
            return getattr(self.base, name)

        def sift_detect_describe(self, img, params=None, cap=None, full=False):
            self.own.append(np.asarray(img).shape)
            return np.zeros((0, 2), np.float32), np.zeros((0, 128), np.float32)

    A = np.zeros((100, 120), np.uint8)
    base = RoutingEngine([1, 7, 9, 5, 10, 10, 6, 0])
    eng = OwnDetector(base)
    st = _stitcher(isa.Stitcher, eng)
    assert hasattr(eng, "attempt_sift_batch") and not st._usesStockOperators()
    ok, _off = st.calculateOffsetForFeatureSearchIncre([A, A])
    assert not ok and eng.own and not base.jobs and not base.generic


# ---- the claim behind the integer matcher ----------------------------------------------------------------------------------------
def _u8_vectors():
    rng = np.random.default_rng(17)
    alt = np.tile([0, 255], 64)
    fixed = [np.zeros(128), np.full(128, 255), alt, 255 - alt, np.full(128, 128), np.full(128, 127)]
    rnd = list(rng.integers(0, 256, (40, 128)))
    sparse = [np.where(rng.random(128) < 0.1, 255, 0) for _ in range(6)]
    return np.array(fixed + rnd + sparse, dtype=np.int64)


def _gen_order_f32(q, t):
    """k_bf_l2_gen<128>: acc += (e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3) over d = 0, 4, ..., every operation rounded to float32"""
    f = np.float32
    acc = f(0)
    for d in range(0, 128, 4):
        e = [f(f(q[d + k]) - f(t[d + k])) for k in range(4)]
        s = f(f(f(e[0] * e[0]) + f(e[1] * e[1])) + f(e[2] * e[2]))
        s = f(s + f(e[3] * e[3]))
        acc = f(acc + s)
    return acc


def test_integer_distances_are_exact_in_float32_and_in_shifted_int32():
    V = _u8_vectors()
    worst = 0
    for q in V:
        for t in V:
            want = int(((q - t) ** 2).sum())                                        # int64
            worst = max(worst, want)
            got = _gen_order_f32(q, t)
            assert got.dtype == np.float32 and float(got) == want and int(got) == want, (q[:4], t[:4])
            qs, ts = (q - 128).astype(np.int8), (t - 128).astype(np.int8)           # what k_pack_i8_d128 stores
            dot = np.int32(0)
            for k in range(128):                                                     # int32 accumulation, as the matrix core's
                dot = np.int32(dot + np.int32(qs[k]) * np.int32(ts[k]))
            nq = np.int32((qs.astype(np.int32) ** 2).sum()); nt = np.int32((ts.astype(np.int32) ** 2).sum())
            assert int(np.int32(np.int32(nt - np.int32(2) * dot) + nq)) == want
            assert abs(int(dot)) <= 1 << 21 and int(nq) <= 1 << 21
    assert worst == 128 * 255 * 255 < 1 << 24
    # every integer below 2^24 is a float32, and sqrtf of it is what the VALU kernel takes the root of
    for v in (0, 1, worst, worst - 1, (1 << 24) - 1):
        assert int(np.float32(v)) == v
