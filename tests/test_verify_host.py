"""CPU tests of offsetVerify = "ncc": the specification tests/verify_ref.py against a per-pixel loop, the measurement behind the default
threshold as assertions on the committed real strips, and the host layers (Method.verifyOffset, Stitcher,
GridRegistrar) that route registration through Engine.verify_ncc and Engine.set_offset_verifier."""
import json
import math
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.grid import GridRegistrar
from imagestitch_amd.utility import roi_rect
import verify_ref as V
from fakes import OracleEngine
from test_oracle_golden import zirconcl_surf_rows

THRESHOLD, MIN_PIXELS = isa.Method.verifyThreshold, isa.Method.verifyMinPixels


# ---- the specification -------------------------------------------------------------------------------------------------------------
def brute(A, B, dx, dy):
    """every B pixel whose partner (r + dx, c + dy) lies inside A, one at a time"""
    h, w = A.shape
    N = Sa = Sb = Saa = Sbb = Sab = 0
    for r in range(h):
        for c in range(w):
            if 0 <= r + dx < h and 0 <= c + dy < w:
                a, b = int(A[r + dx, c + dy]), int(B[r, c])
                N += 1; Sa += a; Sb += b; Saa += a * a; Sbb += b * b; Sab += a * b
    return (N, Sa, Sb, Saa, Sbb, Sab)


def test_known_shift_pins_the_convention():
    """B is a window of a scene, A the window (dx, dy) further up-left: a feature of B at (r, c) sits at (r + dx, c + dy) of A, which is
    the vote int(yA - yB), int(xA - xB) of getOffsetByMode; only that sign scores 1 (up to the rounding of the float64 tail)"""
    rng = np.random.default_rng(1)
    scene = rng.integers(0, 256, (120, 140), dtype=np.uint8)
    for dx, dy in ((7, 0), (-7, 0), (0, 11), (0, -11), (5, -9), (-13, 4)):
        A = scene[40 - dx:40 - dx + 50, 40 - dy:40 - dy + 60]
        B = scene[40:90, 40:100]
        ok, sc, fx, s = V.verify(A, B, dx, dy, 0.99)
        assert ok and 1 - 1e-12 < sc <= 1.0 and fx == V.FIXED_ONE and s[0] == (50 - abs(dx)) * (60 - abs(dy)), (dx, dy, sc)
        assert s[1:] == brute(A, B, dx, dy)[1:]
        assert abs(V.score(V.sums(A, B, -dx, -dy))) < 0.2                       # the mirrored vote is noise


def test_sums_equal_a_per_pixel_loop():
    rng = np.random.default_rng(2)
    A = rng.integers(0, 256, (23, 31), dtype=np.uint8); B = rng.integers(0, 256, (23, 31), dtype=np.uint8)
    for dx, dy in ((0, 0), (3, 0), (-3, 0), (0, 5), (0, -5), (22, 30), (-22, -30), (22, -30), (4, -7), (-9, 2), (23, 0), (0, 31), (-40, 3), (100, 100)):
        s = V.sums(A, B, dx, dy)
        assert s == brute(A, B, dx, dy), (dx, dy)
        r0, r1, c0, c1 = V.overlap(23, 31, dx, dy)
        assert s[0] == max(0, r1 - r0) * max(0, c1 - c0)
    assert V.sums(A, B, 23, 0) == (0,) * 6 and V.verify(A, B, 23, 0, -1.0)[1:3] == (0.0, 0)        # empty overlap
    assert V.verify(A, B, 0, 31, 0.0)[0] is True                                                   # score 0 meets a threshold of 0, not above


def test_score_edge_cases():
    rng = np.random.default_rng(3)
    A = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    flat = np.full((16, 16), 77, np.uint8)
    assert V.score(V.sums(flat, A, 0, 0)) == 0.0 and V.score(V.sums(A, flat, 2, -1)) == 0.0       # a flat side: exactly zero variance
    assert V.score(V.sums(np.full((16, 16), 255, np.uint8), np.full((16, 16), 255, np.uint8), 0, 0)) == 0.0
    assert 1 - 1e-12 < V.score(V.sums(A, A, 0, 0)) <= 1.0 and -1.0 <= V.score(V.sums(A, 255 - A, 0, 0)) < -1 + 1e-12
    s = V.sums(A, A, 4, 4)
    assert s[0] == 144 and V.score(s, 144) != 0.0 and V.score(s, 145) == 0.0                         # N < min_pixels
    assert V.fixed(1.0) == 1 << 20 and V.fixed(-1.0) == -(1 << 20) and V.fixed(0.0) == 0 and V.fixed(0.25) == 1 << 18
    # the float64 tail against exact rational arithmetic
    from fractions import Fraction
    B = rng.integers(0, 256, (16, 16), dtype=np.uint8)
    N, Sa, Sb, Saa, Sbb, Sab = V.sums(A, B, 1, -2)
    num = Fraction(N * Sab - Sa * Sb); den2 = Fraction((N * Saa - Sa * Sa) * (N * Sbb - Sb * Sb))
    assert abs(V.score((N, Sa, Sb, Saa, Sbb, Sab)) - float(num) / math.sqrt(float(den2))) < 1e-12
    # a whole 4096 x 4096 tile of 255s and one darker pixel: the sums exceed what N * Sab holds in int64, the score does not care
    N = 4096 * 4096
    s = (N, 255 * N - 1, 255 * N - 1, 255 * 255 * N - 509, 255 * 255 * N - 509, 255 * 255 * N - 509)
    assert V.score(s) == pytest.approx(1.0, abs=1e-6)
    assert V.verify_row([0, 5, 5, 2, 9, 9, 4, 0], A, A, 0.5) == [0, 5, 5, 2, 9, 9, 4, 0]
    assert V.verify_row([1, 0, 0, 9, 9, 9, 9, 0], A, A, 0.5) == [1, 0, 0, 9, 9, 9, 9, 1 << 20]
    assert V.verify_row([1, 0, 0, 9, 9, 9, 9, 0], A, 255 - A, 0.5) == [0, 0, 0, 9, 9, 9, 9, -(1 << 20)]


# ---- the measurement behind the default threshold ------------------------------------------------------------------------------------
def _raw(off, d, i, shape, rr=0.2):
    """a full-tile offset back to the raw vote of its (direction, i) strips (the inverse of Stitcher.py:352-360)"""
    H, W = shape; off = list(off)
    if d == 1: off[0] -= H - int(i * rr * H)
    elif d == 2: off[1] -= W - int(i * rr * W)
    elif d == 3: off[0] += H - int(i * rr * H)
    else: off[1] += W - int(i * rr * W)
    return off


def dendritic_crop_pairs(golden_dir, which):
    """the committed PIXELS (640-px crops; the frames the parity tests rebuild around them are zero elsewhere) of the (direction, i) strips
    of the 25 neighbourhood pairs, with the raw vote behind the stored row `which` ("expected": SURF, "expected_orb")
    -> [(tile, within one px of Stitcher.py:87, cropA, cropB, [dx, dy], votes)]"""
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    out = []
    for nb in meta:
        def crop(tile, rect):
            for s in nb["strips"]:
                a = g[s["key"]]
                if s["tile"] == tile and s["y0"] >= rect[0] and s["x0"] >= rect[1] and s["y0"] + a.shape[0] <= rect[0] + rect[2] \
                        and s["x0"] + a.shape[1] <= rect[1] + rect[3]:
                    return a, (s["y0"] - rect[0], s["x0"] - rect[1])
            raise KeyError((tile, rect))
        for k, e in enumerate(nb[which]):
            a, oa = crop(nb["tiles"][k], roi_rect(nb["shape"], e["direction"], "first", e["i"] * 0.2))
            b, ob = crop(nb["tiles"][k + 1], roi_rect(nb["shape"], e["direction"], "second", e["i"] * 0.2))
            assert a.shape == b.shape and oa == ob                             # both crops sit at one place of their strips
            within = abs(e["offset"][0] - e["gold"][0]) <= 1 and abs(e["offset"][1] - e["gold"][1]) <= 1
            out.append((e["a"], within, a, b, _raw(e["offset"], e["direction"], e["i"], nb["shape"]), e["votes"]))
    return out


def test_default_threshold_separates_true_from_false_accepts(oracle, golden_dir):
    """on committed real pixels every offset the oracle chain places within 1 px of the truth scores above the
    default threshold with at least verifyMinPixels shared pixels, every listed false accept below it.  Measured ranges: true accepts
    0.844 .. 0.995 (lowest: dendritic tile 29, SURF), false accepts -0.105 .. 0.026."""
    true, false = [], []
    surf = dendritic_crop_pairs(golden_dir, "expected")
    assert len(surf) == 25 and all(w for _t, w, *_ in surf)
    for t, _w, a, b, r, _v in surf:
        true.append(("dendritic surf %d" % t,) + V.verify(a, b, r[0], r[1], THRESHOLD, MIN_PIXELS)[:2] + (V.sums(a, b, *r)[0],))
    orb = dendritic_crop_pairs(golden_dir, "expected_orb")
    assert [t for t, w, *_ in orb if not w] == [14, 61, 74]
    for t, w, a, b, r, v in orb:
        (true if w else false).append(("dendritic orb %d" % t,) + V.verify(a, b, r[0], r[1], THRESHOLD, MIN_PIXELS)[:2] + (V.sums(a, b, *r)[0],))
    # the thinnest true overlap of the vectors: 39 rows (tile 74, raw dx -348 in a 387-row strip)
    thin = [x for x in surf if x[0] == 74][0]
    assert thin[4][0] == -348 and V.sums(thin[2], thin[3], *thin[4])[0] == 39 * 639 >= MIN_PIXELS
    # zirconCL: the 23 SURF rows; ORB's rows, of which pairs 8 and 20 are 3-vote false accepts
    z = np.load(os.path.join(golden_dir, "zirconcl_strips.npz"))
    for k, (A, B, r) in enumerate(zirconcl_surf_rows(oracle, golden_dir)):
        assert r[0] == 1
        true.append(("zirconCL surf %d" % k,) + V.verify(A, B, r[1], r[2], THRESHOLD, MIN_PIXELS)[:2] + (V.sums(A, B, r[1], r[2])[0],))
    rejected = []
    for k in range(23):
        A, B = z["t%d_first" % k], z["t%d_second" % (k + 1)]
        ka, da = oracle.orb_detect_describe(A); kb, db = oracle.orb_detect_describe(B)
        pairs, _ = oracle.bf_hamming_matches(da, db)
        st, off, votes = oracle.mode_offset(np.stack([ka["x"], ka["y"]], 1), np.stack([kb["x"], kb["y"]], 1), pairs, 3)
        row = V.verify_row([int(st), off[0], off[1], votes, len(ka), len(kb), len(pairs), 0], A, B, THRESHOLD, MIN_PIXELS)
        if not row[0]:
            rejected.append(k)
        (false if votes == 3 else true).append(("zirconCL orb %d" % k,) + V.verify(A, B, off[0], off[1], THRESHOLD, MIN_PIXELS)[:2] + (V.sums(A, B, *off)[0],))
    assert rejected == [8, 20]                                 # the oracle's ORB chain + verify_ref: exactly the two false accepts go
    # the two full-width dendritic strips and configs[0]'s iron pair, at the oracle's SURF vote
    mf = json.load(open(os.path.join(golden_dir, "real_full_strips.json")))["pairs"]
    zf = np.load(os.path.join(golden_dir, "real_full_strips.npz"))
    assert len(mf) == 2
    for m in mf:
        A, B = zf["p%d_a" % m["a"]], zf["p%d_b" % m["a"]]
        r = m["expected_surf"]
        assert r[0] == 1 and abs(r[1] + m["tile_shape"][0] - m["roi_first"][2] - m["gold"][0]) <= 1
        true.append(("dendritic full %d" % m["a"],) + V.verify(A, B, r[1], r[2], THRESHOLD, MIN_PIXELS)[:2] + (V.sums(A, B, r[1], r[2])[0],))
    iron = np.load(os.path.join(golden_dir, "demo_strips.npz"))
    true.append(("iron",) + V.verify(iron["d0_roiA"], iron["d0_roiB"], 150, 0, THRESHOLD, MIN_PIXELS)[:2] + (612408,))
    # the first-tried wrong direction at the five turns: the committed frames hold no pixels there (the oracle finds no keypoint, votes
    # nothing); whatever a detector voted on such a strip, a flat side scores 0
    for name, ok, sc, n in sorted(true, key=lambda x: x[2])[:3] + sorted(false, key=lambda x: -x[2])[:3]:
        print("%-22s accepted %d score %.4f N %d" % (name, ok, sc, n))
    assert len(true) == 25 + 22 + 23 + 21 + 2 + 1 and len(false) == 5
    assert all(ok and n >= MIN_PIXELS for _n, ok, _s, n in true), [x for x in true if not x[1]]
    assert not any(ok for _n, ok, _s, _N in false), false
    lo_true, hi_false = min(s for _n, _o, s, _N in true), max(s for _n, _o, s, _N in false)
    assert 0.84 < lo_true < 0.85 and 0.02 < hi_false < 0.03 and min(s for _n, _o, s, _N in false) > -0.11    # the ranges DESIGN.md records
    assert hi_false + 0.3 < THRESHOLD < lo_true - 0.3


# ---- host wiring -------------------------------------------------------------------------------------------------------------------
class VerifyingOracleEngine(OracleEngine):
    """the CPU double plus the verifier: verify_ncc is the specification, set_offset_verifier is recorded, and the fused attempt answers a
    scripted vote per direction and applies the verifier setting in force, as the engine's vote tail does"""

    def __init__(self, oracle=None, votes=None, fail=False):
        super().__init__(oracle)
        self.calls, self.verifier, self.seen, self.tiles, self.votes, self.fail = [], ("none", 0.0, 0), [], {}, votes or {}, fail

    def set_offset_verifier(self, kind="none", threshold=0.0, min_pixels=0):
        self.calls.append(("set_offset_verifier", kind, threshold, min_pixels))
        self.verifier = (kind, threshold, min_pixels)

    def verify_ncc(self, a, b, dx, dy, min_pixels=0):
        self.calls.append(("verify_ncc", a.shape, dx, dy, min_pixels))
        s = V.sums(np.ascontiguousarray(a), np.ascontiguousarray(b), dx, dy)
        sc = V.score(s, min_pixels)
        return s, sc, V.fixed(sc)

    def tile_upload(self, img):
        self.tiles[len(self.tiles) + 1] = img
        return len(self.tiles)

    def tile_free(self, h):
        pass

    def attempt_surf_batch(self, jobs, params=None, ratio=0.75, offset_evaluate=3):
        self.seen.append(("attempt_surf_batch", self.verifier))
        if self.fail:
            raise RuntimeError("batch failed")
        out = np.zeros((len(jobs), 8), np.int32)
        for n, (ta, tb, ay0, ax0, by0, bx0, h, w) in enumerate(jobs):
            d = 1 if (ay0 > 0 and w > h) else 2 if ax0 > 0 else 3 if by0 > 0 else 4
            dx, dy = self.votes.get(d, (0, 0))
            row = [1, dx, dy, 5, 10, 10, 6, 0]
            if self.verifier[0] == "ncc":
                row = V.verify_row(row, self.tiles[ta][ay0:ay0 + h, ax0:ax0 + w], self.tiles[tb][by0:by0 + h, bx0:bx0 + w], *self.verifier[1:])
            out[n] = row
        return out


def _shifted_pair(seed=5):
    """B lies to the RIGHT of A (direction 2): B's column 0 is A's column 160 of a 200 x 240 tile, B's row 3 is A's row 0"""
    scene = np.random.default_rng(seed).integers(0, 256, (260, 460), dtype=np.uint8)
    return np.ascontiguousarray(scene[20:220, 20:260]), np.ascontiguousarray(scene[17:217, 180:420])


class ScriptedOperators(isa.Stitcher):
    """a Stitcher with its own detector, matcher and vote (the host-operator path): the vote of a strip pair is scripted by the strips'
    shape -- direction 1 / 3 strips (wide) get a wrong vote, direction 2 / 4 strips (tall) the true one"""
    wide_vote, tall_vote = [5, 7], [0, 0]

    def detectAndDescribe(self, image, featureMethod):
        self._shape = image.shape
        return np.zeros((4, 2), np.float32), np.zeros((4, 4), np.float32)

    def matchDescriptors(self, featuresA, featuresB):
        return [(0, 0)]

    def getOffsetByMode(self, kpsA, kpsB, matches, offsetEvaluate=10):
        return (True, list(self.wide_vote if self._shape[1] > self._shape[0] else self.tall_vote))


def test_verify_offset_goes_through_the_engine():
    eng = VerifyingOracleEngine()
    m = isa.Method(); m._engine = eng
    A, B = _shifted_pair()
    a, b = A[:, 192:], B[:, :48]                                   # the direction-2 strips at roiRatio 0.2: true raw vote (-3, -32)
    assert m.verifyOffset(a, b, [-3, -32]) == (False, 0.0)          # 197 x 16 shared pixels: fewer than the default verifyMinPixels
    assert eng.calls == [("verify_ncc", (200, 48), -3, -32, isa.Method.verifyMinPixels)]
    m.verifyMinPixels = 1000
    ok, sc = m.verifyOffset(a, b, [-3, -32])
    assert ok and sc > 1 - 1e-12
    ok, sc = m.verifyOffset(a, b, [5, 7])
    assert not ok and abs(sc) < 0.2
    m.verifyMinPixels = 200 * 48
    assert m.verifyOffset(a, b, [-3, -32]) == (False, 0.0)
    assert (isa.Method.offsetVerify, isa.Method.verifyThreshold, isa.Method.verifyMinPixels) == ("none", 0.5, 4096)


def test_none_makes_no_verifier_call():
    """engines and doubles of before this feature (the plain OracleEngine has neither method) keep working"""
    class Plain(VerifyingOracleEngine):
        def __getattribute__(self, name):
            if name in ("set_offset_verifier", "verify_ncc"):
                raise AttributeError(name)
            return super().__getattribute__(name)
    A, B = _shifted_pair()
    st = ScriptedOperators(); st._engine = Plain(); st.isPrintLog = False; st.roiRatio = 0.2; st.direction = 1
    assert st.calculateOffsetForFeatureSearchIncre([A, B]) == (True, [5 + 200 - 40, 7])          # the wrong first candidate is accepted
    assert st.calculateOffsetForFeatureSearch([A, B]) == (True, [5, 7])
    stock = isa.Stitcher(); stock._engine = Plain(votes={1: (5, 7), 2: (-3, -32)}); stock.isPrintLog = False; stock.roiRatio = 0.2; stock.direction = 1
    assert stock._usesStockOperators()
    assert stock.calculateOffsetForFeatureSearchIncre([A, B]) == (True, [5 + 200 - 40, 7])
    assert stock._engine.seen == [("attempt_surf_batch", ("none", 0.0, 0))] and stock._engine.calls == []
    for native in (True, False):
        reg = GridRegistrar(Plain(), method="surf", roiRatio=0.2)
        assert reg.offsetVerify == "none"
        reg.native = False
        table, _d = reg.register([1, 2, 3], [(100, 120)] * 3, 1) if not native else (None, None)
    assert GridRegistrar(Plain(), method="phase", offsetVerify="ncc").offsetVerify == "none"


def test_rejected_first_candidate_falls_through_to_the_next_direction():
    A, B = _shifted_pair()
    # the host-operator branch: Method.verifyOffset on the raw strips after the vote
    eng = VerifyingOracleEngine()
    st = ScriptedOperators(); st._engine = eng; st.isPrintLog = False; st.roiRatio = 0.2; st.direction = 1
    st.offsetVerify = "ncc"; st.tall_vote = [-3, -32]; st.verifyMinPixels = 1000
    assert st.calculateOffsetForFeatureSearchIncre([A, B]) == (True, [-3, -32 + 240 - 48])
    assert st.direction == 2
    assert [c[:4] for c in eng.calls] == [("verify_ncc", (40, 240), 5, 7), ("verify_ncc", (200, 48), -3, -32)]
    # with enhancement the check still reads the RAW strips
    st.direction = 1; st.isEnhance = True; eng.calls.clear()
    eng.enhance = lambda img, mode, clip, tiles: np.zeros_like(img)
    assert st.calculateOffsetForFeatureSearchIncre([A, B]) == (True, [-3, -32 + 240 - 48])
    st.isEnhance = False
    # the whole-tile search: the two tiles after the vote
    st.wide_vote = [-3, 160]; eng.calls.clear()
    assert st.calculateOffsetForFeatureSearch([A, B]) == (True, [-3, 160])
    st.wide_vote = [5, 7]
    assert st.calculateOffsetForFeatureSearch([A, B])[0] is False
    assert [c[:4] for c in eng.calls] == [("verify_ncc", (200, 240), -3, 160), ("verify_ncc", (200, 240), 5, 7)]
    # the fused single attempt: the verifier is set around the engine's call and the engine's row decides
    eng = VerifyingOracleEngine(votes={1: (5, 7), 2: (-3, -32)})
    stock = isa.Stitcher(); stock._engine = eng; stock.isPrintLog = False; stock.roiRatio = 0.2; stock.direction = 1
    stock.offsetVerify = "ncc"; stock.verifyMinPixels = 1000
    assert stock._usesStockOperators()
    assert stock.calculateOffsetForFeatureSearchIncre([A, B]) == (True, [-3, -32 + 240 - 48]) and stock.direction == 2
    assert eng.seen == [("attempt_surf_batch", ("ncc", 0.5, 1000))] * 2 and eng.verifier[0] == "none"
    assert not any(c[0] == "verify_ncc" for c in eng.calls)


def test_line_scans_leave_the_batched_path():
    class Full(VerifyingOracleEngine):
        def features_surf_batch(self, *a, **k):
            raise AssertionError("the whole-tile batch must not run under offsetVerify")

        def attempt_orb_batch(self, *a, **k):
            raise AssertionError("no batch runs here")
    st = isa.Stitcher(); st._engine = Full(); st.featureMethod = "surf"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearch, 4) == "surf_full"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearchIncre, 4) == "surf"
    st.offsetVerify = "ncc"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearch, 4) is None
    assert st._batchedMethod(st.calculateOffsetForFeatureSearchIncre, 4) == "surf"            # the incremental search stays batched
    reg = st._makeRegistrar("surf", 4)
    assert (reg.offsetVerify, reg.verifyThreshold, reg.verifyMinPixels) == ("ncc", 0.5, 4096)
    assert st._makeRegistrar("phase", 4).offsetVerify == "none"
    st.featureMethod = "orb"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearch, 4) is None
    st.offsetVerify = "none"
    assert st._batchedMethod(st.calculateOffsetForFeatureSearch, 4) == "orb_full"


def test_grid_registrar_sets_the_verifier_and_restores_none_after_an_exception():
    A, B = _shifted_pair()
    eng = VerifyingOracleEngine(votes={1: (5, 7), 2: (-3, -32)})
    reg = GridRegistrar(eng, method="surf", roiRatio=0.2, offsetVerify="ncc", verifyThreshold=0.5, verifyMinPixels=1000)
    reg.native = False
    ha, hb = eng.tile_upload(A), eng.tile_upload(B)
    table, d = reg.register([ha, hb], [A.shape, B.shape], 1)
    assert [int(v) for v in table[0][:5]] == [1, -3, -32 + 240 - 48, 2, 1] and d == 2
    assert eng.seen and all(s == ("ncc", 0.5, 1000) for _n, s in eng.seen) and eng.verifier == ("none", 0.0, 0)
    bad = VerifyingOracleEngine(fail=True)
    reg = GridRegistrar(bad, method="surf", roiRatio=0.2, offsetVerify="ncc", verifyThreshold=0.5, verifyMinPixels=1000)
    reg.native = False
    with pytest.raises(RuntimeError):
        reg.register([1, 2, 3], [(100, 120)] * 3, 1)
    assert bad.seen == [("attempt_surf_batch", ("ncc", 0.5, 1000))] and bad.verifier[0] == "none"
    assert bad.calls[-1][:2] == ("set_offset_verifier", "none")
