"""CPU tests of featureMethod "sift": det_exp against the correctly rounded expf on every float32 argument the path forms, the two copies
of det_exp (csrc/detmath.h and tests/sift_ref.py) against each other, the routing of Method.detectAndDescribe, and the specification on
real data: SIFT as tests/sift_ref.py states it registers the real dendriticCrystal strips within 1 px of Stitcher.py:87."""
import os
import re

import numpy as np
import pytest

import sift_ref as S
from test_oracle_golden import _f32_correctly_rounded, pool_size

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class SpecEngine:
    """An engine whose SIFT is the numpy specification; every other operator is the wrapped engine's."""

    def __init__(self, base):
        self.base = base

    def __getattr__(self, name):
        return getattr(self.base, name)

    @staticmethod
    def sift_params(n_octave_layers=3, contrast_threshold=0.04, edge_threshold=10.0, sigma=1.6, n_features=0):
        return S.Params(n_octave_layers, contrast_threshold, edge_threshold, sigma)

    def sift_detect_describe(self, img, params=None, cap=None, full=False):
        return S.sift_detect_describe(np.ascontiguousarray(img), params, full)


# ---- det_exp ---------------------------------------------------------------------------------------------------------------------
def _det_exp_chunk(lo, hi):
    """float32 bit patterns [lo, hi) -> (x of every candidate, det_exp there, numpy's exp there, how many were screened).  A candidate is
    an x where the float32 rounding of det_exp differs from that of numpy's float64 exp, or where numpy's value lies within 16 double
    ulps of a float32 rounding midpoint."""
    x = np.arange(lo, hi, dtype=np.uint32).view(np.float32).astype(np.float64)
    det = S.det_exp(x)
    ref = np.exp(x)
    cand = det.astype(np.float32) != ref.astype(np.float32)
    low = ref.view(np.int64) & ((1 << 29) - 1)
    cand |= np.abs(low - (1 << 28)) <= 16
    idx = np.nonzero(cand)[0]
    return x[idx], det[idx], ref[idx], len(x)


def _sweep(ranges):
    import mpmath
    from concurrent.futures import ThreadPoolExecutor
    CHUNK = 1 << 22
    jobs = [(a, min(a + CHUNK, b)) for a, b in ranges for a in range(a, b, CHUNK)]
    with ThreadPoolExecutor(max_workers=pool_size()) as ex:
        parts = list(ex.map(lambda j: _det_exp_chunk(*j), jobs))
    xs = np.concatenate([p[0] for p in parts]); det = np.concatenate([p[1] for p in parts]); npv = np.concatenate([p[2] for p in parts])
    assert sum(p[3] for p in parts) == sum(b - a for a, b in ranges)
    assert len(xs) <= 20000, ("det_exp disagrees with numpy's exp on too many arguments", len(xs))
    exceptions = []
    with mpmath.workprec(200):
        for x, d, ref in zip(xs, det, npv):
            v = mpmath.exp(mpmath.mpf(float(x)))
            assert abs(v - mpmath.mpf(float(ref))) < 16 * np.spacing(ref), float(x)      # the screen's premise
            if np.float32(d) != _f32_correctly_rounded(v):
                exceptions.append((float(x), float(d)))
    return len(xs), exceptions


def test_det_exp_equals_correctly_rounded_expf_on_the_window_weights():
    """Every float32 x in [-16, 0] (bit patterns 0x80000000 .. 0xC1800000): the Gaussian weights of the orientation histogram
    ((i^2 + j^2) * -1 / (2 sigma^2) >= -10.3 for every sigma >= 1 scale the path forms) and of the descriptor (>= -1.6)."""
    assert np.uint32(0xC1800000).view(np.float32) == np.float32(-16)
    n, exceptions = _sweep([(0x80000000, 0xC1800000 + 1)])
    print("det_exp [-16, 0]: %d candidates settled with mpmath, %d exceptions" % (n, len(exceptions)))
    assert exceptions == []


def test_det_exp_equals_correctly_rounded_expf_on_the_size_term():
    """Every float32 x in [0.04, 1.05]: x = ((layer + xi) / nOctaveLayers) * (float)ln 2 with 1 <= layer <= nOctaveLayers <= 8, |xi| < 0.5"""
    lo, hi = int(np.float32(0.04).view(np.uint32)), int(np.float32(1.05).view(np.uint32))
    assert np.float32(0.5 / 8) * S.LN2F > np.float32(0.04) and np.float32(1.5) * S.LN2F < np.float32(1.05)
    n, exceptions = _sweep([(lo, hi + 1)])
    print("det_exp size term: %d candidates settled with mpmath, %d exceptions" % (n, len(exceptions)))
    assert exceptions == []


def test_det_exp_device_and_spec_copies_agree():
    names = ["INVLN2", "LN2_HI", "LN2_LO", "P1", "P2", "P3", "P4", "P5"]
    txt = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "detmath.h")).read()
    start = txt.index("double det_exp(")
    dev = txt[start:txt.index("\n}", start)]
    # det_sincos comes first and is untouched by det_exp
    assert txt.index("void det_sincos(") < start
    src = open(os.path.join(ROOT, "tests", "sift_ref.py")).read()
    for n in names:
        m = re.findall(r"\b%s\s*=\s*([-+0-9.eE]+)\s*[,;]" % n, dev)
        p = re.findall(r"^%s\s*=\s*([-+0-9.eE]+)\s*$" % n, src, flags=re.M)
        assert len(m) == 1 and len(p) == 1 and m[0] == p[0] and float(m[0]) == getattr(S, n), (n, m, p)
    dexpr = {k: re.sub(r"\s+", "", v) for k, v in re.findall(r"const double (kd|hi|lo|r|t|c|y) = ([^;]+);", dev)}
    pstart = src.index("def det_exp(")
    body = src[pstart:src.index("\n\n", pstart)]
    pexpr = {k: re.sub(r"\s+", "", v).replace("np.", "") for k, v in re.findall(r"^\s+(kd|hi|lo|r|t|c|y) = (.+)$", body, flags=re.M)}
    assert sorted(dexpr) == sorted(pexpr) == sorted(["kd", "hi", "lo", "r", "t", "c", "y"])
    assert dexpr == pexpr
    assert "returnldexp(y,(int)kd)" in re.sub(r"\s+", "", dev) and "returnnp.ldexp(y,kd.astype(np.int32))" in re.sub(r"\s+", "", body)
    # ln 2 split as fdlibm's: LN2_HI has 32 significant bits, so k * LN2_HI and x - k * LN2_HI are exact for the |k| < 2^21 of float x
    hi, lo = S.LN2_HI, S.LN2_LO
    assert hi * 2.0 ** 32 == int(hi * 2.0 ** 32) and abs(hi + lo - np.log(2)) < 1e-16 and S.INVLN2 == 1 / np.log(2)


def test_det_exp_spot_values():
    x = np.array([0.0, -0.0, 1.0, -1.0, -16.0, 0.5, np.log(2)])
    assert np.array_equal(S.det_exp(x[:2]), [1.0, 1.0])
    assert np.all(np.abs(S.det_exp(x) / np.exp(x) - 1) < 4e-16)


# ---- routing -----------------------------------------------------------------------------------------------------------------------
def test_detect_and_describe_routes_sift_to_the_engine():
    """Method.detectAndDescribe(img, "sift") returns the engine's SIFT arrays (here the specification's), ([], None) without keypoints"""
    from imagestitch_amd.utility import Method
    m = Method(); m._engine = SpecEngine(None)
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, (70, 90), dtype=np.uint8)
    kps, feats = m.detectAndDescribe(img, "sift")
    rxy, rdesc = S.sift_detect_describe(img)
    assert len(rxy) > 0 and np.array_equal(kps, rxy) and np.array_equal(feats, rdesc) and feats.shape[1] == 128
    kps, feats = m.detectAndDescribe(np.full((70, 90), 128, np.uint8), "sift")
    assert len(kps) == 0 and feats is None
    with pytest.raises(NotImplementedError):
        m.detectAndDescribe(img, "brisk")


# ---- the specification itself ------------------------------------------------------------------------------------------------------
def test_spec_pyramid_structure():
    img = np.random.default_rng(4).integers(0, 256, (40, 70), dtype=np.uint8)
    g, d = S.pyramid(img)
    assert len(g) == S.n_octaves(40, 70) == int(np.rint(np.log(80) / np.log(2) - 2)) + 1
    assert g[0][0].shape == (80, 140) and g[1][0].shape == (40, 70) and g[2][0].shape == (20, 35)
    assert np.array_equal(g[1][0], g[0][3][::2, ::2])           # even sizes: INTER_NEAREST 2x decimation takes the even samples
    up = S.upsample2x(img.astype(np.float32)).astype(np.float64)
    a = img.astype(np.float64)
    inner = 0.25 * (0.25 * a[:-1, :-1] + 0.75 * a[:-1, 1:]) + 0.75 * (0.25 * a[1:, :-1] + 0.75 * a[1:, 1:])
    assert np.array_equal(up[2::2, 2::2], inner) and np.array_equal(up[0, 0], a[0, 0])
    taps = S.gaussian_taps(1.6)
    assert len(taps) == 15 and abs(float(taps.astype(np.float64).sum()) - 1) < 1e-6 and np.array_equal(taps, taps[::-1])
    for o in range(len(g)):
        for i in range(len(d[o])):
            assert np.array_equal(d[o][i], g[o][i + 1] - g[o][i])


def test_spec_keypoints_are_distinct_and_well_formed():
    img = np.random.default_rng(9).integers(0, 256, (120, 200), dtype=np.uint8)
    xy, desc, kps = S.sift_detect_describe(img, full=True)
    assert len(kps) > 20
    keys = set(zip(kps["x"].tolist(), kps["y"].tolist(), kps["size"].tolist(), kps["angle"].tolist()))
    assert len(keys) == len(kps)
    assert np.all((kps["angle"] >= 0) & (kps["angle"] < 360)) and np.all(kps["class_id"] == -1)
    assert np.all((kps["x"] >= 0) & (kps["x"] < 200) & (kps["y"] >= 0) & (kps["y"] < 120))
    octv = kps["octave"] & 255
    assert set(np.unique(octv)) <= set([255] + list(range(8)))
    assert np.all((desc >= 0) & (desc <= 255) & (desc == np.rint(desc)))


def test_spec_registers_the_real_strips(golden_dir):
    """SIFT as specified, through a Stitcher whose other operators are the CPU oracle's: all three real ROI pairs accepted within 1 px of
    Stitcher.py:87 -- the check that the specification is a SIFT that works, before any GPU is involved"""
    from oracle import oracle as O
    from fakes import OracleEngine
    import imagestitch_amd as isa
    O.build()
    st = isa.Stitcher(); st._engine = SpecEngine(OracleEngine(O))
    st.featureMethod = "sift"; st.isPrintLog = False; st.roiRatio = 0.2
    g = np.load(os.path.join(golden_dir, "real_strips.npz"))
    for n, (a, b, direction, H, W, gdx, gdy) in enumerate(g["meta"]):
        ka, fa = st.detectAndDescribe(g["r%d_roiA" % n], "sift")
        kb, fb = st.detectAndDescribe(g["r%d_roiB" % n], "sift")
        assert fa is not None and fb is not None and len(ka) > 500 and len(kb) > 500
        ok, off = st.getOffsetByMode(ka, kb, st.matchDescriptors(fa, fb), offsetEvaluate=st.offsetEvaluate)
        assert ok, n
        off = st._axisCorrection(list(off), int(direction), 1, np.empty((H, W)), np.empty((H, W)))
        assert abs(off[0] - gdx) <= 1 and abs(off[1] - gdy) <= 1, (a, b, off, (gdx, gdy))


# ---- SIFT constants: both copies against OpenCV 3.3.1 ---------------------------------------------------------------------------
# (name, OpenCV 3.3.1 value, regex in csrc/sift_kernels.hip, regex in tests/sift_ref.py); each regex must match exactly once
_CONSTANTS = [
    ("SIFT_IMG_BORDER", 5, r"#define SIFT_BORDER (\d+)", r"^BORDER = (\d+)"),
    ("SIFT_MAX_INTERP_STEPS", 5, r"#define SIFT_MAX_STEPS (\d+)", r"^MAX_INTERP_STEPS = (\d+)"),
    ("SIFT_ORI_HIST_BINS", 36, r"#define SIFT_ORI_BINS (\d+)", r"^ORI_HIST_BINS = (\d+)"),
    ("SIFT_ORI_PEAK_RATIO", 0.8, r"omax \* ([\d.]+)f;", r"F\(omax \* F\(([\d.]+)\)\)"),
    ("SIFT_ORI_SIG_FCTR", 1.5, r"sigma = ([\d.]+)f \* scl;", r"F\(F\(([\d.]+)\) \* scl\)\)"),
    ("SIFT_ORI_RADIUS", 4.5, r"rintf\(([\d.]+)f \* scl\)", r"cv_round\(F\(([\d.]+)\) \* scl\)"),
    ("SIFT_DESCR_WIDTH", 4, r"constexpr int d = (\d+), n = \d+,", r"^DESCR_WIDTH, DESCR_HIST_BINS = (\d+), \d+"),
    ("SIFT_DESCR_HIST_BINS", 8, r"constexpr int d = \d+, n = (\d+),", r"^DESCR_WIDTH, DESCR_HIST_BINS = \d+, (\d+)"),
    ("SIFT_DESCR_SCL_FCTR", 3.0, r"hist_width = ([\d.]+)f \* scl;", r"hist_width = F\(([\d.]+)\) \* scl"),
    ("SIFT_DESCR_MAG_THR", 0.2, r"sqrtf\(nrm2\) \* ([\d.]+)f;", r"np\.sqrt\(nrm2, dtype=F\) \* F\(([\d.]+)\)"),
    ("SIFT_INT_DESCR_FCTR", 512.0, r"s_scale = ([\d.]+)f /", r"nrm2 = F\(([\d.]+)\) / max"),
    ("SIFT_INIT_SIGMA", 0.5, r"\(([\d.]+)f \* [\d.]+f\) \* 4\.f", r"F\(F\(F\(([\d.]+)\) \* F\([\d.]+\)\) \* F\(4\)\)"),
]


def test_sift_constants_are_opencv_3_3_1_in_both_copies():
    """The SIFT_* constants of OpenCV 3.3.1's sift.cpp, written out here, in the kernel source and in the specification: a slip shared
    by the two copies fails against the pinned value"""
    dev = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "sift_kernels.hip")).read()
    spec = open(os.path.join(ROOT, "tests", "sift_ref.py")).read()
    for name, val, rd, rs in _CONSTANTS:
        md = re.findall(rd, dev, flags=re.M)
        ms = re.findall(rs, spec, flags=re.M)
        assert len(md) == 1 and len(ms) == 1, (name, md, ms)
        assert float(md[0]) == val and float(ms[0]) == val, (name, val, md, ms)
    assert (S.BORDER, S.MAX_INTERP_STEPS, S.ORI_HIST_BINS, S.DESCR_WIDTH, S.DESCR_HIST_BINS) == (5, 5, 36, 4, 8)
    # the initial blur: sqrt(max(sigma^2 - (2 * SIFT_INIT_SIGMA)^2, 0.01)) for sigma 1.6 and 0.9
    assert abs(S.initial_sigma(S.Params()) - np.sqrt(1.6 ** 2 - 1)) < 1e-6 and abs(S.initial_sigma(S.Params(sigma=0.9)) - 0.1) < 1e-7


# ---- fast_atan2_deg against float64 atan2 --------------------------------------------------------------------------------------
def test_fast_atan2_deg_within_a_hundredth_of_a_degree():
    """10^7 float32 pairs whose larger component spans 1e-6 .. 1e30 (the smaller one anything down to signed zero and +-1e-45), plus
    the integer gradients of u8 images: |fast_atan2_deg - atan2| <= 0.01 degrees (circularly), outputs in [0, 360], and 360 itself only
    for y < 0 with |y| << |x|, where the true angle is within 0.01 degrees below 360 and the orientation bin wraps 36 -> 0.  Below
    1e-6 cv::fastAtan2's DBL_EPSILON guard in the divisor dominates (a gradient that small carries no histogram weight); (0, 0) is 0."""
    rng = np.random.default_rng(1)
    n = 10 ** 7
    big = (10.0 ** rng.uniform(-6, 30, n)) * rng.choice([-1.0, 1.0], n)
    small = big * rng.uniform(-1, 1, n) * (10.0 ** rng.uniform(-40, 0, n))
    swap = rng.random(n) < 0.5
    y = np.where(swap, big, small).astype(np.float32); x = np.where(swap, small, big).astype(np.float32)
    sp = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-45, -1e-45], np.float32)
    lg = np.array([1e-6, -1e-6, 1.0, -1.0, 255.0, -255.0, 3e38, -3e38], np.float32)
    A, B = np.meshgrid(sp, lg, indexing="ij")
    gy, gx = np.meshgrid(np.arange(-255, 256, dtype=np.float32), np.arange(-255, 256, dtype=np.float32), indexing="ij")
    y = np.concatenate([y, A.ravel(), B.ravel(), gy.ravel(), np.float32([0, 0, -0.0, -0.0])])
    x = np.concatenate([x, B.ravel(), A.ravel(), gx.ravel(), np.float32([0, -0.0, 0, -0.0])])
    with np.errstate(over="ignore"):
        a = S.fast_atan2_deg(y, x)
    assert a.dtype == np.float32 and np.all((a >= 0) & (a <= 360))
    zero = (y == 0) & (x == 0)
    assert zero.sum() == 5 and np.all(a[zero] == 0)
    ref = np.degrees(np.arctan2(y.astype(np.float64), x.astype(np.float64)))
    d = np.abs((a.astype(np.float64) - ref + 180) % 360 - 180)[~zero]
    print("fast_atan2_deg: max error %.5f degrees over %d pairs" % (d.max(), len(d)))
    assert len(d) >= n and d.max() <= 0.01
    w = a == 360
    assert w.any() and np.all(y[w] < 0) and np.all(ref[w] > -0.01) and np.all(ref[w] < 0)
    b = np.rint(np.float32(36 / 360.0) * a[w]).astype(np.int64)
    assert np.all(np.where(b >= 36, b - 36, b) == 0)


def test_gaussian_taps_are_the_normalised_gaussian():
    """gaussian_taps against the float64 Gaussian: length cvRound(8 sigma + 1) | 1, symmetric, sum 1, each tap within float rounding"""
    import sift_f64 as G
    for sig in [0.1, 0.5, 1.0, 1.2263, 1.6, 2.0, 2.5198, 3.1748, 7.9, 15.8]:
        t = S.gaussian_taps(sig)
        n = int(np.rint(sig * 8 + 1)) | 1
        assert len(t) == n and t.dtype == np.float32 and np.array_equal(t, t[::-1]), sig
        ref = G.taps64(sig)
        assert np.all(np.abs(t.astype(np.float64) - ref) <= 2 * np.spacing(np.float32(ref))), sig
        assert abs(t.astype(np.float64).sum() - 1) < n * 6e-8, sig
        assert np.argmax(t) == n // 2


# ---- the specification judged by the float64 references ------------------------------------------------------------------------
def _spec_cases():
    import sift_f64 as G
    return G.adversarial_images()


def check_adversarial_claims(name, n, stats):
    """each adversarial input reaches what tests/sift_f64.adversarial_images says it does"""
    if name == "spikes":
        assert n == 0, (name, n)
    if name == "reset":
        assert stats["angle_reset"] > 0, (name, stats)
    if name == "duplicates":
        assert stats["rows_before"] > stats["rows_after"], (name, stats)
    if name in ("blobs_int", "blobs_half", "discs", "checker"):
        assert sum(c >= 3 for c in stats["orientations"]) > 0, (name, stats["orientations"])


def test_float64_references_judge_the_spec():
    """The pyramid within 1e-3 grey levels of the float64 pyramid, every keypoint's refinement and orientation peaks against float64,
    on the adversarial inputs, each of which reaches its path: removeDuplicated, 3 or more orientations, the 360 -> 0 reset"""
    import sift_f64 as G
    p = S.Params()
    for name, img in _spec_cases():
        st = {}
        g, d = S.pyramid(img, p)
        k = S.detect(g, d, p, st)
        check_adversarial_claims(name, len(k), st)
        eg, ed = G.pyramid_error(img, g, d)
        ref = G.check_refinement(d, k)
        ori = G.check_orientation(g, k)
        print(name, len(k), "pyramid %.2e / %.2e" % (eg, ed), ref, ori)
        assert eg <= 1e-3 and ed <= 1e-3, name
        assert ref["offset"] <= 1e-3 and ref["size"] <= 1e-5 and ref["response"] <= 1e-5, (name, ref)
        assert ori["angle"] <= 1e-3, (name, ori)
    reset = dict(_spec_cases())["reset"]
    assert S.sift_detect_describe(reset, full=True)[2]["angle"].tolist() == [0.0]


def test_orientation_peak_on_bin_zero_is_reset_to_zero_degrees():
    """A histogram symmetric about bin 0 interpolates to bin 0 exactly: 360 - 0 is reported as 0, never 360; counted by the stats hook"""
    h = np.zeros(36, np.float32)
    h[0], h[1], h[35], h[18] = 10, 4, 4, 9
    st = {}
    a = S.peaks(h, st)
    assert [float(v) for v in a] == [0.0, 180.0] and st["angle_reset"] == 1
    assert all(0 <= v < 360 for v in a)


_MUTATIONS = {
    "cramer_sign": ("x0 = d * ((b0 * (a11 * a22 - a12 * a21) - a01 * (b1", "x0 = d * ((b0 * (a11 * a22 - a12 * a21) + a01 * (b1"),
    "sig_total": ("sig.append(math.sqrt(sig_total * sig_total - sig_prev * sig_prev))", "sig.append(sig_total)"),
    "peak_ratio": ("mag_thr = F(omax * F(0.8))", "mag_thr = F(omax * F(0.79))"),
    "no_angle_reset": ("                a = F(0)\n", "                pass\n"),
}


def _mutant(name):
    import types
    src = open(os.path.join(ROOT, "tests", "sift_ref.py")).read()
    old, new = _MUTATIONS[name]
    assert src.count(old) == 1, name
    m = types.ModuleType("sift_ref_" + name)
    exec(compile(src.replace(old, new), m.__name__, "exec"), m.__dict__)
    return m


@pytest.mark.parametrize("name", sorted(_MUTATIONS))
def test_float64_references_catch_a_slip_shared_with_the_spec(name):
    """The same slip in the kernel and the spec passes every equality test; the float64 references must still fail it.  Each mutant
    of sift_ref.py is run through the whole pipeline on the inputs of test_float64_references_judge_the_spec until one float64 check
    fails (without the reset, the "reset" input's keypoint reports 360 degrees, outside check_orientation's [0, 360))."""
    import sift_f64 as G
    M = _mutant(name)
    p = M.Params()
    failed = []
    for case, img in _spec_cases():
        if any(failed):
            break
        g, d = M.pyramid(img, p)
        k = M.detect(g, d, p)
        try:
            eg, ed = G.pyramid_error(img, g, d)
            ref = G.check_refinement(d, k)
            G.check_orientation(g, k)
            failed.append(eg > 1e-3 or ed > 1e-3 or ref["offset"] > 1e-3 or ref["size"] > 1e-5 or ref["response"] > 1e-5)
        except AssertionError:
            failed.append(True)
    assert any(failed), name
