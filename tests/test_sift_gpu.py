"""GPU tests of featureMethod "sift" (csrc/sift_kernels.hip): the device pyramid, keypoints and descriptors equal the numpy specification
tests/sift_ref.py bit for bit, and the Stitcher registers with SIFT through the generic per-pair path."""
import json
import os

import numpy as np
import pytest

import sift_ref as S

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def _smooth(img, k=5):
    f = img.astype(np.float64)
    for ax in (0, 1):
        f = sum(np.roll(f, s, axis=ax) for s in range(-(k // 2), k // 2 + 1)) / k
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def _images():
    rng = np.random.default_rng(7)
    out = []
    for shape in [(37, 53), (64, 64), (97, 131), (150, 300), (300, 1001)]:
        r = rng.integers(0, 256, shape, dtype=np.uint8)
        out.append(("random%dx%d" % shape, r))
        out.append(("smooth%dx%d" % shape, _smooth(r)))
    return out


def _params(engine, p):
    return engine.sift_params(p.n_octave_layers, p.contrast_threshold, p.edge_threshold, p.sigma)


def _check(engine, img, p=None, label=""):
    p = p or S.Params()
    xy, desc, kps = engine.sift_detect_describe(img, _params(engine, p), full=True)
    rxy, rdesc, rkps = S.sift_detect_describe(np.ascontiguousarray(img), p, full=True)
    assert len(kps) == len(rkps), (label, len(kps), len(rkps))
    for f in FIELDS:
        assert np.array_equal(kps[f], rkps[f]), (label, f, np.nonzero(kps[f] != rkps[f])[0][:5])
    assert np.array_equal(xy, rxy), label
    assert np.array_equal(desc, rdesc), (label, np.nonzero((desc != rdesc).any(1))[0][:5])
    return len(kps)


def test_sift_pyramid_levels_equal_the_spec(engine):
    rng = np.random.default_rng(3)
    for shape in [(37, 53), (120, 257)]:
        img = _smooth(rng.integers(0, 256, shape, dtype=np.uint8), 3)
        g, d = engine.sift_pyramid(img)
        rg, rd = S.pyramid(img)
        assert len(g) == len(rg) == S.n_octaves(*shape)
        for o in range(len(rg)):
            for i in range(len(rg[o])):
                assert np.array_equal(g[o][i], rg[o][i]), (shape, "gauss", o, i)
            for i in range(len(rd[o])):
                assert np.array_equal(d[o][i], rd[o][i]), (shape, "dog", o, i)


@pytest.mark.parametrize("name,img", _images(), ids=[n for n, _ in _images()])
def test_sift_keypoints_and_descriptors_equal_the_spec(engine, name, img):
    n = _check(engine, img, label=name)
    if img.shape[0] >= 97:
        assert n > 0, name


def test_sift_strided_view(engine):
    rng = np.random.default_rng(11)
    big = _smooth(rng.integers(0, 256, (200, 400), dtype=np.uint8), 3)
    view = big[13:170, 21:333]
    assert not view.flags["C_CONTIGUOUS"]
    assert _check(engine, view, label="view") > 0


def test_sift_no_keypoints(engine):
    from imagestitch_amd.utility import Method
    m = Method(); m._engine = engine
    for img in [np.full((120, 160), 77, np.uint8), np.zeros((5, 9), np.uint8), np.full((1, 1), 3, np.uint8), np.full((11, 300), 9, np.uint8)]:
        xy, desc = engine.sift_detect_describe(img)
        assert len(xy) == 0 and desc.shape == (0, 128)
        kps, feats = m.detectAndDescribe(img, "sift")
        assert len(kps) == 0 and feats is None
    rng = np.random.default_rng(5)
    assert _check(engine, rng.integers(0, 256, (9, 40), dtype=np.uint8), label="small") == 0


def test_sift_real_strips(engine, golden_dir):
    g = np.load(os.path.join(golden_dir, "real_strips.npz"))
    for n in range(3):
        for side in ("roiA", "roiB"):
            assert _check(engine, g["r%d_%s" % (n, side)], label="r%d_%s" % (n, side)) > 500


def test_sift_production_strip(engine):
    """the roiRatio 0.2 strip of a 2048 x 2048 tile, 409 x 2048"""
    from imagestitch_amd.synthetic import SyntheticGrid
    A = SyntheticGrid(2, 1, 2048).tiles(threads=1)[0]
    assert _check(engine, np.ascontiguousarray(A[-409:]), label="strip409") > 500


@pytest.mark.parametrize("kw", [dict(n_octave_layers=2), dict(n_octave_layers=4), dict(contrast_threshold=0.02), dict(contrast_threshold=0.08),
                                dict(edge_threshold=5.0), dict(edge_threshold=20.0), dict(sigma=1.2), dict(sigma=2.0)],
                         ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_sift_parameter_variants(engine, kw):
    rng = np.random.default_rng(13)
    img = _smooth(rng.integers(0, 256, (160, 410), dtype=np.uint8), 3)
    assert _check(engine, img, S.Params(**kw), label=str(kw)) > 0


def test_sift_refuses_nfeatures(engine):
    import imagestitch_amd as isa
    with pytest.raises(isa.VfsmsError):
        engine.sift_detect_describe(np.zeros((64, 64), np.uint8), engine.sift_params(n_features=100))
    with pytest.raises(isa.VfsmsError):
        engine.sift_detect_describe(np.zeros((64, 64), np.uint8), engine.sift_params(n_octave_layers=9))


def test_sift_stitcher_on_synthetic_grid(engine):
    """calculateOffsetForFeatureSearchIncre with "sift" over a 2 x 2 grid of 640 px tiles: every pair within 1 px of the truth, the direction
    threaded across the turn of the serpentine path"""
    import imagestitch_amd as isa
    from imagestitch_amd.synthetic import SyntheticGrid
    g = SyntheticGrid(2, 2, 640)
    tiles = g.tiles(threads=1)
    st = isa.Stitcher(); st._engine = engine
    st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = 1
    truth = g.true_offsets()
    dirs = []
    for k in range(len(tiles) - 1):
        ok, off = st.calculateOffsetForFeatureSearchIncre([tiles[k], tiles[k + 1]])
        assert ok, k
        assert abs(off[0] - truth[k][0]) <= 1 and abs(off[1] - truth[k][1]) <= 1, (k, off, truth[k])
        dirs.append(st.direction)
    assert dirs[0] == 1 and dirs[1] != 1


def test_sift_dendritic_pairs(engine, golden_dir):
    """the 25 real dendriticCrystal pairs of tests/golden/real_path_strips (five neighbourhoods around the turns of the path), pair by pair
    through the Stitcher with featureMethod "sift", the direction threaded: the first neighbourhood's rows equal a CPU run of the same
    Stitcher on sift_ref, and the agreement with Stitcher.py:87 is recorded for all 25"""
    import imagestitch_amd as isa
    from test_oracle_golden import _rebuild_frames
    from test_sift_host import SpecEngine
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    g = np.load(os.path.join(golden_dir, "real_path_strips.npz"))
    within, rows = 0, []
    for q, nb in enumerate(meta):
        frames = _rebuild_frames(nb, g)
        runs = [engine] + ([SpecEngine(engine)] if q == 0 else [])
        got = []
        for eng in runs:
            st = isa.Stitcher(); st._engine = eng
            st.featureMethod = "sift"; st.roiRatio = 0.2; st.isPrintLog = False; st.direction = nb["incoming_direction"]
            out = []
            for k in range(len(nb["expected"])):
                ok, off = st.calculateOffsetForFeatureSearchIncre([frames[k], frames[k + 1]])
                out.append((bool(ok), list(off), st.direction))
            got.append(out)
        if q == 0:
            assert got[0] == got[1]
        for e, (ok, off, d) in zip(nb["expected"], got[0]):
            good = ok and abs(off[0] - e["gold"][0]) <= 1 and abs(off[1] - e["gold"][1]) <= 1
            within += good
            rows.append({"turn": nb["turn"], "ok": ok, "offset": off, "direction": d, "gold": e["gold"], "within_1px": bool(good)})
    print("sift dendritic pairs within 1 px of Stitcher.py:87: %d / 25" % within)
    print(json.dumps(rows))
    assert len(rows) == 25 and within == 25


# ---- production sizes ------------------------------------------------------------------------------------------------------------
def spec_job(img):
    """one image through the specification, in a worker process -> (xy, desc, kps)"""
    return S.sift_detect_describe(img, None, full=True)


@pytest.fixture(scope="module")
def production():
    """The ROI shapes registration forms at production sizes, and the specification of each computed once, in parallel worker
    processes (fresh interpreters, at most pool_size()): configs[4]'s roiRatio 0.2 strip of a 4096^2 tile (819 x 4096), a whole
    2048^2 tile as the whole-tile search sees it, and the left / right ROI shape of a 2048^2 tile (2048 x 409)"""
    import multiprocessing as mp
    from concurrent.futures import ProcessPoolExecutor
    from imagestitch_amd.synthetic import SyntheticGrid
    from test_oracle_golden import pool_size
    t4096 = SyntheticGrid(2, 1, 4096).tiles(threads=min(8, pool_size()))[0]
    t2048 = SyntheticGrid(2, 1, 2048).tiles(threads=min(8, pool_size()))[1]
    imgs = {"strip819x4096": np.ascontiguousarray(t4096[-819:]), "tile2048": np.ascontiguousarray(t2048),
            "cols2048x409": np.ascontiguousarray(t2048[:, -409:])}
    with ProcessPoolExecutor(max_workers=min(len(imgs), pool_size()), mp_context=mp.get_context("spawn")) as ex:
        futs = {k: ex.submit(spec_job, v) for k, v in imgs.items()}
        spec = {k: f.result() for k, f in futs.items()}
    return imgs, spec, t2048


def _check_against(engine, img, ref, label, cap=None):
    xy, desc, kps = engine.sift_detect_describe(img, cap=cap, full=True)
    rxy, rdesc, rkps = ref
    assert len(kps) == len(rkps), (label, len(kps), len(rkps))
    for f in FIELDS:
        assert np.array_equal(kps[f], rkps[f]), (label, f, np.nonzero(kps[f] != rkps[f])[0][:5])
    assert np.array_equal(xy, rxy), label
    assert np.array_equal(desc, rdesc), (label, np.nonzero((desc != rdesc).any(1))[0][:5])
    return len(kps)


@pytest.mark.timeout(1200)
def test_sift_production_sizes_equal_the_spec(engine, production):
    imgs, spec, t2048 = production
    for k, img in imgs.items():
        n = _check_against(engine, img, spec[k], k)
        print("%s: %d keypoints" % (k, n))
        assert n > 1000, k
    # strided views: the strip inside a wider buffer, and the right-hand columns of the tile as numpy slices them
    buf = np.zeros((819, 4096 + 96), np.uint8)
    buf[:, 40:40 + 4096] = imgs["strip819x4096"]
    view = buf[:, 40:40 + 4096]
    assert not view.flags["C_CONTIGUOUS"]
    _check_against(engine, view, spec["strip819x4096"], "strided strip")
    cols = t2048[:, -409:]
    assert not cols.flags["C_CONTIGUOUS"]
    _check_against(engine, cols, spec["cols2048x409"], "strided columns")


CAPACITY_ERROR = r"^libvfsms error -2: sift: \d+ keypoints exceed the caller's capacity \d+$"   # VFSMS_ERR_CAPACITY
BAD_ARG_ERROR = r"^libvfsms error -1: sift: (bad parameters|sigma too large for the blur)"   # VFSMS_ERR_BAD_ARG


@pytest.mark.timeout(1200)
def test_sift_context_state_across_sizes(production):
    """One fresh engine: small -> 2048^2 (scratch grows) -> small -> 819 x 4096 -> sift_pyramid -> small, each result equal to the
    specification; then the caller-capacity path (cap = n succeeds, cap = n - 1 is refused and the next call is right, cap = 0)"""
    import imagestitch_amd as isa
    imgs, spec, _ = production
    rng = np.random.default_rng(17)
    small = _smooth(rng.integers(0, 256, (37, 53), dtype=np.uint8), 3)
    mid = _smooth(rng.integers(0, 256, (120, 257), dtype=np.uint8), 3)
    rsmall = S.sift_detect_describe(small, None, full=True)
    eng = isa.Engine(0)
    try:
        _check_against(eng, small, rsmall, "small 1")
        _check_against(eng, imgs["tile2048"], spec["tile2048"], "tile2048")
        _check_against(eng, small, rsmall, "small 2")
        _check_against(eng, imgs["strip819x4096"], spec["strip819x4096"], "strip819x4096")
        g, d = eng.sift_pyramid(mid)
        rg, rd = S.pyramid(mid)
        assert all(np.array_equal(a, b) for o in range(len(rg)) for a, b in zip(g[o] + d[o], rg[o] + rd[o]))
        _check_against(eng, small, rsmall, "small 3")
        rmid = S.sift_detect_describe(mid, None, full=True)
        n = len(rmid[2])
        assert n > 10
        _check_against(eng, mid, rmid, "cap = n", cap=n)
        with pytest.raises(isa.VfsmsError, match=CAPACITY_ERROR):
            eng.sift_detect_describe(mid, cap=n - 1)
        _check_against(eng, mid, rmid, "after the capacity error")
        with pytest.raises(isa.VfsmsError, match=CAPACITY_ERROR):
            eng.sift_detect_describe(mid, cap=0)
        xy, desc = eng.sift_detect_describe(np.full((64, 64), 9, np.uint8), cap=0)
        assert len(xy) == 0 and desc.shape == (0, 128)
        _check_against(eng, small, rsmall, "small 4")
    finally:
        eng.close()


def test_sift_shares_the_context_with_surf(engine):
    """A SURF fused attempt, then SIFT on the same context, then the same SURF attempt: the two SURF rows are equal"""
    rng = np.random.default_rng(23)
    A = _smooth(rng.integers(0, 256, (300, 400), dtype=np.uint8), 3)
    B = np.ascontiguousarray(np.roll(A, (5, -7), (0, 1)))
    ha, hb = engine.tile_upload(A), engine.tile_upload(B)
    try:
        job = [(ha, hb, 20, 20, 20, 20, 200, 300)]
        r1 = engine.attempt_surf_batch(job)
        assert _check(engine, A, label="sift between surf") > 0
        r2 = engine.attempt_surf_batch(job)
        assert np.array_equal(r1, r2)
    finally:
        engine.tile_free(ha); engine.tile_free(hb)


# ---- shape boundaries ------------------------------------------------------------------------------------------------------------
def _octaves_opencv(h, w):
    # OpenCV 3.3.1 with firstOctave = -1: cvRound(log(min(base.cols, base.rows)) / log(2.) - 2) + 1 on the 2x base
    return int(np.rint(np.log2(min(2 * h, 2 * w)) - 2)) + 1


def _shape_cases():
    out = []
    for m in (45, 46, 90, 91, 181, 182, 362, 363):
        out += [(m, m), (m, 2 * m + 7), (3 * m + 1, m)]
    out += [(r, 2048) for r in range(11, 17)] + [(2048, 11), (1, 2048), (2048, 1)]
    return out


@pytest.mark.timeout(900)
def test_sift_shape_boundaries(engine):
    """min side 45 / 46, 90 / 91, 181 / 182, 362 / 363 (where the octave count steps), strips of 11 .. 16 rows (upper octaves inside
    SIFT_BORDER), 2048 x 11, 1 x 2048 and 2048 x 1: the octave count is OpenCV's, the output equals the specification"""
    rng = np.random.default_rng(29)
    steps = {}
    for h, w in _shape_cases():
        img = _smooth(rng.integers(0, 256, (h, w), dtype=np.uint8), 3)
        g, d = engine.sift_pyramid(img)
        assert len(g) == len(d) == _octaves_opencv(h, w), (h, w, len(g))
        steps[min(h, w)] = len(g)
        _check(engine, img, label="%dx%d" % (h, w))
    assert [steps[m] for m in (45, 46, 90, 91, 181, 182, 362, 363)] == [5, 6, 6, 7, 7, 8, 8, 9]


# ---- adversarial content, with the float64 references ------------------------------------------------------------------------------
@pytest.mark.timeout(900)
def test_sift_adversarial_inputs_equal_the_spec_and_float64(engine):
    """Blobs, plateaus, a checkerboard, spikes, the 360 -> 0 reset and removeDuplicated (tests/sift_f64.adversarial_images): the
    device equals the specification, each input reaches the path it was built for, and the device pyramid, refinement and
    orientation peaks agree with the float64 references.  Pyramid: at most 1e-3 grey levels -- float32 taps (each within half an ulp
    of the normalised Gaussian) and float32 sums over up to 8 octaves of 6 blurs leave errors near 1e-4; a wrong sigma schedule or
    tap shifts levels by whole grey levels.  Orientation: every angle in [0, 360), so a peak reported as 360 fails."""
    import sift_f64 as G
    from test_sift_host import check_adversarial_claims
    p = S.Params()
    for name, img in G.adversarial_images():
        _check(engine, img, label=name)
        st = {}
        rg, rd = S.pyramid(img, p)
        n = len(S.detect(rg, rd, p, st))
        check_adversarial_claims(name, n, st)
        g, d = engine.sift_pyramid(img)
        _xy, _desc, kps = engine.sift_detect_describe(img, full=True)
        if name == "reset":
            assert kps["angle"].tolist() == [0.0], kps
        eg, ed = G.pyramid_error(img, g, d)
        ref = G.check_refinement(d, kps)
        ori = G.check_orientation(g, kps)
        print("%s: %d keypoints; float64 max errors: gauss %.2e, dog %.2e, offset %.2e px, size %.2e, response %.2e, angle %.2e deg"
              % (name, len(kps), eg, ed, ref["offset"], ref["size"], ref["response"], ori["angle"]))
        assert eg <= 1e-3 and ed <= 1e-3, name
        assert ref["offset"] <= 1e-3 and ref["size"] <= 1e-5 and ref["response"] <= 1e-5, (name, ref)
        assert ori["angle"] <= 1e-3, (name, ori)


# ---- parameters ----------------------------------------------------------------------------------------------------------------------
def _largest_sigma(L=3):
    """the largest double sigma whose every blur (the initial one and levels 1 .. L + 2, as sift_plan computes them) fits 127 taps"""
    import math

    def fits(s):
        k = math.pow(2.0, 1.0 / L)
        f = np.float32(s)
        sig = [float(np.sqrt(max(f * f - np.float32(1.0), np.float32(0.01)), dtype=np.float32))]
        for i in range(1, L + 3):
            prev = math.pow(k, float(i - 1)) * s
            tot = prev * k
            sig.append(math.sqrt(tot * tot - prev * prev))
        return all(int(np.rint(v * 4 * 2 + 1)) <= 127 for v in sig)
    lo, hi = 1.6, 40.0
    while np.nextafter(lo, np.inf) < hi:
        mid = (lo + hi) / 2
        if mid in (lo, hi):
            mid = float(np.nextafter(lo, np.inf))
        lo, hi = (mid, hi) if fits(mid) else (lo, mid)
    assert fits(lo) and not fits(hi)
    return lo, hi


@pytest.mark.parametrize("kw", [dict(n_octave_layers=1), dict(n_octave_layers=8), dict(contrast_threshold=0.0),
                                dict(edge_threshold=1.01)], ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_sift_parameter_extremes(engine, kw):
    rng = np.random.default_rng(31)
    img = _smooth(rng.integers(0, 256, (96, 160), dtype=np.uint8), 3)
    p = S.Params(**kw)
    g, d = engine.sift_pyramid(img, _params(engine, p))
    rg, rd = S.pyramid(img, p)
    assert all(np.array_equal(a, b) for o in range(len(rg)) for a, b in zip(g[o] + d[o], rg[o] + rd[o]))
    n = _check(engine, img, p, label=str(kw))
    if "edge_threshold" not in kw:
        assert n > 0


def test_sift_largest_blur_and_refusals(engine):
    """the largest sigma whose blurs fit 127 taps equals the spec exactly (pyramid and keypoints); the next double is refused; so are
    layers 0 / 9, sigma 0 / negative / NaN, contrast negative / NaN and edge 0, each leaving the engine usable"""
    import imagestitch_amd as isa
    s_max, s_over = _largest_sigma()
    assert int(np.rint(S.level_sigmas(S.Params(sigma=s_max))[-1] * 8 + 1)) | 1 == 127
    rng = np.random.default_rng(37)
    img = _smooth(rng.integers(0, 256, (64, 96), dtype=np.uint8), 3)
    p = S.Params(sigma=s_max)
    g, d = engine.sift_pyramid(img, _params(engine, p))
    rg, rd = S.pyramid(img, p)
    assert all(np.array_equal(a, b) for o in range(len(rg)) for a, b in zip(g[o] + d[o], rg[o] + rd[o]))
    _check(engine, img, p, label="sigma %.17g" % s_max)
    ok_img = _smooth(rng.integers(0, 256, (80, 120), dtype=np.uint8), 3)
    ref = S.sift_detect_describe(ok_img, None, full=True)
    bad = [dict(sigma=s_over), dict(n_octave_layers=0), dict(n_octave_layers=9), dict(sigma=0.0), dict(sigma=-1.0),
           dict(sigma=float("nan")), dict(contrast_threshold=-0.01), dict(contrast_threshold=float("nan")), dict(edge_threshold=0.0)]
    for kw in bad:
        with pytest.raises(isa.VfsmsError, match=BAD_ARG_ERROR):
            engine.sift_detect_describe(img, engine.sift_params(**kw))
        with pytest.raises(isa.VfsmsError, match=BAD_ARG_ERROR):
            engine.sift_pyramid(img, engine.sift_params(**kw))
        _check_against(engine, ok_img, ref, "after %s" % kw)
