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
