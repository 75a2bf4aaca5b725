"""The orientation kernel in its one-wave-per-keypoint form (-m gpu): k_orientation of csrc/surf_kernels.hip gives every keypoint one
wave (its 113 samples in two rounds, windows 0 .. 63 in that wave) and packs the leftover windows 64 .. 71 of the ORI_K keypoints of a
workgroup into one pass.  Each case requires the engine's keypoints and descriptors to equal the CPU oracle's on the same image: equal
length (a wrong deletion shows here), then array_equal of x, y, size, angle, response, octave, class_id IN ORDER, then array_equal of
the descriptors.  The conditions a case is built for are asserted on the oracle's output alone.

Not reachable from detected keypoints, covered by reading only: the deletion of a keypoint whose gradient wavelet is larger than the
image, and of one with no sample inside (a detected keypoint's own filter fits the image).

Ties of window moduli are planted by sparse images (a few flat rectangles on black): most samples carry a zero gradient, so neighbouring
windows hold the same non-zero samples and their float32 sums are EQUAL.  tests/surf_ori_f32.py, a sequential float32 model of the
reference's sums, tells which windows tie; its angle must equal the oracle's for every keypoint before a tie is believed."""
import numpy as np
import pytest

from imagestitch_amd.synthetic import SyntheticGrid
import surf_f64 as F
import surf_ori_f32 as M

pytestmark = pytest.mark.gpu

N_SAMPLES = 113                # samples of the radius-6 disc

# (seed, blobs) of _blobs -> that many keypoints: every count 1 .. 17, so every residue modulo a workgroup of 2, 4 or 8 keypoints,
# fewer keypoints than one workgroup holds, exactly one and two workgroups, and one more than those
COUNTS = {1: (0, 1), 2: (2, 1), 3: (0, 2), 4: (4, 2), 5: (2, 2), 6: (4, 3), 7: (17, 2), 8: (24, 2), 9: (17, 3), 10: (29, 3),
          11: (24, 3), 12: (9, 4), 13: (18, 4), 14: (17, 4), 15: (0, 5), 16: (24, 4), 17: (30, 5)}


def _rand_img(seed, shape=(90, 150)):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _blobs(seed, n, shape=(90, 150)):
    """a blank image with n Gaussian blobs away from the border"""
    h, w = shape
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.zeros(shape)
    for _ in range(n):
        cy, cx, s = rng.uniform(25, h - 25), rng.uniform(25, w - 25), rng.uniform(3.0, 6.0)
        img += 200.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _border_blobs(shape=(120, 160)):
    """large blobs at the borders and corners of a small image, one small blob in the middle"""
    h, w = shape
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    img = np.full(shape, 20.0)
    for cy, cx, s in [(14, 40, 9), (h - 16, 100, 12), (60, 12, 10), (50, w - 14, 11), (10, 10, 8), (h - 12, w - 12, 10), (60, 80, 6)]:
        img += 180.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2.0 * s * s))
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


def _kp_fields(k):
    return np.stack([k["x"], k["y"], k["size"], k["angle"], k["response"], k["octave"].astype(np.float32), k["class_id"].astype(np.float32)], 1)


def _inside(img, ko):
    """valid orientation samples of each keypoint (tests/surf_f64.py: the disc against the image, from the reported x, y, size)"""
    return F.orientation_samples(img, ko)[3].sum(1)


def _same(engine, img, ko, do, upright=False):
    kxy, desc, kf = engine.surf_detect_describe(img, engine.surf_params(upright=upright), full=True)
    assert len(kf) == len(ko), (img.shape, len(kf), len(ko))
    assert np.array_equal(_kp_fields(kf), _kp_fields(ko)), img.shape
    assert np.array_equal(kxy, np.stack([ko["x"], ko["y"]], 1).reshape(-1, 2))
    assert desc.shape == do.shape and np.array_equal(desc, do), img.shape
    return kf


@pytest.mark.parametrize("count", sorted(COUNTS))
def test_every_keypoint_count_of_the_last_workgroup(engine, oracle, count):
    """1 .. 17 keypoints: the last workgroup of the ROI holds every number of keypoints, the ones behind it none"""
    img = _blobs(*COUNTS[count])
    ko, do = oracle.surf_detect_describe(img)
    assert len(ko) == count
    _same(engine, img, ko, do)


def test_fused_call_with_rois_of_unequal_counts(engine, oracle):
    """one vfsms_features_surf_batch over ROIs of 270, 0, 1, 272, 5, 2 and 11 keypoints and two shapes: the (capacity / ORI_K, ROIs)
    grid, and packed leftover passes whose keypoints are live, beyond the count and mixed.  A feature set holds positions and descriptors
    only (vfsms_features_download): count, order and x, y are compared directly, the angle through the descriptor, whose window turns
    with it; size, response, octave and class_id of these images are compared by the single-ROI tests."""
    imgs = [_rand_img(11), np.full((90, 150), 77, np.uint8), _blobs(*COUNTS[1]), _rand_img(12), _blobs(*COUNTS[5]), _border_blobs(),
            _blobs(*COUNTS[11])]
    want = [oracle.surf_detect_describe(i) for i in imgs]
    assert [len(k) for k, _d in want] == [270, 0, 1, 272, 5, 2, 11]
    hs = [engine.tile_upload(i) for i in imgs]
    feats, counts = engine.features_surf_batch(hs)
    try:
        for j, (f, n, (ko, do)) in enumerate(zip(feats, counts, want)):
            assert n == len(ko), (j, n, len(ko))
            if n == 0:
                continue
            kxy, desc = engine.features_download(f, n)
            assert np.array_equal(kxy, np.stack([ko["x"], ko["y"]], 1)), j
            assert np.array_equal(desc, do), j                 # the descriptor window turns with the angle: a wrong angle shows here
    finally:
        for f in feats:
            if f:
                engine.features_free(f)
        for h in hs:
            engine.tile_free(h)


def test_sample_disc_leaves_the_image(engine, oracle):
    """keypoints with fewer than 113 valid samples: the count over two rounds, the zero gradient of the samples outside"""
    img = _border_blobs()
    ko, do = oracle.surf_detect_describe(img)
    ins = _inside(img, ko)
    assert len(ko) == 2 and ins.min() == 79 and ins.max() == N_SAMPLES, (len(ko), ins)
    _same(engine, img, ko, do)
    img = _rand_img(13)
    ko, do = oracle.surf_detect_describe(img)
    ins = _inside(img, ko)
    assert len(ko) == 270 and (ins < N_SAMPLES).sum() == 100 and ins.min() == 78, (len(ko), (ins < N_SAMPLES).sum(), ins.min())
    assert (ins < 64).sum() == 0 and ((ins > 64) & (ins < N_SAMPLES)).any()       # valid samples in both rounds, fewer than all
    _same(engine, img, ko, do)


def _squares(seed, n=5, shape=(90, 150)):
    """n flat rectangles on black"""
    rng = np.random.default_rng(seed)
    img = np.zeros(shape, np.uint8)
    for _ in range(n):
        y, x, a, b = rng.integers(15, shape[0] - 30), rng.integers(15, shape[1] - 30), rng.integers(3, 14), rng.integers(3, 14)
        img[y:y + a, x:x + b] = rng.integers(120, 256)
    return img


# seed of _squares -> (keypoints, index of a keypoint, the windows that tie for its largest modulus; the first one wins)
TIES = {9: (8, 7, [60, 61, 62, 63, 64, 65]),        # across the seam between the wave's own windows and the packed leftover pass
        5: (17, 12, [0, 70, 71]),                   # window 0 of the wave against two leftover windows
        44: (6, 0, [4, 5, 67, 68]),
        147: (9, 3, [65, 66, 67, 68])}              # among the leftover windows only


@pytest.mark.parametrize("seed", sorted(TIES))
def test_tied_window_moduli_go_to_the_first_window(engine, oracle, seed):
    n, idx, windows = TIES[seed]
    img = _squares(seed)
    ko, do = oracle.surf_detect_describe(img)
    assert len(ko) == n
    S = M.integral(img)
    own = 0
    for j, k in enumerate(ko):
        o = M.orientation(S, k["x"], k["y"], k["size"])
        assert o is not None and o["angle"] == k["angle"], (j, o and o["angle"], k["angle"])        # the model is the oracle's arithmetic
        t = M.ties(o)
        own += len(t) > 1 and t[-1] < 64
        if j == idx:
            assert t == windows and o["best"] == windows[0], (t, o["best"])
    print("seed %d: %d keypoints, %d more with a tie among windows 0 .. 63" % (seed, n, own))
    _same(engine, img, ko, do)


@pytest.mark.parametrize("count", [1, 5, 270])
def test_upright_sets_270_without_window_sums(engine, oracle, count):
    img = _rand_img(11) if count == 270 else _blobs(*COUNTS[count])
    ko, do = oracle.surf_detect_describe(img, upright=True)
    assert len(ko) == count and np.all(ko["angle"] == 270.0)
    kf = _same(engine, img, ko, do, upright=True)
    assert np.all(kf["angle"] == 270.0)


@pytest.fixture(scope="module")
def tile0():
    return SyntheticGrid(10, 9, 2048).tile(0)


@pytest.mark.parametrize("name", ["strip_409x2048", "strip_2048x409"])
def test_production_strip(engine, oracle, tile0, name):
    """the strip shapes of the headline grid"""
    img = np.ascontiguousarray(tile0[-409:, :] if name == "strip_409x2048" else tile0[:, -409:])
    ko, do = oracle.surf_detect_describe(img)
    assert len(ko) > 8000
    _same(engine, img, ko, do)
