"""Small inputs for the float64 SURF checks (tests/surf_f64.py), each named for what it reaches.

    case        image                      parameters               Hessian kernels                              descriptor kernels
    noise       noise 90 x 150             stock                    lds<1>, lds<2> (octaves 2, 3: no keypoints)  k_describe_small, k_describe
    strip       grid tile, last 128 rows   stock                    lds<1>, lds<2>, rows2 (octave 3: no keypoint) k_describe_small, k_describe
    crop        grid tile 200 x 333        stock                    lds<1>, lds<2>, rows2, coarse                k_describe_small, k_describe
    blobs       Gaussian blobs 420 x 420   stock                    lds<1>, lds<2>, rows2, coarse (all 12 cells) both, all four window classes, all borders
    thin        noise 40 x 700             stock                    lds<1> only has room (octave 0)              k_describe_small
    strided     crop inside a wider array  stock                    as crop, row stride 640                      as crop
    extended    blobs                      extended=True            as blobs                                     both, 128-d
    upright     crop                       upright=True             as crop                                      both, axis-aligned window, no orientation
    generic     crop                       n_octaves=3, n_layers=4  k_hessian (6 layers per octave)              both
    hessian400  crop                       hessian=400              as crop                                      both

"stock" is hessian 100, 4 octaves, 3 layers, 64-d, oriented.  k_describe_small serves windows of at most 64 px, k_describe the three
larger classes (> 64, > 128, > 256 px).  The stock pyramid runs k_hessian_lds<1> on octave 0, k_hessian_lds<2> on octave 1,
k_hessian_rows2 on octave 2 and k_hessian_coarse on octave 3; any other layer count runs the generic k_hessian on every octave.  Every
stock case launches all four; the table lists a kernel where its octave gives the case keypoints, so that its output is checked."""
import functools

import numpy as np

STOCK = dict(hessian=100.0, n_octaves=4, n_layers=3, extended=False, upright=False)
BLOB_SIDE = 420


@functools.lru_cache(maxsize=None)
def _tiles():
    from imagestitch_amd.synthetic import SyntheticGrid
    return SyntheticGrid(2, 2, 640).tiles(threads=1)


def _noise(seed, shape):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _crop():
    return np.ascontiguousarray(_tiles()[1][:200, :333])


def _strided():
    wide = np.zeros((200, 640), np.uint8)
    wide[:] = _tiles()[1][:200, :]
    v = wide[:, :333]
    assert v.strides == (640, 1)
    return v


# (y, x, sigma, amplitude) of the eleven large blobs.  Three keypoints in each octave-3 cell need nine extrema of 120 to 264 px
# within the central 140 to 240 px that the layers' margins leave; blobs that large overlap and move each other's maxima, so these
# were tuned by a hill climb on the oracle's keypoint counts, starting from sigma = size * 1.2 / 9 of the three octave-3 layers.
LARGE_BLOBS = (
    (203.61, 144.71, 17.491, 71.60), (209.70, 115.06, 25.448, -69.32), (172.66, 308.10, 34.786, 65.38), (153.94, 193.58, 30.746, 58.47),
    (261.01, 246.46, 23.428, -66.07), (170.44, 325.26, 43.418, -85.39), (301.43, 158.77, 19.745, -54.64), (301.19, 277.31, 26.022, -72.10),
    (165.51, 111.84, 25.400, 95.00), (288.40, 219.75, 44.094, 84.39), (322.72, 271.56, 38.839, 44.01))


@functools.lru_cache(maxsize=None)
def blobs(side=BLOB_SIDE, seed=7):
    """Gaussian blobs on a flat ground plus 2 grey levels of noise: sigma = size * 1.2 / 9 for every middle layer of octaves 0 to 2
    at random places where that layer can hold a maximum, LARGE_BLOBS for octave 3, and a band of small and middle blobs along each
    border at the distance where the keypoint is still found but its descriptor window reaches past the border."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:side, 0:side].astype(np.float64)
    img = np.full((side, side), 110.0)

    def put(cy, cx, sig, amp):
        img[:] += amp * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * sig * sig))

    sign = 1
    for o in range(3):
        for l in range(1, 4):
            size = (9 + 6 * l) << o
            lo = ((9 + 6 * (l + 1)) << o) // 2 + 2 * (1 << o)           # room for the layer above, plus the NMS frame
            for _ in range((8, 6, 4)[o]):
                sign = -sign
                put(rng.uniform(lo, side - lo), rng.uniform(lo, side - lo), size * 1.2 / 9, sign * rng.uniform(50, 90))
    nb = 12
    for border in range(4):                                               # left, right, top, bottom
        for k in range(nb):
            o, l = (0, 1 + k % 3) if k % 2 else (1, 1 + (k // 2) % 3)
            size = (9 + 6 * l) << o
            d = rng.uniform(0.62 * size + 4 * (1 << o), 1.2 * size)       # found, and the 2.8 size window crosses
            t = 20 + (side - 40) * (k + rng.uniform(0.2, 0.8)) / nb
            cy, cx = ((t, d), (t, side - 1 - d), (d, t), (side - 1 - d, t))[border]
            sign = -sign
            put(cy, cx, size * 1.2 / 9, sign * rng.uniform(50, 90))
    img += rng.normal(0, 2, img.shape)
    for cy, cx, sig, amp in LARGE_BLOBS:
        put(cy, cx, sig, amp)
    return np.clip(np.rint(img), 0, 255).astype(np.uint8)


CASES = {
    "noise": (lambda: _noise(4, (90, 150)), {}),
    "strip": (lambda: np.ascontiguousarray(_tiles()[0][-128:, :]), {}),
    "crop": (_crop, {}),
    "blobs": (blobs, {}),
    "thin": (lambda: _noise(3, (40, 700)), {}),
    "strided": (_strided, {}),
    "extended": (blobs, dict(extended=True)),
    "upright": (_crop, dict(upright=True)),
    "generic": (_crop, dict(n_octaves=3, n_layers=4)),
    "hessian400": (_crop, dict(hessian=400.0)),
}
NAMES = tuple(CASES)


def case(name):
    """-> (image, full parameter dict)"""
    fn, kw = CASES[name]
    p = dict(STOCK)
    p.update(kw)
    return fn(), p


def layer_cell(kps, n_layers=3):
    """(octave, middle layer) of each keypoint: the middle layer whose size is nearest the interpolated size"""
    o = kps["octave"].astype(np.int64)
    sizes = np.stack([(9 + 6 * l) * (1 << o) for l in range(1, n_layers + 1)], 1)
    return o, 1 + np.abs(sizes - kps["size"][:, None]).argmin(1)
