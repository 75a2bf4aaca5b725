"""Inputs and parameter sets of the ORB tests (host: reference against oracle; device: engine against reference), by name.
Reference results are cached per process: the host and the GPU suite compute each one once."""
import functools
import os

import numpy as np

import orb_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT = dict(nfeatures=5000, scale_factor=1.2, nlevels=8, edge_threshold=31, first_level=0, patch_size=31, fast_threshold=20)


def smooth(img, k=3):
    f = img.astype(np.float64)
    for ax in (0, 1):
        f = sum(np.roll(f, s, axis=ax) for s in range(-(k // 2), k // 2 + 1)) / k
    return np.clip(np.rint(f), 0, 255).astype(np.uint8)


def texture(h, w, seed=0, k=3):
    return smooth(np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8), k)


def lattice(h, w, period, start=0, fg=220, bg=40):
    """isolated bright pixels every `period` px: every one is a FAST corner of one score, so every keypoint ties"""
    img = np.full((h, w), bg, np.uint8)
    img[start::period, start::period] = fg
    return img


def binary_blocks(h, w, block=16):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((yy // block) + (xx // block)) % 2 * 255).astype(np.uint8)


def wedges(h=160, w=160):
    """a bright pixel with a dimmer neighbour to its right / below / left / above on a flat background: the patch is symmetric about one
    axis, so m01 = 0 or m10 = 0 (angles exactly 0, 90, 180, 270); a lone pixel gives m01 = m10 = 0 (fastAtan2(0, 0))"""
    img = np.full((h, w), 30, np.uint8)
    nb = [(0, 1), (1, 0), (0, -1), (-1, 0), None]
    k = 0
    for cy in range(40, h - 39, 40):
        for cx in range(40, w - 39, 40):
            img[cy, cx] = 250
            if nb[k % 5]:
                img[cy + nb[k % 5][0], cx + nb[k % 5][1]] = 120
            k += 1
    return img


def near_extreme(seed, h=256, w=384):
    """most pixels within 20 of 0, a sparse smoothed bright pattern: centres where v - threshold < 0 (the clipped threshold table)"""
    rng = np.random.default_rng(seed)
    dark = rng.integers(0, 21, (h, w))
    bright = smooth(rng.integers(0, 256, (h, w), dtype=np.uint8), 5) > 150
    return np.where(bright, rng.integers(200, 256, (h, w)), dark).astype(np.uint8)


def real_strip(name="p4_a"):
    return np.load(os.path.join(GOLDEN, "real_full_strips.npz"))[name]


def real_path_strips(k=4):
    z = np.load(os.path.join(GOLDEN, "real_path_strips.npz"))
    names = sorted(z.keys())[:: max(len(z.keys()) // k, 1)][:k]
    return [(n, z[n]) for n in names]


def params(**kw):
    p = dict(DEFAULT)
    p.update(kw)
    return p


# ---- named cases: (image factory, parameters) --------------------------------------------------------------------------------------------
def _cases():
    c = {}
    c["tex409x2048"] = (lambda: texture(409, 2048, 1), params())
    c["tex2048x409"] = (lambda: texture(2048, 409, 2), params())
    c["tex204x2048"] = (lambda: texture(204, 2048, 3), params())
    c["real387x2584"] = (lambda: real_strip("p4_a"), params())
    c["real1936x516"] = (lambda: real_strip("p15_b"), params())
    for n, img in real_path_strips():
        c["path_" + n] = ((lambda im=img: im), params())
    c["flat"] = (lambda: np.full((409, 2048), 128, np.uint8), params())
    c["binary_blocks"] = (lambda: binary_blocks(409, 2048), params())
    for p in (8, 12, 16):
        c["lattice%d" % p] = ((lambda p=p: lattice(409, 2048, p, 3)), params())
    c["near0"] = (lambda: near_extreme(4), params())
    c["near255"] = (lambda: 255 - near_extreme(5), params())
    c["wedges"] = (wedges, params(nlevels=1))
    c["border_lattice"] = (lambda: lattice(128, 160, 8, 31), params(nlevels=1))     # pixels on x, y = 31: exactly at the border distance
    small = lambda: texture(256, 384, 6)
    for nf in (1, 7, 10, 300, 20000):
        c["nfeatures%d" % nf] = (small, params(nfeatures=nf))
    for nl in (1, 2):
        c["nlevels%d" % nl] = (small, params(nlevels=nl))
    for sf in (1.05, 1.5, 2.0):
        c["scale%g" % sf] = ((lambda: texture(409, 600, 7)), params(scale_factor=sf))
    for ps in (31, 30, 15, 2):
        for e in sorted({ps // 2 + 1, 31}):
            c["patch%d_edge%d" % (ps, e)] = (small, params(patch_size=ps, edge_threshold=e))
    c["patch31_edge17"] = (small, params(edge_threshold=17))
    for t in (0, 1, 254):
        c["fast%d" % t] = (small, params(fast_threshold=t))
    return c


CASES = _cases()
# the reads that leave their level when the edge threshold is small (the reference samples the reflect-101 extension)
SMALL_EDGE = ["patch31_edge16", "patch31_edge17", "patch2_edge2"]


@functools.lru_cache(maxsize=None)
def image(name):
    img = CASES[name][0]()
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (keypoints, descriptors, stats with the pyramid and blurred levels) of case `name`"""
    return R.detect_describe(image(name), stats=True, levels_out=True, **CASES[name][1])
