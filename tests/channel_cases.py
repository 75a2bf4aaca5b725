"""Seeded inputs with 2 and 4 channels for every operator whose C ABI takes ch 1..4, shared by tests/test_channel_counts_host.py (which states,
with the references alone, what the cases contain) and tests/test_channel_counts_gpu.py (which holds the kernels to the references on them).
No GPU and nothing from the library: numpy only, the oracle is handed in by the caller.

The int64 regions follow the reference's representation: -1 = empty, and an empty PIXEL has every channel -1 (the sum of its channels is -ch).
A pixel that is black in one channel only (0 there, grey elsewhere) is valid; the fill-ins work on it element by element."""
import functools

import numpy as np

import canvas_cases as cc

CHANNELS = (2, 4)


def old_rule_valid(X):
    """the validity plane as the rule stood before it was stated for any channel count: the reference's BGR test, literally"""
    X = np.asarray(X, np.int64)
    return X.sum(axis=2) != -3


def region(seed, r, c, ch, part=None, dots=0.0, black=0.05, levels=256):
    """int64 regions A, B (r x c x ch) from one stream: `levels` grey levels; `black` of the elements 0 in that channel only; with `part` (tl, tr,
    bl, br) A is valid only on the 3/4 x 3/4 rectangle in that corner (56 %: corner mode, as canvas_cases._corner without bars leaves a ROI);
    `dots` of A's and of B's pixels empty in every channel"""
    rng = np.random.default_rng([seed, r, c, ch])
    A = rng.integers(0, levels, (r, c, ch)).astype(np.int64); B = rng.integers(0, levels, (r, c, ch)).astype(np.int64)
    A[rng.random((r, c, ch)) < black] = 0
    B[rng.random((r, c, ch)) < black] = 0
    if part is not None:
        a, b = max(1, (3 * r) // 4), max(1, (3 * c) // 4)
        keep = np.zeros((r, c), bool)
        keep[(slice(0, a) if part[0] == "t" else slice(r - a, r)), (slice(0, b) if part[1] == "l" else slice(c - b, c))] = True
        A[~keep] = -1
    if dots:
        A[rng.random((r, c)) < dots] = -1
        B[rng.random((r, c)) < dots] = -1
    A.setflags(write=False); B.setflags(write=False)
    return A, B


# ---- fade, trigonometric, ramps, multiband ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fuse_cases(ch):
    """(name, A, B, dx, dy): strips of both kinds with scattered empty pixels and both signs of the offset, the four corner patterns, and sizes
    on both sides of one workgroup's 256 columns"""
    out = []
    k = 0
    for (r, c) in ((40, 17), (17, 40), (33, 300), (300, 33), (1, 7), (7, 1)):
        for dx, dy in ((5, 7), (-5, -7)):
            A, B = region(100 + k, r, c, ch, dots=0.04 if r * c > 7 else 0.0)
            out.append(("strip %dx%d (%d, %d)" % (r, c, dx, dy), A, B, dx, dy)); k += 1
    for (r, c) in ((40, 50), (17, 261)):
        for part in ("tl", "tr", "bl", "br"):
            dx, dy = cc._SIGNS[k % len(cc._SIGNS)]
            A, B = region(100 + k, r, c, ch, part=part, dots=0.02)
            out.append(("corner %s %dx%d" % (part, r, c), A, B, dx, dy)); k += 1
    return tuple(out)


# ---- seam ----------------------------------------------------------------------------------------------------------------------------------------
SEAM_WIDTHS = (1, 64, 65, 257)
SEAM_ROWS = 40
SEAM_TOO_LONG = (2 ** 31 // 5100 + 1, 1)            # 5100 * 421076 > 2^31 - 1: 6.7 MB of int64 per channel pair, small enough to upload


def max_energy_region(ch):
    """A and B opposite 0 / 255 checkerboards in every channel, the squares two pixels wide: d = A - B is +-255, and two pixels on, along a row
    or a column, it has the other sign, so both central differences are 510 and E = 1275 ch in the interior: 5100 at ch = 4, the top of the
    uint16 energy plane.  (One-pixel squares would give central differences of 0.)  40 x 33, a strip of kind 1."""
    i, j = np.mgrid[0:40, 0:33]
    s = ((i >> 1) + (j >> 1)) & 1
    A = np.repeat((255 * s)[:, :, None], ch, axis=2).astype(np.int64)
    B = 255 - A
    A.setflags(write=False); B.setflags(write=False)
    return A, B


@functools.lru_cache(maxsize=None)
def seam_cases(ch):
    """(name, A, B, dx, dy): the widths on 40 rows (width 1: kind 1, the others: kind 2 with 40 positions), two kind-1 strips whose seam has 65
    and 257 positions, one corner-mode region and the max-energy region"""
    out = []
    for k, w in enumerate(SEAM_WIDTHS):
        A, B = region(200 + k, SEAM_ROWS, w, ch, dots=0.05, levels=(4, 256)[k % 2])
        out.append(("%dx%d" % (SEAM_ROWS, w), A, B, (2, -2)[k % 2], (3, -3)[k % 2]))
    for k, w in enumerate((65, 257)):
        A, B = region(210 + k, w + 3, w, ch, dots=0.05, levels=(256, 4)[k % 2])
        out.append(("%dx%d" % (w + 3, w), A, B, (-2, 2)[k % 2], (-3, 3)[k % 2]))
    A, B = region(220, 40, 50, ch, part="br", dots=0.02, levels=7)
    out.append(("corner br 40x50", A, B, 4, -6))
    A, B = max_energy_region(ch)
    out.append(("max energy 40x33", A, B, 1, 1))
    return tuple(out)


# ---- the mosaic canvas -----------------------------------------------------------------------------------------------------------------------------
ROI_WIDTHS = (1, 4, 5, 256, 257, 513)               # of canvas_cases.ROI_WIDTHS
ROI_HEIGHTS = (1, 16, 17, 65)                       # of canvas_cases.ROI_HEIGHTS
TILE_WIDTHS = (5, 1027)                             # of canvas_cases.TILE_WIDTHS
_THIN = ((1, 5, "l"), (1, 257, "r"), (33, 1, "t"), (1, 1, "none"), (3, 3, "none"))
_THIN_RAISES = ((2, 300, "none"), (64, 2, "t"))     # of canvas_cases._THIN_RAISES: getWeightsMatrix divides by zero


@functools.lru_cache(maxsize=None)
def edge_canvases(ch):
    """the edge layouts of canvas_cases.edge_canvases rebuilt with `ch` channels, a subset: strips at the listed ROI widths and heights, tall
    strips, one corner per quadrant in the one-, two- and four-wave layouts of the statistics kernel, the tile widths with a second column
    block and narrower than two quads, ROI edges inside a lane's quad, the canvas border, thin corner ROIs"""
    out = []
    for k, c in enumerate(ROI_WIDTHS):
        r = ROI_HEIGHTS[k % len(ROI_HEIGHTS)]
        out.append(cc._strip("strip %dx%d" % (r, c), r, c, True, k, ch=ch))
    for k, (r, c) in enumerate([(65, 4), (17, 16), (16, 17)]):
        out.append(cc._strip("strip %dx%d" % (r, c), r, c, True, k + 1, ch=ch))
    k = 0
    for (r, c) in ((65, 256), (17, 257), (16, 513)):
        for part in ("tl", "tr", "bl", "br"):
            out.append(cc._corner("corner %s %dx%d" % (part, r, c), r, c, part, True, k, origin=(k % 2, 1 + k % 4), ch=ch))
            k += 1
    out.append(cc._corner("block br 65x257", 65, 257, "br", True, k, bars=False, origin=(2, 2), ch=ch))
    out.append(cc._strip("tile width 1027", 33, 1025, True, 1, margins=(0, 2, 1, 0), origin=(1, 2), ch=ch))
    out.append(cc._strip("tile width 1027 left", 16, 1024, True, 2, margins=(2, 0, 0, 3), origin=(0, 1), ch=ch))
    out.append(cc._strip("tile width 5", 15, 3, True, 3, margins=(1, 1, 1, 1), origin=(0, 1), ch=ch))
    out.append(cc._strip("tile width 5 whole", 4, 5, True, 4, margins=(0, 0, 0, 0), origin=(1, 2), ch=ch))
    for k, (lo, hi) in enumerate(((1, 2), (2, 3), (3, 1))):
        c = 4 * 40 + hi - lo
        out.append(cc._strip("quad strip %d %d" % (lo, hi), 17, c, True, k, margins=(1, lo, 1, 8 - hi), origin=(1, k % 4), ch=ch))
    whole = (0, 0, 65, 257)
    out.append(cc._case("border strip", [whole, whole], [None, whole[:2] + (65, 257)], [(3, -4)], True, ch=ch))
    out.append(cc._case("border corner", [(0, 0, 50, 200), whole], [None, (0, 0, 65, 257)], [(-3, 4)], True, ch=ch))
    out += [cc._thin(r, c, part, True, k, ch=ch) for k, (r, c, part) in enumerate(_THIN)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_verdict_only(ch):
    """shapes on which the reference itself raises: the library must refuse them"""
    return tuple(cc._thin(r, c, part, True, k, ch=ch) for k, (r, c, part) in enumerate(_THIN_RAISES))


def paste_walk(tiles, geom, rows, cols):
    """every tile pasted in order, nothing fused; never-written pixels 0"""
    cv = np.zeros((rows, cols) + tiles[0].shape[2:], np.uint8)
    for t, g in zip(tiles, geom):
        cv[g[0]:g[0] + t.shape[0], g[1]:g[1] + t.shape[1]] = t
    return cv


@functools.lru_cache(maxsize=None)
def multiband_layout(ch):
    """a 2 x 2 layout of 48 x 64 tiles with overlaps of a quarter -> (rows, cols, tiles, geom) with mode 6 (multiBandBlending) rows: the second
    tile meets the first in a tall strip, the third in a wide one, the fourth lies in the L of the three (a corner ROI)"""
    rng = np.random.default_rng([7, ch])
    th, tw = 48, 64
    at = [(0, 2), (3, 2 + tw - 16), (th - 12, 0), (th - 10, tw - 18)]
    tiles = [rng.integers(0, 256, (th, tw, ch), dtype=np.uint8) for _ in at]
    for t in tiles:
        t[rng.random(t.shape) < 0.05] = 0
        t.setflags(write=False)
    rows = max(y for y, _ in at) + th; cols = max(x for _, x in at) + tw
    geom, bbox = [], None
    for k, (y0, x0) in enumerate(at):
        if k == 0:
            geom.append((y0, x0, 0, 0, 0, 0, 0, 0, cc.PASTE))
            bbox = [y0, x0, y0 + th, x0 + tw]
            continue
        roi = (max(y0, bbox[0]), max(x0, bbox[1]), min(y0 + th, bbox[2]), min(x0 + tw, bbox[3]))
        geom.append((y0, x0) + roi + (y0 - at[k - 1][0], x0 - at[k - 1][1], 6))
        bbox = [min(bbox[0], y0), min(bbox[1], x0), max(bbox[2], y0 + th), max(bbox[3], x0 + tw)]
    geom = np.array(geom, np.int32)
    geom.setflags(write=False)
    return rows, cols, tiles, geom


def reference_fuse_walk(tiles, geom, rows, cols, fuse):
    """Stitcher.getStitchByOffset's walk (Stitcher.py:434-486) on the reference's int64 / -1 canvas: fuse(A, B, dx, dy) -> the ROI's bytes, A
    the canvas under the ROI before the paste, B the tile's part -> (canvas bytes, the (A, B, dx, dy) it fused)"""
    cv = np.zeros((rows, cols) + tiles[0].shape[2:], np.int64) - 1
    fused = []
    for t, g in zip(tiles, geom):
        y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
        A = cv[ry0:ry1, rx0:rx1].copy()
        cv[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
        if mode != cc.PASTE and A.size:
            B = cv[ry0:ry1, rx0:rx1].copy()
            cv[ry0:ry1, rx0:rx1] = fuse(A, B, dx, dy)
            fused.append((A, B, dx, dy))
    cv[cv == -1] = 0
    return cv.astype(np.uint8), fused


# ---- tiles for the per-tile operators ---------------------------------------------------------------------------------------------------------
def tiles_u8(seed, n, shape):
    rng = np.random.default_rng([seed] + list(shape))
    out = [rng.integers(0, 256, shape, dtype=np.uint8) for _ in range(n)]
    for t in out:
        t.setflags(write=False)
    return out


SHADING_SHAPES = ((5, 7), (33, 130))
SHADING_RADII = (1, 3, 40)
# the horizontal box pass stages min(1024, w ch - x0) + 2 R ch samples per workgroup in an LDS segment of 1024 + 2 * 127 * 4 = 2040: exactly
# full at ch = 4, R = 127 and a row of at least 1024 samples; at ch = 2 the same radius fills 1532 of it
SHADING_CAPACITY = {4: (3, 257, 4), 2: (3, 513, 2)}
SHADE_SEG, SHADE_LDS = 1024, 1024 + 2 * 127 * 4


def shading_staged(shape, R):
    """samples the first workgroup of a row of the horizontal pass stages"""
    h, w, ch = shape
    return min(SHADE_SEG, w * ch) + 2 * R * ch


LENS_SHAPES = ((1, 1), (5, 7), (33, 130))
EXPOSURE_SHAPE = (40, 60)
EXPOSURE_OFFSETS = ((0, 0), (2, 3), (2, -3), (-2, 3), (-2, -3), (0, 3), (0, -3), (2, 0), (-2, 0), (39, 59), (-39, -59), (40, 0), (0, -60))
