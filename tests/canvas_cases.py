"""Deterministic mosaic-canvas cases and their reference walks, shared by tests/test_canvas_cases_host.py (which states, with the oracle alone,
what the cases contain) and tests/test_canvas_reference_gpu.py (which holds the canvas kernels of csrc/fuse_kernels.hip to the reference on
them).  No GPU and nothing from the library: numpy only, the oracle is handed in by the caller.

A case is (rows, cols, tiles, geom): the canvas size, the tiles (uint8, h x w or h x w x 3) and one 9-int row per tile as
Engine.canvas_assemble_resident takes it: y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode.  Every fused row carries mode FADE; with_mode() swaps
the operator."""
import functools
from collections import namedtuple

import numpy as np

PASTE, FADE, TRIG, AVERAGE, MAXIMUM, MINIMUM = -1, 0, 1, 2, 3, 4

# the values the edge list must contain (tests/test_canvas_cases_host.py checks that each occurs)
ROI_WIDTHS = (1, 2, 3, 4, 5, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1029)      # wx_n switch (256, 512), one workgroup's columns, the quad
ROI_HEIGHTS = (1, 15, 16, 17, 33, 63, 64, 65)                                           # FUSE_SB = 16; 1 x 4, 2 x 2, 4 x 1 workgroup heights
TILE_WIDTHS = (5, 1025, 1027)                                                           # second column block of k_fuse_apply, its nk < 4 tail

EdgeCase = namedtuple("EdgeCase", "name rows cols tiles geom")


def layout_of(c):
    """the wave layout of the statistics kernel for a ROI of c columns: wx_n = 1, 2 or 4"""
    return 1 if c <= 256 else 2 if c <= 512 else 4


def with_mode(geom, mode):
    g = np.array(geom, np.int32).reshape(-1, 9)
    g[g[:, 8] != PASTE, 8] = mode
    return g


# ---- random canvases -----------------------------------------------------------------------------------------------------------------------------
def random_canvases(seed, n=40, colour=False):
    """The generator of test_random_placements_fused_from_the_rectangle_list_equal_the_statistics_path (tests/test_gpu_parity.py), draw for draw:
    tiles dropped left of, above, below and across earlier ones, ROI = tile rectangle cut by the bounding box of what lies there
    (Stitcher.py:446-457) or, every third canvas, a random sub-rectangle of the tile; every fifth canvas with 30 % black pixels.  (That test
    also draws fade or trigonometric per tile: the draw is made and dropped, rows carry FADE.)  Added from a second stream, so that the
    first one and with it the geometry stay as they were: every fifth canvas (case % 5 == 1) with 30 % saturated pixels, and for colour=True
    two more channels per tile with the same shares, zero and saturated element by element (a pixel may be black in one channel only: the
    fill-in of average / maximum / minimum works per element, Stitcher.py:498-504).
    Yields (rows, cols, tiles, geom)."""
    rng = np.random.default_rng(seed)
    extra = np.random.default_rng([seed, 1])
    for case in range(n):
        rows, cols = int(rng.integers(500, 900)), int(rng.integers(500, 900))
        ntile = int(rng.integers(3, 8))
        tiles, geom = [], []
        bbox = None
        for k in range(ntile):
            th, tw = int(rng.integers(90, 320)), int(rng.integers(90, 320))
            y0, x0 = int(rng.integers(0, rows - th)), int(rng.integers(0, cols - tw))
            t = rng.integers(0, 256, (th, tw), dtype=np.uint8)
            if case % 5 == 0:
                t[rng.random((th, tw)) < 0.3] = 0                            # black pixels: the quadrant counts are not the valid areas
            if colour:
                t = np.stack([t, extra.integers(0, 256, (th, tw), dtype=np.uint8), extra.integers(0, 256, (th, tw), dtype=np.uint8)], -1)
                if case % 5 == 0:
                    t[:, :, 1:][extra.random((th, tw, 2)) < 0.3] = 0
            if case % 5 == 1:
                t[extra.random(t.shape) < 0.3] = 255
            t = np.ascontiguousarray(t)
            t.setflags(write=False)
            tiles.append(t)
            if bbox is None:
                geom.append((y0, x0, 0, 0, 0, 0, 0, 0, PASTE))
                bbox = [y0, x0, y0 + th, x0 + tw]
                continue
            if case % 3 == 2:                                                    # any sub-rectangle of the tile
                ry0 = y0 + int(rng.integers(0, th // 2)); rx0 = x0 + int(rng.integers(0, tw // 2))
                ry1 = int(rng.integers(ry0 + 2, y0 + th + 1)); rx1 = int(rng.integers(rx0 + 2, x0 + tw + 1))
            else:
                ry0, rx0, ry1, rx1 = max(y0, bbox[0]), max(x0, bbox[1]), min(y0 + th, bbox[2]), min(x0 + tw, bbox[3])
            if ry1 <= ry0 or rx1 <= rx0:
                geom.append((y0, x0, 0, 0, 0, 0, 0, 0, PASTE))
            else:
                dx, dy, _method = int(rng.integers(-40, 41)), int(rng.integers(-40, 41)), int(rng.integers(0, 2))
                geom.append((y0, x0, ry0, rx0, ry1, rx1, dx, dy, FADE))
            bbox = [min(bbox[0], y0), min(bbox[1], x0), max(bbox[2], y0 + th), max(bbox[3], x0 + tw)]
        geom = np.array(geom, np.int32)
        geom.setflags(write=False)
        yield rows, cols, tiles, geom


# the seeds both test files use (tests/test_canvas_cases_host.py holds them to the shares the GPU test relies on), 40 canvases each
RANDOM_SEEDS = {False: 20190158, True: 2}
_random = {}


def random_cases(colour):
    """the 40 canvases of the gray / colour seed as a list, generated once per process"""
    if colour not in _random:
        _random[colour] = list(random_canvases(RANDOM_SEEDS[colour], 40, colour))
    return _random[colour]


# ---- edge canvases -------------------------------------------------------------------------------------------------------------------------------
def _pixels(rng, th, tw, colour, ch=None):
    """mid greys with 5 % black and 5 % saturated elements; ch: that many channels instead of colour's 1 or 3"""
    shape = (th, tw, ch) if ch is not None else (th, tw, 3) if colour else (th, tw)
    t = rng.integers(1, 255, shape, dtype=np.uint8)
    u = rng.random(shape)
    t[u < 0.05] = 0
    t[u > 0.95] = 255
    t.setflags(write=False)
    return t


def _case(name, rects, rois, dxdy, colour, origin=(0, 0), pad=(0, 0), ch=None):
    """rects: (y0, x0, h, w) per tile in any coordinates (shifted so that the smallest becomes `origin`); rois[k] for tile k >= 1: (ry0, rx0,
    ry1, rx1) in the same coordinates, or None for Stitcher.py:446-457's cut by the bounding box of the earlier tiles.  pad: empty canvas rows /
    columns behind the last tile.  ch (tests/channel_cases.py): tiles of that many channels from a stream of their own; None leaves every draw
    of the gray and colour cases as it was."""
    rng = np.random.default_rng([len(rects), int(colour) if ch is None else 16 + ch] + [int(v) & 0xffff for r in rects for v in r])
    sy = origin[0] - min(r[0] for r in rects); sx = origin[1] - min(r[1] for r in rects)
    tiles, geom, bbox = [], [], None
    for k, (y0, x0, h, w) in enumerate(rects):
        tiles.append(_pixels(rng, h, w, colour, ch))
        if k == 0:
            geom.append((y0 + sy, x0 + sx, 0, 0, 0, 0, 0, 0, PASTE))
            bbox = [y0, x0, y0 + h, x0 + w]
            continue
        roi = rois[k] if rois[k] is not None else (max(y0, bbox[0]), max(x0, bbox[1]), min(y0 + h, bbox[2]), min(x0 + w, bbox[3]))
        assert roi[2] > roi[0] and roi[3] > roi[1] and y0 <= roi[0] and x0 <= roi[1] and roi[2] <= y0 + h and roi[3] <= x0 + w, (name, k, roi)
        dx, dy = dxdy[(k - 1) % len(dxdy)]
        geom.append((y0 + sy, x0 + sx, roi[0] + sy, roi[1] + sx, roi[2] + sy, roi[3] + sx, dx, dy, FADE))
        bbox = [min(bbox[0], y0), min(bbox[1], x0), max(bbox[2], y0 + h), max(bbox[3], x0 + w)]
    rows = max(r[0] + r[2] for r in rects) + sy + pad[0]; cols = max(r[1] + r[3] for r in rects) + sx + pad[1]
    assert rows * cols <= 1500000, (name, rows, cols)
    geom = np.array(geom, np.int32)
    geom.setflags(write=False)
    return EdgeCase(name, rows, cols, tiles, geom)


_SIGNS = ((7, -3), (-5, 9), (0, 0), (4, 4), (-6, -2))


def _strip(name, r, c, colour, k, margins=None, origin=None, ch=None):
    """two tiles, the ROI (r x c, margins (top, left, bottom, right) inside the second tile) fully covered by the first"""
    mt, ml, mb, mr = margins if margins is not None else (k % 3, 1 + k % 4, (k + 1) % 3, (k + 2) % 4)
    oy, ox = origin if origin is not None else (k % 2, 1 + k % 3)            # second tile's x0 = 5 + ox: 6, 7 or 8 (x0 % 4 of 2, 3, 0)
    second = (3, 5, mt + r + mb, ml + c + mr)
    roi = (3 + mt, 5 + ml, 3 + mt + r, 5 + ml + c)
    first = (0, 0, roi[2], roi[3])
    return _case(name, [first, second], [None, roi], [_SIGNS[k % len(_SIGNS)]], colour, origin=(oy, ox), pad=(k % 2, k % 3), ch=ch)


def _corner(name, r, c, part, colour, k, bars=True, margins=(1, 2, 2, 1), origin=(1, 3), ch=None):
    """the last tile's ROI (r x c) with only its `part` (tl, tr, bl, br) valid.  bars: three tiles -- a horizontal bar over the top / bottom
    35 % of the rows and a vertical bar over the left / right 35 % of the columns, both running out of the ROI (the L a mosaic's turn leaves:
    58 % valid); else two tiles, the first covering 75 % x 75 % of the ROI from that corner (56 %)."""
    mt, ml, mb, mr = margins
    tile = (0, 0, mt + r + mb, ml + c + mr)
    roi = (mt, ml, mt + r, ml + c)
    top, left = part[0] == "t", part[1] == "l"
    if bars:
        a, b = max(1, (35 * r) // 100), max(1, (35 * c) // 100)
        hbar = (roi[0] - 9, roi[1] - 7, a + 9, c + 14) if top else (roi[2] - a, roi[1] - 7, a + 9, c + 14)
        vbar = (roi[0] - 9, roi[1] - 7, r + 18, b + 7) if left else (roi[0] - 9, roi[3] - b, r + 18, b + 7)
        return _case(name, [hbar, vbar, tile], [None, None, roi], [_SIGNS[k % len(_SIGNS)], _SIGNS[(k + 1) % len(_SIGNS)]], colour, origin=origin, ch=ch)
    a, b = max(1, (3 * r) // 4), max(1, (3 * c) // 4)
    first = (roi[0] - 5 if top else roi[2] - a, roi[1] - 6 if left else roi[3] - b, a + 5, b + 6)
    return _case(name, [first, tile], [None, roi], [_SIGNS[k % len(_SIGNS)]], colour, origin=origin, ch=ch)


@functools.lru_cache(maxsize=None)
def edge_canvases(colour=False):
    """Two- and three-tile canvases, each aimed at one boundary of k_fuse_apply / k_fuse_simple / k_fuse_stats_weights / k_fuse_counts_pick and
    of the host geometry (corner_picks, canvas_valid_area).  The reference walks all of them (tests/test_canvas_cases_host.py)."""
    out = []
    # 1. ROI width x height around the wave-layout switch, one workgroup's columns, the lane quad, FUSE_SB and the workgroup heights: strips
    for k, c in enumerate(ROI_WIDTHS):
        out.append(_strip("strip %dx%d" % (ROI_HEIGHTS[k % 8], c), ROI_HEIGHTS[k % 8], c, colour, k))
    for k, (r, c) in enumerate([(65, 1024), (1, 5), (257, 64), (513, 33), (64, 64), (17, 16), (16, 17)]):      # tall strips: ramps along the columns
        out.append(_strip("strip %dx%d" % (r, c), r, c, colour, k + 1))
    # 2. one corner ROI per quadrant and wave layout (the strips of each layout are above), heights on both sides of the workgroup heights
    k = 0
    for (r, c) in ((63, 255), (65, 256), (33, 511), (64, 512), (17, 513), (65, 1025)):
        for part in ("tl", "tr", "bl", "br"):
            out.append(_corner("corner %s %dx%d" % (part, r, c), r, c, part, colour, k, origin=(k % 2, 1 + k % 4)))
            k += 1
    for part in ("tl", "tr", "bl", "br"):
        out.append(_corner("block %s 64x257" % part, 64, 257, part, colour, k, bars=False, origin=(2, 2)))
        k += 1
    # 3. tile widths: a second column block of k_fuse_apply holding one and three pixels (gray: one lane with nk < 4), a tile narrower than two quads;
    #    tile column offsets x0 with x0 % 4 != 0
    out.append(_strip("tile width 1025", 17, 1025, colour, 0, margins=(1, 0, 2, 0), origin=(0, 0)))             # x0 = 5
    out.append(_strip("tile width 1027", 33, 1025, colour, 1, margins=(0, 2, 1, 0), origin=(1, 2)))             # x0 = 7, ROI up to the last column
    out.append(_strip("tile width 1027 left", 16, 1024, colour, 2, margins=(2, 0, 0, 3), origin=(0, 1)))        # x0 = 6, the tail pixels outside the ROI
    out.append(_corner("tile width 1027 corner", 63, 1025, "tl", colour, 3, margins=(0, 1, 0, 1), origin=(0, 2)))
    out.append(_strip("tile width 5", 15, 3, colour, 3, margins=(1, 1, 1, 1), origin=(0, 1)))                   # x0 = 6
    out.append(_strip("tile width 5 whole", 4, 5, colour, 4, margins=(0, 0, 0, 0), origin=(1, 2)))              # x0 = 7
    # 4. ROI edges inside a lane's quad: (rx0 - x0) % 4 and (rx1 - x0) % 4 through 1, 2, 3 (tile x0 = 5 + origin), strip and corner
    for k, (lo, hi) in enumerate(((1, 2), (2, 3), (3, 1), (1, 1), (2, 2), (3, 3))):
        c = 4 * 40 + hi - lo
        out.append(_strip("quad strip %d %d" % (lo, hi), 33, c, colour, k, margins=(1, lo, 1, 8 - hi), origin=(1, k % 4)))
        out.append(_corner("quad corner %d %d" % (lo, hi), 64, c, ("tl", "tr", "bl", "br")[k % 4], colour, k, margins=(2, lo, 1, 8 - hi),
                           origin=(0, 9 + (k + 1) % 4)))
    # 5. the ROI on the canvas border: row 0, column 0, the last row and the last column
    whole = (0, 0, 65, 257)
    out.append(_case("border strip", [whole, whole], [None, whole[:2] + (65, 257)], [(3, -4)], colour))
    out.append(_case("border corner", [(0, 0, 50, 200), whole], [None, (0, 0, 65, 257)], [(-3, 4)], colour))
    out.append(_case("border corner br", [(20, 60, 45, 197), whole], [None, (0, 0, 65, 257)], [(2, 2)], colour))
    # 6. corner ROIs of one or two rows or columns, half valid or with nothing underneath -- those the reference walks (edge_verdict_only: the rest)
    out += [_thin(r, c, part, colour, k) for k, (r, c, part) in enumerate(_THIN) if (r, c, part) not in _THIN_RAISES]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_verdict_only(colour=False):
    """Wanted shapes on which the reference itself raises: the library must refuse them, there are no bytes to compare."""
    return tuple(_thin(r, c, part, colour, k) for k, (r, c, part) in enumerate(_THIN) if (r, c, part) in _THIN_RAISES)


def _thin(r, c, part, colour, k, ch=None):
    """a corner ROI, most of one or two rows or columns: the first tile covers its left / right / top / bottom half, or (none) lies beside it"""
    tile = (0, 0, r + 2, c + 3)
    roi = (1, 2, 1 + r, 2 + c)
    first = {"l": (-4, -5, r + 9, 7 + c // 2), "r": (-4, 2 + c - c // 2, r + 9, c // 2 + 6), "t": (-4, -5, 5 + r // 2, c + 11),
             "b": (1 + r - r // 2, -5, r // 2 + 6, c + 11), "none": (-4, -9, r + 9, 7)}[part]
    return _case("thin %s %dx%d" % (part, r, c), [first, tile], [None, roi], [_SIGNS[k % len(_SIGNS)]], colour, origin=(k % 2, 1 + k % 4), ch=ch)


_THIN = ((1, 5, "l"), (1, 5, "r"), (1, 257, "l"), (1, 257, "r"), (1, 1029, "r"), (1, 513, "none"), (33, 1, "t"), (33, 1, "b"), (65, 1, "none"),
         (1, 1, "none"), (2, 1029, "l"), (2, 1029, "r"), (2, 300, "none"), (64, 2, "t"), (64, 2, "b"), (3, 3, "none"), (16, 5, "none"),
         (33, 257, "none"), (65, 600, "none"))             # nothing underneath at size: weights above 1, both clamps of the blend
# getWeightsMatrix divides by row - rowIndex - 1 (col - colIndex - 1) = 0 on the two-row (two-column) ones below; a single row or column passes
_THIN_RAISES = ((2, 1029, "l"), (2, 300, "none"), (64, 2, "t"), (64, 2, "b"))


# ---- reference walks -----------------------------------------------------------------------------------------------------------------------------
def reference_fade_walk(oracle, rows, cols, tiles, geom):
    """Stitcher.getStitchByOffset's walk (Stitcher.py:434-486) on the reference's int64 / -1 canvas with the oracle's fuseByFadeInAndFadeOut.
    -> (canvas bytes, infos, k): infos[i] = the oracle's (mode, quadrant, rowIndex, colIndex) of tile i (None: pasted); k = the first tile on
    which the reference raises (None: none) -- canvas and infos are then those of geom[:k]."""
    cv = np.zeros((rows, cols) + tiles[0].shape[2:], np.int64) - 1
    infos, stop = [], None
    for k, (t, g) in enumerate(zip(tiles, geom)):
        y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
        A = cv[ry0:ry1, rx0:rx1].copy()
        if mode != PASTE and A.size:
            B = t[ry0 - y0:ry1 - y0, rx0 - x0:rx1 - x0].astype(np.int64)          # the ROI lies inside the tile rectangle: B is the tile's part
            try:
                out, info = oracle.fuse_fade(A, B, dx, dy, return_info=True)
            except IndexError:
                stop = k
                break
        cv[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
        if mode != PASTE and A.size:
            cv[ry0:ry1, rx0:rx1] = out
            infos.append(tuple(int(v) for v in info))
        else:
            infos.append(None)
    cv[cv == -1] = 0
    return cv.astype(np.uint8), infos, stop


def reference_simple_walk(tiles, geom, rows, cols, mode):
    """Stitcher.py:434-486 with fuseImage's fill-in (Stitcher.py:498-504) and ImageFusion.py:12-41, in numpy"""
    cv = np.zeros((rows, cols) + tiles[0].shape[2:], np.int64) - 1
    for t, g in zip(tiles, geom):
        y0, x0, ry0, rx0, ry1, rx1 = [int(v) for v in g[:6]]
        A = cv[ry0:ry1, rx0:rx1].copy()
        cv[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = t
        if g[8] == PASTE:
            continue
        B = cv[ry0:ry1, rx0:rx1].copy()
        A[A == -1] = 0
        B[B == -1] = 0
        A[A == 0] = B[A == 0]
        B[B == 0] = A[B == 0]
        cv[ry0:ry1, rx0:rx1] = np.uint8((A + B) / 2) if mode == AVERAGE else np.maximum(A, B) if mode == MAXIMUM else np.minimum(A, B)
    cv[cv == -1] = 0
    return cv.astype(np.uint8)
