"""The reduced levels of a pyramidal mosaic (Stitcher.outputPyramid), in numpy -- the specification csrc/pyramid_kernels.hip equals byte for
byte.  Integer arithmetic only; there is no reference counterpart.

  level 0   the mosaic as canvas_download returns it: u8 (R, C) or (R, C, ch), in the canvas's channel order
  level k   R_k = (R_{k-1} + 1) >> 1 rows, C_k = (C_{k-1} + 1) >> 1 columns; sample (i, j) = (a + b + c + d + 2) >> 2 per channel over
            rows min(2i, R_{k-1} - 1), min(2i + 1, R_{k-1} - 1) and columns min(2j, C_{k-1} - 1), min(2j + 1, C_{k-1} - 1) of level k - 1

Every level is rounded once, from the rounded level below it (a cascade, not a mean over the 2^k x 2^k block), and an edge is replicated at
each level against that level's own size.
"""
import numpy as np

MAX_LEVELS = 10


def level_size(n, k):
    """rows (or columns) of level k of an image with n rows (columns)"""
    for _ in range(k):
        n = (n + 1) >> 1
    return n


def reduce_once(img):
    """level k from level k - 1"""
    R, C = img.shape[:2]
    r0 = np.minimum(2 * np.arange((R + 1) >> 1), R - 1); r1 = np.minimum(r0 + 1, R - 1)
    c0 = np.minimum(2 * np.arange((C + 1) >> 1), C - 1); c1 = np.minimum(c0 + 1, C - 1)
    x = img.astype(np.uint16)
    s = x[r0][:, c0] + x[r0][:, c1] + x[r1][:, c0] + x[r1][:, c1] + 2
    return (s >> 2).astype(np.uint8)


def pyramid_levels(img, levels):
    """-> [level 1, ..., level `levels`] of a u8 image (R, C) or (R, C, ch)"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3) and img.shape[0] >= 1 and img.shape[1] >= 1
    out = []
    for _ in range(levels):
        img = reduce_once(img)
        out.append(img)
    return out


def band_of_level(row0, nrows, R, k):
    """the rows of level k that the band [row0, row0 + nrows) of an R-row mosaic produces -> (first_row, n_rows).  For a band that starts
    at a multiple of 2^levels (levels >= k) and is a multiple of 2^levels rows long -- or ends at the last row -- these rows are complete
    and depend on no other band: the reduction can be streamed."""
    assert 0 <= row0 and nrows >= 1 and row0 + nrows <= R and row0 % (1 << k) == 0
    first = row0 >> k
    end = (row0 + nrows + (1 << k) - 1) >> k
    return first, end - first


def default_levels(R, C, tile):
    """the smallest K >= 0 with max(R_K, C_K) <= tile, at most MAX_LEVELS"""
    K = 0
    while K < MAX_LEVELS and max(level_size(R, K), level_size(C, K)) > tile:
        K += 1
    return K
