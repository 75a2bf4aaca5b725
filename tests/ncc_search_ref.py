"""The specification of the offset search behind Method.globalAdjust = "ncc", restated in numpy.

The reference has no such step, so this is the project's own specification, like verify_ref.py, whose statistic it searches with;
csrc/adjust_kernels.hip equals it bit for bit.

Inputs: whole tiles A and B (uint8, ONE shape h x w), a predicted offset (dx, dy) in verify_ref's convention -- B's pixel (r, c) meets A's
pixel (r + dx, c + dy); for consecutive tiles of a path (dx, dy) is exactly the entry of offsetList -- a radius R (1..16) and min_pixels.

1. Every candidate (i, j), i, j in [-R, R], is the offset (dx + i, dy + j).  Its six integers are verify_ref.sums over ITS overlap
   rectangle (the rectangle depends on the candidate), its score is verify_ref.score(sums, min_pixels): an empty overlap, fewer than
   min_pixels shared pixels or a flat side score 0.
2. surface[i + R, j + R] = verify_ref.fixed(score), int32.
3. The best candidate has the largest DOUBLE score (not the fixed-point one); ties go to the smallest i * i + j * j, then the smallest i,
   then the smallest j.  A flat pair therefore returns (0, 0).
"""
import numpy as np

import verify_ref

MAX_RADIUS = 16


def search(A, B, dx, dy, radius, min_pixels):
    """-> (best_i, best_j, fixed-point score of the best, int32 surface [2R + 1, 2R + 1])"""
    R = int(radius)
    assert 1 <= R <= MAX_RADIUS
    surface = np.zeros((2 * R + 1, 2 * R + 1), np.int32)
    best = None
    for i in range(-R, R + 1):
        for j in range(-R, R + 1):
            sc = verify_ref.score(verify_ref.sums(A, B, int(dx) + i, int(dy) + j), min_pixels)
            surface[i + R, j + R] = verify_ref.fixed(sc)
            key = (-sc, i * i + j * j, i, j)
            if best is None or key < best[0]:
                best = (key, i, j, sc)
    return best[1], best[2], verify_ref.fixed(best[3]), surface


def shared_pixels(shape, dx, dy):
    """N of verify_ref.sums for an offset, from the shape alone"""
    r0, r1, c0, c1 = verify_ref.overlap(shape[0], shape[1], int(dx), int(dy))
    return max(0, r1 - r0) * max(0, c1 - c0)
