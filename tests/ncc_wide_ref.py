"""The specification of the wide two-level offset search behind Method.failedPairRepair = "stage", restated in numpy.

The reference has no such step, so this is the project's own specification, built on verify_ref.py and ncc_search_ref.py;
csrc/wide_kernels.hip (with the search of csrc/adjust_kernels.hip) equals it bit for bit.

Inputs: whole tiles A and B (uint8, ONE shape h x w), a predicted offset (dx, dy) in verify_ref's convention, a radius R in 1..128, a
reduction factor f in {2, 4, 8} with ceil(R / f) <= 16, K in 1..4 peaks and min_pixels.

1. Reduce.  ox, oy = dx mod f, dy mod f (Python's %, so both lie in [0, f)); hc = (h - ox) // f, wc = (w - oy) // f.  Bc[u, v] = (the sum of
   the f x f block of B at (f u, f v) + f * f / 2) >> (2 log2 f); Ac[u, v] the same over the block of A at (ox + f u, oy + f v).  Both are
   hc x wc.  The coarse offset (Dx, Dy) = ((dx - ox) / f, (dy - oy) / f) is exact: B's block (u, v) meets A's block (u + Dx, v + Dy).
2. Coarse surface.  ncc_search_ref.search(Ac, Bc, Dx, Dy, Rc, max(1, min_pixels // (f * f))) with Rc = ceil(R / f); only its int32
   fixed-point surface is used.
3. Seeds.  The coarse candidates (i, j) in the order (-surface, i * i + j * j, i, j), walked in that order; a candidate is kept when its
   Chebyshev distance to every candidate already kept exceeds 1; stop at K.
4. Fine.  rf = min(f, R).  Seed (ci, cj) gives the centre (cx, cy), each component clamp(f * c, -(R - rf), R - rf);
   ncc_search_ref.search(A, B, dx + cx, dy + cy, rf, min_pixels) at full resolution gives (bi, bj) and a fixed-point score; the seed's
   result is (ti, tj) = (cx + bi, cy + bj).
5. Result.  The winner over the seeds has the smallest (-fixed, ti * ti + tj * tj, ti, tj).
   out8 = (ti, tj, fixed, N of the winner, ci, cj of the winning seed, its coarse fixed score, seeds used); the seed table is int32 [4, 6]
   = (ci, cj, coarse fixed, ti, tj, fine fixed) per seed, zeros in unused rows.
"""
import numpy as np

import ncc_search_ref as S
import verify_ref

MAX_RADIUS = 128
MAX_PEAKS = 4
FACTORS = (2, 4, 8)


def check_args(radius, factor, peaks):
    R, f, K = int(radius), int(factor), int(peaks)
    assert 1 <= R <= MAX_RADIUS and f in FACTORS and 1 <= K <= MAX_PEAKS and -(-R // f) <= S.MAX_RADIUS
    return R, f, K


def _block_means(T, r0, c0, hc, wc, f):
    blk = T[r0:r0 + f * hc, c0:c0 + f * wc].astype(np.int64).reshape(hc, f, wc, f).sum(axis=(1, 3))
    return ((blk + (f * f) // 2) >> (2 * (f.bit_length() - 1))).astype(np.uint8)


def reduce_pair(A, B, dx, dy, factor):
    """step 1 -> (Ac, Bc, Dx, Dy)"""
    A = np.asarray(A); B = np.asarray(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8 and A.ndim == 2 and A.shape == B.shape
    f = int(factor)
    h, w = A.shape
    ox, oy = int(dx) % f, int(dy) % f
    hc, wc = (h - ox) // f, (w - oy) // f
    assert hc >= 1 and wc >= 1
    return _block_means(A, ox, oy, hc, wc, f), _block_means(B, 0, 0, hc, wc, f), (int(dx) - ox) // f, (int(dy) - oy) // f


def seeds_of(surface, peaks):
    """step 3 on an int32 surface [2 Rc + 1, 2 Rc + 1] -> [(ci, cj, coarse fixed)], at most `peaks`"""
    Rc = (surface.shape[0] - 1) // 2
    order = sorted((-int(surface[i + Rc, j + Rc]), i * i + j * j, i, j) for i in range(-Rc, Rc + 1) for j in range(-Rc, Rc + 1))
    kept = []
    for neg, _d2, i, j in order:
        if all(max(abs(i - ci), abs(j - cj)) > 1 for ci, cj, _ in kept):
            kept.append((i, j, -neg))
            if len(kept) == int(peaks):
                break
    return kept


def centre(c, factor, radius):
    """step 4: the fine window's centre for a seed component"""
    lim = int(radius) - min(int(factor), int(radius))
    return min(max(int(factor) * int(c), -lim), lim)


def search(A, B, dx, dy, radius, factor, peaks, min_pixels):
    """-> (out8 as a list of 8 ints, int32 seed table [4, 6])"""
    R, f, K = check_args(radius, factor, peaks)
    dx, dy = int(dx), int(dy)
    Ac, Bc, Dx, Dy = reduce_pair(A, B, dx, dy, f)
    _i, _j, _fx, surface = S.search(Ac, Bc, Dx, Dy, -(-R // f), max(1, int(min_pixels) // (f * f)))
    rf = min(f, R)
    table = np.zeros((MAX_PEAKS, 6), np.int32)
    best = None
    kept = seeds_of(surface, K)
    for k, (ci, cj, cfx) in enumerate(kept):
        cx, cy = centre(ci, f, R), centre(cj, f, R)
        bi, bj, fx, _s = S.search(A, B, dx + cx, dy + cy, rf, min_pixels)
        ti, tj = cx + bi, cy + bj
        table[k] = (ci, cj, cfx, ti, tj, fx)
        key = (-fx, ti * ti + tj * tj, ti, tj)
        if best is None or key < best[0]:
            best = (key, k)
    k = best[1]
    ci, cj, cfx, ti, tj, fx = (int(v) for v in table[k])
    return [ti, tj, fx, S.shared_pixels(np.asarray(A).shape, dx + ti, dy + tj), ci, cj, cfx, len(kept)], table


def exhaustive(A, B, dx, dy, radius, min_pixels):
    """the same key over all (2 R + 1)^2 candidates at full resolution -> (ti, tj, fixed)"""
    R = int(radius)
    best = None
    for i in range(-R, R + 1):
        for j in range(-R, R + 1):
            fx = verify_ref.fixed(verify_ref.score(verify_ref.sums(A, B, int(dx) + i, int(dy) + j), min_pixels))
            key = (-fx, i * i + j * j, i, j)
            if best is None or key < best:
                best = key
    return best[2], best[3], -best[0]
