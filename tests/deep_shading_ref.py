"""Flat-field shading correction of 16-bit tiles (vfsms_deep_shading_*) as specified for this project.  Plain numpy, integer arithmetic
only, so the HIP kernels (imagestitch_amd/csrc/deep_shading_kernels.hip, and the box / level / gain kernels of shading_kernels.hip they
share with the 8-bit path) must equal it sample for sample at every step: profile, smoothed field, gain and the corrected tiles.

This docstring IS the specification; there is no reference counterpart (the reference never corrects shading).

Inputs: N tiles of ONE shape (h, w), uint16, 1 <= N <= 4096; percentile 0..100; radius R 1..127; pedestal d 0..65535, the camera's
dark level, one constant for the dataset.

Profile   P[y, x] = the k-th smallest of T_i[y, x] over the N tiles, k = (N - 1) * percentile // 100 (0-based) -> uint16.
Field     F = max(P - d, 0) as uint16 (no Q8 shift: 16-bit samples already have the resolution Q8 gives bytes), then TWO passes of the
          rounded (2R + 1)^2 box filter of shading_ref.box_pass with replicated borders: F' = (boxsum(F) + area // 2) // area, rounded
          once per pass.  boxsum + area // 2 <= 255^2 * 65535 + 32512 = 4 261 445 887 < 2^32: a uint32 accumulator is exact, and a
          rounded mean never exceeds its inputs' maximum, so the second pass has the same bound.
Level     M = (sum(F) + h * w // 2) // (h * w), the sum in 64 bits.
Gain      Q12 in uint16: G = min(65535, (M * 4096 + F // 2) // F) where F > 0, G = 4096 where F == 0
          (65535 * 4096 + 32767 < 2^32).
Apply     p <= d: out = p (left alone).  Otherwise out = min(65535, d + (((p - d) * G + 2048) >> 12))
          (65535 * 65535 + 2048 = 4 294 838 273 < 2^32).
"""
import numpy as np

from shading_ref import GAIN_ONE, MAX_RADIUS, MAX_TILES, box_pass, rank

MAX_SAMPLE = 65535


def _stack(tiles):
    """the stack as (N, h, w) uint16"""
    T = np.stack([np.asarray(t) for t in tiles])
    if T.dtype != np.uint16 or T.ndim != 3:
        raise ValueError("tiles must be uint16 arrays of one shape (h, w)")
    if not 1 <= T.shape[0] <= MAX_TILES:
        raise ValueError("1 <= N <= %d" % MAX_TILES)
    return T


def _pedestal(pedestal):
    if not 0 <= int(pedestal) <= MAX_SAMPLE:
        raise ValueError("pedestal must be 0..65535")
    return int(pedestal)


def profile(tiles, percentile=50):
    """P: the k-th smallest sample over the stack, per position -> uint16 (h, w)"""
    T = _stack(tiles)
    k = rank(T.shape[0], percentile)
    return np.partition(T, k, axis=0)[k]


def smooth(P, R, pedestal=0, passes=2):
    """the smoothed field of a profile: F = max(P - pedestal, 0), then `passes` box passes -> uint16 of the profile's shape"""
    d = _pedestal(pedestal)
    P = np.asarray(P)
    if P.dtype != np.uint16 or P.ndim != 2:
        raise ValueError("the profile is a uint16 (h, w) array")
    F = np.maximum(P.astype(np.int64) - d, 0).astype(np.uint16)[..., None]
    if not 1 <= int(R) <= MAX_RADIUS:
        raise ValueError("radius must be 1..%d" % MAX_RADIUS)
    for _ in range(passes):
        F = box_pass(F, R)
    return F[..., 0]


def level(F):
    """M (a python int)"""
    hw = F.shape[0] * F.shape[1]
    return (int(F.astype(np.uint64).sum()) + hw // 2) // hw


def gain(F):
    """Q12 gain in uint16 of the field's shape"""
    F64 = F.astype(np.uint64)
    M = np.uint64(level(F))
    G = np.full(F.shape, GAIN_ONE, np.uint64)
    nz = F64 > 0
    G[nz] = np.minimum(np.uint64(65535), (M * np.uint64(4096) + F64[nz] // np.uint64(2)) // F64[nz])
    return G.astype(np.uint16)


def apply(tile, G, pedestal=0):
    """the corrected tile: uint16 of the tile's shape"""
    d = _pedestal(pedestal)
    tile = np.asarray(tile)
    if tile.dtype != np.uint16 or tile.shape != G.shape:
        raise ValueError("tile and gain must be uint16 arrays of one shape")
    p = tile.astype(np.int64)
    up = np.minimum(MAX_SAMPLE, d + (((p - d) * G.astype(np.int64) + 2048) >> 12))
    return np.where(p <= d, p, up).astype(np.uint16)


def estimate(tiles, percentile=50, radius=32, pedestal=0):
    """-> (gain uint16 Q12, smoothed field uint16, profile uint16), each of the tile shape"""
    P = profile(tiles, percentile)
    F = smooth(P, radius, pedestal)
    return gain(F), F, P


def correct(tiles, percentile=50, radius=32, pedestal=0):
    """the whole correction of a stack -> list of corrected tiles"""
    G = estimate(tiles, percentile, radius, pedestal)[0]
    return [apply(t, G, pedestal) for t in tiles]
