"""Flat-field shading correction (Method.shadingCorrection = "estimate") as specified for this project.  Plain numpy, integer arithmetic
only, so the HIP kernels (imagestitch_amd/csrc/shading_kernels.hip) must equal it byte for byte at every step: profile, smoothed field,
gain and the corrected tiles.

This docstring IS the specification; there is no reference counterpart (the reference never corrects shading).

Inputs: N tiles of one shape (h, w) or (h, w, ch), uint8, 1 <= N <= 4096.  Interleaved channels are treated independently.

Profile   P[y, x, c] = the k-th smallest of T_i[y, x, c] over the N tiles, k = (N - 1) * percentile // 100 (0-based), percentile an
          integer in 0..100; 50 gives the lower median.
Smooth    Q = P << 8 (Q8 in uint16), then TWO passes of a (2R + 1) x (2R + 1) box filter with replicated borders (indices clamped to the
          plane), 1 <= R <= 127: Q' = (boxsum(Q) + area // 2) // area, area = (2R + 1)^2, rounded once per pass after both axes have
          been summed.  boxsum + area // 2 <= 255^2 * 65280 + 32512 = 4 244 864 512 < 2^32: a uint32 accumulator is exact.
Level     M_c = (sum(Q[:, :, c]) + h * w // 2) // (h * w) per channel, the sum in 64 bits.
Gain      Q12 in uint16: G = min(65535, (M_c * 4096 + Q // 2) // Q) where Q > 0, G = 4096 where Q == 0.
Apply     out = min(255, (p * G + 2048) >> 12).
"""
import numpy as np

MAX_TILES = 4096
MAX_RADIUS = 127
GAIN_ONE = 4096


def _planes(tiles):
    """the stack as (N, h, w, ch) uint8 and whether the tiles were 2-D"""
    T = np.stack([np.asarray(t) for t in tiles])
    if T.dtype != np.uint8 or T.ndim not in (3, 4):
        raise ValueError("tiles must be uint8 arrays of one shape (h, w) or (h, w, ch)")
    if not 1 <= T.shape[0] <= MAX_TILES:
        raise ValueError("1 <= N <= %d" % MAX_TILES)
    return (T[..., None], True) if T.ndim == 3 else (T, False)


def rank(n, percentile):
    if not 0 <= int(percentile) <= 100:
        raise ValueError("percentile must be 0..100")
    return (n - 1) * int(percentile) // 100


def profile(tiles, percentile=50):
    """P: the k-th smallest byte over the stack, per sample -> uint8 of the tile shape"""
    T, gray = _planes(tiles)
    k = rank(T.shape[0], percentile)
    P = np.partition(T, k, axis=0)[k]
    return P[..., 0] if gray else P


def box_pass(Q, R):
    """one rounded pass on a (h, w, ch) uint16 plane; uint32 sums (the bound is in the module docstring)"""
    if not 1 <= int(R) <= MAX_RADIUS:
        raise ValueError("radius must be 1..%d" % MAX_RADIUS)
    R = int(R)
    h, w = Q.shape[:2]
    area = (2 * R + 1) ** 2
    acc = np.zeros(Q.shape, np.uint32)
    rows = np.zeros(Q.shape, np.uint32)
    for d in range(-R, R + 1):
        rows += Q[:, np.clip(np.arange(w) + d, 0, w - 1)]
    for d in range(-R, R + 1):
        acc += rows[np.clip(np.arange(h) + d, 0, h - 1)]
    return ((acc.astype(np.uint64) + area // 2) // area).astype(np.uint16)


def smooth(P, R, passes=2):
    """Q8 field of a profile: uint16 of the profile's shape"""
    gray = P.ndim == 2
    Q = (P[..., None] if gray else P).astype(np.uint16) << 8
    for _ in range(passes):
        Q = box_pass(Q, R)
    return Q[..., 0] if gray else Q


def level(Q):
    """M_c per channel (python ints)"""
    Q3 = Q[..., None] if Q.ndim == 2 else Q
    hw = Q3.shape[0] * Q3.shape[1]
    return [(int(Q3[:, :, c].astype(np.uint64).sum()) + hw // 2) // hw for c in range(Q3.shape[2])]


def gain(Q):
    """Q12 gain in uint16 of the field's shape"""
    Q3 = (Q[..., None] if Q.ndim == 2 else Q).astype(np.uint64)
    M = np.array(level(Q), np.uint64).reshape(1, 1, -1)
    G = np.full(Q3.shape, GAIN_ONE, np.uint64)
    nz = Q3 > 0
    G[nz] = np.minimum(65535, (np.broadcast_to(M * 4096, Q3.shape)[nz] + Q3[nz] // 2) // Q3[nz])
    G = G.astype(np.uint16)
    return G[..., 0] if Q.ndim == 2 else G


def apply(tile, G):
    """the corrected tile: uint8 of the tile's shape"""
    tile = np.asarray(tile)
    if tile.dtype != np.uint8 or tile.shape != G.shape:
        raise ValueError("tile and gain must have one shape")
    return np.minimum(255, (tile.astype(np.uint32) * G.astype(np.uint32) + 2048) >> 12).astype(np.uint8)


def estimate(tiles, percentile=50, radius=32):
    """-> (gain uint16 Q12, smoothed field uint16 Q8, profile uint8), each of the tile shape"""
    P = profile(tiles, percentile)
    Q = smooth(P, radius)
    return gain(Q), Q, P


def correct(tiles, percentile=50, radius=32):
    """the whole correction of a stack -> list of corrected tiles"""
    G = estimate(tiles, percentile, radius)[0]
    return [apply(t, G) for t in tiles]
