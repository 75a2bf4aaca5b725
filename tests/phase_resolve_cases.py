"""Inputs shared by test_phase_resolve_host.py and test_phase_resolve_gpu.py: strips cut from one smooth random field at known offsets,
the burned-in data bar, the refusals, and a 3 x 3 serpentine grid of 256 x 256 tiles.  Everything is deterministic (fixed seeds)."""
import functools

import numpy as np

MIN_PIXELS = 64          # the strips here are small: (-35, 100) on 48 x 160 leaves 13 x 60 = 780 shared pixels
THRESHOLD = 0.5

# (h, w) -> true (dx, dy): B pixel (r, c) meets A pixel (r + dx, c + dy).  Both signs, zero, and beyond half the padded size on each axis.
SHIFTS = {
    (48, 160): [(5, -7), (33, 10), (-35, 100), (20, -120), (0, 0), (-3, 0), (0, 81)],
    (160, 48): [(-7, 5), (10, 33), (100, -35), (-120, 20), (0, 0), (90, 3)],
    (45, 75): [(4, -6), (30, 9), (-31, 50), (22, -44), (0, 0), (-23, 38), (38, 0), (0, -60)],      # odd M and N (45, 75 are their own DFT sizes)
    (49, 97): [(5, -7), (30, 60), (-33, 12), (25, -70), (0, 0), (40, 0), (-26, 51)],               # padded to 50 x 100
}


@functools.lru_cache(maxsize=None)
def field(seed=7, size=640, sigma=0.6):
    """a smooth random field, uint8: white noise low-passed by a Gaussian (sigma px) in the frequency domain.  At sigma 0.6 the reference
    recovers every shift below from one peak; from sigma 0.8 on the strips' own borders start to outweigh small overlaps"""
    rows, cols = size if isinstance(size, tuple) else (size, size)
    rng = np.random.RandomState(seed)
    f = np.fft.rfft2(rng.standard_normal((rows, cols)))
    ky = np.fft.fftfreq(rows)[:, None]; kx = np.fft.rfftfreq(cols)[None, :]
    g = np.fft.irfft2(f * np.exp(-2.0 * (np.pi * sigma) ** 2 * (ky * ky + kx * kx)), s=(rows, cols))
    g = (g - g.min()) / (g.max() - g.min())
    out = np.round(g * 255.0).astype(np.uint8)
    out.setflags(write=False)
    return out


def cut(h, w, dx, dy, seed=7, oy=200, ox=200):
    """(A, B) of h x w with B(r, c) = A(r + dx, c + dy) wherever both exist"""
    F = field(seed)
    A = F[oy:oy + h, ox:ox + w]
    B = F[oy + dx:oy + dx + h, ox + dy:ox + dy + w]
    return np.ascontiguousarray(A), np.ascontiguousarray(B)


def production_pair(dx=300, dy=-1500):
    """one 409 x 2048 strip pair (the strips of 2048^2 tiles at roiRatio 0.2), wrapped on both axes of its 432 x 2048 surface"""
    F = field(31, (768, 3840))
    oy, ox = 20, 1550
    return np.ascontiguousarray(F[oy:oy + 409, ox:ox + 2048]), np.ascontiguousarray(F[oy + dx:oy + dx + 409, ox + dy:ox + dy + 2048])


def bar_pair(h, w, dx, dy, bar_rows, seed=7):
    """both strips carry one identical fixed pattern (a burned-in data bar: black ground, bright ticks) in their last `bar_rows` rows;
    the content above it is shifted by (dx, dy)"""
    if h > w:                                              # a tall strip carries its bar in the last columns
        A, B = bar_pair(w, h, dy, dx, bar_rows, seed)
        return np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    A, B = cut(h, w, dx, dy, seed)
    A = A.copy(); B = B.copy()
    rng = np.random.RandomState(99)
    bar = np.where(rng.rand(bar_rows, w) < 0.3, 255, 0).astype(np.uint8)
    A[h - bar_rows:] = bar; B[h - bar_rows:] = bar
    return A, B


def noisy(B, seed=5, amp=2):
    """B with independent noise of +-amp grey levels: identical strips would make the surface one exact delta over rounding noise, and the
    second peak a matter of the transform's rounding"""
    n = np.random.RandomState(seed).randint(-amp, amp + 1, B.shape)
    return np.clip(B.astype(np.int64) + n, 0, 255).astype(np.uint8)


def disjoint(h, w):
    """two strips of unrelated content (different fields)"""
    return np.ascontiguousarray(field(7)[100:100 + h, 50:50 + w]), np.ascontiguousarray(field(11)[300:300 + h, 260:260 + w])


def flat(h, w):
    """a black strip against content: the transforms of zeros are exact zeros on any IEEE implementation, so the surface is exactly 0"""
    return np.zeros((h, w), np.uint8), cut(h, w, 0, 0)[1]


def grid_tiles(rows=3, cols=3, size=256, step=200, jitter=((0, 0), (3, -2), (-2, 4), (1, 1), (-3, -1), (2, 3), (0, -4), (-1, 2), (4, 0))):
    """a column serpentine of rows x cols tiles of size^2 cut from one field (down the first column, across, up the second, ...)
    -> (tiles in path order, true full-tile offsets [dx, dy] of every consecutive pair, accepted directions)"""
    F = field(23, 1024)
    pos, k = [], 0
    for c in range(cols):
        rr = range(rows) if c % 2 == 0 else range(rows - 1, -1, -1)
        for r in rr:
            jy, jx = jitter[k % len(jitter)]
            pos.append((40 + r * step + jy, 40 + c * step + jx)); k += 1
    tiles = [np.ascontiguousarray(F[y:y + size, x:x + size]) for (y, x) in pos]
    offsets = [[pos[k + 1][0] - pos[k][0], pos[k + 1][1] - pos[k][1]] for k in range(len(pos) - 1)]
    dirs = []
    for (dy_, dx_) in offsets:
        dirs.append((1 if dy_ > 0 else 3) if abs(dy_) > abs(dx_) else (2 if dx_ > 0 else 4))
    return tiles, offsets, dirs
