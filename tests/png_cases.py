"""The images the PNG coder's tests share (tests/test_png_device_host.py: the specification and the host program; tests/test_png_device_gpu.py: the
device), in the file's channel order (R G B).  CASES: (name, image maker, segment_rows)."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def h_ramp(shape):
    """every row the same ramp along x: Up leaves zeros below row 0"""
    img = np.zeros(shape, np.uint8)
    img[...] = ((7 * np.arange(shape[1])) & 255).astype(np.uint8).reshape((1, shape[1]) + (1,) * (len(shape) - 2))
    return img


def v_ramp(shape):
    """every column the same ramp along y"""
    img = np.zeros(shape, np.uint8)
    img[...] = ((5 * np.arange(shape[0]) + 3) & 255).astype(np.uint8).reshape((shape[0], 1) + (1,) * (len(shape) - 2))
    return img


def flat(shape, value=93):
    return np.full(shape, value, np.uint8)


def diagonal(shape):
    """constant along the diagonals, 40 + x - y (mod 256): every pixel equals the one above left, so the Paeth residual (and the Average one) is
    zero over whole rows but their first pixel while Sub and Up leave +-1 everywhere: runs of zeros of a row's length, cut by the next row's
    filter byte 4 (or 3)"""
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    g = ((40 + xx - yy) & 255).astype(np.uint8)
    return g if len(shape) == 2 else np.stack([g] * shape[2], -1)


def real_crop(rows, cols, y0=40, x0=300):
    z = np.load(os.path.join(ROOT, "tests", "golden", "real_full_strips.npz"))
    return np.ascontiguousarray(z["p4_a"][y0:y0 + rows, x0:x0 + cols])


def none_wins():
    """an image on whose rows filter None is the cheapest: samples near 0 and near 255 alike, in no order (every difference is large, the
    bytes themselves are small as signed bytes)"""
    rng = np.random.default_rng(5)
    return (rng.integers(0, 8, (9, 40)) + 248 * rng.integers(0, 2, (9, 40))).astype(np.uint8) ^ 0


def cost_128():
    """a row holding the byte 128 under the filter that wins"""
    img = np.zeros((3, 6), np.uint8)
    img[0] = [128, 0, 128, 0, 0, 128]
    img[1] = [1, 2, 3, 4, 5, 6]
    img[2] = [128, 128, 128, 128, 128, 128]
    return img


_SHAPES = [(1, 1), (1, 7), (5, 1), (17, 5), (33, 50), (1, 1, 3), (3, 2, 3), (40, 21, 3)]

CASES = []
for _k, _s in enumerate(_SHAPES):
    for _S in (1, 16, 64):
        CASES.append(("noise %s S=%d" % ("x".join(map(str, _s)), _S), (lambda s=_s, k=_k: noise(s, 100 + k)), _S))
# gray widths 15, 16 and 30: rows of 16, 17 and 31 bytes
CASES += [("gray %d wide S=%d" % (w, S), (lambda w=w: noise((37, w), w)), S) for w in (15, 16, 30) for S in (1, 16)]
# a segment of exactly one chunk of 4096 bytes (16 rows of 1 + 255), and one of 16 bytes more; 17 and 31 rows: a short last segment
CASES += [("gray %d wide, %d rows, S=16" % (w, r), (lambda w=w, r=r: real_crop(r, w)), 16) for w in (255, 256) for r in (17, 31)]
CASES += [
    ("horizontal ramp", lambda: h_ramp((20, 70)), 16),
    ("vertical ramp", lambda: v_ramp((20, 70)), 16),
    ("vertical ramp, colour", lambda: v_ramp((33, 9, 3)), 16),
    ("flat", lambda: flat((19, 300)), 16),
    ("flat, colour, S=64", lambda: flat((70, 30, 3)), 64),
    ("diagonal: zero Paeth residuals, gray across the wrap", lambda: diagonal((40, 300)), 16),
    ("diagonal, colour: runs of 599 zeros", lambda: diagonal((40, 200, 3)), 16),
    ("diagonal, colour, S=64: runs across chunks", lambda: diagonal((70, 200, 3)), 64),
    ("real strip crop", lambda: real_crop(48, 333), 16),
    ("real strip crop, S=1", lambda: real_crop(9, 333), 1),
    ("none wins", none_wins, 16),
    ("cost 128", cost_128, 16),
]
