"""Synthetic focus series with a known depth map, for the tests of Method.focusStack and tools/bench_focus.py.

The sharp image is random bytes on a 2 x 2 pixel lattice (np.kron(base, ones((2, 2))), cropped to the shape).  A depth map gives every
pixel the plane it is sharp in: "ramp" is x * K // w, "quad" the four quadrants, (2 * (y // (h // 2)) + x // (w // 2)) % K.  In plane z a
pixel of depth d carries the sharp image box-blurred with radius |z - d|: an integer mean over (2r + 1)^2 with clamped borders, rounded
to nearest.  -> (planes, sharp, depth)"""
import numpy as np


def sharp_image(rng, shape):
    h, w = shape[:2]
    base = rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2) + tuple(shape[2:])).astype(np.uint8)
    ones = np.ones((2, 2) + (1,) * (len(shape) - 2), np.uint8)
    return np.ascontiguousarray(np.kron(base, ones)[:h, :w])


def depth_map(kind, h, w, K):
    y, x = np.indices((h, w))
    if kind == "ramp":
        return (x * K // w).astype(np.uint8)
    if kind == "quad":
        return ((2 * (y // max(h // 2, 1)) + x // max(w // 2, 1)) % K).astype(np.uint8)
    raise ValueError("depth map %r" % (kind,))


def box_blur(img, r):
    """the integer mean over (2r + 1)^2, indices clamped, rounded to nearest; r = 0 is the image"""
    if r == 0:
        return img.copy()
    a = img.astype(np.int64)
    h, w = a.shape[:2]
    ys = [np.clip(np.arange(h) + d, 0, h - 1) for d in range(-r, r + 1)]
    xs = [np.clip(np.arange(w) + d, 0, w - 1) for d in range(-r, r + 1)]
    rows = sum(a[:, x] for x in xs)
    s = sum(rows[y] for y in ys)
    area = (2 * r + 1) ** 2
    return ((s + area // 2) // area).astype(np.uint8)


def stack(shape, K, kind="ramp", seed=0):
    """K planes of `shape` ((h, w) or (h, w, 3)) -> (planes, sharp, depth)"""
    return stack_of(sharp_image(np.random.default_rng(seed), shape), K, kind)


def stack_of(sharp, K, kind="ramp"):
    """the same series over a sharp image of the caller's (the end-to-end tests blur tiles that register) -> (planes, sharp, depth)"""
    sharp = np.ascontiguousarray(sharp, np.uint8)
    shape = sharp.shape
    depth = depth_map(kind, shape[0], shape[1], K)
    blurred = [box_blur(sharp, r) for r in range(K)]
    planes = []
    for z in range(K):
        r = np.abs(depth.astype(np.int32) - z)
        p = np.zeros(shape, np.uint8)
        for q in range(K):
            m = r == q
            p[m] = blurred[q][m]
        planes.append(p)
    return planes, sharp, depth
