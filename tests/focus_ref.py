"""The specification of Method.focusStack (imagestitch_amd/csrc/focus_kernels.hip, imagestitch_amd/focus.py): a focus series fused into
one all-in-focus tile.  There is no reference counterpart; plain numpy, integers only, so the device equals every stage byte for byte.

Inputs are N planes, 2 <= N <= 64, uint8, all of one shape (h, w) or (h, w, 3) in B G R order, h, w >= 1.  Plane index 0 is the first
plane given.

  luma     L: gray -- the byte itself; colour -- (29 B + 150 G + 77 R + 128) >> 8
  measure  M[y, x] = |2 L[y, x] - L[y, x-1] - L[y, x+1]| + |2 L[y, x] - L[y-1, x] - L[y+1, x]|, indices clamped to the plane (the
           sum-modified Laplacian); M <= 1020
  focus    F_i = the sum of M_i over the (2R + 1) x (2R + 1) window, indices clamped (replicated borders), both axes summed with no
           rounding; 1 <= R <= 31, F <= 1020 * 63^2 = 4 048 380: uint32 is exact
  index    D[y, x] = the smallest i with F_i[y, x] == max_j F_j[y, x], uint8
  median   (median in {0, 1}) with 1, D is replaced once by the 5th smallest of its 3 x 3 neighbourhood, indices clamped
  compose  out[y, x, :] = plane[D[y, x]][y, x, :]
  scores   S_i = the sum over the plane of M_i, int64
  mode "plane": the whole plane with the smallest i at which S_i is largest; D is constant

fuse(planes, R=4, median=1, mode="pixel") -> (out, D, S)."""
import numpy as np

MIN_PLANES, MAX_PLANES, MAX_RADIUS = 2, 64, 31


def luma(plane):
    """(h, w) or (h, w, 3) B G R uint8 -> int32 (h, w)"""
    p = np.asarray(plane)
    if p.dtype != np.uint8 or p.ndim not in (2, 3) or (p.ndim == 3 and p.shape[2] != 3) or p.shape[0] < 1 or p.shape[1] < 1:
        raise ValueError("a plane is uint8 of shape (h, w) or (h, w, 3), got %s %s" % (p.dtype, p.shape))
    if p.ndim == 2:
        return p.astype(np.int32)
    q = p.astype(np.int32)
    return (29 * q[:, :, 0] + 150 * q[:, :, 1] + 77 * q[:, :, 2] + 128) >> 8


def _shift(a, dy, dx):
    """a[clamp(y + dy), clamp(x + dx)]"""
    h, w = a.shape
    ys = np.clip(np.arange(h) + dy, 0, h - 1)
    xs = np.clip(np.arange(w) + dx, 0, w - 1)
    return a[ys][:, xs]


def measure(L):
    """the sum-modified Laplacian of a luma plane -> int32"""
    L = np.asarray(L, np.int32)
    return np.abs(2 * L - _shift(L, 0, -1) - _shift(L, 0, 1)) + np.abs(2 * L - _shift(L, -1, 0) - _shift(L, 1, 0))


def focus(M, R):
    """the box sum of M over (2R + 1)^2 with clamped indices -> int64 (the values fit uint32)"""
    if not 1 <= int(R) <= MAX_RADIUS:
        raise ValueError("R must lie in 1..%d, got %r" % (MAX_RADIUS, R))
    M = np.asarray(M, np.int64)
    rows = sum(_shift(M, 0, d) for d in range(-R, R + 1))
    return sum(_shift(rows, d, 0) for d in range(-R, R + 1))


def scores(planes):
    """S_i = sum of M_i over the plane -> int64 [N] (planes of any shapes)"""
    return np.array([int(measure(luma(p)).sum()) for p in planes], np.int64)


def median3(D):
    """the 5th smallest of the 3 x 3 neighbourhood, indices clamped -> uint8"""
    D = np.asarray(D, np.uint8)
    nb = np.stack([_shift(D, dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1)])
    return np.sort(nb, axis=0)[4]


def index(planes, R):
    """D before the median: the smallest i of the largest focus measure -> uint8"""
    F = np.stack([focus(measure(luma(p)), R) for p in planes])
    return np.argmax(F, axis=0).astype(np.uint8)       # (argmax returns the first maximum)


def _check(planes):
    planes = [np.asarray(p) for p in planes]
    if not MIN_PLANES <= len(planes) <= MAX_PLANES:
        raise ValueError("a stack has %d..%d planes, got %d" % (MIN_PLANES, MAX_PLANES, len(planes)))
    for p in planes:
        luma(p[:1, :1])
        if p.shape != planes[0].shape:
            raise ValueError("the planes of a stack have one shape, got %s and %s" % (planes[0].shape, p.shape))
    return planes


def fuse(planes, R=4, median=1, mode="pixel"):
    """-> (out uint8 of the planes' shape, D uint8 (h, w), S int64 [N])"""
    planes = _check(planes)
    if median not in (0, 1):
        raise ValueError("median must be 0 or 1, got %r" % (median,))
    if not 1 <= int(R) <= MAX_RADIUS:
        raise ValueError("R must lie in 1..%d, got %r" % (MAX_RADIUS, R))
    S = scores(planes)
    if mode == "plane":
        D = np.full(planes[0].shape[:2], int(np.argmax(S)), np.uint8)
    elif mode == "pixel":
        D = index(planes, R)
        if median:
            D = median3(D)
    else:
        raise ValueError("mode must be 'pixel' or 'plane', got %r" % (mode,))
    stack = np.stack(planes)
    ys, xs = np.indices(D.shape)
    return stack[D, ys, xs], D, S
