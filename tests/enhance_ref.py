"""Plain numpy references for csrc/enhance_kernels.hip, written from OpenCV 3.3.1's sources (imgproc/src/histogram.cpp equalizeHist,
imgproc/src/clahe.cpp CLAHE_Impl::apply for CV_8UC1) and from nothing in the package or the oracle.  float32 exactly where upstream
computes in float, int64 everywhere else; and the case table the host and the device tests share."""
import numpy as np

F = np.float32


def _round_sat_u8(v):
    """saturate_cast<uchar>(cvRound(float)): round half to even, then clamp"""
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def equalize_hist(img):
    """cv2.equalizeHist: i0 = the first non-empty bin; one grey level only -> the image as it is (dst.setTo(i0)); otherwise
    lut[i] = saturate(cvRound(sum_{i0 < j <= i} hist[j] * scale)), scale = 255.f / (total - hist[i0]), lut[i <= i0] = 0."""
    img = np.asarray(img, np.uint8)
    hist = np.bincount(img.ravel(), minlength=256).astype(np.int64)
    total = int(img.size)
    i0 = int(np.flatnonzero(hist)[0])
    if hist[i0] == total:
        return np.full(img.shape, i0, np.uint8)
    scale = F(255.0) / F(total - int(hist[i0]))
    csum = np.cumsum(hist) - hist[i0]                         # sum over i0 < j <= i for i > i0
    lut = _round_sat_u8(csum.astype(F) * scale)
    lut[:i0 + 1] = 0
    return lut[img]


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101): ... 2 1 | 0 1 2 ... n-1 | n-2 n-3 ..., period 2 n - 2; n == 1 -> 0"""
    p = np.asarray(p, np.int64)
    if n == 1:
        return np.zeros_like(p)
    q = np.mod(p, 2 * n - 2)
    return np.where(q >= n, 2 * n - 2 - q, q)


def clahe(img, clip, tiles):
    """cv2.createCLAHE(clip, (tiles, tiles)).apply(img)"""
    img = np.asarray(img, np.uint8)
    h, w = img.shape
    tiles = int(tiles)
    if h % tiles == 0 and w % tiles == 0:
        src = img
    else:                                                     # copyMakeBorder(0, tiles - h % tiles, 0, tiles - w % tiles): a side that divides grows too
        eh, ew = h + (tiles - h % tiles), w + (tiles - w % tiles)
        src = img[reflect101(np.arange(eh), h)][:, reflect101(np.arange(ew), w)]
    th, tw = src.shape[0] // tiles, src.shape[1] // tiles
    area = th * tw
    clip_limit = 0
    if clip > 0.0:
        clip_limit = max(int(float(clip) * area / 256), 1)    # static_cast<int>(clipLimit_ * tileSizeTotal / histSize), clipLimit_ a double
    lut_scale = F(255.0) / F(area)
    luts = np.empty((tiles, tiles, 256), np.uint8)
    for ty in range(tiles):
        for tx in range(tiles):
            hist = np.bincount(src[ty * th:(ty + 1) * th, tx * tw:(tx + 1) * tw].ravel(), minlength=256).astype(np.int64)
            if clip_limit > 0:
                excess = int(np.maximum(hist - clip_limit, 0).sum())
                hist = np.minimum(hist, clip_limit)
                hist += excess // 256
                hist[:excess % 256] += 1
            luts[ty, tx] = _round_sat_u8(np.cumsum(hist).astype(F) * lut_scale)
    # CLAHE_Interpolation_Body: tile coordinates in float, LUT values blended in float, every operation rounded to float32
    inv_tw, inv_th = F(1.0) / F(tw), F(1.0) / F(th)
    txf = np.arange(w).astype(F) * inv_tw - F(0.5)
    tx1 = np.floor(txf).astype(np.int64); tx2 = tx1 + 1
    xa = (txf - tx1.astype(F)).astype(F); xa1 = (F(1.0) - xa).astype(F)
    tx1 = np.maximum(tx1, 0); tx2 = np.minimum(tx2, tiles - 1)
    tyf = np.arange(h).astype(F) * inv_th - F(0.5)
    ty1 = np.floor(tyf).astype(np.int64); ty2 = ty1 + 1
    ya = (tyf - ty1.astype(F)).astype(F); ya1 = (F(1.0) - ya).astype(F)
    ty1 = np.maximum(ty1, 0); ty2 = np.minimum(ty2, tiles - 1)
    v = img.astype(np.int64)
    l11 = luts[ty1[:, None], tx1[None, :], v].astype(F); l12 = luts[ty1[:, None], tx2[None, :], v].astype(F)
    l21 = luts[ty2[:, None], tx1[None, :], v].astype(F); l22 = luts[ty2[:, None], tx2[None, :], v].astype(F)
    xa, xa1, ya, ya1 = xa[None, :], xa1[None, :], ya[:, None], ya1[:, None]
    top = ((l11 * xa1).astype(F) + (l12 * xa).astype(F)).astype(F)
    bot = ((l21 * xa1).astype(F) + (l22 * xa).astype(F)).astype(F)
    res = ((top * ya1).astype(F) + (bot * ya).astype(F)).astype(F)
    return _round_sat_u8(res)


# ---- the case table ------------------------------------------------------------------------------------------------------------------------
SHAPES = ((1, 1), (1, 7), (7, 1), (2, 3), (3, 64), (5, 5), (13, 257), (64, 80), (203, 317), (100, 250), (255, 256), (257, 1025), (40, 40))
CONTENTS = ("uniform", "lowcontrast", "spike")
CLAHE_PARAMS = ((20, 5), (2, 8), (40, 3), (0, 4), (1, 1), (0.01, 2), (20, 64), (3.5, 7))      # (clipLimit, grid)


def image(shape, content, seed=0):
    rng = np.random.default_rng([seed, shape[0], shape[1], CONTENTS.index(content)])
    if content == "uniform":
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "lowcontrast":
        return rng.normal(110, 6, shape).clip(0, 255).astype(np.uint8)
    img = np.full(shape, 200, np.uint8)                       # one grey level but for one pixel (alone, a 1 x 1 image IS that pixel)
    img[shape[0] // 2, shape[1] // 3] = 3
    return img


def cases():
    """[(shape, content, op)], op = None for equalizeHist or (clip, grid): 13 shapes x 3 contents x (1 + 8) = 351"""
    return [(s, c, op) for s in SHAPES for c in CONTENTS for op in (None,) + CLAHE_PARAMS]


def apply(img, op):
    return equalize_hist(img) if op is None else clahe(img, op[0], op[1])
