"""Float64 checks of an ORB result (the numpy reference tests/orb_ref.py or the device): each stage against a plain high-precision
statement of the same quantity.  Every check returns the largest error it saw, so the tests can report it."""
import numpy as np

import orb_ref as R


def wrap_deg(d):
    return (np.asarray(d, np.float64) + 180.0) % 360.0 - 180.0


def check_harris(resp, a, b, c, rel=1e-6, block=7):
    """float32 response vs the float64 value of the same integer a, b, c; the bound is relative to the largest term (the formula cancels).
    -> the largest error relative to that term"""
    a, b, c = (np.asarray(v, np.float64) for v in (a, b, c))
    s4 = (1.0 / (4 * block * 255.0)) ** 4
    exact = (a * b - c * c - 0.04 * (a + b) ** 2) * s4
    term = np.maximum.reduce([a * b, c * c, 0.04 * (a + b) ** 2]) * s4
    err = np.abs(np.asarray(resp, np.float64) - exact) / np.maximum(term, np.finfo(np.float64).tiny)
    worst = float(err.max()) if err.size else 0.0
    assert worst <= rel, ("harris", worst, int(err.argmax()))
    return worst


def check_angle(angle, m01, m10, tol=0.01):
    """fastAtan2 vs float64 atan2(m01, m10) in degrees, wrapped; atan2(0, 0) = 0"""
    ref = np.degrees(np.arctan2(np.asarray(m01, np.float64), np.asarray(m10, np.float64)))
    err = np.abs(wrap_deg(np.asarray(angle, np.float64) - ref))
    worst = float(err.max()) if err.size else 0.0
    assert worst <= tol, ("angle", worst, int(err.argmax()))
    assert np.all((np.asarray(angle) >= 0) & (np.asarray(angle) < 360))
    return worst


def check_coords(kps, lx, ly, scale_factor=1.2, patch_size=31):
    """x, y = level coordinate x float32(scale ** l) within float32 rounding; size = patch_size * scale"""
    oc = kps["octave"].astype(np.int64)
    sc = np.array([float(np.float32(float(np.float32(scale_factor)) ** l)) for l in range(max(oc.max() + 1, 1) if oc.size else 1)])[oc]
    for got, lev in ((kps["x"], lx), (kps["y"], ly)):
        exact = np.asarray(lev, np.float64) * sc
        assert np.all(np.abs(got.astype(np.float64) - exact) <= np.maximum(exact, 1) * 2.0 ** -24), "coordinates"
    assert np.all(np.abs(kps["size"].astype(np.float64) - patch_size * sc) <= patch_size * sc * 2.0 ** -24), "size"
    assert np.all(kps["class_id"] == -1)


def check_descriptors(kps, desc, blurred, lx, ly, patch_size=31, near=1e-4):
    """every bit equals the bit from the pattern rotated in float64 by the keypoint's angle, sampled around the level coordinate on the
    (reflect-101 extended) blurred level, except tests where a rotated coordinate lies within `near` of a half-integer: those may take
    either rounding.  -> (bits checked, tests at a half-integer boundary, how many of those differ from the float64 rounding)"""
    if len(kps) == 0:
        return 0, 0, 0
    pat = R.pattern(patch_size).astype(np.float64)
    bits = np.unpackbits(desc, axis=1, bitorder="little").astype(bool)
    checked = boundary = flipped = 0
    for l in np.unique(kps["octave"]):
        sel = np.nonzero(kps["octave"] == l)[0]
        th = np.radians(kps["angle"][sel].astype(np.float64))
        cs, sn = np.cos(th)[:, None], np.sin(th)[:, None]
        rx = pat[None, :, 0] * cs - pat[None, :, 1] * sn
        ry = pat[None, :, 0] * sn + pat[None, :, 1] * cs
        half = lambda v: np.abs(v - np.floor(v) - 0.5) < near
        amb = half(rx) | half(ry)
        amb = amb[:, 0::2] | amb[:, 1::2]
        cx, cy = np.asarray(lx)[sel], np.asarray(ly)[sel]
        val = R.sample(blurred[l], cy[:, None] + np.floor(ry + 0.5).astype(np.int64),
                       cx[:, None] + np.floor(rx + 0.5).astype(np.int64)).astype(np.int16)
        want = val[:, 0::2] < val[:, 1::2]
        got = bits[sel]
        bad = (got != want) & ~amb
        assert not bad.any(), ("descriptor bits", int(bad.sum()), int(l))
        checked += int((~amb).sum()); boundary += int(amb.sum()); flipped += int(((got != want) & amb).sum())
    return checked, boundary, flipped


def bilinear64(src, dh, dw):
    """float64 resize(INTER_LINEAR): pixel-centre mapping, taps clamped to the image"""
    sh, sw = src.shape
    s = src.astype(np.float64)

    def taps(d, n):
        f = (np.arange(d) + 0.5) * (n / d) - 0.5
        i = np.floor(f).astype(np.int64)
        t = f - i
        t = np.where(i < 0, 0.0, t)
        i0 = np.clip(i, 0, n - 1)
        i1 = np.clip(i + 1, 0, n - 1)
        return i0, i1, t

    y0, y1, ty = taps(dh, sh)
    x0, x1, tx = taps(dw, sw)
    top = s[y0][:, x0] * (1 - tx) + s[y0][:, x1] * tx
    bot = s[y1][:, x0] * (1 - tx) + s[y1][:, x1] * tx
    return top * (1 - ty)[:, None] + bot * ty[:, None]


def check_pyramid(levels, tol=1.0):
    worst = 0.0
    for prev, cur in zip(levels[:-1], levels[1:]):
        ref = bilinear64(prev, *cur.shape)
        e = float(np.abs(cur.astype(np.float64) - ref).max())
        worst = max(worst, e)
    assert worst <= tol, ("pyramid", worst)
    return worst


def gauss64(img, taps=None, sigma=2.0):
    """float64 separable 7-tap filter with reflect-101 borders; taps default to the exact normalised Gaussian of sigma 2"""
    h, w = img.shape
    if taps is None:
        x = np.arange(-3, 4, dtype=np.float64)
        taps = np.exp(-x * x / (2 * sigma * sigma)); taps /= taps.sum()
    s = img.astype(np.float64)[R.reflect101(np.arange(-3, h + 3), h)][:, R.reflect101(np.arange(-3, w + 3), w)]
    rp = sum(taps[i] * s[:, i:i + w] for i in range(7))
    return sum(taps[i] * rp[i:i + h] for i in range(7))


def check_blur(levels, blurred):
    """GaussianBlur(7 x 7, sigma 2) on 8U rounds the normalised taps to 8-bit fixed point: cvRound(256 g) = 18 34 49 55 49 34 18, which
    sum to 257.  So the result is within 0.5 of the float64 filter with those taps / 256 (one final rounding, clipped at 255); against the
    exact Gaussian the taps' own error adds up to 255 x sum |q_i q_j / 256^2 - g_i g_j| (3.1 grey levels with the final rounding) on the worst 8-bit image.  -> (largest error against the quantised taps, against
    the exact Gaussian)"""
    x = np.arange(-3, 4, dtype=np.float64)
    g = np.exp(-x * x / 8.0); g /= g.sum()
    q = np.rint(g * 256)
    assert q.tolist() == [18, 34, 49, 55, 49, 34, 18]
    wq = we = 0.0
    for L, B in zip(levels, blurred):
        b = B.astype(np.float64)
        wq = max(wq, float(np.abs(b - np.minimum(gauss64(L, q / 256), 255.0)).max()))
        we = max(we, float(np.abs(b - gauss64(L)).max()))
    bound = 255 * np.abs(np.outer(q, q) / 65536 - np.outer(g, g)).sum() + 0.5      # the taps' worst case over 8-bit images
    assert wq <= 0.5 + 1e-9, ("blur against the 8-bit taps", wq)
    assert we <= bound, ("blur against the exact Gaussian", we, bound)
    return wq, we


def fast_brute(img, threshold):
    """FAST score by definition: the largest t (>= threshold) for which 9 contiguous ring pixels are all > v + t or all < v - t; 0 where
    the pixel is no corner at `threshold` (the 3 px frame is never scored)"""
    h, w = img.shape
    out = np.zeros((h, w), np.int64)
    if h < 7 or w < 7:
        return out
    im = img.astype(np.int64)
    v = im[3:h - 3, 3:w - 3]
    ring = np.stack([im[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in R.RING])
    t0 = min(max(int(threshold), 0), 255)

    def corner(t):
        ok = np.zeros(v.shape, bool)
        for side in (ring > v + t, ring < v - t):
            for s in range(16):
                run = np.ones(v.shape, bool)
                for j in range(9):
                    run &= side[(s + j) % 16]
                ok |= run
        return ok

    best = np.where(corner(t0), t0, -1)
    for t in range(t0 + 1, 256):
        c = corner(t)
        if not c.any():
            break
        best = np.where(c, t, best)
    out[3:h - 3, 3:w - 3] = np.where(best >= 0, best, 0)
    return out


def check_all(kps, desc, st, scale_factor=1.2, patch_size=31):
    """Harris, angle, coordinates, descriptors, pyramid and blurred levels of one result whose stats (orb_ref.detect_describe(...,
    stats=True, levels_out=True)) describe the same keypoints -> dict of the largest errors"""
    out = {}
    out["harris_rel"] = check_harris(kps["response"], st["a"], st["b"], st["c"])
    out["angle_deg"] = check_angle(kps["angle"], st["m01"], st["m10"])
    check_coords(kps, st["lx"], st["ly"], scale_factor, patch_size)
    if "levels" in st:
        out["pyramid_grey"] = check_pyramid(st["levels"])
        out["blur_grey"] = check_blur(st["levels"], st["blurred"])
        out["desc"] = check_descriptors(kps, desc, st["blurred"], st["lx"], st["ly"], patch_size)
    return out

