"""Independent float64 references for SIFT, written from OpenCV 3.3.1's SIFT_Impl without reusing tests/sift_ref.py's arithmetic.

tests/sift_ref.py is the bit-exact specification of the float32 kernels; a slip that is in both the spec and the kernel passes every
equality test.  The checks here judge the pyramid, the sub-pixel refinement and the orientation peaks of either implementation (the
device output in the GPU tests, the spec's in the CPU tests) against float64 restatements with their own sigma schedule, float64
Gaussian taps, np.linalg.solve and float64 histograms.  Each check returns the maxima it observed so the tests can print them.
The only code shared with the spec is fast_atan2_deg, which tests/test_sift_host.py pins against float64 atan2 on its own.
"""
import math

import numpy as np

import sift_ref as S

BORDER = 5


# ---- pyramid ---------------------------------------------------------------------------------------------------------------------
def sigma_schedule(sigma, L):
    """-> (initial blur of the 2x base, incremental blur of levels 1 .. L + 2).  Level i of an octave has total blur sigma * 2^(i / L);
    level i is level i - 1 blurred by sqrt(total_i^2 - total_{i-1}^2) = sigma * 2^((i - 1) / L) * sqrt(2^(2 / L) - 1).  The input is
    assumed blurred by 0.5, i.e. by 1.0 after the 2x upsample."""
    inc = [sigma * 2.0 ** ((i - 1) / L) * math.sqrt(2.0 ** (2.0 / L) - 1.0) for i in range(1, L + 3)]
    return math.sqrt(max(sigma * sigma - 1.0, 0.01)), inc


def taps64(sig):
    """normalised float64 Gaussian, length cvRound(8 sigma + 1) | 1"""
    n = int(np.rint(sig * 8 + 1)) | 1
    x = np.arange(n) - (n - 1) / 2
    t = np.exp(-x * x / (2 * sig * sig))
    return t / t.sum()


def _reflect101(idx, n):
    idx = np.asarray(idx, np.int64).copy()
    if n == 1:
        return np.zeros_like(idx)
    for _ in range(64):
        idx = np.where(idx < 0, -idx, idx)
        idx = np.where(idx >= n, 2 * n - 2 - idx, idx)
    assert np.all((idx >= 0) & (idx < n))
    return idx


def blur64(a, sig):
    t = taps64(sig)
    r = len(t) // 2
    for ax in (1, 0):
        n = a.shape[ax]
        acc = np.zeros_like(a)
        for k, w in enumerate(t):
            acc += w * np.take(a, _reflect101(np.arange(n) + k - r, n), axis=ax)
        a = acc
    return a


def upsample64(img):
    """bilinear 2x: destination d samples source (d + 0.5) / 2 - 0.5, clamped at the edges"""
    a = np.asarray(img, np.float64)
    for ax in (1, 0):
        n = a.shape[ax]
        s = (np.arange(2 * n) + 0.5) / 2 - 0.5
        i0 = np.floor(s).astype(np.int64)
        f = s - i0
        sh = [1, 1]; sh[ax] = 2 * n
        a = (np.take(a, np.clip(i0, 0, n - 1), axis=ax) * (1 - f).reshape(sh) +
             np.take(a, np.clip(i0 + 1, 0, n - 1), axis=ax) * f.reshape(sh))
    return a


def decimate64(a):
    h, w = a.shape
    dh, dw = h // 2, w // 2
    sy = np.minimum((np.arange(dh) * h) // dh, h - 1)
    sx = np.minimum((np.arange(dw) * w) // dw, w - 1)
    return a[sy][:, sx]


def n_octaves_cv(h, w):
    """cvRound(log2(min(2h, 2w)) - 2) + 1 (firstOctave = -1)"""
    return int(np.rint(math.log2(min(2 * h, 2 * w)) - 2)) + 1


def pyramid64(img, sigma=1.6, L=3):
    sig0, inc = sigma_schedule(sigma, L)
    gauss, dog = [], []
    for o in range(n_octaves_cv(*np.shape(img))):
        lv = [blur64(upsample64(img), sig0) if o == 0 else decimate64(gauss[-1][L])]
        for i in range(1, L + 3):
            lv.append(blur64(lv[-1], inc[i - 1]))
        gauss.append(lv)
        dog.append([lv[i + 1] - lv[i] for i in range(L + 2)])
    return gauss, dog


def pyramid_error(img, gauss, dog, sigma=1.6, L=3):
    """max |level - float64 level| over every Gaussian and DoG level -> (max gauss error, max dog error)"""
    g64, d64 = pyramid64(img, sigma, L)
    assert len(gauss) == len(g64) and len(dog) == len(d64)
    eg = ed = 0.0
    for o in range(len(g64)):
        assert len(gauss[o]) == L + 3 and len(dog[o]) == L + 2
        for i in range(L + 3):
            assert gauss[o][i].shape == g64[o][i].shape, (o, i)
            eg = max(eg, float(np.abs(gauss[o][i] - g64[o][i]).max()))
        for i in range(L + 2):
            ed = max(ed, float(np.abs(dog[o][i] - d64[o][i]).max()))
    return eg, ed


# ---- keypoints -> their octave-internal candidate --------------------------------------------------------------------------------
def unpack(kps, sigma, L):
    """keypoint fields -> float64 arrays o (octave of the pyramid, 0 = the 2x base), layer, u = c + xc, v = r + xr, xi"""
    octv = kps["octave"].astype(np.int64) & 255
    octv = np.where(octv < 128, octv, octv - 256)
    o = octv + 1
    layer = (kps["octave"].astype(np.int64) >> 8) & 255
    s = np.ldexp(1.0, o.astype(np.int32))
    u = kps["x"].astype(np.float64) * 2 / s
    v = kps["y"].astype(np.float64) * 2 / s
    t = np.log2(kps["size"].astype(np.float64) * 2 / (2 * float(np.float32(sigma)) * s)) * L
    return o, layer, u, v, t - layer


# ---- refinement ------------------------------------------------------------------------------------------------------------------
def _grad_hess(D, l, r, c):
    """float64 first derivatives and Hessian (rows x, y, s) of the DoG stack D at integer points, in grey levels / 255"""
    at = lambda dl, dr, dc: D[l + dl, r + dr, c + dc].astype(np.float64) / 255.0
    v = at(0, 0, 0)
    g = np.stack([(at(0, 0, 1) - at(0, 0, -1)) / 2, (at(0, 1, 0) - at(0, -1, 0)) / 2, (at(1, 0, 0) - at(-1, 0, 0)) / 2], -1)
    dxx = at(0, 0, 1) + at(0, 0, -1) - 2 * v
    dyy = at(0, 1, 0) + at(0, -1, 0) - 2 * v
    dss = at(1, 0, 0) + at(-1, 0, 0) - 2 * v
    dxy = (at(0, 1, 1) - at(0, 1, -1) - at(0, -1, 1) + at(0, -1, -1)) / 4
    dxs = (at(1, 0, 1) - at(1, 0, -1) - at(-1, 0, 1) + at(-1, 0, -1)) / 4
    dys = (at(1, 1, 0) - at(1, -1, 0) - at(-1, 1, 0) + at(-1, -1, 0)) / 4
    H = np.stack([np.stack([dxx, dxy, dxs], -1), np.stack([dxy, dyy, dys], -1), np.stack([dxs, dys, dss], -1)], -2)
    return v, g, H


def _offset(H, g):
    """-H^-1 g by np.linalg.solve; a singular H gives 0 (Matx::solve's zeros)"""
    out = np.zeros_like(g)
    ok = np.abs(np.linalg.det(H)) > 0
    if ok.any():
        out[ok] = -np.linalg.solve(H[ok], g[ok][..., None])[..., 0]
    return out


def detect64(dog, contrast=0.04, edge=10.0, L=3, rel=1e-5, near=1e-4):
    """findScaleSpaceExtrema + adjustLocalExtrema in float64 on given DoG levels -> (survivors, marginal).  survivors maps
    (o, layer, r, c) -> (xc, xr, xi, |contrast|); marginal holds every location a candidate visited whose fate hangs on a comparison
    within `near` of a rounding boundary or `rel` (relative) of a threshold, where float32 and float64 may disagree."""
    thr = math.floor(0.5 * contrast / L * 255)
    surv, marg = {}, set()
    for o in range(len(dog)):
        D = np.stack(dog[o]).astype(np.float32)
        n, R, C = D.shape
        if R <= 2 * BORDER or C <= 2 * BORDER:
            continue
        cand = []
        for l in range(1, L + 1):
            v = D[l, BORDER:R - BORDER, BORDER:C - BORDER]
            nb = [D[l + a, BORDER + b:R - BORDER + b, BORDER + c:C - BORDER + c]
                  for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1) if (a, b, c) != (0, 0, 0)]
            mx = np.max(nb, 0); mn = np.min(nb, 0)
            m = (np.abs(v) > thr) & (((v > 0) & (v >= mx)) | ((v < 0) & (v <= mn)))
            rr, cc = np.nonzero(m)
            cand += [(l, int(a) + BORDER, int(b) + BORDER) for a, b in zip(rr, cc)]
        for l, r, c in cand:
            visited, marginal, x = [], False, None
            for _ in range(5):
                visited.append((o, l, r, c))
                _v, g, H = _grad_hess(D, l, r, c)
                x = _offset(H, g)
                ax = np.abs(x)
                marginal |= bool(np.any(np.abs(ax - 0.5) < near))
                if np.all(ax < 0.5):
                    break
                if np.any(ax > 2147483647 // 3):
                    x = None
                    break
                rd = np.rint(x)
                marginal |= bool(np.any(np.abs(np.abs(x - np.floor(x)) - 0.5) < near))
                c += int(rd[0]); r += int(rd[1]); l += int(rd[2])
                if l < 1 or l > L or c < BORDER or c >= C - BORDER or r < BORDER or r >= R - BORDER:
                    x = None
                    break
            else:
                x = None
            key = (o, l, r, c)
            if x is not None:
                v, g, H = _grad_hess(D, l, r, c)
                contr = v + 0.5 * float(g @ x)
                a = abs(contr) * L
                marginal |= abs(a - contrast) <= rel * contrast
                ok = a >= contrast
                dxx, dyy, dxy = H[0, 0], H[1, 1], H[0, 1]
                tr, det = dxx + dyy, dxx * dyy - dxy * dxy
                lhs, rhs = tr * tr * edge, (edge + 1) ** 2 * det
                marginal |= abs(lhs - rhs) <= rel * max(abs(lhs), abs(rhs)) or abs(det) <= rel * abs(dxx * dyy)
                ok = ok and det > 0 and lhs < rhs
                if ok:
                    surv[key] = (x[0], x[1], x[2], abs(contr))
            if marginal:
                marg.update(visited + [key])
    return surv, marg


def check_refinement(dog, kps, contrast=0.04, edge=10.0, sigma=1.6, L=3):
    """Every keypoint's candidate against detect64 on the same DoG levels: the same set of (octave, layer, row, col) survives
    (marginal decisions excepted), and on common candidates the offsets, size and response agree.  -> dict of maxima"""
    surv, marg = detect64(dog, contrast, edge, L)
    o, layer, u, v, xi = unpack(kps, sigma, L)
    c = np.rint(u).astype(np.int64); r = np.rint(v).astype(np.int64)
    dev = {}
    for q in range(len(kps)):
        dev.setdefault((int(o[q]), int(layer[q]), int(r[q]), int(c[q])), q)
    missing = [k for k in surv if k not in dev and k not in marg]
    extra = [k for k in dev if k not in surv and k not in marg]
    assert not missing, ("float64 keypoints the implementation lacks", len(missing), missing[:5])
    assert not extra, ("keypoints float64 rejects", len(extra), extra[:5])
    e_px = e_size = e_resp = 0.0
    for k, q in dev.items():
        if k not in surv:
            continue
        xc, xr, xs, resp = surv[k]
        _o, l, rr, cc = k
        e_px = max(e_px, abs(u[q] - cc - xc), abs(v[q] - rr - xr), abs(xi[q] - xs))
        s = 2.0 ** _o
        size64 = sigma * 2.0 ** ((l + xs) / L) * s * 2 * 0.5
        e_size = max(e_size, abs(float(kps["size"][q]) / size64 - 1))
        e_resp = max(e_resp, abs(float(kps["response"][q]) / resp - 1))
    return dict(n_dev=len(dev), n_f64=len(surv), n_marginal=len(marg), offset=e_px, size=e_size, response=e_resp)


# ---- orientation -----------------------------------------------------------------------------------------------------------------
def orientation_peaks64(img, px, py, scl):
    """float64 calcOrientationHist at integer (px, py) of a Gaussian level -> (smoothed 36-bin histogram, its max)"""
    rows, cols = img.shape
    radius = int(np.rint(4.5 * scl))
    sig = 1.5 * scl
    ii = np.arange(-radius, radius + 1)
    I, J = np.meshgrid(ii[(py + ii > 0) & (py + ii < rows - 1)], ii[(px + ii > 0) & (px + ii < cols - 1)], indexing="ij")
    y = py + I.ravel(); x = px + J.ravel()
    dx = img[y, x + 1] - img[y, x - 1]
    dy = img[y - 1, x] - img[y + 1, x]
    ori = S.fast_atan2_deg(dy, dx).astype(np.float64)
    w = np.exp(-(I.ravel() ** 2 + J.ravel() ** 2) / (2 * sig * sig)) * np.hypot(dx.astype(np.float64), dy.astype(np.float64))
    b = np.rint(ori * 36 / 360).astype(np.int64) % 36
    h = np.bincount(b, w, 36)
    hs = (np.roll(h, 2) + np.roll(h, -2)) / 16 + (np.roll(h, 1) + np.roll(h, -1)) * 4 / 16 + h * 6 / 16
    return hs


def check_orientation(gauss, kps, sigma=1.6, L=3, ratio=0.8, margin=1e-4, tol=1e-3):
    """Keypoints grouped by (x, y, size): every angle lies in [0, 360) within tol degrees of a float64 peak at or above
    ratio * max (less margin), and every float64 peak clearly above it (by margin, relative) is present.  -> dict of maxima"""
    o, layer, u, v, _xi = unpack(kps, sigma, L)
    groups = {}
    for q in range(len(kps)):
        groups.setdefault((float(kps["x"][q]), float(kps["y"][q]), float(kps["size"][q])), []).append(q)
    assert np.all((kps["angle"] >= 0) & (kps["angle"] < 360)), "angles outside [0, 360)"
    e_ang, n_multi = 0.0, 0
    for qs in groups.values():
        q = qs[0]
        s = 2.0 ** o[q]
        scl = float(kps["size"][q]) * 2 * 0.5 / s
        hs = orientation_peaks64(gauss[int(o[q])][int(layer[q])], int(np.rint(u[q])), int(np.rint(v[q])), scl)
        hmax = hs.max()
        hl, hr = np.roll(hs, 1), np.roll(hs, -1)
        is_pk = (hs > hl) & (hs > hr)
        j = np.arange(36)
        with np.errstate(divide="ignore", invalid="ignore"):
            b = j + 0.5 * (hl - hr) / (hl - 2 * hs + hr)
        ang = np.mod(360 - 10 * b, 360)
        loose = is_pk & (hs >= ratio * hmax * (1 - margin))
        strict = is_pk & (hs >= ratio * hmax * (1 + margin)) & (hs - np.maximum(hl, hr) > margin * hmax)
        dev = np.array([float(kps["angle"][k]) for k in qs])
        n_multi += len(qs) >= 3
        d = lambda a, bb: np.abs((a - bb + 180) % 360 - 180)
        for a in dev:
            err = d(a, ang[loose]).min() if loose.any() else np.inf
            assert err <= tol, ("angle matches no float64 peak", a, ang[loose], hs[loose] / hmax)
            e_ang = max(e_ang, float(err))
        for a in ang[strict]:
            assert d(dev, a).min() <= tol, ("float64 peak missing", a, dev)
    return dict(groups=len(groups), angle=e_ang, multi=n_multi)


# ---- inputs where kernels go wrong -------------------------------------------------------------------------------------------------
def adversarial_images():
    """-> [(name, u8 image)], each built to reach a path that benign inputs miss:
      blobs_int, blobs_half  symmetric Gaussian blobs on integer and half-integer centres: near-tied histogram bins, candidates
                             with 3 or more orientations;
      discs                  saturated discs on a flat background: 0 / 255 plateaus, >= ties in the 26-neighbour test;
      checker                a checkerboard: ties everywhere, many orientations per candidate;
      spikes                 isolated single-pixel spikes: the DoG response falls monotonically with scale, so there is no
                             scale-space extremum and the result must be empty after a non-trivial pyramid;
      reset                  a ramp and a blob centred on original row 31.75, which octave 1 samples as its row 32, so the
                             gradient histogram there is nearly symmetric about 0 degrees; two pixels are nudged by one grey level
                             (found by search) so that the float32 peak interpolation gives bin +2.2e-7, i.e. 360 - 10 * bin == 360:
                             the keypoint's angle reaches the 360 -> 0 reset;
      duplicates             smoothed noise (seed chosen by search) where two candidates refine to the same keypoint, which
                             removeDuplicated drops."""
    out = []
    yy, xx = np.mgrid[0:128, 0:160].astype(np.float64)
    for name, off in (("blobs_int", 0.0), ("blobs_half", 0.5)):
        f = np.full(yy.shape, 20.0)
        for cy in range(16, 128, 32):
            for cx in range(16, 160, 32):
                f += 200 * np.exp(-((yy - cy - off) ** 2 + (xx - cx - off) ** 2) / (2 * 4.0 ** 2))
        out.append((name, np.clip(np.rint(f), 0, 255).astype(np.uint8)))
    d = np.zeros((120, 150), np.uint8)
    y, x = np.mgrid[0:120, 0:150]
    for cy in range(15, 120, 30):
        for cx in range(15, 150, 30):
            d[(y - cy) ** 2 + (x - cx) ** 2 <= (3 + (cx // 30) % 3 * 2) ** 2] = 255
    out.append(("discs", d))
    out.append(("checker", (((y // 8 + x // 8) % 2) * 255).astype(np.uint8)))
    s = np.zeros((96, 128), np.uint8)
    s[7::17, 9::19] = 255
    out.append(("spikes", s))
    yy, xx = np.mgrid[0:64, 0:80].astype(np.float64)
    r = np.clip(np.rint(40 + 1.5 * xx + 150 * np.exp(-((yy - 31.75) ** 2 + (xx - 40.25) ** 2) / (2 * 5.0 ** 2))), 0, 255).astype(np.uint8)
    r[40, 43] += 1
    r[32, 27] -= 1
    out.append(("reset", r))
    n = np.random.default_rng(55).integers(0, 256, (64, 96), dtype=np.uint8).astype(np.float64)
    for ax in (0, 1):
        n = sum(np.roll(n, k, axis=ax) for k in range(-2, 3)) / 5
    out.append(("duplicates", np.clip(np.rint(n), 0, 255).astype(np.uint8)))
    return out
