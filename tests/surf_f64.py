"""Float64 checks of a SURF result (the CPU oracle's or the device's): every stage of surf.cpp stated once more in plain numpy float64,
from the pixels up, with nothing imported from the library or the oracle.  Each check takes a result, asserts its bound and returns what
it saw (the largest error, the number of items it exempted), so the tests can report them.

How the bounds were set: every *_MEASURED constant is the largest error of the CPU oracle against this reference over all cases of
tests/surf_f64_cases.py (tests/test_surf_f64_host.py prints the figures again on every run); the bound beside it is that figure times 4.
The device's output never entered a bound.  The epsilons and caps are stated conditions, not measurements.

The keyword arguments `corner`, `xy_weight`, `sigma` and `rot_sign` exist so that the host test can plant one transcription mistake at a
time and see the oracle's results fall outside the bounds; the defaults are surf.cpp's."""
import numpy as np

# ---- measured on the CPU (oracle against this reference, worst over all cases) and the bounds that follow: bound = 4 x measured ----
LAYER_MEASURED = 1.21e-7          # |det32 - det64| / (Ax Ay + 0.81 Axy^2), A = sum of the absolute Haar terms of a response
LAYER_BOUND = 4 * LAYER_MEASURED
POS_MEASURED = 8.4e-5             # keypoint against the float64 keypoint, in layer steps: |dx|, |dy| / sampling step, |dsize| / size step
POS_BOUND = 4 * POS_MEASURED
ORI_MEASURED = 0.0091             # degrees, over the keypoints that needed no exemption
ORI_BOUND = 4 * ORI_MEASURED
DESC_CAP = 1.9e-2                 # a descriptor bound at or above 2e-2 no longer separates the planted mistakes: where 4 x measured
                                  # would pass it, the bound is this (narrower) figure instead
DESC_Q_MEASURED = 7.7e-3          # descriptor component, reference rounded to 8 bits after sampling and after the resize
DESC_Q_BOUND = min(4 * DESC_Q_MEASURED, DESC_CAP)
DESC_R_MEASURED = 9.4e-3          # descriptor component, reference never rounded
DESC_R_BOUND = min(4 * DESC_R_MEASURED, DESC_CAP)

# ---- stated conditions ----
EPS_GAP = 1e-6                  # a maximum / threshold decision is firm when its margin exceeds this fraction of the error scale
EPS_STEP = 1e-3                 # |x| <= 1 is firm when 1 - max|x| exceeds this
COND_FIRM = 1e3                 # a 3 x 3 system with a larger condition number is ill-conditioned: never firm
ORI_TIE = 1e-3                  # a second window within this fraction of the best modulus may win instead: float32 sums of up to
                                # 113 terms differ from the float64 ones by less than 113 x 2^-24 = 7e-6 of the modulus
ANGLE_EPS = 0.0125              # degrees: fastAtan2 is a degree-7 polynomial, within 0.01 degree of atan2; a sample angle this close
                                # to x.5 may round to either whole degree, which moves it between windows
HALF_EPS = 1e-4                 # a coordinate this close to a half-integer may round either way
CAP_NONFIRM = 0.02              # per case: share of float64 keypoints that may be non-firm
CAP_ORI_EXEMPT = 0.01           # per case: share of keypoints that may be exempt from the orientation check

HAAR_DX = ((0, 2, 3, 7, 1), (3, 2, 6, 7, -2), (6, 2, 9, 7, 1))
HAAR_DY = ((2, 0, 7, 3, 1), (2, 3, 7, 6, -2), (2, 6, 7, 9, 1))
HAAR_DXY = ((1, 1, 4, 4, 1), (5, 1, 8, 4, -1), (1, 5, 4, 8, -1), (5, 5, 8, 8, 1))
ORI_RADIUS, ORI_SIGMA, PATCH, DESC_SIGMA = 6, 2.5, 20, 3.3


def wrap_deg(d):
    return (np.asarray(d, np.float64) + 180.0) % 360.0 - 180.0


def integral64(img):
    h, w = img.shape
    S = np.zeros((h + 1, w + 1), np.float64)
    S[1:, 1:] = np.asarray(img, np.float64).cumsum(0).cumsum(1)
    return S


def layer_size(o, l):
    return (9 + 6 * l) << o


def _haar(S, yy, xx, spec, size, corner):
    """sum of box means of one 9 x 9 pattern stretched to `size`; corners rounded as resizeHaarPattern rounds them
    -> (response, sum of the absolute terms)"""
    r = np.float32(size) / np.float32(9)
    tot = mag = 0.0
    for a, b, c, d, wt in spec:
        x0, y0, x1, y1 = (int(corner(r * np.float32(v))) for v in (a, b, c, d))
        v = (S[yy + y1, xx + x1] - S[yy + y0, xx + x1] - S[yy + y1, xx + x0] + S[yy + y0, xx + x0]) * (wt / ((x1 - x0) * (y1 - y0)))
        tot = tot + v
        mag = mag + np.abs(v)
    return tot, mag


def layers(img, n_octaves=4, n_layers=3, corner=np.rint, xy_weight=0.81):
    """calcLayerDetAndTrace from pixel box sums -> list over o * (n_layers + 2) + l of dicts: size, step, det, trace and the error scale
    Ax Ay + 0.81 Axy^2 (the response cancels, so its own size is no scale); all three are zero outside the cells a layer samples"""
    h, w = img.shape
    S = integral64(img)
    out = []
    for o in range(n_octaves):
        step = 1 << o
        for l in range(n_layers + 2):
            size = layer_size(o, l)
            det = np.zeros((h // step, w // step)); tr = np.zeros_like(det); sc = np.zeros_like(det); ts = np.zeros_like(det)
            if size <= h and size <= w:
                ni, nj, m = 1 + (h - size) // step, 1 + (w - size) // step, (size // 2) // step
                yy, xx = np.meshgrid(np.arange(ni) * step, np.arange(nj) * step, indexing="ij")
                dx, ax = _haar(S, yy, xx, HAAR_DX, size, corner)
                dy, ay = _haar(S, yy, xx, HAAR_DY, size, corner)
                dxy, axy = _haar(S, yy, xx, HAAR_DXY, size, corner)
                det[m:m + ni, m:m + nj] = dx * dy - xy_weight * dxy * dxy
                tr[m:m + ni, m:m + nj] = dx + dy
                sc[m:m + ni, m:m + nj] = ax * ay + xy_weight * axy * axy
                ts[m:m + ni, m:m + nj] = ax + ay
            out.append(dict(size=size, step=step, det=det, trace=tr, scale=sc, trace_scale=ts))
    return out


def check_layers(ref, got, bound=None):
    """float32 layers [(det, trace), ...] in the order of layers() against the float64 ones -> largest det error relative to the scale.
    The trace is a plain sum: each Haar weight is rounded to float32 once, each response once (it is accumulated in double) and their
    sum once, so it lies within 3 x 2^-24 of Ax + Ay; it is held to 2^-22 of that."""
    bound = LAYER_BOUND if bound is None else bound
    worst = 0.0
    for L, (d32, t32) in zip(ref, got):
        assert d32.shape == L["det"].shape
        on = L["scale"] > 0
        assert np.all(np.asarray(d32)[~on] == 0) and np.all(np.asarray(t32)[~on] == 0), "layer cells outside the sampled area"
        if not on.any():
            continue
        e = np.abs(d32[on].astype(np.float64) - L["det"][on]) / L["scale"][on]
        worst = max(worst, float(e.max()))
        et = np.abs(t32[on].astype(np.float64) - L["trace"][on]) / L["trace_scale"][on]
        assert float(et.max()) <= 2.0 ** -22, ("layer trace", float(et.max()), L["size"])
    assert worst <= bound, ("layer det", worst, bound)
    return worst


KP64 = np.dtype([("octave", "i4"), ("layer", "i4"), ("i", "i4"), ("j", "i4"), ("x", "f8"), ("y", "f8"), ("size", "f8"), ("response", "f8"),
                 ("scale", "f8"), ("class_id", "i4"), ("step", "i4"), ("ds", "i4"), ("gap", "f8"), ("xm", "f8"), ("cond", "f8"), ("firm", "?")])


def keypoints64(L, shape, hessian=100.0, n_octaves=4, n_layers=3):
    """findMaximaInLayer + interpolateKeypoint on the float64 layers: every strict 26-neighbour maximum above the threshold whose
    3 x 3 system (numpy.linalg.solve) gives |x| <= 1 with not all components zero -- and, marked not firm, every candidate within
    the epsilons of those decisions.  gap = the smallest of the 26 neighbour margins and the threshold margin, relative to the scale"""
    h, w = shape
    out = []
    for o in range(n_octaves):
        step = 1 << o
        lr, lc = h // step, w // step
        for l in range(1, n_layers + 1):
            k = o * (n_layers + 2) + l
            size, m = L[k]["size"], (L[k + 1]["size"] // 2) // step + 1
            if lr - m <= m or lc - m <= m:
                continue
            cell = lambda A, di, dj: A[m + di:lr - m + di, m + dj:lc - m + dj]
            N = np.stack([cell(L[k + a]["det"], di, dj) for a in (-1, 0, 1) for di in (-1, 0, 1) for dj in (-1, 0, 1)])
            E = np.max(np.stack([cell(L[k + a]["scale"], di, dj) for a in (-1, 0, 1) for di in (-1, 0, 1) for dj in (-1, 0, 1)]), 0)
            v = N[13]
            gap = np.minimum(v - np.max(np.delete(N, 13, 0), 0), v - hessian)
            ii, jj = np.nonzero((gap > -EPS_GAP * E) & (E > 0))
            if len(ii) == 0:
                continue
            n = N[:, ii, jj].reshape(3, 9, -1)
            b = -np.stack([(n[1, 5] - n[1, 3]) / 2, (n[1, 7] - n[1, 1]) / 2, (n[2, 4] - n[0, 4]) / 2], -1)
            a01 = (n[1, 8] - n[1, 6] - n[1, 2] + n[1, 0]) / 4
            a02 = (n[2, 5] - n[2, 3] - n[0, 5] + n[0, 3]) / 4
            a12 = (n[2, 7] - n[2, 1] - n[0, 7] + n[0, 1]) / 4
            A = np.stack([np.stack([n[1, 3] - 2 * n[1, 4] + n[1, 5], a01, a02], -1),
                          np.stack([a01, n[1, 1] - 2 * n[1, 4] + n[1, 7], a12], -1),
                          np.stack([a02, a12, n[0, 4] - 2 * n[1, 4] + n[2, 4]], -1)], -2)
            cond = np.linalg.cond(A)
            ok = np.isfinite(cond) & (cond < 1e15)
            x = np.zeros_like(b)
            x[ok] = np.linalg.solve(A[ok], b[ok][..., None])[..., 0]
            xm = 1 - np.abs(x).max(1)
            ok &= (xm >= -EPS_STEP) & np.any(x != 0, 1)
            r = np.zeros(int(ok.sum()), KP64)
            ii, jj, x, xm, cond = ii[ok] + m, jj[ok] + m, x[ok], xm[ok], cond[ok]
            ds = size - L[k - 1]["size"]
            r["octave"], r["layer"], r["i"], r["j"], r["step"], r["ds"] = o, l, ii, jj, step, ds
            r["x"] = step * (jj - (size // 2) // step) + (size - 1) * 0.5 + x[:, 0] * step
            r["y"] = step * (ii - (size // 2) // step) + (size - 1) * 0.5 + x[:, 1] * step
            r["size"] = size + x[:, 2] * ds
            r["response"] = L[k]["det"][ii, jj]
            r["scale"] = E[ii - m, jj - m]
            r["class_id"] = np.sign(L[k]["trace"][ii, jj]).astype(np.int32)
            r["gap"], r["xm"], r["cond"] = gap[ii - m, jj - m] / r["scale"], xm, cond
            r["firm"] = (r["gap"] > EPS_GAP) & (xm > EPS_STEP) & (cond < COND_FIRM)
            out.append(r)
    return np.concatenate(out) if out else np.zeros(0, KP64)


def check_order(kps):
    """KeypointGreater: response, size and octave descending, then y descending, then x ascending"""
    if len(kps) < 2:
        return
    a, b = kps[:-1], kps[1:]
    later = np.zeros(len(a), bool)          # True where a must come after b
    tied = np.ones(len(a), bool)
    for f, sign in (("response", 1), ("size", 1), ("octave", 1), ("y", 1), ("x", -1)):
        u, v = a[f].astype(np.float64) * sign, b[f].astype(np.float64) * sign
        later |= tied & (u < v)
        tied &= u == v
    assert not later.any(), ("keypoint order", int(np.nonzero(later)[0][0]))


def check_keypoints(img, kps, params=None, L=None, pos_bound=None, layer_bound=None):
    """Both directions.  Every reported keypoint has a float64 keypoint of its octave within POS_BOUND layer steps (x, y in sampling
    steps; size against size + x2 ds in size steps, after the half unit that rounding to an integer may take), met by no other reported
    keypoint, of equal class_id, with the response within LAYER_BOUND of the float64 det of that cell.  Every firm float64 keypoint is
    reported.  The list is in KeypointGreater order.
    -> dict: n, n64, nonfirm (float64 keypoints not firm), unreported (of those), pos (largest position error), resp (largest response
    error relative to the scale), size_exempt (sizes that differ from the rounded float64 size, within the bound of a half-integer),
    match (index of the float64 keypoint per reported one) and k64"""
    p = dict(hessian=100.0, n_octaves=4, n_layers=3)
    p.update({k: v for k, v in (params or {}).items() if k in p})
    pos_bound = POS_BOUND if pos_bound is None else pos_bound
    layer_bound = LAYER_BOUND if layer_bound is None else layer_bound
    if L is None:
        L = layers(img, p["n_octaves"], p["n_layers"])
    k64 = keypoints64(L, img.shape, **p)
    check_order(kps)
    assert np.all((kps["octave"] >= 0) & (kps["octave"] < p["n_octaves"])), "octave"
    assert np.all(kps["size"] == np.rint(kps["size"])), "size is an integer"
    match = np.full(len(kps), -1, np.int64)
    err = np.zeros(len(kps))
    for o in range(p["n_octaves"]):
        a, b = np.nonzero(kps["octave"] == o)[0], np.nonzero(k64["octave"] == o)[0]
        if len(a) == 0:
            continue
        assert len(b) > 0, ("no float64 keypoint in octave", o)
        q = k64[b]
        d = np.maximum(np.abs(kps["x"][a, None] - q["x"][None]), np.abs(kps["y"][a, None] - q["y"][None])) / (1 << o)
        d = np.maximum(d, np.maximum(np.abs(kps["size"][a, None] - q["size"][None]) - 0.5, 0) / q["ds"][None])
        best = d.argmin(1)
        match[a], err[a] = b[best], d[np.arange(len(a)), best]
    worst = float(err.max()) if len(kps) else 0.0
    assert worst <= pos_bound, ("keypoint without a float64 keypoint", worst, int(err.argmax()))
    assert len(np.unique(match)) == len(match), "two reported keypoints at one float64 keypoint"
    m = k64[match]
    assert np.array_equal(kps["class_id"], m["class_id"]), ("class_id", int(np.nonzero(kps["class_id"] != m["class_id"])[0][0]))
    cellscale = np.array([L[o * (p["n_layers"] + 2) + l]["scale"][i, j] for o, l, i, j in zip(m["octave"], m["layer"], m["i"], m["j"])])
    rerr = np.abs(kps["response"].astype(np.float64) - m["response"]) / cellscale if len(kps) else np.zeros(0)
    resp = float(rerr.max()) if len(kps) else 0.0
    assert resp <= layer_bound, ("response", resp, int(rerr.argmax()))
    assert np.all(kps["response"] > np.float32(p["hessian"])), "response not above the threshold"
    seen = np.zeros(len(k64), bool)
    seen[match] = True
    missing = k64["firm"] & ~seen
    assert not missing.any(), ("firm float64 keypoint not reported", int(missing.sum()), k64[missing][:3])
    return dict(n=len(kps), n64=len(k64), nonfirm=int((~k64["firm"]).sum()), unreported=int((~seen).sum()), pos=worst, resp=resp,
                size_exempt=int((kps["size"] != np.rint(m["size"])).sum()), match=match, k64=k64)


def gauss(n, sigma):
    x = np.arange(n) - (n - 1) * 0.5
    g = np.exp(-x * x / (2 * sigma * sigma))
    return g / g.sum()


def sample_scale(size):
    """s = size * 1.2f / 9.0f as float32 arithmetic evaluates it: the integer decisions below (wavelet and window side) hang on it"""
    return np.asarray(size, np.float32) * np.float32(1.2) / np.float32(9.0)


def wavelet_side(size):
    return 2 * np.rint(np.float32(2) * sample_scale(size)).astype(np.int64)


def window_side(size):
    return (np.float32(PATCH + 1) * sample_scale(size)).astype(np.int64)


def orientation_samples(img, kps):
    """For each keypoint (from its reported x, y, size): the 113 samples of the radius-6 disc, exact integer Haar sums of side
    2 round(2s) weighted by the float64 Gaussian, and their float64 atan2 in degrees -> (X, Y, angle, inside, near_half)"""
    h, w = img.shape
    S = integral64(img)
    g = gauss(2 * ORI_RADIUS + 1, ORI_SIGMA)
    pts = [(i, j) for i in range(-ORI_RADIUS, ORI_RADIUS + 1) for j in range(-ORI_RADIUS, ORI_RADIUS + 1) if i * i + j * j <= ORI_RADIUS ** 2]
    pi, pj = np.array(pts).T
    wt = g[pi + ORI_RADIUS] * g[pj + ORI_RADIUS]
    s = sample_scale(kps["size"]).astype(np.float64)[:, None]
    gws = wavelet_side(kps["size"])[:, None]
    assert np.all(gws <= min(h, w) + 1), "a keypoint the reference deletes (wavelet larger than the integral)"
    fx = kps["x"].astype(np.float64)[:, None] + pi[None] * s - (gws - 1) / 2
    fy = kps["y"].astype(np.float64)[:, None] + pj[None] * s - (gws - 1) / 2
    half = lambda v: np.abs(v - np.floor(v) - 0.5) < HALF_EPS
    near_half = (half(fx) | half(fy)).any(1)
    x, y = np.rint(fx).astype(np.int64), np.rint(fy).astype(np.int64)
    inside = (y >= 0) & (y < h + 1 - gws) & (x >= 0) & (x < w + 1 - gws)
    x, y = np.where(inside, x, 0), np.where(inside, y, 0)
    hs = gws // 2
    box = lambda x0, y0, x1, y1: S[y + y1, x + x1] - S[y + y0, x + x1] - S[y + y1, x + x0] + S[y + y0, x + x0]
    area = (hs * gws).astype(np.float64)
    X = np.where(inside, (box(hs, 0, gws, gws) - box(0, 0, hs, gws)) / area * wt[None], 0.0)
    Y = np.where(inside, (box(0, 0, gws, hs) - box(0, hs, gws, gws)) / area * wt[None], 0.0)
    return X, Y, np.degrees(np.arctan2(Y, X)) % 360.0, inside, near_half


def orientation_windows(X, Y, ra, inside):
    """the 72 sliding windows of 60 degrees over the rounded sample angles `ra` -> (directions in degrees, moduli), each [n, 72]"""
    X, Y, ra, inside = np.broadcast_arrays(X, Y, ra, inside)
    sx = np.zeros(X.shape[:-1] + (72,)); sy = np.zeros_like(sx)
    for k in range(72):
        d = np.abs(ra - 5 * k)
        m = inside & ((d < 30) | (d > 330))
        sx[..., k], sy[..., k] = (X * m).sum(-1), (Y * m).sum(-1)
    return np.degrees(np.arctan2(-sy, sx)) % 360.0, sx * sx + sy * sy


def check_orientation(img, kps, upright=False, bound=None):
    """Reported angle against the float64 one: window membership by the rounded float64 angle, the first best of the 72 windows.
    A keypoint beyond the bound passes only as one of these, and is then counted as exempt:
      - the angle is within the bound of the direction of a second window whose modulus lies within ORI_TIE of the best;
      - the same after samples whose float64 angle lies within ANGLE_EPS of a rounding boundary are rounded the other way (every
        combination of them is tried: the reported angle must still be one concrete float64 answer);
      - a sample coordinate lies within HALF_EPS of a half-integer.
    -> dict: worst (largest error among the keypoints that needed none of this: the figure the bound comes from), exempt, n"""
    bound = ORI_BOUND if bound is None else bound
    ang = kps["angle"].astype(np.float64)
    if upright:
        assert np.all(ang == 270.0), "upright keypoints have angle 270"
        return dict(worst=0.0, exempt=0, n=len(kps))
    assert np.all((ang >= 0) & (ang <= 360)), "angle range"
    if len(kps) == 0:
        return dict(worst=0.0, exempt=0, n=0)
    X, Y, sa, inside, near_half = orientation_samples(img, kps)
    assert np.all(inside.any(1)), "a keypoint the reference deletes (no orientation sample inside)"
    dirs, mod = orientation_windows(X, Y, np.rint(sa), inside)
    r = np.arange(len(kps))
    err = np.abs(wrap_deg(ang - dirs[r, mod.argmax(1)]))
    exempt = 0
    for n in np.nonzero(err > bound)[0]:
        frac = sa[n] - np.floor(sa[n])
        amb = np.nonzero(inside[n] & (np.abs(frac - 0.5) < ANGLE_EPS))[0][:10]        # 113 x 2 x 0.0125 = 3 expected; 2^10 at the most
        flips = ((np.arange(1 << len(amb))[:, None] >> np.arange(len(amb))[None]) & 1).astype(bool)
        ra = np.repeat(np.rint(sa[n])[None], len(flips), 0)
        ra[:, amb] = np.where(flips, np.floor(sa[n][amb]) + (frac[amb] < 0.5), ra[:, amb])
        d, m = orientation_windows(X[n][None], Y[n][None], ra, inside[n][None])
        e = np.where(m >= (1 - ORI_TIE) * m.max(1, keepdims=True), np.abs(wrap_deg(ang[n] - d)), np.inf)
        assert e.min() <= bound or near_half[n], ("orientation", int(n), float(err[n]), float(e.min()))
        exempt += 1
    ok = err <= bound
    return dict(worst=float(err[ok].max()) if ok.any() else 0.0, exempt=exempt, n=len(kps))


def area_matrix(ss, ds=PATCH + 1):
    """exact INTER_AREA ss -> ds: each output is the mean of its source interval of length ss / ds"""
    M = np.zeros((ds, ss))
    sc = ss / ds
    for d in range(ds):
        a, b = d * sc, min((d + 1) * sc, ss)
        for sx in range(int(np.floor(a)), min(int(np.ceil(b)), ss)):
            M[d, sx] = max(0.0, min(b, sx + 1) - max(a, sx))
        M[d] /= M[d].sum()
    return M


_DW = {}


def window64(img, kx, ky, size, angle, upright=False, rot_sign=-1):
    """the win x win sampling window around (kx, ky), rotated by -angle: sample positions in closed form, bilinear inside the image,
    nearest pixel clamped to the image elsewhere (upright: the integer lattice from round(kx + offset), round(ky - offset))"""
    h, w = img.shape
    I = np.asarray(img, np.float64)
    ws = int(window_side(size))
    off = -(ws - 1) / 2
    ii, jj = np.meshgrid(np.arange(ws), np.arange(ws), indexing="ij")
    if upright:
        return I[np.clip(int(np.rint(ky - off)) - jj, 0, h - 1), np.clip(int(np.rint(kx + off)) + ii, 0, w - 1)]
    th = np.radians(np.float64(angle))
    sd, cd = rot_sign * np.sin(th), np.cos(th)
    px = kx + (off + jj) * cd + (off + ii) * sd
    py = ky - (off + jj) * sd + (off + ii) * cd
    ix, iy = np.floor(px).astype(np.int64), np.floor(py).astype(np.int64)
    inside = (ix >= 0) & (ix < w - 1) & (iy >= 0) & (iy < h - 1)
    ixc, iyc = np.clip(ix, 0, w - 2), np.clip(iy, 0, h - 2)
    a, b = px - ix, py - iy
    bil = I[iyc, ixc] * (1 - a) * (1 - b) + I[iyc, ixc + 1] * a * (1 - b) + I[iyc + 1, ixc] * (1 - a) * b + I[iyc + 1, ixc + 1] * a * b
    nx, ny = np.clip(np.rint(px).astype(np.int64), 0, w - 1), np.clip(np.rint(py).astype(np.int64), 0, h - 1)
    return np.where(inside, bil, I[ny, nx])


def gradients64(win, rounded, sigma=DESC_SIGMA):
    """window -> 21 x 21 by exact area averaging -> the 20 x 20 Haar differences (dx, dy) and the float64 Gaussian weights.
    rounded: to 8 bits after sampling and after the resize, halves up after the resize (the exact 2:1 shrink is the one side at which
    halves occur, and there the reference computes (a + b + c + d + 2) >> 2)"""
    if sigma not in _DW:
        g = gauss(PATCH, sigma)
        _DW[sigma] = np.outer(g, g)
    M = area_matrix(win.shape[0])
    if rounded:
        win = np.rint(win)
    P = M @ win @ M.T
    if rounded:
        P = np.clip(np.floor(P + 0.5), 0, 255)
    dx = P[:-1, 1:] - P[:-1, :-1] + P[1:, 1:] - P[1:, :-1]
    dy = P[1:, :-1] - P[:-1, :-1] + P[1:, 1:] - P[:-1, 1:]
    return dx, dy, _DW[sigma]


def _cells(A):
    return A.reshape(4, 5, 4, 5).sum((1, 3)).ravel()


def descriptor64(win, rounded, sigma=DESC_SIGMA):
    """Haar differences x Gaussian -> 4 x 4 cells of 5 x 5 -> (sum dx, sum dy, sum |dx|, sum |dy|) per cell -> unit norm"""
    dx, dy, dw = gradients64(win, rounded, sigma)
    vx, vy = dx * dw, dy * dw
    v = np.stack([_cells(vx), _cells(vy), _cells(np.abs(vx)), _cells(np.abs(vy))], 1).ravel()
    return v / (np.sqrt((v * v).sum()) + np.finfo(np.float64).eps)


def fold_extended(d):
    """the sign-split sums of one 128-d descriptor added back into the 64-d layout, renormalised"""
    d = np.asarray(d, np.float64).reshape(16, 8)
    v = np.stack([d[:, 0] + d[:, 2], d[:, 4] + d[:, 6], d[:, 1] + d[:, 3], d[:, 5] + d[:, 7]], -1).ravel()
    return v / (np.sqrt((v * v).sum()) + np.finfo(np.float64).eps)


def split_error(win, d, sigma=DESC_SIGMA):
    """128-d descriptor against the sign-split sums of the rounded reference.  A sample whose other gradient is within one grey level
    of zero may fall on either side of the split (one patch pixel rounded the other way moves it across), so each component is held to
    the interval between the sums with all such samples out and all of them in.  The descriptor's own norm changes with the split:
    it is taken back to the reference's units by the norm of the folded sums, which no split changes.
    -> largest distance outside the interval, in units of the descriptor"""
    dx, dy, dw = gradients64(win, True, sigma)
    vx, vy = dx * dw, dy * dw
    firm_y, firm_x = np.abs(dy) > 1, np.abs(dx) > 1
    fy, fx = np.where(firm_y, (dy >= 0) * 1.0, 0.0), np.where(firm_x, (dx >= 0) * 1.0, 0.0)        # firm samples on the >= 0 side
    gy, gx = np.where(firm_y, (dy < 0) * 1.0, 0.0), np.where(firm_x, (dx < 0) * 1.0, 0.0)          # firm samples on the < 0 side
    ay, ax = (~firm_y) * 1.0, (~firm_x) * 1.0
    neg, pos = lambda v: np.minimum(v, 0), lambda v: np.maximum(v, 0)
    st = lambda *c: np.stack([_cells(u) for u in c], 1).ravel()
    lo = st(vx * fy + neg(vx) * ay, np.abs(vx) * fy, vx * gy + neg(vx) * ay, np.abs(vx) * gy,
            vy * fx + neg(vy) * ax, np.abs(vy) * fx, vy * gx + neg(vy) * ax, np.abs(vy) * gx)
    hi = st(vx * fy + pos(vx) * ay, np.abs(vx) * (fy + ay), vx * gy + pos(vx) * ay, np.abs(vx) * (gy + ay),
            vy * fx + pos(vy) * ax, np.abs(vy) * (fx + ax), vy * gx + pos(vy) * ax, np.abs(vy) * (gx + ax))
    v64 = np.stack([_cells(vx), _cells(vy), _cells(np.abs(vx)), _cells(np.abs(vy))], 1).ravel()
    n64 = np.sqrt((v64 * v64).sum())
    e = np.asarray(d, np.float64).reshape(16, 8)
    f = np.stack([e[:, 0] + e[:, 2], e[:, 4] + e[:, 6], e[:, 1] + e[:, 3], e[:, 5] + e[:, 7]], -1).ravel()
    nf = np.sqrt((f * f).sum())
    if n64 == 0 or nf == 0:
        return 0.0 if n64 == nf else 1.0
    u = np.asarray(d, np.float64) * (n64 / nf)
    return float(np.maximum(np.maximum(lo - u, u - hi), 0).max() / n64)


def check_descriptors(img, kps, desc, extended=False, upright=False, bounds=None, sigma=DESC_SIGMA, rot_sign=-1):
    """every descriptor from its reported (x, y, size, angle) against both float64 variants, each with its own bound; no keypoint is
    exempt.  Also: unit norm or the zero vector.  The 128-d layout is compared after its sign-split halves are added back (the same 64
    sums), and the split itself is held to the rounded reference by split_error, within the rounded bound.
    -> dict: rounded, plain (largest component errors), split (largest split error), n"""
    bq, br = (DESC_Q_BOUND, DESC_R_BOUND) if bounds is None else bounds
    dim = 128 if extended else 64
    assert desc.shape == (len(kps), dim)
    d = np.asarray(desc, np.float64)
    assert np.all(wavelet_side(kps["size"]) <= min(img.shape) + 1), "a keypoint the reference deletes (wavelet larger than the integral)"
    norm = np.sqrt((d * d).sum(1))
    assert np.all((np.abs(norm - 1) <= (dim + 2) * 2.0 ** -24) | np.all(d == 0, 1)), ("norm", norm.min() if len(d) else 0, norm.max() if len(d) else 0)
    if extended:
        e = d.reshape(-1, 16, 8)
        assert np.all(e[..., 1::2] >= 0) and np.all(np.abs(e[..., 0::2]) <= e[..., 1::2] * (1 + 2.0 ** -20)), "sign-split sums"
    wq = wr = ws = 0.0
    for n, k in enumerate(kps):
        win = window64(img, float(k["x"]), float(k["y"]), k["size"], float(k["angle"]), upright, rot_sign)
        got = fold_extended(d[n]) if extended else d[n]
        eq = float(np.abs(descriptor64(win, True, sigma) - got).max())
        er = float(np.abs(descriptor64(win, False, sigma) - got).max())
        es = split_error(win, d[n], sigma) if extended else 0.0
        wq, wr, ws = max(wq, eq), max(wr, er), max(ws, es)
        assert eq <= bq, ("descriptor against the rounded reference", n, eq)
        assert er <= br, ("descriptor against the plain reference", n, er)
        assert es <= bq, ("sign-split sums against the rounded reference", n, es)
    return dict(rounded=wq, plain=wr, split=ws, n=len(kps))


def window_corners(kps, upright=False):
    """corners of each keypoint's sampling window, in pixels -> (xmin, xmax, ymin, ymax)"""
    ws = window_side(kps["size"]).astype(np.float64)
    th = np.radians(np.where(upright, 270.0, kps["angle"].astype(np.float64)))
    sd, cd = -np.sin(th), np.cos(th)
    u = np.array([-1, -1, 1, 1])[:, None] * (ws - 1) / 2
    v = np.array([-1, 1, -1, 1])[:, None] * (ws - 1) / 2
    px = kps["x"].astype(np.float64)[None] + v * cd + u * sd
    py = kps["y"].astype(np.float64)[None] - v * sd + u * cd
    return px.min(0), px.max(0), py.min(0), py.max(0)


def window_class(kps):
    """size class of the sampling window: 0 (> 256 px), 1 (> 128), 2 (> 64), 3 (the rest)"""
    ws = window_side(kps["size"])
    return np.where(ws > 256, 0, np.where(ws > 128, 1, np.where(ws > 64, 2, 3)))


def border_crossings(kps, shape, upright=False):
    """bool[4, n]: the window reaches past the left, right, top, bottom border of the image"""
    x0, x1, y0, y1 = window_corners(kps, upright)
    return np.stack([x0 < 0, x1 > shape[1] - 1, y0 < 0, y1 > shape[0] - 1])


def subsample(kps, shape, upright=False, limit=150):
    """deterministic choice of at most `limit` keypoints for the per-keypoint references: every window that crosses a border, every
    window of the two largest classes, and the rest of the room filled evenly from the remaining list.  A small image, where most windows
    cross a border, has more of those than the limit: they are then thinned evenly instead (the blob case, built to hold them all, fits)"""
    must = border_crossings(kps, shape, upright).any(0) | (window_class(kps) <= 1)
    idx = np.nonzero(must)[0]
    if len(idx) > limit:
        return idx[np.unique(np.linspace(0, len(idx) - 1, limit).astype(np.int64))]
    rest = np.nonzero(~must)[0]
    room = limit - len(idx)
    if room > 0 and len(rest) > 0:
        idx = np.concatenate([idx, rest[np.unique(np.linspace(0, len(rest) - 1, min(room, len(rest))).astype(np.int64))]])
    return np.sort(idx)


def check_all(img, params, detected, kps, desc, L=None, sample=None):
    """the four checks and the caps on one result: `detected` is the detect-only list, (kps, desc) the described one; `sample` limits the
    orientation and descriptor references to subsample() (the keypoint check always runs on every keypoint) -> dict of figures"""
    p = params
    out = check_keypoints(img, detected, p, L=L)
    # description deletes nothing here (the wavelet always fits and a sample always lies inside): the lists are the same keypoints
    assert len(kps) == len(detected) and all(np.array_equal(kps[f], detected[f]) for f in ("x", "y", "size", "response", "octave", "class_id"))
    assert out["nonfirm"] <= CAP_NONFIRM * out["n64"], ("non-firm float64 keypoints", out["nonfirm"], out["n64"])
    idx = np.arange(len(kps)) if sample is None else subsample(kps, img.shape, p["upright"], sample)
    o = check_orientation(img, kps[idx], p["upright"])
    assert o["exempt"] <= CAP_ORI_EXEMPT * len(kps), ("orientation exemptions", o["exempt"], len(kps))
    d = check_descriptors(img, kps[idx], desc[idx], p["extended"], p["upright"])
    out.pop("match"); out.pop("k64")
    out.update(ori=o["worst"], ori_exempt=o["exempt"], desc_rounded=d["rounded"], desc_plain=d["plain"], desc_split=d["split"], described=len(idx))
    return out
