"""A sequential float32 model of the SURF orientation of ONE keypoint, operation for operation as the reference orders them
(surf.cpp SURFInvoker; oracle/vfsms_oracle.c surf_describe_one): the 113 samples of the radius-6 disc in table order, two Haar boxes per
gradient (int box sum times float weight, accumulated in double, rounded to float), the Gaussian weight, the polynomial fastAtan2,
membership of the rounded angle in the 72 windows of 60 degrees, the window sums over the samples IN INDEX ORDER, and the first window
whose modulus exceeds every earlier one.

It exists to tell, on the host, whether two windows of a keypoint have EQUAL float32 moduli (a tie the kernel's argmax has to resolve
towards the lower window); tests/test_orientation_waves_gpu.py checks the model's angle against the oracle's before it trusts a tie."""
import numpy as np

F = np.float32
ORI_RADIUS = 6
_S = F(180 / 3.1415926535897932384626433832795)
_P1, _P3 = F(0.9997878412794807) * _S, F(-0.3258083974640975) * _S
_P5, _P7 = F(0.1555786518463281) * _S, F(-0.04432655554792128) * _S
_EPS = F(2.220446049250313e-16)


def _gauss_f32(n, sigma):
    x = np.arange(n) - (n - 1) * 0.5
    cf = np.exp((-0.5 / (sigma * sigma)) * x * x).astype(F)
    return (cf.astype(np.float64) * (1.0 / cf.astype(np.float64).sum())).astype(F)


_G = _gauss_f32(2 * ORI_RADIUS + 1, 2.5)
APT = [(i, j, F(_G[i + ORI_RADIUS] * _G[j + ORI_RADIUS])) for i in range(-ORI_RADIUS, ORI_RADIUS + 1)
       for j in range(-ORI_RADIUS, ORI_RADIUS + 1) if i * i + j * j <= ORI_RADIUS * ORI_RADIUS]


def fast_atan2_deg(y, x):
    y, x = F(y), F(x)
    ax, ay = np.abs(x), np.abs(y)
    if ax >= ay:
        c = ay / (ax + _EPS)
        c2 = c * c
        a = (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    else:
        c = ax / (ay + _EPS)
        c2 = c * c
        a = F(90.0) - (((_P7 * c2 + _P5) * c2 + _P3) * c2 + _P1) * c
    if x < 0:
        a = F(180.0) - a
    if y < 0:
        a = F(360.0) - a
    return F(a)


def _rint(v):
    return int(np.rint(F(v)))


def integral(img):
    s = np.zeros((img.shape[0] + 1, img.shape[1] + 1), np.int64)
    s[1:, 1:] = img.astype(np.int64).cumsum(0).cumsum(1)
    return s


def orientation(S, kx, ky, size):
    """-> None for a keypoint the reference deletes, else dict(angle, best, mod[72], sx[72], sy[72], nvalid); S = integral(img)"""
    srows, scols = S.shape
    s = F(size) * F(1.2) / F(9.0)
    gws = 2 * _rint(F(2) * s)
    if srows < gws or scols < gws:
        return None
    ratio = F(gws) / F(4)

    def pattern(src):
        out = []
        for x1, y1, x2, y2, wt in src:
            dx1, dy1, dx2, dy2 = _rint(ratio * F(x1)), _rint(ratio * F(y1)), _rint(ratio * F(x2)), _rint(ratio * F(y2))
            out.append((dx1, dy1, dx2, dy2, F(wt) / (F(dx2 - dx1) * F(dy2 - dy1))))
        return out

    def haar(y, x, pat):
        d = 0.0
        for dx1, dy1, dx2, dy2, wt in pat:
            box = int(S[y + dy1, x + dx1] + S[y + dy2, x + dx2] - S[y + dy2, x + dx1] - S[y + dy1, x + dx2])
            d += float(F(box) * wt)
        return F(d)

    dxp = pattern([(0, 0, 2, 4, -1), (2, 0, 4, 4, 1)])
    dyp = pattern([(0, 0, 4, 2, 1), (0, 2, 4, 4, -1)])
    half = F(gws - 1) / F(2)
    X, Y, A = [], [], []
    for i, j, wt in APT:
        x, y = _rint(F(kx) + F(i) * s - half), _rint(F(ky) + F(j) * s - half)
        if y < 0 or y >= srows - gws or x < 0 or x >= scols - gws:
            continue
        vx, vy = haar(y, x, dxp) * wt, haar(y, x, dyp) * wt
        X.append(vx); Y.append(vy); A.append(_rint(fast_atan2_deg(vy, vx)))
    if not X:
        return None
    A = np.array(A)
    w5 = 5 * np.arange(72)
    d = np.abs(A[None, :] - w5[:, None])
    member = (d < 30) | (d > 330)                               # [window, sample]
    sx, sy = np.zeros(72, F), np.zeros(72, F)
    for j in range(len(X)):                                     # every window's sum visits the samples in index order
        sx = np.where(member[:, j], sx + X[j], sx).astype(F)
        sy = np.where(member[:, j], sy + Y[j], sy).astype(F)
    mod = (sx * sx + sy * sy).astype(F)
    best, bm = -1, F(0)
    for w in range(72):
        if mod[w] > bm:
            bm, best = mod[w], w
    bx, by = (sx[best], sy[best]) if best >= 0 else (F(0), F(0))
    return dict(angle=fast_atan2_deg(-by, bx), best=best, mod=mod, sx=sx, sy=sy, nvalid=len(X))


def ties(o):
    """windows whose modulus EQUALS the winning one, the winner first"""
    if o is None or o["best"] < 0:
        return []
    return [int(w) for w in np.nonzero(o["mod"] == o["mod"][o["best"]])[0]]
