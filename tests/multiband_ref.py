"""multiBandBlending as specified for this project: a Laplacian-pyramid blend of two int64 regions (-1 = empty) with a hard seam
where the fadeInAndFadeOut weights are equal.  A pixel of ch channels is empty iff every channel is -1, i.e. the sum of its channels is
-ch (what corner_ramps scans for; seam_ref.pixel_valid).  Plain numpy float32, every expression in the order the HIP kernels
(imagestitch_amd/csrc/multiband_kernels.hip) evaluate it, so their bytes must equal these bit for bit.

These formulas ARE the specification; they are not claimed to match cv2.pyrDown / cv2.pyrUp or the reference's
ImageFusion.fuseByMultiBandBlending byte for byte (neither can be run here)."""
import numpy as np

F = np.float32
F4, F6 = F(4), F(6)
INV256, INV64 = F(1.0 / 256), F(1.0 / 64)


def level_sizes(n, levels):
    """sizes of levels 0..levels along one axis: level k + 1 has (n + 1) // 2 of level k's"""
    out = [int(n)]
    for _ in range(levels):
        out.append((out[-1] + 1) // 2)
    return out


def reflect101(i, n):
    """BORDER_REFLECT_101 index (-1 -> 1, -2 -> 2, n -> n - 2, n + 1 -> n - 3), iterated until in range; a 1-pixel axis maps to 0"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * n - 2 - i
    return i


def _idx(ids, n):
    return np.array([reflect101(int(i), n) for i in ids], np.int64)


def pyr_down(S):
    """S: float32 [n][m] or [n][m][ch] -> [(n + 1) // 2][(m + 1) // 2](...): 5-tap rows at destination-column resolution, then columns."""
    S = np.asarray(S, F)
    n, m = S.shape[:2]
    dn, dm = (n + 1) // 2, (m + 1) // 2
    x = np.arange(dm) * 2
    c = [S[:, _idx(x + d, m)] for d in (-2, -1, 0, 1, 2)]
    R = ((c[2] * F6 + (c[1] + c[3]) * F4) + c[0]) + c[4]
    y = np.arange(dn) * 2
    r = [R[_idx(y + d, n)] for d in (-2, -1, 0, 1, 2)]
    return ((((r[2] * F6 + (r[1] + r[3]) * F4) + r[0]) + r[4]) * INV256).astype(F)


def _up_idx(w):
    """neighbour indices of pyrUp: -1 reflects to 1 (0 on a 1-pixel axis), w replicates to w - 1"""
    x = np.arange(w)
    xm = np.where(x - 1 < 0, 1 if w > 1 else 0, x - 1)
    xp = np.minimum(x + 1, w - 1)
    return x, xm, xp


def pyr_up(S, out_h, out_w):
    """S: float32 [h][w](...) -> [out_h][out_w](...), out_h in (2h - 1, 2h), out_w in (2w - 1, 2w)."""
    S = np.asarray(S, F)
    h, w = S.shape[:2]
    assert out_h in (2 * h - 1, 2 * h) and out_w in (2 * w - 1, 2 * w), (S.shape, out_h, out_w)
    x, xm, xp = _up_idx(w)
    R = np.empty((h, 2 * w) + S.shape[2:], F)
    R[:, 0::2] = (S[:, xm] + S[:, x] * F6) + S[:, xp]
    R[:, 1::2] = (S[:, x] + S[:, xp]) * F4
    R = R[:, :out_w]
    y, ym, yp = _up_idx(h)
    U = np.empty((2 * h, out_w) + S.shape[2:], F)
    U[0::2] = ((R[ym] + R[y] * F6) + R[yp]) * INV64
    U[1::2] = ((R[y] + R[yp]) * F4) * INV64
    return U[:out_h]


def fade_weights(A, dx, dy, corner_ramps):
    """fuseByFadeInAndFadeOut's per-pixel float32 (wA, wB) from A's -1 pattern: the strip ramps (more than 65 % of the elements
    valid) or getWeightsMatrix's corner ramps through `corner_ramps(A) -> (wB_r, wB_c, info)` (oracle.corner_ramps; raises
    IndexError where the reference's getWeightsMatrix raises)."""
    A = np.asarray(A, np.int64)
    r, c = A.shape[:2]
    if np.count_nonzero(A > -1) / A.size > 0.65:
        wAr = np.ones(r, F); wBr = np.ones(r, F); wAc = np.ones(c, F); wBc = np.ones(c, F)
        if c <= r:
            i = np.arange(c)
            f = (i if dy >= 0 else c - i).astype(F)
            wAc[c - i - 1] = f / F(c)
            wBc[i] = f / F(c)
        else:
            i = np.arange(r)
            f = (i if dx <= 0 else r - i).astype(F)
            wAr[i] = f / F(r)
            wBr[r - i - 1] = f / F(r)
        return wAr[:, None] * wAc[None, :], wBr[:, None] * wBc[None, :]
    wr, wc, _info = corner_ramps(A)
    wB = np.asarray(wr, F)[:, None] * np.asarray(wc, F)[None, :]
    return F(1) - wB, wB


def seam_mask(A, dx, dy, corner_ramps):
    wA, wB = fade_weights(A, dx, dy, corner_ramps)
    return (wA >= wB).astype(F)


def fill(A, B):
    """A' = A where A >= 0 else B; B' = B where B >= 0 else A'; elements empty in both -> 0"""
    A = np.asarray(A, np.int64); B = np.asarray(B, np.int64)
    A1 = np.where(A >= 0, A, B)
    B1 = np.where(B >= 0, B, A1)
    return np.maximum(A1, 0), np.maximum(B1, 0)


def blend_planes(GA0, GB0, M0, levels):
    """the pyramid blend of float32 planes (channels last or none) with a single-channel mask -> float32 O_0"""
    ch_axis = GA0.ndim == 3
    GA, GB, M = [GA0], [GB0], [M0]
    for _ in range(levels):
        GA.append(pyr_down(GA[-1])); GB.append(pyr_down(GB[-1])); M.append(pyr_down(M[-1]))

    def mk(k):
        return M[k][:, :, None] if ch_axis else M[k]
    O = (mk(levels) * GA[levels]) + ((F(1) - mk(levels)) * GB[levels])
    for k in range(levels - 1, -1, -1):
        h, w = GA[k].shape[:2]
        LA = GA[k] - pyr_up(GA[k + 1], h, w)
        LB = GB[k] - pyr_up(GB[k + 1], h, w)
        LC = (mk(k) * LA) + ((F(1) - mk(k)) * LB)
        O = pyr_up(O, h, w) + LC
    return O


def multiband(A, B, dx, dy, levels=4, corner_ramps=None):
    """int64 regions A, B ([r][c] or [r][c][ch], -1 = empty) -> uint8 blend"""
    if corner_ramps is None:
        from oracle import oracle as O
        corner_ramps = O.corner_ramps
    if not 1 <= levels <= 8:
        raise ValueError("levels must be 1..8")
    M0 = seam_mask(A, dx, dy, corner_ramps)
    A1, B1 = fill(A, B)
    O0 = blend_planes(A1.astype(F), B1.astype(F), M0, levels)
    return np.clip(np.rint(O0), 0, 255).astype(np.uint8)
