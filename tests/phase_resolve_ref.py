"""The specification of Stitcher.phaseResolve = "ncc", restated in numpy (normative; csrc/phase_resolve_kernels.hip follows it).

The reference has no such step: it takes the one arg-max of cv2.phaseCorrelate's shifted surface, adds it with the feature path's sign
(mirrored), cannot tell a shift from the same shift plus or minus the padded size (the transform is circular) and gates
on the 5 x 5 response sum, which falls with the overlap.  This is the project's own specification, like verify_ref.py, whose statistic
it uses: a few peaks of the correlation surface, every circular reading of each scored by the normalised cross-correlation of the pixels
the two strips share under it, the best one kept.

Inputs: strips A and B (uint8, one shape h x w), `peaks` K (1 .. MAX_PEAKS), `threshold` and `min_pixels`.

1. Surface.  R is the unshifted, unscaled inverse transform of cv2.phaseCorrelate's cross-power spectrum: M x N with M, N =
   getOptimalDFTSize(h), (w), the strips zero-padded on the bottom / right, P = F(A) conj F(B), C = P |P| / (|P|^2 + eps) with the
   packed format's quirk on the purely real bins (x / (x^2 + eps)), R = idft(C) without scaling -- phasecorr.cpp BEFORE fftShift.
   B(r, c) = A(r + dx, c + dy) puts the peak of R at (dx mod M, dy mod N).
2. Peaks.  Element p of R is a peak when, for each of its eight circular neighbours q = ((y + i) mod M, (x + j) mod N), (i, j) != (0, 0),
   R[p] >= R[q], and R[p] > R[q] for those q whose row-major index y N + x is smaller than p's.  (A neighbour that coincides with p
   itself -- M or N below 3 -- passes by that rule.  On a constant surface element (0, 0) is the only peak.)  The K largest peaks are
   taken, ordered by value descending, then by row-major index ascending; absent peaks are (-1, -1).
3. Candidates.  Peak k at (uy, ux) gives, in this order, the readings (dx, dy) = (uy, ux), (uy - M, ux), (uy, ux - N), (uy - M, ux - N),
   candidate index 4 k + position.  A reading is KEPT when |dx| < h and |dy| < w (the strips share at least one pixel); a dropped reading
   scores 0 over 0 pixels, a reading of an absent peak is the all-zero record.
4. Score.  Every kept candidate is scored exactly as verify_ref.sums / verify_ref.score score one vote (B pixel (r, c) meets A pixel
   (r + dx, c + dy); fewer than min_pixels shared pixels or a flat side: 0).
5. Winner.  The kept candidate with the largest float64 score, ties to the lowest candidate index.  (Every present peak keeps at least one
   reading: M < 2 h and N < 2 w.)  Row = {status, dx, dy, 0, 1, 1, candidate index, fixed(score)}, status = score >= threshold; a row
   with status 0 still carries the best candidate.  Without any kept candidate (a surface without a peak: NaN) the row is
   {0, 0, 0, 0, 1, 1, 0, 0}.  cv2.phaseCorrelate's response plays no part.

Odd sizes.  The (uy, ux) reading is taken from the surface BEFORE fftShift, so OpenCV's treatment of an odd last row or column (it stays
where it is while the quadrants swap) never enters: the rule above is the same for even and odd M, N, and test_phase_resolve_host.py
checks it on 45 x 75.  Reading the SHIFTED surface instead would need the inverse of that quadrant swap first (phase_kernels.hip:
unshift2), which is the identity on an odd last row / column.
"""
import numpy as np

from phase_numpy import optimal_dft_size
import verify_ref

MAX_PEAKS = 8


def surface(a, b):
    """R of step 1, float64 M x N"""
    a = np.asarray(a, np.float64); b = np.asarray(b, np.float64)
    assert a.shape == b.shape and a.ndim == 2
    h, w = a.shape
    M, N = optimal_dft_size(h), optimal_dft_size(w)
    pa = np.zeros((M, N)); pb = np.zeros((M, N))
    pa[:h, :w] = a; pb[:h, :w] = b
    F1, F2 = np.fft.rfft2(pa), np.fft.rfft2(pb)
    P = F1 * np.conj(F2)
    eps = np.finfo(np.float64).eps
    mag = np.abs(P)
    C = P * mag / (mag * mag + eps)
    for u in [0] + ([M // 2] if M % 2 == 0 else []):
        for v in [0] + ([N // 2] if N % 2 == 0 else []):
            x = P[u, v].real
            C[u, v] = x / (x * x + eps)
    return np.fft.irfft2(C, s=(M, N)) * (M * N)


def peak_mask(R):
    """step 2's predicate for every element"""
    M, N = R.shape
    idx = np.arange(M * N, dtype=np.int64).reshape(M, N)
    ok = np.ones((M, N), bool)
    for i in (-1, 0, 1):
        for j in (-1, 0, 1):
            if i == 0 and j == 0:
                continue
            q = np.roll(R, (-i, -j), (0, 1))              # q[y, x] = R[(y + i) mod M, (x + j) mod N]
            qi = np.roll(idx, (-i, -j), (0, 1))
            ok &= np.where(qi < idx, R > q, R >= q)
    return ok


def peaks(R, K):
    """-> [(uy, ux)] * K (absent: (-1, -1)) and their values"""
    M, N = R.shape
    flat = np.flatnonzero(peak_mask(R).reshape(-1))
    vals = R.reshape(-1)[flat]
    order = np.lexsort((flat, -vals))[:K]                 # value descending, then index ascending
    pos = [(int(flat[o] // N), int(flat[o] % N)) for o in order]
    val = [float(vals[o]) for o in order]
    return pos + [(-1, -1)] * (K - len(pos)), val


def candidates(pk, M, N, h, w):
    """step 3 -> [(dx, dy, kept)] * 4 K; readings of an absent peak are (0, 0, False)"""
    out = []
    for (uy, ux) in pk:
        for (dx, dy) in ((uy, ux), (uy - M, ux), (uy, ux - N), (uy - M, ux - N)):
            if uy < 0:
                out.append((0, 0, False))
            else:
                out.append((dx, dy, abs(dx) < h and abs(dy) < w))
    return out


def resolve(A, B, peaks_k=2, threshold=0.5, min_pixels=4096, R=None):
    """-> dict(row int32[8], cands int32[4 K, 4] = {dx, dy, fixed score, shared pixels}, peaks int32[K, 2], scores [float] * 4 K,
    values: the peak values)"""
    A = np.asarray(A); B = np.asarray(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8 and A.shape == B.shape and 1 <= peaks_k <= MAX_PEAKS
    h, w = A.shape
    if R is None:
        R = surface(A, B)
    M, N = R.shape
    pk, val = peaks(R, peaks_k)
    cands = np.zeros((4 * peaks_k, 4), np.int32)
    scores = [0.0] * (4 * peaks_k)
    best = -1
    for c, (dx, dy, kept) in enumerate(candidates(pk, M, N, h, w)):
        cands[c, 0], cands[c, 1] = dx, dy
        if not kept:
            continue
        s = verify_ref.sums(A, B, dx, dy)
        scores[c] = verify_ref.score(s, min_pixels)
        cands[c, 2], cands[c, 3] = verify_ref.fixed(scores[c]), s[0]
        if best < 0 or scores[c] > scores[best]:
            best = c
    row = np.array([0, 0, 0, 0, 1, 1, 0, 0], np.int32)
    if best >= 0:
        row[:] = [int(scores[best] >= threshold), cands[best, 0], cands[best, 1], 0, 1, 1, best, cands[best, 2]]
    return dict(row=row, cands=cands, peaks=np.array(pk, np.int32).reshape(peaks_k, 2), scores=scores, values=val)


def peak_gap_ok(R, K, gap=1e-6):
    """Can a transform that rounds differently (1e-13 relative elsewhere in the suite) change the peak list?  Not when the reference
    shows the top K + 1 peak values a relative `gap` apart from each other and each of the top K peaks the same gap above its eight
    neighbours.  `gap` is relative to the largest peak."""
    M, N = R.shape
    pk, val = peaks(R, K + 1)
    if not val:
        return False
    tol = gap * abs(val[0])
    for a, b in zip(val, val[1:]):
        if not a - b >= tol:
            return False
    for (uy, ux), v in list(zip(pk, val))[:K]:
        for i in (-1, 0, 1):
            for j in (-1, 0, 1):
                q = ((uy + i) % M, (ux + j) % N)
                if q != (uy, ux) and not v - R[q] >= tol:
                    return False
    return True
