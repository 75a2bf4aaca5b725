"""The specification of Method.offsetVerify = "ncc", restated in numpy.

The reference has no such step (a candidate is accepted on its vote count alone, ImageUtility.py:139-178), so this is the project's own
specification, like consensus_ref.py and multiband_ref.py; csrc/verify_kernels.hip equals it bit for bit.

Inputs: strips A and B (uint8, one shape h x w, the RAW tile pixels even when isEnhance is set), the raw vote (dx, dy) exactly as
getOffsetByMode returns it for (query A, train B) before the axis correction, and min_pixels.

1. Overlap.  The vote is dx = int(yA - yB), dy = int(xA - xB): a feature at row yB, column xB of B sits at row yB + dx, column xB + dy of A.
   So pixel (r, c) of B has its partner at pixel (r + dx, c + dy) of A, and the overlap is the rectangle of B pixels whose partner lies
   inside A:  r in [max(0, -dx), min(h, h - dx)),  c in [max(0, -dy), min(w, w - dy)).
2. Six exact integers over the overlap (a = the A pixel, b = its B partner): N, Sa = sum a, Sb = sum b, Saa = sum a*a, Sbb = sum b*b,
   Sab = sum a*b.  All fit int64 (Sab <= 2^40 for a whole 4096 x 4096 tile).
3. The score, in IEEE float64, every line ONE correctly rounded operation per operator, in exactly this order (no N * Sab in integers: it
   overflows int64 for a whole tile):
       n = float(N); sa = float(Sa); sb = float(Sb)
       ma = sa / n;  mb = sb / n
       va  = float(Saa) - sa * ma
       vb  = float(Sbb) - sb * mb
       cab = float(Sab) - sa * mb
       score = cab / (sqrt(va) * sqrt(vb)),  clamped to [-1, 1]
   N < min_pixels, N == 0, va <= 0 or vb <= 0 (a flat side: Sa * ma is exact there, so va is exactly 0): score = 0.
4. Accept iff score >= threshold.  The integer reported in the attempt row's 8th int is  fixed = floor(score * 2^20 + 0.5).
"""
import math

import numpy as np

FIXED_ONE = 1 << 20


def overlap(h, w, dx, dy):
    """(r0, r1, c0, c1) of the B pixels whose partner (r + dx, c + dy) lies inside A; empty when r1 <= r0 or c1 <= c0"""
    return max(0, -dx), min(h, h - dx), max(0, -dy), min(w, w - dy)


def sums(A, B, dx, dy):
    """(N, Sa, Sb, Saa, Sbb, Sab) as Python ints"""
    A = np.asarray(A); B = np.asarray(B)
    assert A.dtype == np.uint8 and B.dtype == np.uint8 and A.ndim == 2 and A.shape == B.shape
    h, w = A.shape
    r0, r1, c0, c1 = overlap(h, w, int(dx), int(dy))
    if r1 <= r0 or c1 <= c0:
        return (0, 0, 0, 0, 0, 0)
    b = B[r0:r1, c0:c1].astype(np.int64)
    a = A[r0 + dx:r1 + dx, c0 + dy:c1 + dy].astype(np.int64)
    return (int(a.size), int(a.sum()), int(b.sum()), int((a * a).sum()), int((b * b).sum()), int((a * b).sum()))


def score(s, min_pixels=0):
    """step 3 on the six integers (Python floats are IEEE float64; /, *, -, math.sqrt are correctly rounded)"""
    N, Sa, Sb, Saa, Sbb, Sab = s
    if N <= 0 or N < min_pixels:
        return 0.0
    n = float(N); sa = float(Sa); sb = float(Sb)
    ma = sa / n
    mb = sb / n
    va = float(Saa) - sa * ma
    vb = float(Sbb) - sb * mb
    cab = float(Sab) - sa * mb
    if not va > 0.0 or not vb > 0.0:
        return 0.0
    sc = cab / (math.sqrt(va) * math.sqrt(vb))
    return min(1.0, max(-1.0, sc))


def fixed(sc):
    return int(math.floor(sc * float(FIXED_ONE) + 0.5))


def verify(A, B, dx, dy, threshold, min_pixels=0):
    """-> (accepted, score, fixed-point score, the six sums)"""
    s = sums(A, B, dx, dy)
    sc = score(s, min_pixels)
    return (sc >= threshold, sc, fixed(sc), s)


def verify_row(row, A, B, threshold, min_pixels=0):
    """an attempt row {status, dx, dy, votes, nA, nB, nMatches, 0} as the engine leaves it with the verifier on: a row whose vote was not
    accepted is untouched; otherwise int 7 = the fixed-point score and status is cleared when the score is below the threshold"""
    row = [int(v) for v in row]
    if not row[0]:
        return row
    ok, _sc, fx, _s = verify(A, B, row[1], row[2], threshold, min_pixels)
    row[7] = fx
    if not ok:
        row[0] = 0
    return row
