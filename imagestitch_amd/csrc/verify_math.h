// verify_math.h -- the overlap rectangle and the score of tests/verify_ref.py, shared by the kernels that judge an offset by the
// correlation of the pixels two images share under it: verify_kernels.hip (offsetVerify = "ncc"), adjust_kernels.hip (the offset search
// of globalAdjust = "ncc") and phase_resolve_kernels.hip (phaseResolve = "ncc"); exposure_kernels.hip shares their sums' machinery
// (overlap_sums.h, which includes this header) but has no score.  One definition, so that all equal the specification bit for bit.
#pragma once
#include "common.h"

struct Overlap { int r0, r1, c0, c1; };
__device__ __forceinline__ Overlap verify_overlap(int h, int w, int dx, int dy)
{
    Overlap o;
    o.r0 = max(0, -dx); o.r1 = min(h, h - dx);
    o.c0 = max(0, -dy); o.c1 = min(w, w - dy);
    return o;
}

// tests/verify_ref.py: score() -- every operation is one correctly rounded IEEE double operation, in this order
__device__ __forceinline__ double verify_score(long long N, long long Sa, long long Sb, long long Saa, long long Sbb, long long Sab, int min_pixels)
{
    if (N <= 0 || N < (long long)min_pixels) return 0.0;
    const double n = (double)N, sa = (double)Sa, sb = (double)Sb;
    const double ma = sa / n, mb = sb / n;
    const double va = (double)Saa - sa * ma;
    const double vb = (double)Sbb - sb * mb;
    const double cab = (double)Sab - sa * mb;
    if (!(va > 0.0) || !(vb > 0.0)) return 0.0;
    const double s = cab / (sqrt(va) * sqrt(vb));
    return fmin(1.0, fmax(-1.0, s));
}
__device__ __forceinline__ int verify_fixed(double score) { return (int)floor(score * (double)VFSMS_VERIFY_FIXED_ONE + 0.5); }

// the tail of every user: the overlap of an h x w pair under (dx, dy), its pixel count (0 when empty) -> *N_out, and the score of the
// five sums s5 = Sa, Sb, Saa, Sbb, Sab over it
__device__ __forceinline__ double overlap_score(int h, int w, int dx, int dy, const unsigned long long *s5, int min_pixels, long long *N_out)
{
    const Overlap o = verify_overlap(h, w, dx, dy);
    const long long N = (long long)max(0, o.r1 - o.r0) * (long long)max(0, o.c1 - o.c0);
    *N_out = N;
    return verify_score(N, (long long)s5[0], (long long)s5[1], (long long)s5[2], (long long)s5[3], (long long)s5[4], min_pixels);
}
