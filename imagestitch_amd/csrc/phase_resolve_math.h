// phase_resolve_math.h -- the integer side of Stitcher.phaseResolve = "ncc" (tests/phase_resolve_ref.py, steps 3 and the argument rules):
// the circular readings of a peak of the correlation surface and the checks of the entry points' arguments.  Plain C++ without a HIP type
// in it, so the device kernels (phase_resolve_kernels.hip), the C API (api.hip) and a host program under a sanitizer
// (tools/phase_resolve_host_check.cpp) compile the same lines.
#pragma once
#include <stdint.h>

#ifndef VFSMS_PHASE_MAX_PEAKS
#define VFSMS_PHASE_MAX_PEAKS 8
#endif

#ifdef __HIPCC__
#define PR_HD __host__ __device__
#else
#define PR_HD
#endif

struct PhaseCand { int dx, dy, present, kept; };      // present: the peak exists; kept: |dx| < h and |dy| < w (the strips share a pixel)

// reading `pos` (0..3) of the peak at row-major index `idx` (< 0: absent) of the M x N surface, for strips of h x w:
// (uy, ux), (uy - M, ux), (uy, ux - N), (uy - M, ux - N)
PR_HD inline PhaseCand phase_candidate(long long idx, int pos, int M, int N, int h, int w)
{
    PhaseCand c; c.dx = 0; c.dy = 0; c.present = 0; c.kept = 0;
    if (idx < 0 || M <= 0 || N <= 0 || idx >= (long long)M * N) return c;
    const int uy = (int)(idx / N), ux = (int)(idx - (long long)uy * N);
    c.present = 1;
    c.dx = (pos & 1) ? uy - M : uy;
    c.dy = (pos & 2) ? ux - N : ux;
    c.kept = (c.dx < h && c.dx > -h && c.dy < w && c.dy > -w) ? 1 : 0;
    return c;
}

// vfsms_ctx_set_phase_resolver / vfsms_attempt_phase_resolve_batch / vfsms_phase_resolve_u8: 1 = acceptable
PR_HD inline int phase_resolve_params_ok(int peaks, double threshold, int min_pixels)
{
    return peaks >= 1 && peaks <= VFSMS_PHASE_MAX_PEAKS && threshold >= -1.0 && threshold <= 1.0 && min_pixels >= 0;      // a NaN threshold fails both compares
}
PR_HD inline int phase_resolver_ok(int resolver) { return resolver == 0 || resolver == 1; }
