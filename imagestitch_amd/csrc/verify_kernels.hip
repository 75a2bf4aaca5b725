// verify_kernels.hip -- the overlap-correlation acceptance check of Method.offsetVerify = "ncc" for gfx950.
//
// Specification: tests/verify_ref.py (the device equals it bit for bit).  The vote of a fused attempt is dx = int(yA - yB),
// dy = int(xA - xB) with A the query strip (k_merge_ratio), so pixel (r, c) of strip B has its partner at pixel (r + dx, c + dy) of
// strip A; the overlap is the rectangle of B pixels whose partner lies inside A.  Over it: N and the five exact integer sums Sa, Sb,
// Saa, Sbb, Sab, then a handful of IEEE double operations in a fixed order (verify_score) -- so the reduction order is free.
//
// Runs behind the vote tail (k_scan_mode / k_consensus_pick wrote result[0..7]) when the context's verifier is on:
//   k_verify_clear   (one lane per job)        -> the job's sums = 0
//   k_verify_ncc     (row blocks x jobs)       -> sums, one 64-bit atomic add per workgroup and sum; leaves at once when status == 0
//   k_verify_decide  (one lane per job)        -> result[7] = fixed-point score, result[0] = 0 when score < threshold
// The result row is read on the device: no host synchronisation inside a batch.
#include "common.h"
#include "overlap_sums.h"
#include <algorithm>

#define VERIFY_WG 64         // workgroups per job at most: 256 waves, a wave per overlap row

// vsum layout (MatchDev::vsum, 8 x uint64): [0] N, [1] Sa, [2] Sb, [3] Saa, [4] Sbb, [5] Sab, [6] bits of the double score, [7] fixed point
__global__ __launch_bounds__(64) void k_verify_clear(const MatchDev *jobs, int njobs)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    unsigned long long *s = jobs[j].vsum;
    for (int k = 0; k < 8; k++) s[k] = 0ull;
}

// A wave per overlap row (overlap_rows_sums of overlap_sums.h), VERIFY_WG row blocks of 4 waves at most.
__global__ __launch_bounds__(256) void k_verify_ncc(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int status = __builtin_amdgcn_readfirstlane(J.result[0]);
    if (!status) return;
    const int dx = __builtin_amdgcn_readfirstlane(J.result[1]), dy = __builtin_amdgcn_readfirstlane(J.result[2]);
    const Overlap o = verify_overlap(J.vh, J.vw, dx, dy);
    if (o.r1 <= o.r0 || o.c1 <= o.c0) return;
    overlap_rows_sums(J.va, J.vsa, J.vb, J.vsb, o, dx, dy, J.vsum + 1);
}

__global__ __launch_bounds__(64) void k_verify_decide(const MatchDev *jobs, int njobs, double threshold, int min_pixels)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const MatchDev &J = jobs[j];
    if (!J.result[0]) return;                             // int 7 of a row without an accepted vote stays 0
    unsigned long long *s = J.vsum;
    long long N;
    const double score = overlap_score(J.vh, J.vw, J.result[1], J.result[2], s + 1, min_pixels, &N);
    const int fx = verify_fixed(score);
    s[0] = (unsigned long long)N;
    s[6] = (unsigned long long)__double_as_longlong(score);
    s[7] = (unsigned long long)(long long)fx;
    J.result[7] = fx;
    if (!(score >= threshold)) J.result[0] = 0;
}

// the three kernels for njobs jobs whose result rows the vote tail has written and whose strips (va, vb, ...) the caller has filled
int launch_verify(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, double threshold, int min_pixels)
{
    if (njobs <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "verify");
    const int gx = std::max(4, std::min(VERIFY_WG, 4096 / njobs));
    hipLaunchKernelGGL(k_verify_clear, dim3((njobs + 63) / 64), dim3(64), 0, ctx->stream, d_jobs, njobs);
    hipLaunchKernelGGL(k_verify_ncc, dim3(gx, njobs), dim3(256), 0, ctx->stream, d_jobs);
    hipLaunchKernelGGL(k_verify_decide, dim3((njobs + 63) / 64), dim3(64), 0, ctx->stream, d_jobs, njobs, threshold, min_pixels);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
