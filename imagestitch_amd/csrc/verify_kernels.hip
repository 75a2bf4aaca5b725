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
#include "verify_math.h"
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

struct Sums { uint32_t a, b, aa, bb, ab; };
__device__ __forceinline__ void acc4(uint32_t a, uint32_t b, Sums &s)
{
    s.a = __builtin_amdgcn_sad_u8(a, 0u, s.a);
    s.b = __builtin_amdgcn_sad_u8(b, 0u, s.b);
    s.aa = __builtin_amdgcn_udot4(a, a, s.aa, false);
    s.bb = __builtin_amdgcn_udot4(b, b, s.bb, false);
    s.ab = __builtin_amdgcn_udot4(a, b, s.ab, false);
}

// A wave per overlap row.  Strip B's row is cut at its 16-byte boundaries: the body is read as aligned uint4, the partner bytes of strip A
// (shifted by dy and by the strips' own column offsets inside their tiles, so at any byte alignment) as the five aligned dwords around them,
// funnel-shifted into place; heads and tails (< 16 bytes each) are single bytes on the first lanes.  Per-row sums are 32-bit (a lane sees
// at most w / 64 + 30 pixels of a row: 65025 * 158 at w = 8192), the running sums 64-bit.
__global__ __launch_bounds__(256) void k_verify_ncc(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int status = __builtin_amdgcn_readfirstlane(J.result[0]);
    if (!status) return;
    const int dx = __builtin_amdgcn_readfirstlane(J.result[1]), dy = __builtin_amdgcn_readfirstlane(J.result[2]);
    const Overlap o = verify_overlap(J.vh, J.vw, dx, dy);
    if (o.r1 <= o.r0 || o.c1 <= o.c0) return;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int L = o.c1 - o.c0;
    unsigned long long t[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int r = o.r0 + (int)blockIdx.x * 4 + wid; r < o.r1; r += (int)gridDim.x * 4) {
        const uint8_t *pb = J.vb + (size_t)r * J.vsb + o.c0;
        const uint8_t *pa = J.va + (size_t)(r + dx) * J.vsa + (o.c0 + dy);
        const int head = min(L, (int)((16u - (unsigned)((uintptr_t)pb & 15u)) & 15u));
        const int nb = (L - head) >> 4, tail = L - head - (nb << 4);
        Sums s = {0u, 0u, 0u, 0u, 0u};
        const unsigned m = (unsigned)((uintptr_t)(pa + head) & 3u);          // the same for every chunk of the row
        for (int k = lane; k < nb; k += 64) {
            const uint4 b = *reinterpret_cast<const uint4 *>(pb + head + 16 * (size_t)k);
            const uint32_t *a4 = reinterpret_cast<const uint32_t *>(pa + head + 16 * (size_t)k - m);
            const uint32_t d0 = a4[0], d1 = a4[1], d2 = a4[2], d3 = a4[3], d4 = m ? a4[4] : 0u;   // a4[4] holds bytes of the chunk when m != 0
            acc4(__builtin_amdgcn_alignbyte(d1, d0, m), b.x, s);
            acc4(__builtin_amdgcn_alignbyte(d2, d1, m), b.y, s);
            acc4(__builtin_amdgcn_alignbyte(d3, d2, m), b.z, s);
            acc4(__builtin_amdgcn_alignbyte(d4, d3, m), b.w, s);
        }
        int e = -1;                                       // head byte `lane`, tail byte `lane - 32`
        if (lane < head) e = lane;
        else if (lane >= 32 && lane - 32 < tail) e = head + (nb << 4) + lane - 32;
        if (e >= 0) acc4((uint32_t)pa[e], (uint32_t)pb[e], s);
        t[0] += s.a; t[1] += s.b; t[2] += s.aa; t[3] += s.bb; t[4] += s.ab;
    }
    __shared__ unsigned long long part[4][5];
#pragma unroll
    for (int q = 0; q < 5; q++) {
        unsigned long long v = t[q];
        for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
        if (lane == 0) part[wid][q] = v;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const unsigned long long v = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
        if (v) atomicAdd(J.vsum + 1 + threadIdx.x, v);
    }
}

__global__ __launch_bounds__(64) void k_verify_decide(const MatchDev *jobs, int njobs, double threshold, int min_pixels)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    const MatchDev &J = jobs[j];
    if (!J.result[0]) return;                             // int 7 of a row without an accepted vote stays 0
    const Overlap o = verify_overlap(J.vh, J.vw, J.result[1], J.result[2]);
    const long long N = (long long)max(0, o.r1 - o.r0) * (long long)max(0, o.c1 - o.c0);
    unsigned long long *s = J.vsum;
    const double score = verify_score(N, (long long)s[1], (long long)s[2], (long long)s[3], (long long)s[4], (long long)s[5], min_pixels);
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
