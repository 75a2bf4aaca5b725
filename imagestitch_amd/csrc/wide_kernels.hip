// wide_kernels.hip -- the two-level offset search of Method.failedPairRepair = "stage" for gfx950: the window search of adjust_kernels.hip,
// first on a pair of tiles reduced by F x F block means, then at full resolution around the best coarse candidates.
//
// Specification: tests/ncc_wide_ref.py (the device equals it bit for bit: every value below is an integer or comes out of the search's
// own kernels).
//
//   k_wide_reduce     grid (blocks of output dwords, plane A / B, jobs): both tiles of a job -> two hc x wc planes in arena scratch
//   (launch_adjust_search on the reduced pairs, with the surface)
//   k_wide_seeds      a workgroup per job: the K best coarse candidates that are no neighbours of each other -> seed table, fine jobs
//   (launch_adjust_search on the n x K fine jobs)
//   k_wide_pick       a lane per job: the best fine result over the job's seeds -> out8, the seed table completed
// No host synchronisation between them.  k_wide_sums (vfsms_overlap_sums_batch) is overlap_rows_sums of overlap_sums.h for whole tiles.
//
// k_wide_reduce is the one kernel that streams whole tiles.  A lane makes FOUR output bytes of one plane: it reads 4 F source bytes of
// each of F rows -- one aligned 16-byte load per row at F = 4 where the row's address allows it (tile B's rows always do for the
// library's own tiles; tile A's blocks start at column dy mod F), else the F + 1 aligned dwords around them, funnel-shifted into
// place (load_partner) -- sums each block row with sad_u8, rounds and stores one dword.  The planes' row stride is a multiple of 16 and
// 64 bytes follow the last row: the search reads its operands as aligned dwords that hold at least one byte of the row.
#include "common.h"
#include "overlap_sums.h"
#include <algorithm>

#define WIDE_THREADS 256
#define WIDE_MAX_GX 4096
#define WIDE_MAX_C (2 * VFSMS_ADJUST_MAX_RADIUS + 1)        // the coarse surface is at most 33 x 33

// 4 F bytes of a source row from column c on (address p) as F dwords; the row's columns are [0, w)
template <int F>
__device__ __forceinline__ void wide_load(uintptr_t p, int c, int w, uint32_t e[F])
{
    if constexpr (F == 2) {
        if ((p & 7u) == 0 && c + 8 <= w) { const uint2 v = *reinterpret_cast<const uint2 *>(p); e[0] = v.x; e[1] = v.y; return; }
    } else {
        if ((p & 15u) == 0 && c + 4 * F <= w) {
#pragma unroll
            for (int q = 0; q < F; q += 4) {
                const uint4 v = *reinterpret_cast<const uint4 *>(p + 4 * q);
                e[q] = v.x; e[q + 1] = v.y; e[q + 2] = v.z; e[q + 3] = v.w;
            }
            return;
        }
    }
    load_partner<F>(p, c, w, e);
}

template <int F>
__global__ __launch_bounds__(WIDE_THREADS) void k_wide_reduce(const WideJob *jobs)
{
    constexpr int LOG2 = F == 2 ? 2 : F == 4 ? 4 : 6;         // 2 log2 F
    const WideJob J = jobs[blockIdx.z];
    const bool planeA = blockIdx.y != 0;
    const uint8_t *src = planeA ? J.src.a : J.src.b;
    const int ss = planeA ? J.src.sa : J.src.sb, r_off = planeA ? J.ox : 0, c_off = planeA ? J.oy : 0;
    uint8_t *dst = planeA ? J.ac : J.bc;
    const int ng = (J.wc + 3) >> 2, items = J.hc * ng;        // output dwords per row, per plane
    for (int item = (int)blockIdx.x * WIDE_THREADS + (int)threadIdx.x; item < items; item += (int)gridDim.x * WIDE_THREADS) {
        const int u = item / ng, g = item - u * ng;
        const int c = c_off + 4 * F * g;                      // the first source column; rows r_off + F u + t <= r_off + F hc - 1 < h
        uint32_t acc[4] = {0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < F; t++) {
            uint32_t e[F];
            wide_load<F>((uintptr_t)(src + (size_t)(r_off + F * u + t) * ss) + (uintptr_t)c, c, J.src.w, e);
#pragma unroll
            for (int q = 0; q < 4; q++) {
                if constexpr (F == 2) acc[q] = __builtin_amdgcn_sad_u8((q & 1) ? e[q >> 1] >> 16 : e[q >> 1] & 0xffffu, 0u, acc[q]);
                else if constexpr (F == 4) acc[q] = __builtin_amdgcn_sad_u8(e[q], 0u, acc[q]);
                else acc[q] = __builtin_amdgcn_sad_u8(e[2 * q + 1], 0u, __builtin_amdgcn_sad_u8(e[2 * q], 0u, acc[q]));
            }
        }
        uint32_t out = 0u;
#pragma unroll
        for (int q = 0; q < 4; q++)                           // (bytes of the last dword beyond wc: zeros)
            if (4 * g + q < J.wc) out |= ((acc[q] + (uint32_t)(F * F / 2)) >> LOG2) << (8 * q);
        *reinterpret_cast<uint32_t *>(dst + (size_t)u * J.sc + 4 * g) = out;      // sc is a multiple of 16 >= 4 ng
    }
}

int launch_wide_reduce(vfsms_ctx *ctx, const WideJob *d_jobs, const WideJob *h_jobs, int njobs, int factor)
{
    if (njobs <= 0) return VFSMS_OK;
    long long items = 1;
    for (int k = 0; k < njobs; k++) items = std::max(items, (long long)h_jobs[k].hc * ((h_jobs[k].wc + 3) >> 2));
    const dim3 grid((unsigned)std::min<long long>(WIDE_MAX_GX, (items + WIDE_THREADS - 1) / WIDE_THREADS), 2, (unsigned)njobs);
    if (factor == 2) hipLaunchKernelGGL(k_wide_reduce<2>, grid, dim3(WIDE_THREADS), 0, ctx->stream, d_jobs);
    else if (factor == 4) hipLaunchKernelGGL(k_wide_reduce<4>, grid, dim3(WIDE_THREADS), 0, ctx->stream, d_jobs);
    else hipLaunchKernelGGL(k_wide_reduce<8>, grid, dim3(WIDE_THREADS), 0, ctx->stream, d_jobs);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// A workgroup per job.  The coarse candidates in the order (-surface, i^2 + j^2, i, j) -- one 64-bit key, candidates numbered i-major --
// walked greedily: a candidate is kept when no kept one is its neighbour (Chebyshev distance <= 1), at most K.  Seed k of the job:
// seeds[k] = {ci, cj, coarse score, cx, cy, 0} ((cx, cy): the centre of its fine window; k_wide_pick turns them into the result) and
// the fine job k.  Fine jobs beyond the seeds used repeat seed 0 (they are searched and not read).
__global__ __launch_bounds__(WIDE_THREADS) void k_wide_seeds(const WideJob *jobs, const int32_t *surface, int R, int F, int K, AdjJob *fine,
                                                             int32_t *seeds, int32_t *out8)
{
    const int Rc = (R + F - 1) / F, C = 2 * Rc + 1, CC = C * C;
    __shared__ int32_t s_surf[WIDE_MAX_C * WIDE_MAX_C];
    __shared__ uint8_t s_dead[WIDE_MAX_C * WIDE_MAX_C];
    __shared__ unsigned long long s_best;
    const int job = blockIdx.x, tid = threadIdx.x;
    for (int c = tid; c < CC; c += WIDE_THREADS) { s_surf[c] = surface[(size_t)job * CC + c]; s_dead[c] = 0; }
    const AdjJob S = jobs[job].src;
    const int rf = min(F, R), lim = R - rf;
    int32_t *row = seeds + (size_t)job * VFSMS_WIDE_MAX_PEAKS * 6;
    AdjJob *fj = fine + (size_t)job * K;
    int used = 0;
    for (int k = 0; k < K; k++) {
        if (tid == 0) s_best = 0ull;
        __syncthreads();
        unsigned long long best = 0ull;
        for (int c = tid; c < CC; c += WIDE_THREADS) {
            if (s_dead[c]) continue;
            const int i = c / C - Rc, j = c - (c / C) * C - Rc;
            const unsigned long long key = ((unsigned long long)((uint32_t)s_surf[c] ^ 0x80000000u) << 32) |
                                           ((unsigned long long)(1023 - (i * i + j * j)) << 12) | (unsigned long long)(4095 - c);
            best = key > best ? key : best;
        }
        if (best) atomicMax(&s_best, best);
        __syncthreads();
        const unsigned long long b = s_best;                  // the same for every lane
        if (!b) break;
        const int cw = 4095 - (int)(b & 4095ull), ci = cw / C - Rc, cj = cw - (cw / C) * C - Rc;
        for (int c = tid; c < CC; c += WIDE_THREADS) {
            const int i = c / C - Rc, j = c - (c / C) * C - Rc;
            if (abs(i - ci) <= 1 && abs(j - cj) <= 1) s_dead[c] = 1;
        }
        if (tid == 0) {
            const int cx = min(max(F * ci, -lim), lim), cy = min(max(F * cj, -lim), lim);
            row[k * 6] = ci; row[k * 6 + 1] = cj; row[k * 6 + 2] = s_surf[cw]; row[k * 6 + 3] = cx; row[k * 6 + 4] = cy; row[k * 6 + 5] = 0;
            AdjJob f = S; f.dx = S.dx + cx; f.dy = S.dy + cy;
            fj[k] = f;
        }
        used++;
        __syncthreads();
    }
    if (tid == 0) {
        for (int k = used; k < VFSMS_WIDE_MAX_PEAKS; k++) {
            for (int q = 0; q < 6; q++) row[k * 6 + q] = 0;
            if (k < K) { AdjJob f = S; f.dx = S.dx + row[3]; f.dy = S.dy + row[4]; fj[k] = f; }
        }
        out8[(size_t)job * 8 + 7] = used;
    }
}

int launch_wide_seeds(vfsms_ctx *ctx, const WideJob *d_jobs, int njobs, int radius, int factor, int peaks, const int32_t *d_surface,
                      AdjJob *d_fine, int32_t *d_seeds, int32_t *d_out8)
{
    if (njobs <= 0) return VFSMS_OK;
    hipLaunchKernelGGL(k_wide_seeds, dim3(njobs), dim3(WIDE_THREADS), 0, ctx->stream, d_jobs, d_surface, radius, factor, peaks, d_fine, d_seeds, d_out8);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// A lane per job: seed k's result is (cx + bi, cy + bj) with the fixed-point score of its fine search; the winner has the smallest
// (-fixed, ti^2 + tj^2, ti, tj)
__global__ __launch_bounds__(WIDE_THREADS) void k_wide_pick(int njobs, int K, const int32_t *fine_best4, int32_t *seeds, int32_t *out8)
{
    const int job = (int)blockIdx.x * WIDE_THREADS + (int)threadIdx.x;
    if (job >= njobs) return;
    int32_t *row = seeds + (size_t)job * VFSMS_WIDE_MAX_PEAKS * 6, *out = out8 + (size_t)job * 8;
    const int used = out[7];
    int w = -1, wi = 0, wj = 0, wf = 0, wd = 0;
    for (int k = 0; k < used; k++) {
        const int32_t *b4 = fine_best4 + 4 * ((size_t)job * K + k);
        const int ti = row[k * 6 + 3] + b4[0], tj = row[k * 6 + 4] + b4[1], fx = b4[2], d2 = ti * ti + tj * tj;
        row[k * 6 + 3] = ti; row[k * 6 + 4] = tj; row[k * 6 + 5] = fx;
        if (w < 0 || fx > wf || (fx == wf && (d2 < wd || (d2 == wd && (ti < wi || (ti == wi && tj < wj)))))) { w = k; wi = ti; wj = tj; wf = fx; wd = d2; }
    }
    out[0] = wi; out[1] = wj; out[2] = wf; out[3] = fine_best4[4 * ((size_t)job * K + w) + 3];
    out[4] = row[w * 6]; out[5] = row[w * 6 + 1]; out[6] = row[w * 6 + 2];
}

int launch_wide_pick(vfsms_ctx *ctx, int njobs, int peaks, const int32_t *d_fine_best4, int32_t *d_seeds, int32_t *d_out8)
{
    if (njobs <= 0) return VFSMS_OK;
    hipLaunchKernelGGL(k_wide_pick, dim3((njobs + WIDE_THREADS - 1) / WIDE_THREADS), dim3(WIDE_THREADS), 0, ctx->stream, njobs, peaks, d_fine_best4, d_seeds, d_out8);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// out6[job] = {N, Sa, Sb, Saa, Sbb, Sab} at the job's own offset (cleared by the caller): a workgroup of 4 waves per block of rows
__global__ __launch_bounds__(WIDE_THREADS) void k_wide_sums(const AdjJob *jobs, unsigned long long *out6)
{
    const AdjJob J = jobs[blockIdx.y];
    const Overlap o = verify_overlap(J.h, J.w, J.dx, J.dy);
    if (o.r1 <= o.r0 || o.c1 <= o.c0) return;
    unsigned long long *out = out6 + 6 * (size_t)blockIdx.y;
    if (blockIdx.x == 0 && threadIdx.x == 0) out[0] = (unsigned long long)(o.r1 - o.r0) * (unsigned long long)(o.c1 - o.c0);
    overlap_rows_sums(J.a, J.sa, J.b, J.sb, o, J.dx, J.dy, out + 1);
}

// njobs <= 65535
int launch_overlap_sums(vfsms_ctx *ctx, const AdjJob *d_jobs, const AdjJob *h_jobs, int njobs, unsigned long long *d_out6)
{
    if (njobs <= 0) return VFSMS_OK;
    int rows = 1;
    for (int k = 0; k < njobs; k++) rows = std::max(rows, h_jobs[k].h);
    HIP_TRY(hipMemsetAsync(d_out6, 0, sizeof(unsigned long long) * 6 * (size_t)njobs, ctx->stream));
    hipLaunchKernelGGL(k_wide_sums, dim3((unsigned)std::min(64, (rows + 31) / 32), (unsigned)njobs), dim3(WIDE_THREADS), 0, ctx->stream, d_jobs, d_out6);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
