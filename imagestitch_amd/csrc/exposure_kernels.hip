// exposure_kernels.hip -- Method.exposureCompensation = "gain": the overlap statistic of pairs of resident tiles and the per-tile Q12 gain,
// for gfx950.
//
// Specification: tests/exposure_ref.py (everything is integer, so the device equals it exactly; there is no reference counterpart).
//   statistic  tile B's pixel (r, c) meets tile A's pixel (r + dx, c + dy); over every sample (byte) of the B pixels whose partner lies
//              inside A, with lo <= a <= hi and lo <= b <= hi: N = their number, Sa / Sb = the sums of the A / B samples.  The sums are
//              integers, so the reduction order is free.
//   apply      out = min(255, (p * Q + 2048) >> 12) on every sample of a tile, Q its Q12 gain (the arithmetic of the shading apply)
//
// A tile is h rows of w * ch bytes; both kernels work on bytes and never look at the channel count: the host cuts the rectangle in bytes
// (column offset dy * ch), and a pixel's channels meet the same channels of its partner.
//
//   (memset)         the three sums of every job = 0
//   k_overlap_stats  grid (row groups, jobs).  No host synchronisation between the two.
//   k_exposure_apply grid (4 KiB blocks of a tile, tiles whose gain is not 4096)
//
// k_overlap_stats.  The rows of a job's rectangle are cut into groups of exp_rows_per_group rows, one workgroup each; its lanes take the
// (row, chunk) items of the group, a chunk being 16 bytes of a B row cut at B's 16-byte ADDRESS boundaries -- so a row's first and last
// chunk are ragged, and a 16-bit column mask zeroes what lies outside the rectangle: nothing is restricted to an aligned core.  A chunk
// that lies inside the row is one aligned uint4 load, a ragged one the aligned dwords that hold a byte of the row.  The 16 partner bytes
// of A come from the five aligned dwords around them, those that hold a byte of A's row, funnel-shifted (alignbyte) by their alignment
// (load_partner of overlap_sums.h, which also holds the masks and the workgroup reduction).  The band is a
// byte mask computed four bytes at a time (exp_band) on both operands; N is the population count of the combined mask / 8.
//
// 32-bit lane sums.  A lane sees at most EXP_LANE_CAP chunks of 16 bytes: its sums are at most 65536 * 16 * 255 = 267 386 880 and its
// mask bits 65536 * 128 = 8 388 608, both < 2^32.  overlap_stats_device sizes the grid for about EXP_LANE_ITEMS chunks per lane and refuses
// a job that would exceed the cap.  64 bits from the wave reduction on; one 64-bit vector atomic add per workgroup and sum.
#include "common.h"
#include "tile_table.h"
#include "overlap_sums.h"
#include <algorithm>

#define EXP_THREADS 256
#define EXP_LANE_ITEMS 16    // chunks a lane should get before a job takes another workgroup: 4096 chunks = 64 KiB of B per workgroup
#define EXP_LANE_CAP 65536   // chunks a lane may get, at most (see above)
#define EXP_MAX_GX 1024      // row groups of a job, at most

// rows per workgroup of a job of nrows rows of at most cpr chunks on a grid of gx row groups: as many groups as give every lane about
// EXP_LANE_ITEMS chunks, all gx when that is not enough.  The host sizes gx and checks the cap with the same function.
__host__ __device__ __forceinline__ int exp_rows_per_group(int nrows, int cpr, int gx)
{
    const long long per = (long long)EXP_THREADS * EXP_LANE_ITEMS;
    long long ng = ((long long)nrows * cpr + per - 1) / per;
    ng = ng < 1 ? 1 : (ng > gx ? gx : ng);
    return (int)((nrows + ng - 1) / ng);
}
// chunks of any row of a rectangle whose byte columns are [c0, c1), at most: the first chunk may start up to 15 bytes before c0
__host__ __device__ __forceinline__ int exp_chunks_per_row(int c0, int c1) { return ((c1 - c0 + 15) >> 4) + 1; }

// 0xff in every byte x of v with lo <= x <= hi.  Two bytes at a time in 16-bit fields: bit 8 of x + (256 - lo) is set iff x >= lo, bit 8
// of (256 + hi) - x iff x <= hi (both stay below 512, so no field reaches its neighbour); klo = (256 - lo) * 0x00010001, khi = (256 + hi) * 0x00010001
__device__ __forceinline__ uint32_t exp_band(uint32_t v, uint32_t klo, uint32_t khi)
{
    const uint32_t e = v & 0x00ff00ffu, o = (v >> 8) & 0x00ff00ffu;
    const uint32_t te = ((e + klo) & (khi - e) & 0x01000100u) >> 8, to = ((o + klo) & (khi - o) & 0x01000100u) >> 8;
    return (te * 0xffu) | ((to * 0xffu) << 8);
}

// out3: [job][3] uint64 = N, Sa, Sb
__global__ __launch_bounds__(EXP_THREADS) void k_overlap_stats(const ExpJob *jobs, unsigned long long *out3, int lo, int hi)
{
    const ExpJob J = jobs[blockIdx.y];
    if (J.nrows <= 0) return;
    const int cpr = exp_chunks_per_row(J.c0, J.c1);
    const int rpg = exp_rows_per_group(J.nrows, cpr, (int)gridDim.x);
    const int g0 = (int)blockIdx.x * rpg;
    if (g0 >= J.nrows) return;
    const int items = min(rpg, J.nrows - g0) * cpr;
    const uint32_t klo = (256u - (uint32_t)lo) * 0x00010001u, khi = (256u + (uint32_t)hi) * 0x00010001u;

    uint32_t bits = 0u, sa = 0u, sb = 0u;
    for (int item = threadIdx.x; item < items; item += EXP_THREADS) {
        const int rr = item / cpr, k = item - rr * cpr;
        const int r = J.r0 + g0 + rr;
        const uintptr_t pb = (uintptr_t)(J.b + (size_t)r * J.sb);
        const int c = J.c0 - (int)((pb + (uintptr_t)J.c0) & 15u) + (k << 4);      // the chunk's first column: pb + c is 16-byte aligned
        if (c >= J.c1) continue;
        const uint32_t m16 = range_bits(c, J.c0, J.c1, 16);
        // B: the chunk's four dwords, those that hold a byte of the row
        uint32_t b[4];
        const uintptr_t qb = pb + (uintptr_t)(intptr_t)c;
        if (c >= 0 && c + 16 <= J.wb) {
            const uint4 v = *reinterpret_cast<const uint4 *>(qb);
            b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w;
        } else {
            const uint32_t *b4 = reinterpret_cast<const uint32_t *>(qb);
#pragma unroll
            for (int t = 0; t < 4; t++) b[t] = (c + 4 * t + 3 >= 0 && c + 4 * t < J.wb) ? b4[t] : 0u;
        }
        // A: the 16 partner bytes from the aligned dwords around them, those that hold a byte of A's row
        const int ca = c + J.dyb;
        const uintptr_t pa = (uintptr_t)(J.a + (size_t)(r + J.dx) * J.sa) + (uintptr_t)(intptr_t)ca;
        uint32_t e[4];
        load_partner<4>(pa, ca, J.wa, e);
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const uint32_t a = e[t];
            const uint32_t keep = byte_mask((m16 >> (4 * t)) & 15u) & exp_band(a, klo, khi) & exp_band(b[t], klo, khi);
            bits += __popc(keep);
            sa = __builtin_amdgcn_sad_u8(a & keep, 0u, sa);
            sb = __builtin_amdgcn_sad_u8(b[t] & keep, 0u, sb);
        }
    }

    const unsigned long long v3[3] = {bits >> 3, sa, sb};
    wg_add_u64<3, EXP_THREADS / 64>(v3, out3 + 3 * (size_t)blockIdx.y);
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------------
struct ExpTile { uint8_t *ptr; int stride, h, wb; uint32_t gain; int dense; };

__device__ __forceinline__ uint32_t exp_px(uint32_t p, uint32_t g) { return min(255u, (p * g + 2048u) >> 12); }
__device__ __forceinline__ uint32_t exp_word(uint32_t v, uint32_t g)
{
    return exp_px(v & 255u, g) | (exp_px((v >> 8) & 255u, g) << 8) | (exp_px((v >> 16) & 255u, g) << 16) | (exp_px(v >> 24, g) << 24);
}

// grid (16-byte blocks of the largest tile / 256, tiles): the access pattern of k_shade_apply, one gain per tile instead of a gain plane
__global__ __launch_bounds__(EXP_THREADS) void k_exposure_apply(const ExpTile *tiles)
{
    const ExpTile T = tiles[blockIdx.y];
    const size_t total = (size_t)T.h * T.wb, e0 = ((size_t)blockIdx.x * EXP_THREADS + threadIdx.x) * 16u;
    if (e0 >= total) return;
    if (T.dense && e0 + 16 <= total) {                       // dense: stride wb and a 16-byte aligned base
        uint4 *p = (uint4 *)(T.ptr + e0);
        uint4 v = *p;
        v.x = exp_word(v.x, T.gain); v.y = exp_word(v.y, T.gain); v.z = exp_word(v.z, T.gain); v.w = exp_word(v.w, T.gain);
        *p = v;
        return;
    }
    for (size_t e = e0; e < min(e0 + 16, total); e++) {      // the tile's last bytes, or a tile with row padding
        uint8_t *p = T.ptr + (e / T.wb) * T.stride + e % T.wb;
        *p = (uint8_t)exp_px(*p, T.gain);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
// the rectangle of B that has a partner in A, in bytes; 64-bit arithmetic: any int offset is an argument, far outside included
static ExpJob exp_job(const ExpPairHost &P)
{
    ExpJob J{P.a, P.b, P.sa, P.sb, P.wa, P.wb, 0, 0, 0, 0, 0, 0};
    const long long dx = P.dx, dyb = (long long)P.dy * P.ch;
    const long long r0 = std::max(0ll, -dx), r1 = std::min<long long>(P.hb, P.ha - dx);
    const long long c0 = std::max(0ll, -dyb), c1 = std::min<long long>(P.wb, P.wa - dyb);
    if (r1 > r0 && c1 > c0) { J.r0 = (int)r0; J.nrows = (int)(r1 - r0); J.c0 = (int)c0; J.c1 = (int)c1; J.dx = P.dx; J.dyb = (int)dyb; }
    return J;
}

// N, Sa, Sb of n pairs into d_out3 ([n][3] uint64), enqueued on the context's stream; the arena holds the job records
int overlap_stats_device(vfsms_ctx *ctx, const ExpPairHost *pairs, int n, int lo, int hi, unsigned long long *d_out3)
{
    if (n <= 0) return VFSMS_OK;
    std::vector<ExpJob> H(n);
    long long gx = 1;
    for (int k = 0; k < n; k++) {
        H[k] = exp_job(pairs[k]);
        const long long items = (long long)H[k].nrows * exp_chunks_per_row(H[k].c0, H[k].c1);
        gx = std::max(gx, (items + EXP_THREADS * EXP_LANE_ITEMS - 1) / (EXP_THREADS * EXP_LANE_ITEMS));
    }
    gx = std::min<long long>(gx, EXP_MAX_GX);
    for (int k = 0; k < n; k++) {
        const int cpr = exp_chunks_per_row(H[k].c0, H[k].c1);
        const long long per_lane = ((long long)exp_rows_per_group(H[k].nrows, cpr, (int)gx) * cpr + EXP_THREADS - 1) / EXP_THREADS;
        if (per_lane > EXP_LANE_CAP) { vfsms_set_error("overlap_stats: the overlap of job %d is too large for 32-bit lane sums", k); return VFSMS_ERR_UNSUPPORTED; }
    }
    ExpJob *d_jobs;
    TRY(ctx_upload_small(ctx, H.data(), sizeof(ExpJob) * (size_t)n, (void **)&d_jobs));
    ProfScope ps(ctx, "exposure");
    HIP_TRY(hipMemsetAsync(d_out3, 0, sizeof(unsigned long long) * 3 * (size_t)n, ctx->stream));
    const int part = 32768;                                  // jobs per launch (a grid dimension holds 65535)
    for (int k0 = 0; k0 < n; k0 += part)
        hipLaunchKernelGGL(k_overlap_stats, dim3((unsigned)gx, (unsigned)std::min(part, n - k0)), dim3(EXP_THREADS), 0, ctx->stream,
                           d_jobs + k0, d_out3 + 3 * (size_t)k0, lo, hi);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// the n tiles corrected in place, tile i by gain_q12[i]; a gain of 4096 changes no byte, so such a tile gets no workgroup
static_assert(sizeof(ExpTile) <= 2 * sizeof(TileView), "api.hip reserves two TileView per tile for the table and its staging");
int exposure_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, const uint16_t *gain_q12)
{
    std::vector<ExpTile> T;
    size_t most = 0;
    for (int i = 0; i < n; i++) {
        if (gain_q12[i] == 4096) continue;
        const TileView &t = tiles[i];
        const int wb = t.w * t.ch;                             // a row in bytes
        T.push_back(ExpTile{t.ptr, t.stride, t.h, wb, gain_q12[i], t.stride == wb && ((uintptr_t)t.ptr & 15u) == 0});
        most = std::max(most, (size_t)t.h * wb);
    }
    if (T.empty() || most == 0) return VFSMS_OK;
    const size_t gx = (most + 16 * EXP_THREADS - 1) / (16 * EXP_THREADS);
    if (gx > 0x7fffffffu) { vfsms_set_error("exposure_apply: a tile is too large"); return VFSMS_ERR_UNSUPPORTED; }
    ExpTile *d_tiles;
    TRY(ctx_upload_small(ctx, T.data(), sizeof(ExpTile) * T.size(), (void **)&d_tiles));
    ProfScope ps(ctx, "exposure");
    hipLaunchKernelGGL(k_exposure_apply, dim3((unsigned)gx, (unsigned)T.size()), dim3(EXP_THREADS), 0, ctx->stream, d_tiles);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
