// shading_kernels.hip -- Method.shadingCorrection: a flat-field gain estimated from the tile stack of a mosaic, for gfx950.
//
// The arithmetic is this project's specification (tests/shading_ref.py restates it in numpy; everything is integer, so every stage must
// equal it exactly; there is no reference counterpart):
//   profile  P = the k-th smallest byte over the N tiles per sample, k = (N - 1) * percentile / 100
//   smooth   Q = P << 8 (Q8, uint16), two passes of Q' = (boxsum(Q) + area / 2) / area over (2R + 1)^2 with clamped indices, rounded once
//            per pass after both axes
//   level    M_c = (sum Q_c + h w / 2) / (h w) per channel, 64-bit sum
//   gain     G = min(65535, (M_c * 4096 + Q / 2) / Q), 4096 where Q == 0 (Q12, uint16)
//   apply    out = min(255, (p * G + 2048) >> 12), in place
//
// A tile is h rows of wb = w * ch bytes; the kernels work on bytes and know the channel count only where neighbours (ch bytes apart) or
// channel sums matter.
//   k_shade_select  one wave64 per 256 consecutive samples, 4 adjacent bytes per lane.  Up to SHADE_LDS_MAX_N tiles the wave stages its
//                   N x 256 B slab in LDS (each lane its own dword per tile: no lane reads another's, so no barrier) and the 8 steps of the
//                   bitwise descent run from there: the stack is read from HBM once.  Above, every step re-reads the slab from global memory.
//   k_shade_box_h   row sums of 2R + 1 clamped neighbours from an LDS copy of the row segment -> uint32
//   k_shade_box_v   running column sums over bands of SHADE_BAND rows, rounding division -> uint16
//   k_shade_level   per-channel 64-bit sums (LDS atomics per workgroup, one vector atomic per workgroup and channel), k_shade_gain the division
//                   (box passes, level and gain are shade_field_device: the deep path's 16-bit field, deep_shading_kernels.hip, goes through it too)
//   k_shade_apply   grid over 16-byte blocks of a tile, inner loop over the tiles: a gain vector is loaded once and used N times
#include "common.h"
#include "tile_table.h"
#include <algorithm>

#define SHADE_LDS_MAX_N 320            // tiles a wave stages in LDS: 320 x 256 B = 80 KiB, two waves per CU
#define SHADE_BAND 32                  // rows per thread of the vertical running sum
#define SHADE_SEG 1024                 // samples per workgroup of the horizontal pass
#define SHADE_LEVEL_BLOCKS 96          // 96 x 256 threads: a multiple of every channel count 1..4, so a thread stays on one channel

struct ShadeTile { uint8_t *ptr; int stride, pad; };

// ---- profile -------------------------------------------------------------------------------------------------------------------------------
// sample e of the plane (row-major over h x wb) inside a tile with its own row stride
__device__ __forceinline__ size_t shade_off(unsigned e, int wb, int stride) { return (size_t)(e / wb) * stride + e % wb; }

template <bool STAGED>
__global__ __launch_bounds__(64) void k_shade_select(const ShadeTile *tiles, int n, int k, unsigned total, int wb, int dense, uint8_t *prof)
{
    extern __shared__ uint32_t slab[];                       // STAGED: [n][64]
    const unsigned lane = threadIdx.x, e0 = (blockIdx.x * 64u + lane) * 4u;
    if (e0 >= total) return;
    const bool word = dense && e0 + 4 <= total;              // dense: every tile has stride wb and a 4-byte aligned base -> one aligned dword
    auto fetch = [&](int i) -> uint32_t {
        const ShadeTile t = tiles[i];
        if (word) return *(const uint32_t *)(t.ptr + e0);
        uint32_t v = 0;
        for (unsigned j = 0; j < 4 && e0 + j < total; j++) v |= (uint32_t)t.ptr[shade_off(e0 + j, wb, t.stride)] << (8 * j);
        return v;
    };
    if (STAGED)
        for (int i = 0; i < n; i++) slab[i * 64 + lane] = fetch(i);
    // the largest c with #{x < c} <= k is the k-th smallest (0-based): bit by bit from the top
    uint32_t pre0 = 0, pre1 = 0, pre2 = 0, pre3 = 0;
    for (int bit = 7; bit >= 0; bit--) {
        const uint32_t c0 = pre0 | (1u << bit), c1 = pre1 | (1u << bit), c2 = pre2 | (1u << bit), c3 = pre3 | (1u << bit);
        int n0 = 0, n1 = 0, n2 = 0, n3 = 0;
        for (int i = 0; i < n; i++) {
            const uint32_t v = STAGED ? slab[i * 64 + lane] : fetch(i);
            n0 += (v & 255u) < c0; n1 += ((v >> 8) & 255u) < c1; n2 += ((v >> 16) & 255u) < c2; n3 += (v >> 24) < c3;
        }
        if (n0 <= k) pre0 = c0;
        if (n1 <= k) pre1 = c1;
        if (n2 <= k) pre2 = c2;
        if (n3 <= k) pre3 = c3;
    }
    if (e0 + 4 <= total) *(uint32_t *)(prof + e0) = pre0 | (pre1 << 8) | (pre2 << 16) | (pre3 << 24);     // prof is dense and 256-byte aligned
    else {
        const uint32_t p[4] = {pre0, pre1, pre2, pre3};
        for (unsigned j = 0; e0 + j < total; j++) prof[e0 + j] = (uint8_t)p[j];
    }
}

__global__ __launch_bounds__(256) void k_shade_q8(const uint8_t *prof, uint16_t *q, unsigned total)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e < total) q[e] = (uint16_t)(prof[e] << 8);
}

// ---- box passes ------------------------------------------------------------------------------------------------------------------------------
// The plane is any uint16: the Q8 profile of the 8-bit path (at most 255 << 8) or the 16-bit field of the deep path (ch = 1, at most 65535).
// uint32 is exact: a row sum is at most 255 * 65535, a window sum plus area / 2 at most 255^2 * 65535 + 32512 = 4 261 445 887 < 2^32
// (R <= 127; a rounded mean never exceeds its inputs' maximum, so the second pass has the same bound)
__global__ __launch_bounds__(256) void k_shade_box_h(const uint16_t *q, uint32_t *rows, int w, int ch, int R)
{
    __shared__ uint16_t seg[SHADE_SEG + 2 * 127 * 4];
    const int wb = w * ch, x0 = blockIdx.x * SHADE_SEG, y = blockIdx.y, halo = R * ch;
    const int len = min(SHADE_SEG, wb - x0) + 2 * halo;
    const uint16_t *src = q + (size_t)y * wb;
    // staged sample i is byte column x0 - halo + i: its channel is that of x0 + i (halo is a whole number of pixels), its pixel clamped to the row
    for (int i = threadIdx.x; i < len; i += 256) {
        const int c = (x0 + i) % ch;
        const int p = min(max((x0 + i - c) / ch - R, 0), w - 1);
        seg[i] = src[p * ch + c];
    }
    __syncthreads();
    for (int i = threadIdx.x; i < len - 2 * halo; i += 256) {
        uint32_t s = 0;
        for (int d = 0; d <= 2 * R; d++) s += seg[i + d * ch];
        rows[(size_t)y * wb + x0 + i] = s;
    }
}

__global__ __launch_bounds__(256) void k_shade_box_v(const uint32_t *rows, uint16_t *q, int h, int wb, int R)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y0 = blockIdx.y * SHADE_BAND;
    if (x >= wb) return;
    const uint32_t area = (uint32_t)(2 * R + 1) * (2 * R + 1);
    uint32_t s = 0;
    for (int d = -R; d <= R; d++) s += rows[(size_t)min(max(y0 + d, 0), h - 1) * wb + x];
    const int y1 = min(y0 + SHADE_BAND, h);
    for (int y = y0; y < y1; y++) {
        q[(size_t)y * wb + x] = (uint16_t)((s + area / 2) / area);
        s += rows[(size_t)min(y + R + 1, h - 1) * wb + x] - rows[(size_t)max(y - R, 0) * wb + x];      // (unsigned wrap cancels: the true sum is in range)
    }
}

// ---- level and gain ----------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_shade_level(const uint16_t *q, unsigned total, int ch, unsigned long long *sums)
{
    __shared__ unsigned long long part[4];
    if (threadIdx.x < 4) part[threadIdx.x] = 0;
    __syncthreads();
    const unsigned T = SHADE_LEVEL_BLOCKS * 256u, g = blockIdx.x * 256u + threadIdx.x;
    unsigned long long s = 0;
    for (unsigned e = g; e < total; e += T) s += q[e];       // T % ch == 0: every e of this thread has channel g % ch
    atomicAdd(&part[g % ch], s);
    __syncthreads();
    if (threadIdx.x < ch) atomicAdd(&sums[threadIdx.x], part[threadIdx.x]);
}

__global__ void k_shade_mean(const unsigned long long *sums, unsigned long long hw, int ch, uint32_t *mean)
{
    if ((int)threadIdx.x < ch) mean[threadIdx.x] = (uint32_t)((sums[threadIdx.x] + hw / 2) / hw);
}

__global__ __launch_bounds__(256) void k_shade_gain(const uint16_t *q, const uint32_t *mean, unsigned total, int ch, uint16_t *gain)
{
    const unsigned e = blockIdx.x * 256u + threadIdx.x;
    if (e >= total) return;
    const uint32_t v = q[e], m = mean[e % ch];               // m * 4096 + v / 2 <= 65535 * 4096 + 32767 < 2^32
    gain[e] = v ? (uint16_t)min(65535u, (m * 4096u + v / 2) / v) : (uint16_t)4096;
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t shade_px(uint32_t p, uint32_t g) { return min(255u, (p * g + 2048u) >> 12); }
__device__ __forceinline__ uint32_t shade_word(uint32_t v, uint32_t g01, uint32_t g23)
{
    return shade_px(v & 255u, g01 & 0xffffu) | (shade_px((v >> 8) & 255u, g01 >> 16) << 8) |
           (shade_px((v >> 16) & 255u, g23 & 0xffffu) << 16) | (shade_px(v >> 24, g23 >> 16) << 24);
}

__global__ __launch_bounds__(256) void k_shade_apply(const ShadeTile *tiles, int n, const uint16_t *gain, unsigned total, int wb, int dense)
{
    const unsigned e0 = (blockIdx.x * 256u + threadIdx.x) * 16u;
    if (e0 >= total) return;
    if (dense && e0 + 16 <= total) {                         // dense: stride wb and a 16-byte aligned base for every tile
        const uint4 ga = *(const uint4 *)(gain + e0), gb = *(const uint4 *)(gain + e0 + 8);
        for (int i = 0; i < n; i++) {
            uint4 *p = (uint4 *)(tiles[i].ptr + e0);
            uint4 v = *p;
            v.x = shade_word(v.x, ga.x, ga.y); v.y = shade_word(v.y, ga.z, ga.w);
            v.z = shade_word(v.z, gb.x, gb.y); v.w = shade_word(v.w, gb.z, gb.w);
            *p = v;
        }
        return;
    }
    for (unsigned e = e0; e < min(e0 + 16u, total); e++) {   // the plane's last bytes, or tiles with row padding
        const uint32_t g = gain[e];
        for (int i = 0; i < n; i++) {
            uint8_t *p = tiles[i].ptr + shade_off(e, wb, tiles[i].stride);
            *p = (uint8_t)shade_px(*p, g);
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
static_assert(sizeof(ShadeTile) <= 2 * sizeof(TileView), "api.hip reserves two TileView per tile for the table and its staging");
static int shade_table(vfsms_ctx *ctx, const TileView *tiles, int n, int wb, size_t align, ShadeTile **d_tiles, int *dense)
{
    std::vector<ShadeTile> T(n);
    *dense = 1;
    for (int i = 0; i < n; i++) {
        T[i].ptr = tiles[i].ptr; T[i].stride = tiles[i].stride; T[i].pad = 0;
        if (tiles[i].stride != wb || ((uintptr_t)tiles[i].ptr & (align - 1))) *dense = 0;
    }
    return ctx_upload_small(ctx, T.data(), sizeof(ShadeTile) * n, (void **)d_tiles);
}

// What follows a profile, for the 8-bit and the deep path alike: the uint16 plane q (h rows of w * ch samples) smoothed in place by two
// box passes, its channel levels, and the gain plane.  The caller has checked the plane's size (shade_plane_fits)
int shade_field_device(vfsms_ctx *ctx, uint16_t *q, int h, int w, int ch, int radius, uint16_t *gain)
{
    const int wb = w * ch;
    const size_t total64 = (size_t)h * wb;
    const unsigned total = (unsigned)total64, eb = (total + 255) / 256;
    // scratch: the uint32 row sums, then 4 channel sums and 4 channel means
    TRY(ctx->shade_scratch.reserve(total64 * 4 + 256, ctx->stream));
    uint32_t *rows = ctx->shade_scratch.as<uint32_t>();
    unsigned long long *sums = (unsigned long long *)(ctx->shade_scratch.as<char>() + ((total64 * 4 + 63) & ~(size_t)63));
    uint32_t *mean = (uint32_t *)(sums + 4);
    for (int pass = 0; pass < 2; pass++) {
        hipLaunchKernelGGL(k_shade_box_h, dim3((wb + SHADE_SEG - 1) / SHADE_SEG, h), dim3(256), 0, ctx->stream, q, rows, w, ch, radius);
        hipLaunchKernelGGL(k_shade_box_v, dim3((wb + 255) / 256, (h + SHADE_BAND - 1) / SHADE_BAND), dim3(256), 0, ctx->stream, rows, q, h, wb, radius);
    }
    HIP_TRY(hipMemsetAsync(sums, 0, 4 * sizeof(unsigned long long), ctx->stream));
    hipLaunchKernelGGL(k_shade_level, dim3(SHADE_LEVEL_BLOCKS), dim3(256), 0, ctx->stream, q, total, ch, sums);
    hipLaunchKernelGGL(k_shade_mean, dim3(1), dim3(64), 0, ctx->stream, sums, (unsigned long long)h * w, ch, mean);
    hipLaunchKernelGGL(k_shade_gain, dim3(eb), dim3(256), 0, ctx->stream, q, mean, total, ch, gain);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
// the planes those kernels index with 32 bits and a 16-bit grid row: `who` names the refused call
int shade_plane_fits(const char *who, int h, size_t row_samples)
{
    if ((size_t)h * row_samples <= 0x7fffffffu && h <= 65535) return VFSMS_OK;
    vfsms_set_error("%s: tiles of more than 2^31 - 1 samples or 65535 rows are not supported", who);
    return VFSMS_ERR_UNSUPPORTED;
}

// profile, smoothed field and gain of n tiles (h rows of w * ch bytes each) into the three planes of a field
int shade_estimate_device(vfsms_ctx *ctx, const TileView *tiles, int n, int h, int w, int ch, int percentile, int radius,
                          uint16_t *gain, uint16_t *q8, uint8_t *prof)
{
    const int wb = w * ch;
    TRY(shade_plane_fits("shading_estimate", h, (size_t)wb));
    const unsigned total = (unsigned)((size_t)h * wb);
    ShadeTile *d_tiles; int dense;
    TRY(shade_table(ctx, tiles, n, wb, 4, &d_tiles, &dense));
    const int k = (int)((long long)(n - 1) * percentile / 100);
    ProfScope ps(ctx, "shading");
    const unsigned sel_blocks = (total + 255) / 256;
    if (n <= SHADE_LDS_MAX_N) {
        HIP_TRY(hipFuncSetAttribute((const void *)k_shade_select<true>, hipFuncAttributeMaxDynamicSharedMemorySize, SHADE_LDS_MAX_N * 256));   // (per device: not cached)
        hipLaunchKernelGGL(k_shade_select<true>, dim3(sel_blocks), dim3(64), (size_t)n * 256, ctx->stream, d_tiles, n, k, total, wb, dense, prof);
    } else
        hipLaunchKernelGGL(k_shade_select<false>, dim3(sel_blocks), dim3(64), 0, ctx->stream, d_tiles, n, k, total, wb, dense, prof);
    hipLaunchKernelGGL(k_shade_q8, dim3((total + 255) / 256), dim3(256), 0, ctx->stream, prof, q8, total);
    return shade_field_device(ctx, q8, h, w, ch, radius, gain);
}

// the n tiles corrected in place by a field's gain
int shade_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, int h, int w, int ch, const uint16_t *gain)
{
    const int wb = w * ch;
    const size_t total64 = (size_t)h * wb;
    if (total64 > 0x7fffffffu) { vfsms_set_error("shading_apply: tiles of more than 2^31 - 1 bytes are not supported"); return VFSMS_ERR_UNSUPPORTED; }
    ShadeTile *d_tiles; int dense;
    TRY(shade_table(ctx, tiles, n, wb, 16, &d_tiles, &dense));
    ProfScope ps(ctx, "shading");
    hipLaunchKernelGGL(k_shade_apply, dim3((unsigned)((total64 + 4095) / 4096)), dim3(256), 0, ctx->stream, d_tiles, n, gain, (unsigned)total64, wb, dense);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
