// deep_shading_kernels.hip -- flat-field correction of 16-bit gray tiles (vfsms_deep_shading_*), for gfx950.
//
// The arithmetic is this project's specification (tests/deep_shading_ref.py restates it in numpy; everything is integer, so every stage
// must equal it exactly; there is no reference counterpart):
//   profile  P = the k-th smallest sample over the N tiles per position, k = (N - 1) * percentile / 100 (uint16)
//   field    F = max(P - d, 0) with d the camera's pedestal, then the two rounded box passes, the level M and the Q12 gain of the 8-bit
//            path, on the SAME kernels (shade_field_device, shading_kernels.hip: the field is a uint16 plane with ch = 1; no Q8 shift)
//   apply    out = p where p <= d, else min(65535, d + (((p - d) * G + 2048) >> 12)), in place
//
// A deep tile is dense (h * w samples from a 256-byte aligned base), so the kernels see one run of samples per tile and never a row.
//   k_deep_shade_select  one wave64 per 128 consecutive samples, one dword (two adjacent samples) per lane.  Up to DEEP_SHADE_LDS_MAX_N tiles
//                        the wave stages its N x 256 B slab in LDS (lane l reads and writes only word l of every row: no barrier, and bank
//                        l % 32 with lanes l and l + 32 in different halves: conflict-free) and the 16 steps of the bitwise descent run from
//                        there: the stack is read from HBM once.  Above, every step re-reads the slab from global memory.
//                        Both samples of a dword are compared at once with packed 16-bit arithmetic (deep_lt2) and both counts (at most
//                        4096: 13 bits) ride in the halves of one register, added with one 32-bit add.  P and F are stored together.
//   k_deep_shade_apply   grid over 16-byte blocks (8 samples) of a tile, inner loop over the tiles: a gain vector is loaded once and used N
//                        times; the tiles go four at a time, loads before stores (a tile is named once per call, so they do not alias)
#include "common.h"
#include <vector>

#define DEEP_SHADE_LDS_MAX_N 320       // tiles a wave stages in LDS: 320 x 256 B = 80 KiB, two waves per CU (as SHADE_LDS_MAX_N)

typedef unsigned short deep_us2 __attribute__((ext_vector_type(2)));
typedef const __attribute__((address_space(1))) uint32_t *deep_gword;      // a pointer read from the tile table is generic to the compiler: this says global
typedef uint32_t deep_u4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) deep_u4 *deep_gblock;            // likewise, 16 bytes of a tile
__device__ __forceinline__ deep_us2 deep_as_us2(uint32_t v) { return __builtin_bit_cast(deep_us2, v); }
__device__ __forceinline__ uint32_t deep_as_u32(deep_us2 v) { return __builtin_bit_cast(uint32_t, v); }

// ---- profile ---------------------------------------------------------------------------------------------------------------------------------
// (lo(v) < lo(c)) | (hi(v) < hi(c)) << 16: the saturating c - v is positive exactly where v < c, and min(., 1) makes that a count.  Two
// packed instructions for two samples; written as instructions because the compiler turns the same expression in C++ back into two
// 16-bit compares, two selects and a byte permute (five).  one2: 1 in both halves
__device__ __forceinline__ uint32_t deep_lt2(uint32_t v, uint32_t c, uint32_t one2)
{
    uint32_t d, r;
    asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(d) : "v"(c), "v"(v));
    asm("v_pk_min_u16 %0, %1, %2" : "=v"(r) : "v"(d), "v"(one2));
    return r;
}

// Rows i = 0 .. n - 1 in groups of 8: get(i) is a row's dword, use(i, v) what becomes of it.  The 8 reads of a group are issued together, and
// the next group's before this group is used (a loop of read, wait, use would expose the whole LDS or HBM latency once per row, and with a
// slab of n x 256 B a CU holds few waves to hide it behind)
template <typename Get, typename Use>
__device__ __forceinline__ void deep_rows8(int n, Get get, Use use)
{
    uint32_t a[8], b[8];
    auto load = [&](uint32_t *v, int i) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = get(i + j);
    };
    auto spend = [&](const uint32_t *v, int i) {
#pragma unroll
        for (int j = 0; j < 8; j++) use(i + j, v[j]);
    };
    int i = 0;
    if (n >= 8) {
        load(a, 0);
        for (; i + 24 <= n; i += 16) {                       // a holds rows i .. i + 7; no branch and no register copy inside: either would
            load(b, i + 8); spend(a, i);                     // turn the counted waits into waits for everything in flight
            load(a, i + 16); spend(b, i + 8);
        }
        spend(a, i); i += 8;
        if (i + 8 <= n) { load(b, i); spend(b, i); i += 8; }
    }
    for (; i < n; i++) use(i, get(i));
}

// The descent of one lane's dword over the n tiles; fetch(i): the lane's dword of tile i.  STAGED: through the wave's LDS slab [n][64]
template <bool STAGED, typename Fetch>
__device__ __forceinline__ uint32_t deep_shade_descend(uint32_t *slab, unsigned lane, int n, int k, Fetch fetch)
{
    if (STAGED) deep_rows8(n, fetch, [&](int i, uint32_t v) { slab[i * 64 + lane] = v; });
    // the largest c with #{x < c} <= k is the k-th smallest (0-based): bit by bit from the top, both samples of the dword at once
    const uint32_t one2 = 0x00010001u;
    uint32_t pre = 0;
    for (int bit = 15; bit >= 0; bit--) {
        const uint32_t c = pre | (one2 << bit);
        uint32_t cnt = 0;                                    // the two counts, at most n <= 4096 each: no carry between the halves
        deep_rows8(n, [&](int i) -> uint32_t { return STAGED ? slab[i * 64 + lane] : fetch(i); }, [&](int, uint32_t v) { cnt += deep_lt2(v, c, one2); });
        if ((cnt & 0xffffu) <= (uint32_t)k) pre |= 1u << bit;
        if ((cnt >> 16) <= (uint32_t)k) pre |= 0x10000u << bit;
    }
    return pre;
}

// prof, field: dense planes of `total` samples, 256-byte aligned like the tiles: dword 2 * lane-index is 4-byte aligned in all of them
template <bool STAGED>
__global__ __launch_bounds__(64) void k_deep_shade_select(const uint16_t *const *tiles, int n, int k, unsigned total, uint32_t ped2,
                                                          uint16_t *prof, uint16_t *field)
{
    extern __shared__ uint32_t slab[];                       // STAGED: [n][64]
    const unsigned lane = threadIdx.x, e0 = (blockIdx.x * 64u + lane) * 2u;
    if (e0 >= total) return;
    const bool word = e0 + 2 <= total;                       // not the last sample of a plane with an odd count
    uint32_t pre;
    if (blockIdx.x * 128u + 128u <= total)                   // every wave but the plane's last: plain dword loads, nothing in their way
        pre = deep_shade_descend<STAGED>(slab, lane, n, k, [&](int i) -> uint32_t { return *(deep_gword)(tiles[i] + e0); });
    else
        pre = deep_shade_descend<STAGED>(slab, lane, n, k, [&](int i) -> uint32_t {
            const uint16_t *t = tiles[i];
            return word ? *(deep_gword)(t + e0) : (uint32_t)t[e0];      // the guarded 2-byte path of the last odd sample
        });
    const uint32_t f = deep_as_u32(__builtin_elementwise_sub_sat(deep_as_us2(pre), deep_as_us2(ped2)));      // F = max(P - d, 0)
    if (word) { *(uint32_t *)(prof + e0) = pre; *(uint32_t *)(field + e0) = f; }
    else { prof[e0] = (uint16_t)pre; field[e0] = (uint16_t)f; }
}

// ---- apply -------------------------------------------------------------------------------------------------------------------------------------
// min(p, d) + (((max(p, d) - d) * g + 2048) >> 12) is the specification's two cases in one: at p <= d the product is 0 and the sum is p, above
// it the sum starts at d.  No branch and no select (written as the two cases, the compiler branched around every sample).
// uint32 is exact: (p - d) * g + 2048 <= 65535 * 65535 + 2048 = 4 294 838 273 < 2^32, and its >> 12 plus d stays below 2^21
__device__ __forceinline__ uint32_t deep_shade_px(uint32_t p, uint32_t g, uint32_t d)
{
    return min(65535u, min(p, d) + (((max(p, d) - d) * g + 2048u) >> 12));
}
__device__ __forceinline__ uint32_t deep_shade_word(uint32_t v, uint32_t g, uint32_t d)
{
    return deep_shade_px(v & 0xffffu, g & 0xffffu, d) | (deep_shade_px(v >> 16, g >> 16, d) << 16);
}
__device__ __forceinline__ deep_u4 deep_shade_block(deep_u4 v, deep_u4 g, uint32_t d)
{
    v.x = deep_shade_word(v.x, g.x, d); v.y = deep_shade_word(v.y, g.y, d);
    v.z = deep_shade_word(v.z, g.z, d); v.w = deep_shade_word(v.w, g.w, d);
    return v;
}

// (__restrict__: the table and the gain are not what the stores write, so the table's pointers stay in scalar registers)
__global__ __launch_bounds__(256) void k_deep_shade_apply(uint16_t *const *__restrict__ tiles, int n, const uint16_t *__restrict__ gain, unsigned total,
                                                          uint32_t d)
{
    const unsigned e0 = (blockIdx.x * 256u + threadIdx.x) * 8u;      // (total <= 2^30 and the grid covers it with less than 2048 to spare)
    if (e0 >= total) return;
    if (e0 + 8 <= total) {                                   // 16-byte aligned in the gain and in every tile
        const deep_u4 g = *(const deep_u4 *)(gain + e0);
        int i = 0;
        for (; i + 4 <= n; i += 4) {
            const deep_gblock p0 = (deep_gblock)(tiles[i] + e0), p1 = (deep_gblock)(tiles[i + 1] + e0), p2 = (deep_gblock)(tiles[i + 2] + e0), p3 = (deep_gblock)(tiles[i + 3] + e0);
            const deep_u4 v0 = *p0, v1 = *p1, v2 = *p2, v3 = *p3;
            *p0 = deep_shade_block(v0, g, d); *p1 = deep_shade_block(v1, g, d);
            *p2 = deep_shade_block(v2, g, d); *p3 = deep_shade_block(v3, g, d);
        }
        for (; i < n; i++) {
            const deep_gblock p = (deep_gblock)(tiles[i] + e0);
            *p = deep_shade_block(*p, g, d);
        }
        return;
    }
    for (unsigned e = e0; e < total; e++) {                  // the plane's last samples (fewer than 8)
        const uint32_t g = gain[e];
        for (int i = 0; i < n; i++) tiles[i][e] = (uint16_t)deep_shade_px(tiles[i][e], g, d);
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------------------
static int deep_shade_table(vfsms_ctx *ctx, const DeepSrc *tiles, int n, uint16_t ***d_tiles)
{
    std::vector<const uint16_t *> T(n);
    for (int i = 0; i < n; i++) T[i] = tiles[i].src;
    return ctx_upload_small(ctx, T.data(), sizeof(T[0]) * n, (void **)d_tiles);
}

// profile, smoothed field and gain of n deep tiles of h x w samples into the three planes of a field
int deep_shade_estimate_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int h, int w, int percentile, int radius, int pedestal,
                               uint16_t *gain, uint16_t *field, uint16_t *prof)
{
    TRY(shade_plane_fits("deep_shading_estimate", h, (size_t)w));
    const unsigned total = (unsigned)((size_t)h * w);
    uint16_t **d_tiles;
    TRY(deep_shade_table(ctx, tiles, n, &d_tiles));
    const int k = (int)((long long)(n - 1) * percentile / 100);
    const uint32_t ped2 = (uint32_t)pedestal * 0x00010001u;
    ProfScope ps(ctx, "deep_shading");
    const unsigned blocks = (total + 127) / 128;
    if (n <= DEEP_SHADE_LDS_MAX_N) {
        HIP_TRY(hipFuncSetAttribute((const void *)k_deep_shade_select<true>, hipFuncAttributeMaxDynamicSharedMemorySize, DEEP_SHADE_LDS_MAX_N * 256));   // (per device: not cached)
        hipLaunchKernelGGL(k_deep_shade_select<true>, dim3(blocks), dim3(64), (size_t)n * 256, ctx->stream, (const uint16_t *const *)d_tiles, n, k, total, ped2, prof, field);
    } else
        hipLaunchKernelGGL(k_deep_shade_select<false>, dim3(blocks), dim3(64), 0, ctx->stream, (const uint16_t *const *)d_tiles, n, k, total, ped2, prof, field);
    return shade_field_device(ctx, field, h, w, 1, radius, gain);
}

// the n deep tiles corrected in place by a field's gain
int deep_shade_apply_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int h, int w, int pedestal, const uint16_t *gain)
{
    const size_t total64 = (size_t)h * w;                    // at most 2^30: the sides of a deep tile end at 32768
    uint16_t **d_tiles;
    TRY(deep_shade_table(ctx, tiles, n, &d_tiles));
    ProfScope ps(ctx, "deep_shading");
    hipLaunchKernelGGL(k_deep_shade_apply, dim3((unsigned)((total64 + 2047) / 2048)), dim3(256), 0, ctx->stream, (uint16_t *const *)d_tiles, n, gain,
                       (unsigned)total64, (uint32_t)pedestal);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
