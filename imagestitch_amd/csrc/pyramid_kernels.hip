// pyramid_kernels.hip -- the reduced levels of a pyramidal mosaic (Stitcher.outputPyramid), one pass over a band of the canvas, for gfx950.
//
// The arithmetic is this project's specification (tests/pyramid_ref.py restates it in numpy; everything is integer, so every level must
// equal it exactly; there is no reference counterpart):
//   R_k = (R_{k-1} + 1) >> 1, C_k = (C_{k-1} + 1) >> 1
//   level k (i, j) = (a + b + c + d + 2) >> 2 per channel over rows min(2i, R_{k-1} - 1), min(2i + 1, R_{k-1} - 1) and columns
//   min(2j, C_{k-1} - 1), min(2j + 1, C_{k-1} - 1) of level k - 1 -- a cascade, every level rounded once from the rounded level below,
//   an edge replicated at each level against that level's FULL-CANVAS size (not the band's, not the region's)
//
// k_pyramid<CH, RW, RH>: a workgroup of 256 threads stages a region of RH rows x RW pixels (RW * CH <= 256 bytes a row) of the source in
// LDS, reduces it level by level inside LDS as deep as asked (at most log2(RH) levels) and writes every level it formed.
//   load    aligned dword loads: the region's row starts at any byte (the canvas pitch is cols * ch), so a thread loads the two aligned
//           dwords around its four bytes and shifts them together (the second load is a neighbour's first: it hits the same lines).  Rows
//           and bytes outside the source are not loaded and never read: a valid sample (i, j) of level k only ever reads samples
//           (2i | 2i + 1, 2j | 2j + 1) of level k - 1 that are valid or clamped back to valid ones
//   reduce  while a region row of the level holds >= 4 pixels a thread forms 4 pixels (CH dwords) from CH 8-byte LDS reads of each of the
//           two rows; with ch = 3 the horizontal partner of a byte is 3 bytes away, so the bytes are picked out of the registers by
//           compile-time positions.  The narrow deep levels (a few bytes per region) are done byte by byte
//   store   a level's row lands at any byte of the level buffer (pitch C_k * ch): whole aligned dwords where all four bytes belong to
//           the region's row, single bytes at its two ends (the neighbouring regions write the other bytes of those dwords)
// The band's bytes are read from HBM once.  Levels deeper than the region allows (7 .. 10) come from a second launch of the same kernel
// with a 16 x 16 region over the deepest level of the first.
// LDS: region 16 KiB + its levels 5.4 KiB = 21.5 KiB per workgroup -> 7 workgroups (28 waves) per CU.
#include "common.h"

#define PYR_MAX_STEP 6                  // levels one launch forms: log2 of the region height of the first launch

struct PyrArgs {
    const uint8_t *src; size_t src_bytes;       // the source level: rows [src_row0, ...) of it, densely packed; bytes that may be read
    int src_row0;                               // (absolute row of the source level stored first at `src`)
    int R0, C0;                                 // full size of the source level
    int row_begin, row_end;                     // the band in rows of the source level; row_begin % 2^nl == 0
    int nl;                                     // levels to form (1 .. log2 RH)
    uint8_t *dst[PYR_MAX_STEP];                 // level k + 1 of the source: the rows from row_begin >> (k + 1) on, densely packed
};

// four bytes at byte offset g of `p` (any alignment) out of aligned dword loads; nothing at or beyond `bytes` is touched
__device__ __forceinline__ uint32_t pyr_load4(const uint8_t *p, size_t g, size_t bytes)
{
    const unsigned sh = (unsigned)((uintptr_t)(p + g) & 3);
    const long long A = (long long)g - sh, n = (long long)bytes;                 // (A < 0: `p` itself is not dword-aligned and g < sh)
    uint32_t lo = 0, hi = 0;
    if (A >= 0 && A + 4 <= n) lo = *(const uint32_t *)(p + A);
    else for (int b = 0; b < 4; b++) if (A + b >= 0 && A + b < n) lo |= (uint32_t)p[A + b] << (8 * b);
    if (sh) {
        if (A + 8 <= n) hi = *(const uint32_t *)(p + A + 4);
        else for (int b = 0; b < 4; b++) if (A + 4 + b < n) hi |= (uint32_t)p[A + 4 + b] << (8 * b);
    }
    return __builtin_amdgcn_alignbyte(hi, lo, sh);
}

template <int CH, int RW, int RH>
struct PyrLds {
    static constexpr int off(int k) { return k == 0 ? 0 : off(k - 1) + (((RH >> (k - 1)) * (RW >> (k - 1)) * CH + 15) & ~15); }
    static constexpr int levels = RH == 64 ? 6 : RH == 16 ? 4 : -1;
    static constexpr int bytes = off(levels) + 16;
};

template <int CH, int RW, int RH>
__global__ __launch_bounds__(256) void k_pyramid(PyrArgs a)
{
    using L = PyrLds<CH, RW, RH>;
    __shared__ __attribute__((aligned(16))) uint8_t lds[L::bytes];
    const int tid = threadIdx.x;
    const int ry0 = a.row_begin + (int)blockIdx.y * RH, rx0 = (int)blockIdx.x * RW;      // the region in the source level
    // ---- the region: RH rows of RW * CH bytes, row r at lds[r * RW * CH]
    {
        constexpr int DPR = RW * CH / 4;
        const int rlim = min(a.R0, a.row_end);
        const size_t pitch = (size_t)a.C0 * CH;
        for (int idx = tid; idx < RH * DPR; idx += 256) {
            const int row = idx / DPR, d = idx % DPR;
            const int r = ry0 + row;
            const size_t xb = (size_t)rx0 * CH + 4 * d;
            if (r >= rlim || xb >= pitch) continue;
            *(uint32_t *)(lds + row * (RW * CH) + 4 * d) = pyr_load4(a.src, (size_t)(r - a.src_row0) * pitch + xb, a.src_bytes);
        }
    }
    __syncthreads();
    // ---- level k from level k - 1, inside LDS
    int Rp = a.R0, Cp = a.C0;                                                            // full size of level k - 1
    int lp = 0;                                                                          // LDS offset of level k - 1
#pragma unroll
    for (int k = 1; k <= L::levels; k++) {
        if (k > a.nl) break;
        const int hk = RH >> k, wk = RW >> k;                                            // the region at level k
        const int lk = L::off(k <= L::levels ? k : 0);
        const int I0 = ry0 >> k, J0 = rx0 >> k;
        const int sp = (wk * 2) * CH, sk = wk * CH;                                      // LDS row strides of levels k - 1 and k
        if (wk >= 4) {
            const int upr = wk / 4;
            for (int u = tid; u < hk * upr; u += 256) {
                const int i = u / upr, t = u % upr;
                const int ra = 2 * i, rb = (2 * (I0 + i) + 1 < Rp) ? ra + 1 : ra;
                uint32_t w0[2 * CH], w1[2 * CH], o[CH];
                const uint2 *p0 = (const uint2 *)(lds + lp + ra * sp + 8 * CH * t), *p1 = (const uint2 *)(lds + lp + rb * sp + 8 * CH * t);
#pragma unroll
                for (int q = 0; q < CH; q++) { const uint2 v0 = p0[q], v1 = p1[q]; w0[2 * q] = v0.x; w0[2 * q + 1] = v0.y; w1[2 * q] = v1.x; w1[2 * q + 1] = v1.y; }
#pragma unroll
                for (int q = 0; q < CH; q++) o[q] = 0;
#pragma unroll
                for (int p = 0; p < 4; p++) {
                    const bool pair = 2 * (J0 + 4 * t + p) + 1 < Cp;                     // the right-hand column exists at level k - 1
#pragma unroll
                    for (int c = 0; c < CH; c++) {
                        const int b0 = 2 * p * CH + c, b1 = b0 + CH, ob = p * CH + c;
                        const uint32_t x00 = (w0[b0 >> 2] >> (8 * (b0 & 3))) & 0xff, x10 = (w1[b0 >> 2] >> (8 * (b0 & 3))) & 0xff;
                        const uint32_t x01 = pair ? (w0[b1 >> 2] >> (8 * (b1 & 3))) & 0xff : x00;
                        const uint32_t x11 = pair ? (w1[b1 >> 2] >> (8 * (b1 & 3))) & 0xff : x10;
                        o[ob >> 2] |= ((x00 + x01 + x10 + x11 + 2) >> 2) << (8 * (ob & 3));
                    }
                }
                uint32_t *po = (uint32_t *)(lds + lk + i * sk + 4 * CH * t);
#pragma unroll
                for (int q = 0; q < CH; q++) po[q] = o[q];
            }
        } else {
            for (int e = tid; e < hk * sk; e += 256) {
                const int i = e / sk, j = (e % sk) / CH, c = e % CH;
                const int ra = 2 * i, rb = (2 * (I0 + i) + 1 < Rp) ? ra + 1 : ra;
                const int ca = 2 * j, cb = (2 * (J0 + j) + 1 < Cp) ? ca + 1 : ca;
                const uint8_t *q0 = lds + lp + ra * sp + c, *q1 = lds + lp + rb * sp + c;
                lds[lk + e] = (uint8_t)(((uint32_t)q0[ca * CH] + q0[cb * CH] + q1[ca * CH] + q1[cb * CH] + 2) >> 2);
            }
        }
        __syncthreads();
        Rp = (Rp + 1) >> 1; Cp = (Cp + 1) >> 1; lp = lk;
        // ---- the level's rows of this region to the level buffer (Rp, Cp: now the full size of level k)
        const int Iend = min(Rp, (a.row_end + (1 << k) - 1) >> k);                       // the band's rows of level k end here
        const int nb = min(wk, Cp - J0) * CH;                                            // bytes of a region row that exist
        if (nb > 0) {
            const size_t pk = (size_t)Cp * CH;
            uint8_t *dst = a.dst[k - 1];
            const int first = a.row_begin >> k;
            const int slots = sk / 4 + 2;
            for (int e = tid; e < hk * slots; e += 256) {
                const int i = e / slots, s = e % slots;
                if (I0 + i >= Iend) continue;
                uint8_t *row = dst + (size_t)(I0 + i - first) * pk + (size_t)J0 * CH;
                const int q0 = 4 * s - (int)((uintptr_t)row & 3);                        // the slot: bytes [q0, q0 + 4) of the row, dword-aligned in memory
                if (q0 >= nb) continue;
                const uint8_t *l = lds + lk + i * sk;
                if (q0 >= 0 && q0 + 4 <= nb)
                    *(uint32_t *)(row + q0) = (uint32_t)l[q0] | (uint32_t)l[q0 + 1] << 8 | (uint32_t)l[q0 + 2] << 16 | (uint32_t)l[q0 + 3] << 24;
                else
                    for (int q = max(q0, 0); q < min(q0 + 4, nb); q++) row[q] = l[q];
            }
        }
    }
}

template <int CH, int RW, int RH>
static void pyr_launch(vfsms_ctx *ctx, const PyrArgs &a)
{
    const dim3 grid((unsigned)((a.C0 + RW - 1) / RW), (unsigned)((a.row_end - a.row_begin + RH - 1) / RH));
    hipLaunchKernelGGL((k_pyramid<CH, RW, RH>), grid, dim3(256), 0, ctx->stream, a);
}
template <int RH>
static void pyr_launch_ch(vfsms_ctx *ctx, int ch, const PyrArgs &a)
{
    // the first launch's region is 64 rows of 256 bytes (192 with three channels); the second's 16 x 16 pixels
    if (RH == 64) {
        if (ch == 1) pyr_launch<1, 256, 64>(ctx, a); else if (ch == 2) pyr_launch<2, 128, 64>(ctx, a);
        else if (ch == 3) pyr_launch<3, 64, 64>(ctx, a); else pyr_launch<4, 64, 64>(ctx, a);
    } else {
        if (ch == 1) pyr_launch<1, 16, 16>(ctx, a); else if (ch == 2) pyr_launch<2, 16, 16>(ctx, a);
        else if (ch == 3) pyr_launch<3, 16, 16>(ctx, a); else pyr_launch<4, 16, 16>(ctx, a);
    }
}

static inline int pyr_size(int n, int k) { for (; k > 0; k--) n = (n + 1) >> 1; return n; }

// bytes of levels 1 .. levels of the band [row0, row0 + nrows) of a rows x cols x ch canvas, back to back (tests/pyramid_ref.py: band_of_level)
size_t pyramid_band_bytes(int rows, int cols, int ch, int row0, int nrows, int levels)
{
    size_t total = 0;
    for (int k = 1; k <= levels; k++) {
        const int first = row0 >> k, end = (int)(((long long)row0 + nrows + (1 << k) - 1) >> k);
        total += (size_t)(end - first) * pyr_size(cols, k) * ch;
    }
    return total;
}

// levels 1 .. levels of that band into d_levels (pyramid_band_bytes of it), laid out as they leave the library.  api.hip has checked the
// band: row0 % 2^levels == 0, and nrows % 2^levels == 0 unless the band ends at the last row
int pyramid_band_device(vfsms_ctx *ctx, const CanvasRec *cv, int row0, int nrows, int levels, uint8_t *d_levels)
{
    uint8_t *lvl[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
    for (int k = 1; k <= levels; k++) lvl[k] = d_levels + pyramid_band_bytes(cv->rows, cv->cols, cv->ch, row0, nrows, k - 1);
    return pyramid_band_device_at(ctx, cv, row0, nrows, levels, lvl, "pyramid");
}

// the same band with every level at a place of its own: level k's rows, densely packed, from lvl[k] on (k = 1 .. levels)
int pyramid_band_device_at(vfsms_ctx *ctx, const CanvasRec *cv, int row0, int nrows, int levels, uint8_t *const *lvl, const char *stage)
{
    size_t lvl_bytes[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
    for (int k = 1; k <= levels; k++)
        lvl_bytes[k] = pyramid_band_bytes(cv->rows, cv->cols, cv->ch, row0, nrows, k) - pyramid_band_bytes(cv->rows, cv->cols, cv->ch, row0, nrows, k - 1);
    ProfScope ps(ctx, stage);
    PyrArgs a;
    a.src = cv->pix.as<uint8_t>(); a.src_bytes = (size_t)cv->rows * cv->cols * cv->ch; a.src_row0 = 0;
    a.R0 = cv->rows; a.C0 = cv->cols; a.row_begin = row0; a.row_end = row0 + nrows;
    a.nl = levels < PYR_MAX_STEP ? levels : PYR_MAX_STEP;
    for (int k = 0; k < PYR_MAX_STEP; k++) a.dst[k] = k < a.nl ? lvl[k + 1] : nullptr;
    pyr_launch_ch<64>(ctx, cv->ch, a);
    if (levels > PYR_MAX_STEP) {
        const int s = PYR_MAX_STEP;
        a.src = lvl[s]; a.src_bytes = lvl_bytes[s]; a.src_row0 = row0 >> s;
        a.R0 = pyr_size(cv->rows, s); a.C0 = pyr_size(cv->cols, s);
        a.row_begin = row0 >> s; a.row_end = (int)(((long long)row0 + nrows + (1 << s) - 1) >> s);
        a.nl = levels - s;
        for (int k = 0; k < PYR_MAX_STEP; k++) a.dst[k] = k < a.nl ? lvl[s + k + 1] : nullptr;
        pyr_launch_ch<16>(ctx, cv->ch, a);
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
