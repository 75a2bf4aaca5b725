// multiband_kernels.hip -- fuseMethod "multiBandBlending": a Laplacian-pyramid blend of the overlap for gfx950.
//
// The arithmetic is this project's specification (tests/multiband_ref.py restates it in numpy, bit for bit; it is not claimed to
// equal cv2.pyrDown / cv2.pyrUp or the reference's ImageFusion.fuseByMultiBandBlending):
//   seam   M0 = 1 where the fade gives A at least B's weight (SeamGeom, fuse_geom.h), else 0; one plane for every channel
//   fill   A' = A where A is valid else B;  B' = B where valid else A';  empty in both -> 0
//   pyrDown: 5-tap [1 4 6 4 1] rows at destination-column resolution, then columns, * 1/256; indices reflected (BORDER_REFLECT_101)
//   pyrUp:   even / odd taps [1 6 1] / [4 4] on rows, then columns, * 1/64; neighbour -1 reflects to 1, neighbour w replicates w - 1
//   blend    LCk = Mk (GAk - up GAk+1) + (1 - Mk) (GBk - up GBk+1),  top T = MN GAN + (1 - MN) GBN,  Ok = up Ok+1 + LCk
//   output   uint8(clamp(rint(O0), 0, 255))
// float32 everywhere, every expression in the order written (-ffp-contract=off).
//
// Launches per blend: one pyrDown per level (the first reads level 0 straight from the canvas + validity plane + tile, or from the
// int64 regions: level 0 is never stored), then one fused reconstruct per level (upsamples O, GA and GB of the level above on the fly
// and never stores a Laplacian; the coarsest one forms T on the fly).  The level-0 reconstruct writes the uint8 result into the
// canvas ROI, pastes the tile outside it and marks the tile rectangle valid.  The fp32 planes of levels 1..N live in a per-context
// scratch that grows to the largest blend seen (mb_scratch) and is freed with the context.
#include "common.h"
#include "fuse_geom.h"

#define MB_TH 8                        // destination tile of a pyrDown workgroup: 8 rows x 32 columns, one output per thread
#define MB_TW 32
#define MB_WH (2 * MB_TH + 3)          // its source window
#define MB_WW (2 * MB_TW + 3)

__device__ __forceinline__ int mb_reflect101(int i, int n)
{
    if (n == 1) return 0;
    while (i < 0 || i >= n) i = i < 0 ? -i : 2 * n - 2 - i;
    return i;
}

// ---- level-0 sources: (A', B', M0) of pixel (i, j) of the region ---------------------------------------------------------------
template <int CH>
struct Mb0Canvas {                     // A = canvas before the paste (pixels + validity), B = the tile
    const uint8_t *pix, *mask; int ccols, ry0, rx0;
    const uint8_t *tile; int tw, ty0, tx0;
    SeamGeom G;
    __device__ __forceinline__ void load(int i, int j, float *a, float *b, float &m) const
    {
        const size_t co = (size_t)(ry0 + i) * ccols + rx0 + j, to = (size_t)(ty0 + i) * tw + tx0 + j;
        const bool av = mask[co] != 0;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const float bv = (float)tile[to * CH + k];
            b[k] = bv;
            a[k] = av ? (float)pix[co * CH + k] : bv;
        }
        m = G.m0(i, j);
    }
};
template <int CH>
struct Mb0I64 {                        // the reference's representation: int64 [r][c][ch], -1 = empty
    const long long *A, *B; int c;
    SeamGeom G;
    __device__ __forceinline__ void load(int i, int j, float *a, float *b, float &m) const
    {
        const size_t e = ((size_t)i * c + j) * CH;
#pragma unroll
        for (int k = 0; k < CH; k++) {
            const long long av = A[e + k], bv = B[e + k];
            const long long a1 = av >= 0 ? av : bv, b1 = bv >= 0 ? bv : a1;
            a[k] = (float)(a1 > 0 ? a1 : 0);
            b[k] = (float)(b1 > 0 ? b1 : 0);
        }
        m = G.m0(i, j);
    }
};
template <int CH>
struct MbPlanes {                      // level k >= 1: GA, GB interleaved [h][w][CH], M [h][w]
    const float *ga, *gb, *m; int w;
    __device__ __forceinline__ void load(int i, int j, float *a, float *b, float &mm) const
    {
        const size_t e = (size_t)i * w + j;
#pragma unroll
        for (int k = 0; k < CH; k++) { a[k] = ga[e * CH + k]; b[k] = gb[e * CH + k]; }
        mm = m[e];
    }
};

// ---- pyrDown of GA, GB and M together: LDS-staged source window, row pass at destination-column resolution, column pass ----------
template <int CH, class Src>
__global__ __launch_bounds__(256) void k_mb_down(Src S, int n, int m, float *ga, float *gb, float *gm, int dn, int dm)
{
    constexpr int P = 2 * CH + 1;
    __shared__ float raw[P][MB_WH][MB_WW];
    __shared__ float rowp[P][MB_WH][MB_TW];
    const int t = threadIdx.x;
    const int dy0 = blockIdx.y * MB_TH, dx0 = blockIdx.x * MB_TW;
    const int sy0 = 2 * dy0 - 2, sx0 = 2 * dx0 - 2;
    for (int e = t; e < MB_WH * MB_WW; e += 256) {
        const int wy = e / MB_WW, wx = e - wy * MB_WW;
        float a[CH], b[CH], mm;
        S.load(mb_reflect101(sy0 + wy, n), mb_reflect101(sx0 + wx, m), a, b, mm);
#pragma unroll
        for (int k = 0; k < CH; k++) { raw[k][wy][wx] = a[k]; raw[CH + k][wy][wx] = b[k]; }
        raw[2 * CH][wy][wx] = mm;
    }
    __syncthreads();
    for (int e = t; e < MB_WH * MB_TW; e += 256) {
        const int wy = e / MB_TW, x = e - wy * MB_TW, c0 = 2 * x + 2;
#pragma unroll
        for (int p = 0; p < P; p++) {
            const float *L = raw[p][wy];
            rowp[p][wy][x] = ((L[c0] * 6.f + (L[c0 - 1] + L[c0 + 1]) * 4.f) + L[c0 - 2]) + L[c0 + 2];
        }
    }
    __syncthreads();
    const int tx = t % MB_TW, ty = t / MB_TW;
    const int y = dy0 + ty, x = dx0 + tx;
    if (y >= dn || x >= dm) return;
    const int r0 = 2 * ty + 2;
    float v[P];
#pragma unroll
    for (int p = 0; p < P; p++)
        v[p] = (((rowp[p][r0][tx] * 6.f + (rowp[p][r0 - 1][tx] + rowp[p][r0 + 1][tx]) * 4.f) + rowp[p][r0 - 2][tx]) + rowp[p][r0 + 2][tx]) * (1.f / 256.f);
    const size_t o = (size_t)y * dm + x;
#pragma unroll
    for (int k = 0; k < CH; k++) { ga[o * CH + k] = v[k]; gb[o * CH + k] = v[CH + k]; }
    gm[o] = v[2 * CH];
}

// ---- pyrUp taps ------------------------------------------------------------------------------------------------------------------------
template <int CH>
struct MbPlane {                       // one interleaved plane of the coarser level
    const float *p; int w;
    __device__ __forceinline__ float at(int i, int j, int k) const { return p[((size_t)i * w + j) * CH + k]; }
};
template <int CH>
struct MbCoarseO {                     // O of the coarser level: a stored plane, or (top) T = M GA + (1 - M) GB formed per tap
    const float *o, *ga, *gb, *m; int w, top;
    __device__ __forceinline__ float at(int i, int j, int k) const
    {
        const size_t e = (size_t)i * w + j;
        if (!top) return o[e * CH + k];
        const float mm = m[e];
        return (mm * ga[e * CH + k]) + ((1.f - mm) * gb[e * CH + k]);
    }
};
// up(S)(y, x) for an h1 x w1 source
template <class S>
__device__ __forceinline__ float mb_up(const S &s, int h1, int w1, int y, int x, int k)
{
    const int sy = y >> 1, sx = x >> 1;
    const int xm = sx > 0 ? sx - 1 : (w1 > 1 ? 1 : 0), xp = min(sx + 1, w1 - 1);
    const int ym = sy > 0 ? sy - 1 : (h1 > 1 ? 1 : 0), yp = min(sy + 1, h1 - 1);
    auto R = [&](int row) -> float {
        return (x & 1) ? (s.at(row, sx, k) + s.at(row, xp, k)) * 4.f : (s.at(row, xm, k) + s.at(row, sx, k) * 6.f) + s.at(row, xp, k);
    };
    if (y & 1) return ((R(sy) + R(yp)) * 4.f) * (1.f / 64.f);
    return ((R(ym) + R(sy) * 6.f) + R(yp)) * (1.f / 64.f);
}
// Ok(i, j) = up(Ok+1) + (Mk (GAk - up GAk+1) + (1 - Mk) (GBk - up GBk+1))
template <int CH, class Fine>
__device__ __forceinline__ void mb_px(const Fine &F, const MbPlane<CH> &GA1, const MbPlane<CH> &GB1, const MbCoarseO<CH> &O1, int h1, int w1,
                                      int i, int j, float *o)
{
    float a[CH], b[CH], m;
    F.load(i, j, a, b, m);
#pragma unroll
    for (int k = 0; k < CH; k++) {
        const float LA = a[k] - mb_up(GA1, h1, w1, i, j, k);
        const float LB = b[k] - mb_up(GB1, h1, w1, i, j, k);
        const float LC = (m * LA) + ((1.f - m) * LB);
        o[k] = mb_up(O1, h1, w1, i, j, k) + LC;
    }
}
__device__ __forceinline__ uint8_t mb_u8(float v)
{
    v = rintf(v);                      // round half to even
    v = v < 0.f ? 0.f : v;
    v = v > 255.f ? 255.f : v;
    return (uint8_t)v;
}

// reconstruct of a level k >= 1 into a float plane
template <int CH>
__global__ __launch_bounds__(256) void k_mb_up(MbPlanes<CH> F, MbPlane<CH> GA1, MbPlane<CH> GB1, MbCoarseO<CH> O1, int h1, int w1, int h, int w, float *out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= w || i >= h) return;
    float o[CH];
    mb_px<CH>(F, GA1, GB1, O1, h1, w1, i, j, o);
#pragma unroll
    for (int k = 0; k < CH; k++) out[((size_t)i * w + j) * CH + k] = o[k];
}
// level-0 reconstruct on the canvas: the grid covers the tile rectangle (th x tw at canvas (y0, x0)); ROI pixels get the blend, the rest
// the tile, and every pixel of the rectangle becomes valid
template <int CH>
__global__ __launch_bounds__(256) void k_mb_up_canvas(Mb0Canvas<CH> F, MbPlane<CH> GA1, MbPlane<CH> GB1, MbCoarseO<CH> O1, int h1, int w1,
                                                      uint8_t *pix, uint8_t *mask, int y0, int x0, int th, int tw, int r, int c)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= tw || y >= th) return;
    const size_t co = (size_t)(y0 + y) * F.ccols + x0 + x;
    const int i = y0 + y - F.ry0, j = x0 + x - F.rx0;
    if (i >= 0 && i < r && j >= 0 && j < c) {
        float o[CH];
        mb_px<CH>(F, GA1, GB1, O1, h1, w1, i, j, o);
#pragma unroll
        for (int k = 0; k < CH; k++) pix[co * CH + k] = mb_u8(o[k]);
    } else {
#pragma unroll
        for (int k = 0; k < CH; k++) pix[co * CH + k] = F.tile[((size_t)y * tw + x) * CH + k];
    }
    mask[co] = 1;
}
// level-0 reconstruct of the int64 operator into a dense u8 [r][c][CH]
template <int CH>
__global__ __launch_bounds__(256) void k_mb_up_i64(Mb0I64<CH> F, MbPlane<CH> GA1, MbPlane<CH> GB1, MbCoarseO<CH> O1, int h1, int w1, int r, int c, uint8_t *out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= c || i >= r) return;
    float o[CH];
    mb_px<CH>(F, GA1, GB1, O1, h1, w1, i, j, o);
#pragma unroll
    for (int k = 0; k < CH; k++) out[((size_t)i * c + j) * CH + k] = mb_u8(o[k]);
}

// ---- host: pyramid layout in the context's scratch, launch chain ----------------------------------------------------------------------
struct MbPyr { int N; int h[VFSMS_MB_MAX_LEVELS + 1], w[VFSMS_MB_MAX_LEVELS + 1]; float *ga[VFSMS_MB_MAX_LEVELS + 1], *gb[VFSMS_MB_MAX_LEVELS + 1], *m[VFSMS_MB_MAX_LEVELS + 1]; float *o[2]; };

// levels 1..N: GA, GB (ch floats per pixel) and M; two O planes of level-1 size (levels N-1..1 ping-pong through them)
static size_t mb_layout(int r, int c, int ch, int N, MbPyr *P, char *base)
{
    size_t off = 0;
    auto take = [&](size_t n) { float *p = base ? (float *)(base + off) : nullptr; off += (n * sizeof(float) + 255) & ~(size_t)255; return p; };
    P->N = N; P->h[0] = r; P->w[0] = c;
    for (int k = 1; k <= N; k++) {
        P->h[k] = (P->h[k - 1] + 1) / 2; P->w[k] = (P->w[k - 1] + 1) / 2;
        const size_t px = (size_t)P->h[k] * P->w[k];
        P->ga[k] = take(px * ch); P->gb[k] = take(px * ch); P->m[k] = take(px);
    }
    const size_t px1 = N > 1 ? (size_t)P->h[1] * P->w[1] * ch : 0;
    P->o[0] = take(px1); P->o[1] = take(px1);
    return off;
}

template <int CH>
static MbCoarseO<CH> mb_coarse_o(const MbPyr &P, int k)      // O of level k (k >= 1) as the reconstruct of level k - 1 reads it
{
    if (k == P.N) return MbCoarseO<CH>{nullptr, P.ga[k], P.gb[k], P.m[k], P.w[k], 1};
    return MbCoarseO<CH>{P.o[k & 1], nullptr, nullptr, nullptr, P.w[k], 0};
}

// pyrDown chain + reconstruct of levels N-1..1; the caller launches the level-0 reconstruct
template <int CH, class Src0>
static int mb_pyramid(vfsms_ctx *ctx, const MbPyr &P, const Src0 &S0)
{
    hipLaunchKernelGGL((k_mb_down<CH, Src0>), dim3((P.w[1] + MB_TW - 1) / MB_TW, (P.h[1] + MB_TH - 1) / MB_TH), dim3(256), 0, ctx->stream,
                       S0, P.h[0], P.w[0], P.ga[1], P.gb[1], P.m[1], P.h[1], P.w[1]);
    for (int k = 1; k < P.N; k++) {
        const MbPlanes<CH> Sk = {P.ga[k], P.gb[k], P.m[k], P.w[k]};
        hipLaunchKernelGGL((k_mb_down<CH, MbPlanes<CH>>), dim3((P.w[k + 1] + MB_TW - 1) / MB_TW, (P.h[k + 1] + MB_TH - 1) / MB_TH), dim3(256), 0,
                           ctx->stream, Sk, P.h[k], P.w[k], P.ga[k + 1], P.gb[k + 1], P.m[k + 1], P.h[k + 1], P.w[k + 1]);
    }
    for (int k = P.N - 1; k >= 1; k--) {
        const MbPlanes<CH> Fk = {P.ga[k], P.gb[k], P.m[k], P.w[k]};
        hipLaunchKernelGGL((k_mb_up<CH>), dim3((P.w[k] + 255) / 256, P.h[k]), dim3(256), 0, ctx->stream,
                           Fk, MbPlane<CH>{P.ga[k + 1], P.w[k + 1]}, MbPlane<CH>{P.gb[k + 1], P.w[k + 1]}, mb_coarse_o<CH>(P, k + 1),
                           P.h[k + 1], P.w[k + 1], P.h[k], P.w[k], P.o[k & 1]);
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

template <int CH>
static int mb_canvas_ch(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, const SeamGeom &G, const MbPyr &P)
{
    const Mb0Canvas<CH> S0 = {cv->pix.as<uint8_t>(), cv->mask.as<uint8_t>(), cv->cols, p.ry0, p.rx0, d_tile, p.w, p.ry0 - p.y0, p.rx0 - p.x0, G};
    TRY(mb_pyramid<CH>(ctx, P, S0));
    hipLaunchKernelGGL((k_mb_up_canvas<CH>), dim3((p.w + 255) / 256, p.h), dim3(256), 0, ctx->stream, S0, MbPlane<CH>{P.ga[1], P.w[1]},
                       MbPlane<CH>{P.gb[1], P.w[1]}, mb_coarse_o<CH>(P, 1), P.h[1], P.w[1], cv->pix.as<uint8_t>(), cv->mask.as<uint8_t>(), p.y0, p.x0, p.h, p.w, p.r(), p.c());
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// The placement's ROI blended with the tile, the tile pasted around it.  Enqueue only; the caller marks the rectangle in the canvas's list.
int mb_blend_canvas(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, const SeamGeom &G, int levels)
{
    ProfScope ps(ctx, "fuse_multiband");
    MbPyr P;
    TRY(ctx->mb_scratch.reserve(mb_layout(p.r(), p.c(), cv->ch, levels, &P, nullptr), ctx->stream));
    mb_layout(p.r(), p.c(), cv->ch, levels, &P, ctx->mb_scratch.as<char>());
    switch (cv->ch) {
    case 1: return mb_canvas_ch<1>(ctx, cv, d_tile, p, G, P);
    case 2: return mb_canvas_ch<2>(ctx, cv, d_tile, p, G, P);
    case 3: return mb_canvas_ch<3>(ctx, cv, d_tile, p, G, P);
    case 4: return mb_canvas_ch<4>(ctx, cv, d_tile, p, G, P);
    }
    vfsms_set_error("fuse_multiband: 1 to 4 channels");
    return VFSMS_ERR_BAD_ARG;
}

template <int CH>
static int mb_i64_ch(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, const SeamGeom &G, const MbPyr &P, uint8_t *d_out)
{
    const Mb0I64<CH> S0 = {dA, dB, c, G};
    TRY(mb_pyramid<CH>(ctx, P, S0));
    hipLaunchKernelGGL((k_mb_up_i64<CH>), dim3((c + 255) / 256, r), dim3(256), 0, ctx->stream, S0, MbPlane<CH>{P.ga[1], P.w[1]},
                       MbPlane<CH>{P.gb[1], P.w[1]}, mb_coarse_o<CH>(P, 1), P.h[1], P.w[1], r, c, d_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// int64 regions (device) -> u8 [r][c][ch] (device); enqueue only
int mb_blend_i64(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, int ch, const SeamGeom &G, int levels, uint8_t *d_out)
{
    ProfScope ps(ctx, "fuse_multiband");
    MbPyr P;
    TRY(ctx->mb_scratch.reserve(mb_layout(r, c, ch, levels, &P, nullptr), ctx->stream));
    mb_layout(r, c, ch, levels, &P, ctx->mb_scratch.as<char>());
    switch (ch) {
    case 1: return mb_i64_ch<1>(ctx, dA, dB, r, c, G, P, d_out);
    case 2: return mb_i64_ch<2>(ctx, dA, dB, r, c, G, P, d_out);
    case 3: return mb_i64_ch<3>(ctx, dA, dB, r, c, G, P, d_out);
    case 4: return mb_i64_ch<4>(ctx, dA, dB, r, c, G, P, d_out);
    }
    vfsms_set_error("fuse_multiband: 1 to 4 channels");
    return VFSMS_ERR_BAD_ARG;
}
