// lens_kernels.hip -- Method.lensCorrection for gfx950: the block displacement field between pairs of resident tiles, from which the host
// fits one radial model per dataset (imagestitch_amd/lens.py), and the resampling of the tiles under that model.
//
// Specification: tests/lens_ref.py (no reference counterpart).  Both kernels are integer arithmetic but for the score of a candidate, which
// is verify_math.h's -- so the device equals the specification bit for bit.
//
//   k_lens_blocks  grid (blocks of all jobs): a workgroup per BLOCK of the lattice, not per job
//   k_lens_remap   grid (64 x 4 pixel patches of one tile)
//
// k_lens_blocks.  A job is a pair of tiles of one shape and an offset: B's pixel (r, c) meets A's pixel (r + dx, c + dy).  The overlap
// rectangle (verify_overlap), shrunk by the radius R on all four sides, is cut into whole block x block squares from its top-left corner
// (lens_lattice: the host checks the caller's `first` against it).  A workgroup finds its job by bisection of `first`, then copies B's block
// (block^2 samples) and A's window ((block + 2R)^2 samples, all of them inside A because of the shrinking) into LDS -- as bytes, a colour
// tile as its luma (29 B + 150 G + 77 R + 128) >> 8 -- from any base address and row stride.  The (2R + 1)^2 candidates times S row slices
// are the items the lanes share: an item walks its rows a dword of B at a time, A's four partner bytes come from two consecutive LDS
// dwords through alignbyte by (R + j) & 3, which is constant per candidate, and sad_u8 / udot4 form Sa, Saa, Sab in 32 bits
// (128^2 * 255^2 < 2^32), added to the candidate's LDS sums by one LDS atomic each.  Sb and Sbb do not depend on the candidate.  N is
// block^2 for every candidate.  Then verify_score / verify_fixed per candidate -> surface, and the best under the tie rule of
// k_adjust_pick (largest double score, smallest i^2 + j^2, smallest i, smallest j) -> best4.
//
// k_lens_remap.  A lane per output pixel.  The source position in 1/256 px is a polynomial in the squared radius in Q30 (the one
// quotient per pixel from a double estimate corrected by its exact remainder); bilinear or Catmull-Rom taps with a replicated border,
// int64 accumulators; the taps of an interior pixel are read a row at a time.  The kernel never reads the buffer it writes:
// lens_apply_device copies a tile into the context's lens scratch first and resamples from there.
#include "common.h"
#include "tile_table.h"
#include "verify_math.h"
#include <algorithm>

#define LENS_THREADS 256

struct LensJob { const uint8_t *a, *b; int sa, sb, ch, dx, dy, r0, c0, nbx; };

// the lattice of a job on h x w tiles: the top-left corner (r0, c0) in B's coordinates and nby x nbx whole blocks (both 0 when none fits)
void lens_lattice(int h, int w, int dx, int dy, int block, int radius, int *r0, int *c0, int *nby, int *nbx)
{
    const long long ra = std::max(0ll, -(long long)dx) + radius, rb = std::min<long long>(h, (long long)h - dx) - radius;
    const long long ca = std::max(0ll, -(long long)dy) + radius, cb = std::min<long long>(w, (long long)w - dy) - radius;
    const long long by = rb > ra ? (rb - ra) / block : 0, bx = cb > ca ? (cb - ca) / block : 0;
    *r0 = (int)std::min<long long>(ra, h); *c0 = (int)std::min<long long>(ca, w);
    *nby = by > 0 && bx > 0 ? (int)by : 0; *nbx = by > 0 && bx > 0 ? (int)bx : 0;
}

__device__ __forceinline__ uint32_t lens_sample(const uint8_t *p, int ch)
{
    return ch == 1 ? (uint32_t)p[0] : (29u * p[0] + 150u * p[1] + 77u * p[2] + 128u) >> 8;
}

// the LDS of a workgroup, in bytes from a 16-byte aligned base: A's window (rows pa bytes apart, 16 spare bytes behind the last: the
// second dword of the last chunk), B's block, the candidates' three sums, Sb and Sbb, the arrays of the pick
__host__ __device__ __forceinline__ int lens_pitch(int block, int R) { return (block + 2 * R + 3) & ~3; }
__host__ __device__ __forceinline__ size_t lens_off_b(int block, int R) { return ((size_t)lens_pitch(block, R) * (block + 2 * R) + 16 + 15) & ~(size_t)15; }
__host__ __device__ __forceinline__ size_t lens_off_sums(int block, int R) { return lens_off_b(block, R) + (size_t)block * block; }
__host__ __device__ __forceinline__ size_t lens_off_pick(int block, int R)
{
    const int C = 2 * R + 1;
    return (lens_off_sums(block, R) + sizeof(uint32_t) * (3 * (size_t)C * C + 2) + 15) & ~(size_t)15;
}
static size_t lens_lds_bytes(int block, int R) { return lens_off_pick(block, R) + (sizeof(double) + 2 * sizeof(int)) * LENS_THREADS; }

__global__ __launch_bounds__(LENS_THREADS) void k_lens_blocks(const LensJob *jobs, const long long *first, int njobs, int block, int R,
                                                              int32_t *best4, int32_t *surface)
{
    extern __shared__ uint4 lens_lds[];
    uint8_t *const lds = reinterpret_cast<uint8_t *>(lens_lds);
    const long long blk = blockIdx.x;
    int lo = 0, hi = njobs;                                   // first[lo] <= blk < first[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= blk) lo = mid; else hi = mid;
    }
    const LensJob J = jobs[lo];
    const int local = (int)(blk - first[lo]), by = local / J.nbx, bx = local - by * J.nbx;
    const int C = 2 * R + 1, CC = C * C, W = block + 2 * R, pa = lens_pitch(block, R);
    const int yb = J.r0 + by * block, xb = J.c0 + bx * block;            // the block's corner in B
    const int ya = yb + J.dx - R, xa = xb + J.dy - R;                    // the window's corner in A: inside A, the lattice is shrunk by R
    uint8_t *const sA = lds, *const sB = lds + lens_off_b(block, R);
    uint32_t *const sS = reinterpret_cast<uint32_t *>(lds + lens_off_sums(block, R));   // [CC][3] = Sa, Saa, Sab; then Sb, Sbb
    const int tid = threadIdx.x;

    for (int k = tid; k < W * W; k += LENS_THREADS) {
        const int yy = k / W, xx = k - yy * W;
        sA[yy * pa + xx] = (uint8_t)lens_sample(J.a + (size_t)(ya + yy) * J.sa + (size_t)(xa + xx) * J.ch, J.ch);
    }
    for (int k = tid; k < pa * W + 16 - W * W; k += LENS_THREADS) {        // the row padding and the spare bytes: read, never used
        const int rowpad = pa - W, npad = rowpad * W;
        if (k < npad) sA[(k / rowpad) * pa + W + k % rowpad] = 0; else sA[pa * W + (k - npad)] = 0;
    }
    for (int k = tid; k < block * block; k += LENS_THREADS) {
        const int yy = k / block, xx = k - yy * block;
        sB[k] = (uint8_t)lens_sample(J.b + (size_t)(yb + yy) * J.sb + (size_t)(xb + xx) * J.ch, J.ch);
    }
    for (int k = tid; k < 3 * CC + 2; k += LENS_THREADS) sS[k] = 0u;
    __syncthreads();

    {   // Sb, Sbb
        uint32_t sb = 0u, sbb = 0u;
        const uint32_t *b4 = reinterpret_cast<const uint32_t *>(sB);
        for (int k = tid; k < block * block / 4; k += LENS_THREADS) {
            sb = __builtin_amdgcn_sad_u8(b4[k], 0u, sb);
            sbb = __builtin_amdgcn_udot4(b4[k], b4[k], sbb, false);
        }
        for (int d = 32; d > 0; d >>= 1) { sb += __shfl_down(sb, d, 64); sbb += __shfl_down(sbb, d, 64); }
        if ((tid & 63) == 0) { atomicAdd(&sS[3 * CC], sb); atomicAdd(&sS[3 * CC + 1], sbb); }
    }
    // the items (row slice, candidate): consecutive lanes take consecutive column shifts
    const int want = min(block, (2048 + CC - 1) / CC), rps = (block + want - 1) / want, S = (block + rps - 1) / rps;
    for (int item = tid; item < CC * S; item += LENS_THREADS) {
        const int s = item / CC, c = item - s * CC, ci = c / C, cj = c - ci * C;
        const unsigned m = (unsigned)cj & 3u;
        const int q = cj >> 2;
        uint32_t a1 = 0u, a2 = 0u, ab = 0u;
        for (int y = s * rps; y < min(block, (s + 1) * rps); y++) {
            const uint32_t *ar = reinterpret_cast<const uint32_t *>(sA + (y + ci) * pa) + q;
            const uint32_t *br = reinterpret_cast<const uint32_t *>(sB + y * block);
            uint32_t l = ar[0];
            for (int k = 0; k < block / 4; k++) {
                const uint32_t hgh = ar[k + 1];
                const uint32_t a = __builtin_amdgcn_alignbyte(hgh, l, m);
                l = hgh;
                a1 = __builtin_amdgcn_sad_u8(a, 0u, a1);
                a2 = __builtin_amdgcn_udot4(a, a, a2, false);
                ab = __builtin_amdgcn_udot4(a, br[k], ab, false);
            }
        }
        atomicAdd(&sS[3 * c], a1); atomicAdd(&sS[3 * c + 1], a2); atomicAdd(&sS[3 * c + 2], ab);
    }
    __syncthreads();

    // the score of every candidate in the specification's order of operations; the best one as k_adjust_pick picks it
    const long long N = (long long)block * block, Sb = sS[3 * CC], Sbb = sS[3 * CC + 1];
    double bs = -2.0; int bd2 = 0x7fffffff, bc = 0x7fffffff;
    for (int c = tid; c < CC; c += LENS_THREADS) {
        const int i = c / C - R, j = c % C - R;
        const double score = verify_score(N, (long long)sS[3 * c], Sb, (long long)sS[3 * c + 1], Sbb, (long long)sS[3 * c + 2], 0);
        if (surface) surface[(size_t)blk * CC + c] = verify_fixed(score);
        const int d2 = i * i + j * j;
        if (score > bs || (score == bs && (d2 < bd2 || (d2 == bd2 && c < bc)))) { bs = score; bd2 = d2; bc = c; }
    }
    double *const p_s = reinterpret_cast<double *>(lds + lens_off_pick(block, R));
    int *const p_d = reinterpret_cast<int *>(p_s + LENS_THREADS), *const p_c = p_d + LENS_THREADS;
    p_s[tid] = bs; p_d[tid] = bd2; p_c[tid] = bc;
    __syncthreads();
    for (int d = LENS_THREADS / 2; d > 0; d >>= 1) {
        if (tid < d) {
            const double os = p_s[tid + d]; const int od = p_d[tid + d], oc = p_c[tid + d];
            const double ms = p_s[tid]; const int md = p_d[tid], mc = p_c[tid];
            if (os > ms || (os == ms && (od < md || (od == md && oc < mc)))) { p_s[tid] = os; p_d[tid] = od; p_c[tid] = oc; }
        }
        __syncthreads();
    }
    if (tid == 0) {
        int32_t *out = best4 + 4 * (size_t)blk;
        out[0] = p_c[0] / C - R; out[1] = p_c[0] % C - R; out[2] = verify_fixed(p_s[0]); out[3] = (int32_t)N;
    }
}

// the displacement field of njobs jobs whose lattices hold `total` blocks in all (h_first[njobs]); d_first, d_best4, d_surface (or null): arena
int lens_blocks_device(vfsms_ctx *ctx, const LensBlockHost *jobs, const long long *h_first, int njobs, int block, int radius,
                       int32_t *d_best4, int32_t *d_surface)
{
    const long long total = h_first[njobs];
    if (total <= 0) return VFSMS_OK;
    if (total > 0x7fffffffll) { vfsms_set_error("block_ncc: %lld blocks in one call", total); return VFSMS_ERR_UNSUPPORTED; }
    std::vector<LensJob> H(njobs);
    for (int k = 0; k < njobs; k++) {
        const LensBlockHost &P = jobs[k];
        int r0, c0, nby, nbx;
        lens_lattice(P.h, P.w, P.dx, P.dy, block, radius, &r0, &c0, &nby, &nbx);
        H[k] = LensJob{P.a, P.b, P.sa, P.sb, P.ch, P.dx, P.dy, r0, c0, nbx};
    }
    LensJob *d_jobs; long long *d_first;
    TRY(ctx_upload_small(ctx, H.data(), sizeof(LensJob) * (size_t)njobs, (void **)&d_jobs));
    TRY(ctx_upload_small(ctx, h_first, sizeof(long long) * ((size_t)njobs + 1), (void **)&d_first));
    ProfScope ps(ctx, "lens_blocks");
    hipLaunchKernelGGL(k_lens_blocks, dim3((unsigned)total), dim3(LENS_THREADS), lens_lds_bytes(block, radius), ctx->stream,
                       d_jobs, d_first, njobs, block, radius, d_best4, d_surface);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// ---- resampling ------------------------------------------------------------------------------------------------------------------------------
struct LensMap { long long a1, a2, D2; double inv; int cy2, cx2, h, w, ch; };   // inv = 2^30 / D2, the quotient's first guess

// tests/lens_ref.py: source_position -- (sy, sx) in 1/256 px of output pixel (y, x); >> is arithmetic.  rho = floor(r2 2^30 / D2) exactly,
// without a 64-bit division: r2 < 2^33 is exact in a double, r2 * inv is within 1e-5 of the true quotient (< 2^33), so its floor is the
// quotient or one off, and the remainder -- exact in wrapping 64-bit arithmetic, r2 2^30 < 2^63 -- says which
__device__ __forceinline__ void lens_source(const LensMap &M, int y, int x, long long *sy, long long *sx)
{
    const long long Y = 2ll * y - M.cy2, X = 2ll * x - M.cx2;
    const unsigned long long r2 = (unsigned long long)(X * X + Y * Y);
    long long rho = (long long)((double)r2 * M.inv);
    long long rem = (long long)((r2 << 30) - (unsigned long long)rho * (unsigned long long)M.D2);
    while (rem < 0) { rho--; rem += M.D2; }
    while (rem >= M.D2) { rho++; rem -= M.D2; }
    const long long rho4 = (rho * rho) >> 30;
    const long long f = ((M.a1 * rho) >> 30) + ((M.a2 * rho4) >> 30);
    *sy = 256ll * y + ((Y * f + (1ll << 22)) >> 23);
    *sx = 256ll * x + ((X * f + (1ll << 22)) >> 23);
}
__device__ __forceinline__ int lens_clampi(long long v, int n) { return (int)(v < 0 ? 0 : (v > n - 1 ? n - 1 : v)); }
// the Catmull-Rom weights of phase f (0..255) in units of 2^-25: they sum to 2^25, each fits 32 bits (|w| < 1.27 2^25 in all)
__device__ __forceinline__ void lens_cubic(int f, int w[4])
{
    const int f2 = f * f, f3 = f2 * f;
    w[0] = -f3 + 512 * f2 - 65536 * f;
    w[1] = 3 * f3 - 1280 * f2 + (1 << 25);
    w[2] = -3 * f3 + 1024 * f2 + 65536 * f;
    w[3] = f3 - 256 * f2;
}
__device__ __forceinline__ uint8_t lens_bilinear(int fy, int fx, int p00, int p01, int p10, int p11)
{
    return (uint8_t)(((256 - fy) * ((256 - fx) * p00 + fx * p01) + fy * ((256 - fx) * p10 + fx * p11) + 32768) >> 16);
}
__device__ __forceinline__ uint8_t lens_round50(long long acc)
{
    const long long v = (acc + (1ll << 49)) >> 50;
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// src: dense h x w x ch (rows w * ch bytes); dst: rows `dstride` bytes apart; never the same memory.  TAPS 2: bilinear, 4: Catmull-Rom.
// CH 1 or 3: a pixel whose TAPS columns are all inside the row takes each row's TAPS * CH consecutive bytes in one unaligned read (one to
// three dwords instead of up to twelve byte loads); at the border, and for CH 0 (any channel count, read from M.ch), every tap is clamped
// and read by itself.  Both give the same bytes.
template <int CH, int TAPS>
__global__ __launch_bounds__(LENS_THREADS) void k_lens_remap(const uint8_t *src, uint8_t *dst, int dstride, LensMap M)
{
    const int x = (int)blockIdx.x * 64 + (int)(threadIdx.x & 63), y = (int)blockIdx.y * 4 + (int)(threadIdx.x >> 6);
    if (x >= M.w || y >= M.h) return;
    long long sy, sx;
    lens_source(M, y, x, &sy, &sx);
    const long long iy = sy >> 8, ix = sx >> 8;
    const int fy = (int)(sy & 255), fx = (int)(sx & 255);
    const int ch = CH ? CH : M.ch, lead = TAPS == 4 ? 1 : 0;             // the first tap is `lead` before the integer position
    const size_t pitch = (size_t)M.w * ch;
    uint8_t *out = dst + (size_t)y * dstride + (size_t)x * ch;
    int wy[4] = {256 - fy, fy, 0, 0}, wx[4] = {256 - fx, fx, 0, 0};
    if (TAPS == 4) { lens_cubic(fy, wy); lens_cubic(fx, wx); }
    int yy[TAPS];
#pragma unroll
    for (int t = 0; t < TAPS; t++) yy[t] = lens_clampi(iy - lead + t, M.h);
    if (CH && ix - lead >= 0 && ix - lead + TAPS <= M.w) {
        long long acc[CH ? CH : 1] = {};
#pragma unroll
        for (int t = 0; t < TAPS; t++) {
            uint8_t b[TAPS * (CH ? CH : 1)];
            __builtin_memcpy(b, src + yy[t] * pitch + (size_t)(ix - lead) * ch, sizeof(b));
#pragma unroll
            for (int c = 0; c < CH; c++) {
                long long r = 0;
#pragma unroll
                for (int u = 0; u < TAPS; u++) r += (long long)wx[u] * (int)b[u * CH + c];
                acc[c] += (long long)wy[t] * r;
            }
        }
#pragma unroll
        for (int c = 0; c < CH; c++) out[c] = TAPS == 4 ? lens_round50(acc[c]) : (uint8_t)((acc[c] + 32768) >> 16);
        return;
    }
    int xx[TAPS];
#pragma unroll
    for (int u = 0; u < TAPS; u++) xx[u] = lens_clampi(ix - lead + u, M.w);
    for (int c = 0; c < ch; c++) {
        long long acc = 0;
#pragma unroll
        for (int t = 0; t < TAPS; t++) {
            const uint8_t *row = src + yy[t] * pitch + c;
            long long r = 0;
#pragma unroll
            for (int u = 0; u < TAPS; u++) r += (long long)wx[u] * (int)row[(size_t)xx[u] * ch];
            acc += (long long)wy[t] * r;
        }
        out[c] = TAPS == 4 ? lens_round50(acc) : (uint8_t)((acc + 32768) >> 16);
    }
}

static LensMap lens_map(int h, int w, int ch, int a1_q30, int a2_q30, int cy2, int cx2)
{
    const long long D2 = std::max(1ll, (long long)(h - 1) * (h - 1) + (long long)(w - 1) * (w - 1));
    return LensMap{a1_q30, a2_q30, D2, 1073741824.0 / (double)D2, cy2 < 0 ? h - 1 : cy2, cx2 < 0 ? w - 1 : cx2, h, w, ch};
}
static void lens_remap_launch(vfsms_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, int dstride, const LensMap &M, int interp)
{
    const dim3 grid((unsigned)((M.w + 63) / 64), (unsigned)((M.h + 3) / 4)), wg(LENS_THREADS);
#define LENS_REMAP(CH) \
    do { if (interp) hipLaunchKernelGGL((k_lens_remap<CH, 4>), grid, wg, 0, ctx->stream, d_src, d_dst, dstride, M); \
         else hipLaunchKernelGGL((k_lens_remap<CH, 2>), grid, wg, 0, ctx->stream, d_src, d_dst, dstride, M); } while (0)
    if (M.ch == 1) LENS_REMAP(1); else if (M.ch == 3) LENS_REMAP(3); else LENS_REMAP(0);
#undef LENS_REMAP
}

// one dense h x w x ch image resampled from d_src into d_dst (rows dstride bytes apart), enqueued
int lens_remap_device(vfsms_ctx *ctx, const uint8_t *d_src, uint8_t *d_dst, int dstride, int h, int w, int ch, int a1_q30, int a2_q30,
                      int cy2, int cx2, int interp)
{
    ProfScope ps(ctx, "lens_apply");
    lens_remap_launch(ctx, d_src, d_dst, dstride, lens_map(h, w, ch, a1_q30, a2_q30, cy2, cx2), interp);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// the n tiles resampled in place, one after the other through the context's lens scratch (grown to the largest tile under device_buf.h's
// rule): the copy and the kernel that reads it are ordered by the stream, and so is the next tile's copy behind that kernel
int lens_apply_device(vfsms_ctx *ctx, const TileView *tiles, int n, int a1_q30, int a2_q30, int cy2, int cx2, int interp)
{
    size_t most = 0;
    for (int i = 0; i < n; i++) most = std::max(most, (size_t)tiles[i].h * tiles[i].w * tiles[i].ch);
    TRY(ctx->lens_scratch.reserve(most, ctx->stream));
    ProfScope ps(ctx, "lens_apply");
    for (int i = 0; i < n; i++) {
        const TileView &t = tiles[i];
        const size_t rowb = (size_t)t.w * t.ch;
        if ((size_t)t.stride == rowb) HIP_TRY(hipMemcpyAsync(ctx->lens_scratch.as<void>(), t.ptr, rowb * t.h, hipMemcpyDeviceToDevice, ctx->stream));
        else HIP_TRY(hipMemcpy2DAsync(ctx->lens_scratch.as<void>(), rowb, t.ptr, (size_t)t.stride, rowb, (size_t)t.h, hipMemcpyDeviceToDevice, ctx->stream));
        lens_remap_launch(ctx, ctx->lens_scratch.as<uint8_t>(), t.ptr, t.stride, lens_map(t.h, t.w, t.ch, a1_q30, a2_q30, cy2, cx2), interp);
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
