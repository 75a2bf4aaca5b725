// deep_kernels.hip -- 16-bit gray tiles resident on the device (vfsms_deep_*), for gfx950.
//
// The arithmetic is this project's specification (tests/deep_ref.py restates it in numpy; everything is integer, so every stage must equal
// it exactly; there is no reference counterpart):
//   window  lo, hi = the samples of rank (N - 1) * ppm / 10^6 among ALL samples of ALL tiles, sorted
//   reduce  out = ((clamp(v, lo, hi) - lo) * 255 + D / 2) / D, D = hi - lo: the 8-bit registration view
//   mosaic  per canvas pixel, over the tiles that cover it: the sample of the largest tile index (mode 0), or (sum w p + (sum w) / 2) / sum w
//           with w = min(r + 1, h - r, c + 1, w - c), cut at `feather` when that is positive (mode 1); 0 where nothing covers
//
// A deep tile is dense on the device (vfsms_deep_upload packs the caller's rows): h * w samples from a 256-byte aligned base, so window and
// reduce see one run of samples per tile and never a row.  Their grid is cut into chunks of DEEP_CHUNK samples; a workgroup finds its tile by
// bisection in the chunk offsets of the span table (wave-uniform: scalar loads).
//   k_deep_hist<1>   the exact radix select, pass 1: the HIGH byte of every sample, counted in LDS (256 bins x 32 copies, copy = lane % 32: the
//                    lanes of a half wave never share an address, which matters because real data sits in a few bins), flushed to 64-bit
//                    counts in global memory (one atomic per non-empty bin and workgroup).  The host locates the high byte of both ranks.
//   k_deep_hist<2>   pass 2: the LOW byte of the samples whose high byte is one of those two (2 tables x 256 bins x 16 copies).
//                    Both passes stream the tiles once with 16-byte loads, and count the 8 samples of a load as runs of equal counters.
//   k_deep_reduce    2 B in, 1 B out per sample, 16 samples a lane and step: two 16-byte loads, one 16-byte store.  The division is by the
//                    call's D with a numerator below 2^24: a float reciprocal (of the host) and one integer fix-up, see deep_div.
//   k_deep_mosaic<T> the gather, one launch per band.  One workgroup per DEEP_BIN_H x DEEP_BIN_W block of the band walks the tiles its bin lists
//                    (deep_bins.h).  A block whose bin holds one tile, and every block in mode 0, copies (no weights, no division); up to 4 tiles
//                    it sums in 32 bits (4 x 16384 x 65535 + 32768 < 2^32: exact), beyond that in 64.  Only pixels with two or more covers
//                    divide.  T is the sample type: uint16_t here.
#include "common.h"
#include "deep_bins.h"
#include <algorithm>
#include <type_traits>

#define DEEP_CHUNK 16384u              // samples per workgroup of window and reduce (32 KB in)

// one tile as window and reduce read it: `count` samples at src, the tile's first chunk among the call's; dst: the reduced tile (reduce only)
struct DeepSpan { const uint16_t *src; uint8_t *dst; unsigned long long count; unsigned chunk0, pad; };

__device__ __forceinline__ DeepSpan deep_span_of(const DeepSpan *spans, int n, unsigned chunk)
{
    int lo = 0, hi = n - 1;                                  // the last span with chunk0 <= chunk
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (spans[mid].chunk0 <= chunk) lo = mid; else hi = mid - 1;
    }
    return spans[lo];
}

// ---- window ---------------------------------------------------------------------------------------------------------------------------------
// the LDS counter of sample v for this lane, or DEEP_NONE: pass 1 counts every sample by its high byte, pass 2 the low byte of the
// samples whose high byte is sel0 (table 0) or sel1 (table 1)
#define DEEP_NONE 0xffffffffu
template <int PASS>
__device__ __forceinline__ unsigned deep_slot(unsigned v, unsigned lane, int sel0, int sel1)
{
    if (PASS == 1) return (v >> 8) * 32u + (lane & 31u);
    const int hb = (int)(v >> 8);
    if (hb == sel0) return (v & 255u) * 16u + (lane & 15u);
    if (hb == sel1) return 4096u + (v & 255u) * 16u + (lane & 15u);
    return DEEP_NONE;
}
// Neighbouring pixels mostly share a counter (a high byte spans 256 levels): the 8 samples of a load are counted as RUNS of equal
// counters, one LDS atomic per run instead of one per sample
struct DeepRun {
    unsigned slot = DEEP_NONE, n = 0;
    __device__ __forceinline__ void flush(uint32_t *H) { if (slot != DEEP_NONE) atomicAdd(&H[slot], n); }
    __device__ __forceinline__ void add(uint32_t *H, unsigned s) { if (s == slot) n++; else { flush(H); slot = s; n = 1; } }
};

// counts: PASS 1 [256], PASS 2 [2][256] (table 1 stays empty when sel1 == sel0: the host reads table 0 for both ranks)
template <int PASS>
__global__ __launch_bounds__(256) void k_deep_hist(const DeepSpan *spans, int n, int sel0, int sel1, unsigned long long *counts)
{
    __shared__ uint32_t H[8192];
    for (unsigned i = threadIdx.x; i < 8192u; i += 256u) H[i] = 0;
    __syncthreads();
    const DeepSpan s = deep_span_of(spans, n, blockIdx.x);
    const unsigned long long base = (unsigned long long)(blockIdx.x - s.chunk0) * DEEP_CHUNK;
    const unsigned long long end = min(base + DEEP_CHUNK, s.count);
    const unsigned lane = threadIdx.x;
    for (unsigned long long i = base + threadIdx.x * 8u; i < end; i += 2048u) {
        if (i + 8 <= end) {                                  // (base and i are multiples of 8 samples: 16-byte aligned)
            const uint4 v = *(const uint4 *)(s.src + i);
            const unsigned w[4] = {v.x, v.y, v.z, v.w};
            DeepRun run;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                run.add(H, deep_slot<PASS>(w[k] & 0xffffu, lane, sel0, sel1));
                run.add(H, deep_slot<PASS>(w[k] >> 16, lane, sel0, sel1));
            }
            run.flush(H);
        } else {
            DeepRun run;
            for (unsigned long long j = i; j < end; j++) run.add(H, deep_slot<PASS>(s.src[j], lane, sel0, sel1));
            run.flush(H);
        }
    }
    __syncthreads();
    if (PASS == 1) {
        uint32_t c = 0;
        for (unsigned k = 0; k < 32u; k++) c += H[threadIdx.x * 32u + ((k + threadIdx.x) & 31u)];      // (rotated: the lanes start on different banks)
        if (c) atomicAdd(&counts[threadIdx.x], (unsigned long long)c);
    } else {
        for (unsigned t = 0; t < 2u; t++) {
            uint32_t c = 0;
            for (unsigned k = 0; k < 16u; k++) c += H[t * 4096u + threadIdx.x * 16u + ((k + threadIdx.x) & 15u)];
            if (c) atomicAdd(&counts[t * 256u + threadIdx.x], (unsigned long long)c);
        }
    }
}

// ---- reduce ---------------------------------------------------------------------------------------------------------------------------------
// num / D for num < 2^24 and 1 <= D <= 65535 with num / D <= 255 (num = c * 255 + D / 2, c <= D).  rcp = 1.0f / D rounded once, num is exact
// in a float, the product is rounded once: the estimate is off from num / D by at most 255.5 * 2^-23, so its truncation is the quotient or one
// beside it, and one remainder test settles which
__device__ __forceinline__ uint32_t deep_div(uint32_t num, uint32_t D, float rcp)
{
    uint32_t q = (uint32_t)((float)num * rcp);
    const int r = (int)num - (int)(q * D);
    if (r < 0) q--;
    else if (r >= (int)D) q++;
    return q;
}
__device__ __forceinline__ uint32_t deep_red(uint32_t v, uint32_t lo, uint32_t hi, uint32_t D, float rcp)
{
    return deep_div((min(max(v, lo), hi) - lo) * 255u + (D >> 1), D, rcp);
}
__device__ __forceinline__ uint32_t deep_red4(uint32_t a, uint32_t b, uint32_t lo, uint32_t hi, uint32_t D, float rcp)
{
    return deep_red(a & 0xffffu, lo, hi, D, rcp) | (deep_red(a >> 16, lo, hi, D, rcp) << 8) |
           (deep_red(b & 0xffffu, lo, hi, D, rcp) << 16) | (deep_red(b >> 16, lo, hi, D, rcp) << 24);
}

__global__ __launch_bounds__(256) void k_deep_reduce(const DeepSpan *spans, int n, uint32_t lo, uint32_t hi, float rcp)
{
    const DeepSpan s = deep_span_of(spans, n, blockIdx.x);
    const unsigned long long base = (unsigned long long)(blockIdx.x - s.chunk0) * DEEP_CHUNK;
    const unsigned long long end = min(base + DEEP_CHUNK, s.count);
    const uint32_t D = hi - lo;
    for (unsigned long long i = base + threadIdx.x * 16u; i < end; i += 4096u) {
        if (i + 16 <= end) {                                 // (multiples of 16 samples: the loads are 32-byte, the store 16-byte aligned)
            const uint4 a = *(const uint4 *)(s.src + i), b = *(const uint4 *)(s.src + i + 8);
            uint4 o;
            o.x = deep_red4(a.x, a.y, lo, hi, D, rcp); o.y = deep_red4(a.z, a.w, lo, hi, D, rcp);
            o.z = deep_red4(b.x, b.y, lo, hi, D, rcp); o.w = deep_red4(b.z, b.w, lo, hi, D, rcp);
            *(uint4 *)(s.dst + i) = o;
        } else
            for (unsigned long long j = i; j < end; j++) s.dst[j] = (uint8_t)deep_red(s.src[j], lo, hi, D, rcp);      // a tile's last samples
    }
}

// ---- mosaic ---------------------------------------------------------------------------------------------------------------------------------
template <typename T> struct DeepTileT { const T *ptr; int y0, x0, h, w; };                  // dense: row r starts at ptr + r * w
template <typename T> struct __attribute__((packed, aligned(sizeof(T)))) DeepGroup { T v[8]; };   // 8 samples at any sample-aligned address

// ACC 0: the last covering tile's sample; 1: weighted sums in 32 bits (at most 4 tiles in the bin); 2: in 64 bits
template <typename T, int ACC>
__device__ __forceinline__ void deep_gather(const DeepTileT<T> *tiles, const uint32_t *list, uint32_t s, uint32_t e, int x, int ry, int cols,
                                            int row0, int nrows, int feather, T *out)
{
    typedef typename std::conditional<ACC == 2, unsigned long long, uint32_t>::type acc_t;
    for (int k = 0; k < DEEP_BIN_H / 8; k++) {               // rows ry, ry + 8, ... of the block (ry: one of its first 8)
        const int r = ry + 8 * k, y = row0 + r;
        if (r >= nrows) break;
        T val[8];
        uint32_t cnt[8], sw[8]; acc_t sp[8];
        for (int j = 0; j < 8; j++) { val[j] = 0; cnt[j] = 0; sw[j] = 0; sp[j] = 0; }
        for (uint32_t i = s; i < e; i++) {
            const DeepTileT<T> t = tiles[list[i]];
            const int tr = y - t.y0, c0 = x - t.x0;
            if ((unsigned)tr >= (unsigned)t.h || c0 + 8 <= 0 || c0 >= t.w) continue;
            const T *rowp = t.ptr + (size_t)tr * t.w;
            const bool full = c0 >= 0 && c0 + 8 <= t.w;
            T p[8];
            if (full) { const DeepGroup<T> g = *(const DeepGroup<T> *)(rowp + c0); for (int j = 0; j < 8; j++) p[j] = g.v[j]; }
            else for (int j = 0; j < 8; j++) p[j] = (unsigned)(c0 + j) < (unsigned)t.w ? rowp[c0 + j] : (T)0;
            const int dy = min(tr + 1, t.h - tr);
            for (int j = 0; j < 8; j++) {
                const int c = c0 + j;
                if (!full && (unsigned)c >= (unsigned)t.w) continue;
                val[j] = p[j];
                if (ACC) {
                    const int d = min(dy, min(c + 1, t.w - c));
                    const uint32_t wg = (uint32_t)(feather > 0 ? min(d, feather) : d);
                    sw[j] += wg; sp[j] += (acc_t)wg * p[j]; cnt[j]++;
                }
            }
        }
        if (ACC)
            for (int j = 0; j < 8; j++)
                if (cnt[j] >= 2) val[j] = (T)((sp[j] + (sw[j] >> 1)) / sw[j]);
        T *dst = out + (size_t)r * cols + x;
        if (x + 8 <= cols) { DeepGroup<T> g; for (int j = 0; j < 8; j++) g.v[j] = val[j]; *(DeepGroup<T> *)dst = g; }
        else for (int j = 0; x + j < cols; j++) dst[j] = val[j];
    }
}

// out: the band, dense [nrows][cols]; grid: one workgroup per block of the bin table, row-major
template <typename T>
__global__ __launch_bounds__(256) void k_deep_mosaic(const DeepTileT<T> *tiles, const uint32_t *start, const uint32_t *list, int nbx, int cols,
                                                     int row0, int nrows, int mode, int feather, T *out)
{
    const unsigned b = blockIdx.x;
    const int bx = (int)(b % (unsigned)nbx), by = (int)(b / (unsigned)nbx);
    const uint32_t s = start[b], e = start[b + 1];
    const int x = bx * DEEP_BIN_W + (int)(threadIdx.x & 31u) * 8, ry = by * DEEP_BIN_H + (int)(threadIdx.x >> 5);
    if (x >= cols) return;
    if (mode == 0 || e - s <= 1u) deep_gather<T, 0>(tiles, list, s, e, x, ry, cols, row0, nrows, feather, out);
    else if (e - s <= 4u) deep_gather<T, 1>(tiles, list, s, e, x, ry, cols, row0, nrows, feather, out);
    else deep_gather<T, 2>(tiles, list, s, e, x, ry, cols, row0, nrows, feather, out);
}

// ---- launchers ------------------------------------------------------------------------------------------------------------------------------
// the span table of n tiles -> the device, and the call's chunk count
static int deep_spans(vfsms_ctx *ctx, const DeepSrc *tiles, int n, DeepSpan **d_spans, unsigned *chunks)
{
    std::vector<DeepSpan> S(n);
    unsigned long long c = 0;
    for (int i = 0; i < n; i++) {
        const unsigned long long count = (unsigned long long)tiles[i].h * tiles[i].w;
        S[i] = DeepSpan{tiles[i].src, tiles[i].dst, count, (unsigned)c, 0};
        c += (count + DEEP_CHUNK - 1) / DEEP_CHUNK;           // (4096 tiles of 2^30 samples: 2^28 chunks)
    }
    *chunks = (unsigned)c;
    return ctx_upload_small(ctx, S.data(), sizeof(DeepSpan) * n, (void **)d_spans);
}
size_t deep_table_bytes(int n) { return sizeof(DeepSpan) * (size_t)n + 512 * sizeof(unsigned long long) + 4096; }

// the value of rank k (0-based) in a histogram: its bin, and the rank that is left inside the bin
static int deep_rank_bin(const unsigned long long *H, unsigned long long k, unsigned long long *inside)
{
    unsigned long long before = 0;
    for (int b = 0; b < 256; b++) {
        if (k < before + H[b]) { *inside = k - before; return b; }
        before += H[b];
    }
    return -1;
}

// the samples of ranks k_lo <= k_hi among all samples of the tiles (tests/deep_ref.py: window, before hi == lo is opened).  Synchronises.
int deep_window_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, unsigned long long k_lo, unsigned long long k_hi, int *lo, int *hi)
{
    DeepSpan *d_spans; unsigned chunks;
    TRY(deep_spans(ctx, tiles, n, &d_spans, &chunks));
    unsigned long long *d_counts = (unsigned long long *)ctx_arena_alloc(ctx, 512 * sizeof(unsigned long long));
    if (!d_counts) { vfsms_set_error("arena exhausted (deep_window)"); return VFSMS_ERR_CAPACITY; }
    unsigned long long H[512];
    ProfScope ps(ctx, "deep_window");
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(H), ctx->stream));
    hipLaunchKernelGGL(k_deep_hist<1>, dim3(chunks), dim3(256), 0, ctx->stream, d_spans, n, -1, -1, d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(H, d_counts, 256 * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long in_lo = 0, in_hi = 0;
    const int hb_lo = deep_rank_bin(H, k_lo, &in_lo), hb_hi = deep_rank_bin(H, k_hi, &in_hi);
    if (hb_lo < 0 || hb_hi < 0) { vfsms_set_error("deep_window: the high-byte counts do not reach the ranks"); return VFSMS_ERR_HIP; }
    HIP_TRY(hipMemsetAsync(d_counts, 0, sizeof(H), ctx->stream));
    hipLaunchKernelGGL(k_deep_hist<2>, dim3(chunks), dim3(256), 0, ctx->stream, d_spans, n, hb_lo, hb_hi == hb_lo ? -1 : hb_hi, d_counts);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(H, d_counts, sizeof(H), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    unsigned long long unused;
    const int lb_lo = deep_rank_bin(H, in_lo, &unused), lb_hi = deep_rank_bin(hb_hi == hb_lo ? H : H + 256, in_hi, &unused);
    if (lb_lo < 0 || lb_hi < 0) { vfsms_set_error("deep_window: the low-byte counts do not reach the ranks"); return VFSMS_ERR_HIP; }
    *lo = hb_lo << 8 | lb_lo; *hi = hb_hi << 8 | lb_hi;
    return VFSMS_OK;
}

// every tile's 8-bit view into its dst (dense, 256-byte aligned bases)
int deep_reduce_device(vfsms_ctx *ctx, const DeepSrc *tiles, int n, int lo, int hi)
{
    DeepSpan *d_spans; unsigned chunks;
    TRY(deep_spans(ctx, tiles, n, &d_spans, &chunks));
    ProfScope ps(ctx, "deep_reduce");
    hipLaunchKernelGGL(k_deep_reduce, dim3(chunks), dim3(256), 0, ctx->stream, d_spans, n, (uint32_t)lo, (uint32_t)hi, 1.0f / (float)(hi - lo));
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

size_t deep_mosaic_table_bytes(int n, const DeepBins &B)
{
    return sizeof(DeepTileT<uint16_t>) * (size_t)n + sizeof(uint32_t) * (B.start.size() + B.list.size()) + 4096;
}
// the band of B (rows [row0, row0 + nrows) of a canvas `cols` wide) gathered from the tiles at `at` into d_out, dense
int deep_mosaic_device(vfsms_ctx *ctx, const DeepSrc *tiles, const DeepRect *at, int n, const DeepBins &B, int cols, int row0, int nrows, int mode,
                       int feather, uint16_t *d_out)
{
    std::vector<DeepTileT<uint16_t>> T(n);
    for (int i = 0; i < n; i++) T[i] = DeepTileT<uint16_t>{tiles[i].src, at[i].y0, at[i].x0, at[i].h, at[i].w};
    DeepTileT<uint16_t> *d_tiles; uint32_t *d_start, *d_list;
    TRY(ctx_upload_small(ctx, T.data(), sizeof(T[0]) * n, (void **)&d_tiles));
    TRY(ctx_upload_small(ctx, B.start.data(), sizeof(uint32_t) * B.start.size(), (void **)&d_start));
    const uint32_t none = 0;                                 // (a band no tile touches: an empty list, never read)
    TRY(ctx_upload_small(ctx, B.list.empty() ? &none : B.list.data(), sizeof(uint32_t) * std::max<size_t>(B.list.size(), 1), (void **)&d_list));
    ProfScope ps(ctx, "deep_mosaic");
    hipLaunchKernelGGL(k_deep_mosaic<uint16_t>, dim3((unsigned)(B.start.size() - 1)), dim3(256), 0, ctx->stream, d_tiles, d_start, d_list, B.nbx, cols,
                       row0, nrows, mode, feather, d_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
