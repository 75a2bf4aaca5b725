// adjust_kernels.hip -- the offset search of Method.globalAdjust = "ncc" for gfx950: the statistic of verify_kernels.hip, evaluated for every
// offset of a (2R + 1) x (2R + 1) window around a predicted one, for a batch of pairs of resident tiles.
//
// Specification: tests/ncc_search_ref.py (the device equals it bit for bit).  Tile B's pixel (r, c) meets tile A's pixel (r + dx + i,
// c + dy + j) for the candidate (i, j), i, j in [-R, R]; over the rectangle of B pixels whose partner lies inside A -- it depends on
// (i, j) -- the five exact integer sums Sa, Sb, Saa, Sbb, Sab, then verify_score / verify_fixed of verify_math.h.  The sums are integers,
// so the reduction order is free.
//
//   (memset)          the sums of every (job, candidate) = 0
//   k_adjust_sums     grid (row-and-chunk blocks, row shifts i x tiles of ADJ_JT column shifts j, jobs)
//   k_adjust_pick     a workgroup per job: the score of every candidate -> surface, the best one under the tie rule -> best4
// No host synchronisation between them.
//
// k_adjust_sums.  A workgroup has ONE row shift i and ADJ_JT consecutive column shifts; a lane takes 16-byte chunks of B rows, cut at
// B's 16-byte address boundaries.  A chunk is loaded once (one aligned uint4) and used for all ADJ_JT column shifts: the 24 bytes of the
// partner row of A that they cover are loaded once as the aligned dwords around them and funnel-shifted (alignbyte) into place, first by
// the row's own byte alignment, then by the shift (a compile-time amount).  The 2R + 1 row shifts of a job read the same rows of A from
// different workgroups at about the same time: that reuse is the cache's.  Accumulation is sad_u8 / udot4 into 32-bit lane sums (a
// lane sees at most 2048 chunks: launch_adjust_search sizes the grid), 64-bit from the wave reduction on, one 64-bit atomic add per
// workgroup and sum -- the 45 sums of a workgroup are contiguous in memory.
//
// Heads and tails.  The overlap's columns depend on j, so a chunk is INTERIOR when all its 16 columns are shared under every shift of the
// tile, else an EDGE chunk: at most four per row (two at each end), processed in a second loop over (row, edge slot) items with the
// same data path plus a byte mask per (chunk, shift) that zeroes both operands outside the shared columns.  Nothing is restricted to a
// common core.  The masks, the guarded loader of A's bytes and the workgroup reduction are overlap_sums.h's.
#include "common.h"
#include "overlap_sums.h"
#include <algorithm>

#define ADJ_JT 9             // column shifts per workgroup: 9 x 5 lane sums
#define ADJ_THREADS 256
#define ADJ_EDGE 4           // edge slots per row (the last one takes every edge chunk from the fourth on: there is none)
#define ADJ_LANE_ITEMS 32    // chunks a lane should get, at least, before the grid grows
#define ADJ_LANE_CAP 1024    // chunks a lane may get per loop, at most: 2 x 1024 x 4 x 4 x 255^2 < 2^32
#define ADJ_MAX_GX 64

// the chunks of B row r for a workgroup whose shared columns are [cl, ch) (under any shift of its tile) and [kl, kh) (under all of them):
// chunk k covers the columns [c0 + 16 k, c0 + 16 k + 16), k in [0, nk); [ki0, ki1) are interior
struct AdjRow { const uint8_t *pb; int c0, nk, ki0, ki1; };
__device__ __forceinline__ AdjRow adj_row(const AdjJob &J, int r, int cl, int ch, int kl, int kh)
{
    AdjRow g;
    g.pb = J.b + (size_t)r * J.sb;
    g.c0 = cl - (int)((uintptr_t)(g.pb + cl) & 15u);
    g.nk = (ch - g.c0 + 15) >> 4;
    g.ki0 = min(g.nk, kl > g.c0 ? (kl - g.c0 + 15) >> 4 : 0);
    g.ki1 = min(g.nk, max(g.ki0, kh > g.c0 ? (kh - g.c0) >> 4 : 0));
    return g;
}

// dword t of the chunk's partner bytes under column shift JJ of the tile; e: the 24 bytes of A that the tile's shifts cover (load_partner<6>)
template <int JJ>
__device__ __forceinline__ uint32_t adj_shifted(const uint32_t e[6], int t)
{
    constexpr int q = JJ >> 2, mm = JJ & 3;
    if constexpr (mm == 0) return e[q + t];
    else return __builtin_amdgcn_alignbyte(e[q + t + 1], e[q + t], (unsigned)mm);
}

template <int JJ>
__device__ __forceinline__ void adj_interior(const uint32_t e[6], const uint4 &bv, Sums5 acc[ADJ_JT])
{
    const uint32_t b[4] = {bv.x, bv.y, bv.z, bv.w};
    Sums5 &s = acc[JJ];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t a = adj_shifted<JJ>(e, t);
        s.a = __builtin_amdgcn_sad_u8(a, 0u, s.a);
        s.aa = __builtin_amdgcn_udot4(a, a, s.aa, false);
        s.ab = __builtin_amdgcn_udot4(a, b[t], s.ab, false);
    }
    if constexpr (JJ + 1 < ADJ_JT) adj_interior<JJ + 1>(e, bv, acc);
}

template <int JJ>
__device__ __forceinline__ void adj_edge(const uint32_t e[6], const uint32_t b[4], uint32_t mB, uint32_t mA, Sums5 acc[ADJ_JT])
{
    const uint32_t m16 = mB & (mA >> JJ);
    Sums5 &s = acc[JJ];
#pragma unroll
    for (int t = 0; t < 4; t++) {
        const uint32_t bm = byte_mask((m16 >> (4 * t)) & 15u);
        acc4(adj_shifted<JJ>(e, t) & bm, b[t] & bm, s);
    }
    if constexpr (JJ + 1 < ADJ_JT) adj_edge<JJ + 1>(e, b, mB, mA, acc);
}

// sums: [job][row shift][njt * ADJ_JT column-shift slots][5] uint64 = Sa, Sb, Saa, Sbb, Sab (slots beyond 2R + 1 stay 0)
__global__ __launch_bounds__(ADJ_THREADS) void k_adjust_sums(const AdjJob *jobs, unsigned long long *sums, int R, int njt)
{
    const AdjJob J = jobs[blockIdx.z];
    const int C = 2 * R + 1;
    const int ci = (int)blockIdx.y / njt, jt = (int)blockIdx.y - ci * njt;
    const int di = J.dx + ci - R;                         // the workgroup's row shift
    const int j0 = jt * ADJ_JT - R;
    const int jte = min(ADJ_JT, R - j0 + 1);              // column shifts of this tile that exist
    const int dj0 = J.dy + j0, dj1 = dj0 + jte - 1;       // its first and last column shift
    const int h = J.h, w = J.w;
    const int r0 = max(0, -di), r1 = min(h, h - di);
    const int cl = max(0, -dj1), ch = min(w, w - dj0);    // B columns shared under some shift of the tile
    const int kl = max(0, -dj0), kh = min(w, w - dj1);    //                  ... under every one
    if (r1 <= r0 || ch <= cl) return;
    const int nrows = r1 - r0;
    const int stride = (int)gridDim.x * ADJ_THREADS, first = (int)blockIdx.x * ADJ_THREADS + (int)threadIdx.x;

    Sums5 acc[ADJ_JT];
#pragma unroll
    for (int q = 0; q < ADJ_JT; q++) acc[q] = {0u, 0u, 0u, 0u, 0u};
    uint32_t sbI = 0u, sbbI = 0u;                         // Sb, Sbb of the interior chunks: the same for every shift of the tile

    // interior chunks: items (row, k - ki0) of a nrows x cpr rectangle (cpr >= the chunks of any row)
    {
        const int cpr = ((ch - cl + 15) >> 4) + 1;
        const int srow = stride / cpr, scol = stride - srow * cpr;
        int rr = first / cpr, kk = first - rr * cpr;
        while (rr < nrows) {
            const int r = r0 + rr;
            const AdjRow g = adj_row(J, r, cl, ch, kl, kh);
            const int k = g.ki0 + kk;
            if (k < g.ki1) {
                const int c = g.c0 + (k << 4);
                const uint4 bv = *reinterpret_cast<const uint4 *>(g.pb + c);
                uint32_t e[6];
                load_partner<6>((uintptr_t)(J.a + (size_t)(r + di) * J.sa) + (uintptr_t)(intptr_t)(c + dj0), c + dj0, min(w, c + dj0 + jte + 15), e);
                sbI = __builtin_amdgcn_sad_u8(bv.x, 0u, sbI); sbI = __builtin_amdgcn_sad_u8(bv.y, 0u, sbI);
                sbI = __builtin_amdgcn_sad_u8(bv.z, 0u, sbI); sbI = __builtin_amdgcn_sad_u8(bv.w, 0u, sbI);
                sbbI = __builtin_amdgcn_udot4(bv.x, bv.x, sbbI, false); sbbI = __builtin_amdgcn_udot4(bv.y, bv.y, sbbI, false);
                sbbI = __builtin_amdgcn_udot4(bv.z, bv.z, sbbI, false); sbbI = __builtin_amdgcn_udot4(bv.w, bv.w, sbbI, false);
                adj_interior<0>(e, bv, acc);
            }
            rr += srow; kk += scol;
            if (kk >= cpr) { kk -= cpr; rr++; }
        }
    }
    // edge chunks: items (row, edge slot); edge chunk number n of a row is chunk n when n < ki0, else chunk ki1 + n - ki0
    for (int item = first; item < nrows * ADJ_EDGE; item += stride) {
        const int r = r0 + item / ADJ_EDGE, slot = item % ADJ_EDGE;
        const AdjRow g = adj_row(J, r, cl, ch, kl, kh);
        const int nedge = g.ki0 + g.nk - g.ki1;
        for (int n = slot; n < nedge; n += (slot == ADJ_EDGE - 1 ? 1 : nedge)) {
            const int k = n < g.ki0 ? n : g.ki1 + n - g.ki0;
            const int c = g.c0 + (k << 4);
            const uint32_t *b4 = reinterpret_cast<const uint32_t *>((uintptr_t)g.pb + (uintptr_t)(intptr_t)c);
            uint32_t b[4];
#pragma unroll
            for (int t = 0; t < 4; t++) b[t] = (c + 4 * t + 3 >= 0 && c + 4 * t < w) ? b4[t] : 0u;
            uint32_t e[6];
            load_partner<6>((uintptr_t)(J.a + (size_t)(r + di) * J.sa) + (uintptr_t)(intptr_t)(c + dj0), c + dj0, w, e);
            adj_edge<0>(e, b, range_bits(c, 0, w, 16), range_bits(c + dj0, 0, w, 24), acc);
        }
    }

    unsigned long long v[ADJ_JT * 5];
#pragma unroll
    for (int jj = 0; jj < ADJ_JT; jj++) {
        v[jj * 5] = acc[jj].a; v[jj * 5 + 1] = (unsigned long long)acc[jj].b + sbI; v[jj * 5 + 2] = acc[jj].aa;
        v[jj * 5 + 3] = (unsigned long long)acc[jj].bb + sbbI; v[jj * 5 + 4] = acc[jj].ab;
    }
    wg_add_u64<ADJ_JT * 5, ADJ_THREADS / 64>(v, sums + ((size_t)(blockIdx.z * C + ci) * (size_t)(njt * ADJ_JT) + (size_t)(jt * ADJ_JT)) * 5, jte * 5);
}

// A workgroup per job: score every candidate in the specification's order of operations, keep the best double score; ties go to the
// smallest i^2 + j^2, then the smallest i, then the smallest j (candidates are numbered i-major, so: the smallest number).
__global__ __launch_bounds__(ADJ_THREADS) void k_adjust_pick(const AdjJob *jobs, const unsigned long long *sums, int R, int njt, int min_pixels,
                                                             int32_t *best4, int32_t *surface)
{
    const AdjJob J = jobs[blockIdx.x];
    const int C = 2 * R + 1, CC = C * C;
    double bs = -2.0; int bd2 = 0x7fffffff, bc = 0x7fffffff;
    for (int cidx = threadIdx.x; cidx < CC; cidx += ADJ_THREADS) {
        const int ci = cidx / C, cj = cidx - ci * C, i = ci - R, j = cj - R;
        long long N;
        const double score = overlap_score(J.h, J.w, J.dx + i, J.dy + j, sums + ((size_t)(blockIdx.x * C + ci) * (size_t)(njt * ADJ_JT) + cj) * 5, min_pixels, &N);
        if (surface) surface[(size_t)blockIdx.x * CC + cidx] = verify_fixed(score);
        const int d2 = i * i + j * j;
        if (score > bs || (score == bs && (d2 < bd2 || (d2 == bd2 && cidx < bc)))) { bs = score; bd2 = d2; bc = cidx; }
    }
    __shared__ double s_s[ADJ_THREADS]; __shared__ int s_d[ADJ_THREADS], s_c[ADJ_THREADS];
    s_s[threadIdx.x] = bs; s_d[threadIdx.x] = bd2; s_c[threadIdx.x] = bc;
    __syncthreads();
    for (int d = ADJ_THREADS / 2; d > 0; d >>= 1) {
        if ((int)threadIdx.x < d) {
            const double os = s_s[threadIdx.x + d]; const int od = s_d[threadIdx.x + d], oc = s_c[threadIdx.x + d];
            const double ms = s_s[threadIdx.x]; const int md = s_d[threadIdx.x], mc = s_c[threadIdx.x];
            if (os > ms || (os == ms && (od < md || (od == md && oc < mc)))) { s_s[threadIdx.x] = os; s_d[threadIdx.x] = od; s_c[threadIdx.x] = oc; }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const int cidx = s_c[0], ci = cidx / C, cj = cidx - ci * C;
        long long N;                                          // the winner's shared pixels; its score is s_s[0]
        (void)overlap_score(J.h, J.w, J.dx + ci - R, J.dy + cj - R, sums + ((size_t)(blockIdx.x * C + ci) * (size_t)(njt * ADJ_JT) + cj) * 5, min_pixels, &N);
        int32_t *out = best4 + 4 * (size_t)blockIdx.x;
        out[0] = ci - R; out[1] = cj - R; out[2] = verify_fixed(s_s[0]); out[3] = (int32_t)N;
    }
}

size_t adjust_sums_bytes(int njobs, int radius)
{
    const int C = 2 * radius + 1, njt = (C + ADJ_JT - 1) / ADJ_JT;
    return sizeof(unsigned long long) * 5 * (size_t)njobs * C * njt * ADJ_JT;
}

// the search for njobs (<= 65535) jobs: h_jobs is the host's copy of d_jobs (it sizes the grid); d_sums holds adjust_sums_bytes(njobs, radius)
int launch_adjust_search(vfsms_ctx *ctx, const AdjJob *d_jobs, const AdjJob *h_jobs, int njobs, int radius, int min_pixels,
                         unsigned long long *d_sums, int32_t *d_best4, int32_t *d_surface)
{
    if (njobs <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "adjust");
    const int C = 2 * radius + 1, njt = (C + ADJ_JT - 1) / ADJ_JT;
    long long items = 1;                                  // the chunks (interior or edge slots) a workgroup's lanes share, at most
    for (int k = 0; k < njobs; k++) {
        const AdjJob &J = h_jobs[k];
        const long long rows = std::max(0, std::min(J.h, J.h - std::abs(J.dx) + radius));
        const long long cols = std::max(0, std::min(J.w, J.w - std::abs(J.dy) + radius + ADJ_JT));
        items = std::max(items, rows * std::max<long long>(ADJ_EDGE, ((cols + 15) >> 4) + 1));
    }
    long long gx = std::min<long long>(ADJ_MAX_GX, (items + ADJ_THREADS * ADJ_LANE_ITEMS - 1) / (ADJ_THREADS * ADJ_LANE_ITEMS));
    gx = std::max(gx, (items + (long long)ADJ_THREADS * ADJ_LANE_CAP - 1) / ((long long)ADJ_THREADS * ADJ_LANE_CAP));
    if (gx > 65535) { vfsms_set_error("ncc_search: a tile is too large"); return VFSMS_ERR_BAD_ARG; }
    HIP_TRY(hipMemsetAsync(d_sums, 0, adjust_sums_bytes(njobs, radius), ctx->stream));
    hipLaunchKernelGGL(k_adjust_sums, dim3((unsigned)gx, C * njt, njobs), dim3(ADJ_THREADS), 0, ctx->stream, d_jobs, d_sums, radius, njt);
    hipLaunchKernelGGL(k_adjust_pick, dim3(njobs), dim3(ADJ_THREADS), 0, ctx->stream, d_jobs, d_sums, radius, njt, min_pixels, d_best4, d_surface);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
