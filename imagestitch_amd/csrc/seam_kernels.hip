// seam_kernels.hip -- fuseMethod "optimalSeamLine": the overlap cut along a minimum-cost connected seam, for gfx950.
//
// The arithmetic is this project's specification (tests/seam_ref.py restates it in numpy; everything is integer, so pixels AND seam
// must equal it exactly; no parity with the reference's interactive ImageFusion.fuseByOptimalSeamLine is claimed):
//   fill     A' = A where valid else B;  B' = B where valid else A';  empty in both -> 0
//   energy   E = sum_k |d_k| + sum_k (|d_k(i, j+1) - d_k(i, j-1)| + |d_k(i+1, j) - d_k(i-1, j)|), d = A' - B', neighbours clamped to the
//            region, E = 0 where A or B is empty (<= 5100 for ch <= 4: uint16)
//   geometry the fade's: a strip (kind 1: one column per row, kind 2: one row per column) or, in corner mode, a horizontal seam inside the
//            row arm and a vertical seam inside the column arm (the index ranges the corner ramps of fuse_geom.h are written on)
//   seam     C(t, p) = E(t, p) + min(C(t-1, p-1), C(t-1, p), C(t-1, p+1)), lowest index first; end = lowest-index minimum of the last step
//   label    A iff A-valid and on A's side of either seam; out = A' there, B' elsewhere ("none"), or the label plane becomes M0 of the
//            Laplacian-pyramid blend of multiband_kernels.hip ("multiBandBlending")
//
// Stages, all on the context's stream, no host round trip between them:
//   k_seam_energy  fully parallel; writes the energy in the DP's own layout: one padded row of 64 K uint16 per seam step, so a lane's K
//                  positions are one aligned vector load (the horizontal seam's plane is the transpose)
//   k_seam_dp      ONE wave64 per seam (two workgroups of one launch in corner mode).  Lane l keeps positions [l K, l K + K) of the running
//                  cost row in registers (K = 4 .. 64, picked on the device from the seam's real width); per step it exchanges its two edge costs with its neighbours by cross-lane shuffle, and the
//                  energy rows are fetched SEAM_PF steps ahead.  No LDS, no barrier in the loop.  One predecessor byte per cell.
//   k_seam_dp_wide any width above 64 * 64 positions: one workgroup per seam, cost rows ping-pong in global scratch, a barrier per step
//   k_seam_trace   one workgroup per seam: the predecessor bytes the walk can reach in the next SEAM_TR steps (a cone of 2 SEAM_TR + 1
//                  columns) are staged in LDS by all threads, one lane walks them there, the chunk of s[] is written out by all threads
//   k_seam_apply_* parallel: label + select (or k_seam_label_* + the pyramid kernels)
#include "common.h"
#include "fuse_geom.h"
#include <stdlib.h>
#include <algorithm>

#define SEAM_INF 0x7fffffff             // above every real cost (<= 5100 L <= 2^31 - 2: seam_setup refuses longer seams); never added to
#define SEAM_PF 4                      // energy rows in flight per lane
#define SEAM_TR 128                    // steps per backtrace chunk
#define SEAM_KMAX 64                   // positions per lane of the register path: widths up to 64 * 64

struct SeamArgs {
    int hostkind;                      // 1 / 2: a strip decided by the host; 0: read mode[] = {corner, ., index, rowIndex, colIndex, err}
    int r, c, dx, dy;
    const int *mode;
    uint16_t *E[2];                    // [0] vertical seam: [r][pitch], [1] horizontal seam: [c][pitch]
    uint8_t *P[2];                     // predecessor bytes, same layout: 0 / 1 / 2 = from p - 1 / p / p + 1
    int pitch;
    int *s;                            // [r] vertical seam's column per row | [c] horizontal seam's row per column; -1 = no such seam
    int *end;                          // [2] end position (arm coordinates) of each seam
    int *wide;                         // k_seam_dp_wide: 2 seams x 2 cost rows of `pitch` ints
    int kcap;                          // most positions per lane the register path may use (SEAM_KMAX; VFSMS_SEAM_REG_CAP lowers it)
};
// positions per lane of the register path for a seam of W positions (4, 8, .. kcap), 0: the wide kernel.  Chosen on the device from the seam's
// REAL width: the arms of a corner ROI are about as wide as the overlap, far narrower than the region
__host__ __device__ inline int seam_k(int W, int kcap)
{
    for (int k = 4; k <= kcap; k *= 2)
        if (W <= 64 * k) return k;
    return 0;
}
// seam q (0 vertical, 1 horizontal): L steps, positions lo .. lo + W - 1 of the other axis, A's side below (alow) or above the seam
struct SeamPlan { int ex[2], L[2], lo[2], W[2], alow[2]; };

__device__ __forceinline__ SeamPlan seam_plan(const SeamArgs &a)
{
    SeamPlan P = {{0, 0}, {a.r, a.c}, {0, 0}, {0, 0}, {0, 0}};
    const int corner = a.hostkind ? 0 : a.mode[0];
    if (!a.hostkind && a.mode[5]) return P;                    // a geometry the fade refuses: no seam, everything B
    if (!corner) {
        const int kind = a.hostkind ? a.hostkind : (a.c <= a.r ? 1 : 2);
        if (kind == 1) { P.ex[0] = 1; P.W[0] = a.c; P.alow[0] = a.dy >= 0; }
        else { P.ex[1] = 1; P.W[1] = a.r; P.alow[1] = a.dx > 0; }
        return P;
    }
    const int index = a.mode[2];
    const bool row_up = index == 2 || index == 1, col_up = index == 2 || index == 3;
    seam_arm(a.c, a.mode[4], col_up, P.lo[0], P.W[0]); P.ex[0] = P.W[0] > 0; P.alow[0] = col_up;
    seam_arm(a.r, a.mode[3], row_up, P.lo[1], P.W[1]); P.ex[1] = P.W[1] > 0; P.alow[1] = row_up;
    return P;
}

// ---- sources: validity and filled values of region pixel (i, j) --------------------------------------------------------------------------------
struct SeamCanvas {                    // A = canvas before the paste (pixels + validity), B = the tile (always valid)
    const uint8_t *pix, *mask; int ccols, ch, ry0, rx0;
    const uint8_t *tile; int tw, ty0, tx0;
    __device__ __forceinline__ bool av(int i, int j) const { return mask[(size_t)(ry0 + i) * ccols + rx0 + j] != 0; }
    __device__ __forceinline__ bool bv(int, int) const { return true; }
    __device__ __forceinline__ void ab(int i, int j, int k, int &a1, int &b1) const
    {
        const size_t co = (size_t)(ry0 + i) * ccols + rx0 + j;
        b1 = tile[((size_t)(ty0 + i) * tw + tx0 + j) * ch + k];
        a1 = mask[co] ? (int)pix[co * ch + k] : b1;
    }
};
struct SeamI64 {                       // the reference's representation: int64 [r][c][ch], -1 = empty
    const long long *A, *B; int c, ch;
    __device__ __forceinline__ bool valid(const long long *p) const
    {
        if (ch == 1) return p[0] != -1;
        long long s = 0; for (int k = 0; k < ch; k++) s += p[k];
        return s != -ch;                   // empty = every channel -1, as I64View::a_valid
    }
    __device__ __forceinline__ bool av(int i, int j) const { return valid(A + ((size_t)i * c + j) * ch); }
    __device__ __forceinline__ bool bv(int i, int j) const { return valid(B + ((size_t)i * c + j) * ch); }
    __device__ __forceinline__ void ab(int i, int j, int k, int &a1, int &b1) const
    {
        const size_t e = ((size_t)i * c + j) * ch + k;
        const long long x = A[e], y = B[e];
        const long long xa = x >= 0 ? x : y, yb = y >= 0 ? y : xa;
        a1 = (int)(xa > 0 ? xa : 0); b1 = (int)(yb > 0 ? yb : 0);
    }
};
template <class Src>
__device__ __forceinline__ int seam_d(const Src &S, int i, int j, int k)
{
    int a1, b1;
    S.ab(i, j, k, a1, b1);
    return a1 - b1;
}

// ---- energy --------------------------------------------------------------------------------------------------------------------------------------
template <class Src>
__global__ __launch_bounds__(256) void k_seam_energy(Src S, SeamArgs a, int ch)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= a.c || i >= a.r) return;
    const SeamPlan P = seam_plan(a);
    const int pv = j - P.lo[0], ph = i - P.lo[1];
    const bool wv = P.ex[0] && pv >= 0 && pv < P.W[0], wh = P.ex[1] && ph >= 0 && ph < P.W[1];
    if (!wv && !wh) return;
    int e = 0;
    if (S.av(i, j) && S.bv(i, j)) {
        const int jm = max(j - 1, 0), jp = min(j + 1, a.c - 1), im = max(i - 1, 0), ip = min(i + 1, a.r - 1);
        for (int k = 0; k < ch; k++)
            e += abs(seam_d(S, i, j, k)) + abs(seam_d(S, i, jp, k) - seam_d(S, i, jm, k)) + abs(seam_d(S, ip, j, k) - seam_d(S, im, j, k));
    }
    if (wv) a.E[0][(size_t)i * a.pitch + pv] = (uint16_t)e;
    if (wh) a.E[1][(size_t)j * a.pitch + ph] = (uint16_t)e;
}

// ---- forward pass: one wave per seam, the cost row in registers ------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void seam_dp_body(const SeamArgs &a, const SeamPlan &P, int q)
{
    const int lane = threadIdx.x;
    const int L = P.L[q], W = P.W[q], p0 = lane * K;
    const uint16_t *E = a.E[q];
    uint8_t *PR = a.P[q];
    const size_t pitch = (size_t)a.pitch;
    uint32_t buf[SEAM_PF][K / 2];
    auto fetch = [&](int t, uint32_t *w) {
        const uint32_t *src = (const uint32_t *)__builtin_assume_aligned(E + (size_t)t * pitch + p0, K >= 8 ? 16 : 2 * K);
#pragma unroll
        for (int x = 0; x < K / 2; x++) w[x] = src[x];
    };
    int cost[K];
    fetch(0, buf[0]);
#pragma unroll
    for (int k = 0; k < K; k++) cost[k] = p0 + k < W ? (int)((buf[0][k >> 1] >> (16 * (k & 1))) & 0xffff) : SEAM_INF;
#pragma unroll
    for (int d = 0; d < SEAM_PF; d++)
        if (1 + d < L) fetch(1 + d, buf[d]);
    for (int t0 = 1; t0 < L; t0 += SEAM_PF) {
#pragma unroll
        for (int d = 0; d < SEAM_PF; d++) {
            const int t = t0 + d;
            if (t < L) {                                            // wave-uniform
                int left = __shfl_up(cost[K - 1], 1, 64), right = __shfl_down(cost[0], 1, 64);
                if (lane == 0) left = SEAM_INF;
                if (lane == 63) right = SEAM_INF;
                uint32_t dirs[K / 4];
#pragma unroll
                for (int x = 0; x < K / 4; x++) dirs[x] = 0;
                int prev = left;                                    // the OLD cost of position p - 1
#pragma unroll
                for (int k = 0; k < K; k++) {
                    const int mid = cost[k], nxt = k + 1 < K ? cost[k + 1] : right;
                    int best = prev; uint32_t dir = 0;
                    if (mid < best) { best = mid; dir = 1; }
                    if (nxt < best) { best = nxt; dir = 2; }
                    const int e = (int)((buf[d][k >> 1] >> (16 * (k & 1))) & 0xffff);
                    prev = mid;
                    cost[k] = p0 + k < W ? (int)((unsigned)best + (unsigned)e) : SEAM_INF;
                    dirs[k >> 2] |= dir << (8 * (k & 3));
                }
                uint32_t *dst = (uint32_t *)(PR + (size_t)t * pitch + p0);
#pragma unroll
                for (int x = 0; x < K / 4; x++) dst[x] = dirs[x];
                if (t + SEAM_PF < L) fetch(t + SEAM_PF, buf[d]);
            }
        }
    }
    // the lowest-index minimum of the last row: (cost, position) keys, minimum over the wave
    unsigned long long key = ~0ull;
#pragma unroll
    for (int k = 0; k < K; k++) {
        const unsigned long long kk = ((unsigned long long)(unsigned)cost[k] << 32) | (unsigned)(p0 + k);
        key = kk < key ? kk : key;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o < key ? o : key;
    }
    if (lane == 0) a.end[q] = (int)(key & 0xffffffffu);
}
__global__ __launch_bounds__(64) void k_seam_dp(SeamArgs a)
{
    const int q = blockIdx.x;
    const SeamPlan P = seam_plan(a);
    if (!P.ex[q]) return;
    switch (seam_k(P.W[q], a.kcap)) {                           // wave-uniform; 0: k_seam_dp_wide takes this seam
    case 4: seam_dp_body<4>(a, P, q); break;
    case 8: seam_dp_body<8>(a, P, q); break;
    case 16: seam_dp_body<16>(a, P, q); break;
    case 32: seam_dp_body<32>(a, P, q); break;
    case 64: seam_dp_body<64>(a, P, q); break;
    }
}

// any width: one workgroup per seam, the two cost rows in global scratch (read back by other threads of the same workgroup after a barrier)
__global__ __launch_bounds__(1024) void k_seam_dp_wide(SeamArgs a)
{
    const int q = blockIdx.x, t_ = threadIdx.x;
    const SeamPlan P = seam_plan(a);
    if (!P.ex[q] || seam_k(P.W[q], a.kcap)) return;            // (the register path has this seam)
    const int L = P.L[q], W = P.W[q];
    const uint16_t *E = a.E[q];
    uint8_t *PR = a.P[q];
    const size_t pitch = (size_t)a.pitch;
    int *row[2] = {a.wide + (size_t)(2 * q) * pitch, a.wide + (size_t)(2 * q + 1) * pitch};
    for (int p = t_; p < W; p += 1024) row[0][p] = E[p];
    __threadfence_block();
    __syncthreads();
    for (int t = 1; t < L; t++) {
        const int *src = row[(t - 1) & 1];
        int *dst = row[t & 1];
        for (int p = t_; p < W; p += 1024) {
            const int left = p > 0 ? __hip_atomic_load(src + p - 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : SEAM_INF;
            const int mid = __hip_atomic_load(src + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            const int nxt = p + 1 < W ? __hip_atomic_load(src + p + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) : SEAM_INF;
            int best = left, dir = 0;
            if (mid < best) { best = mid; dir = 1; }
            if (nxt < best) { best = nxt; dir = 2; }
            __hip_atomic_store(dst + p, best + (int)E[(size_t)t * pitch + p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            PR[(size_t)t * pitch + p] = (uint8_t)dir;
        }
        __threadfence_block();
        __syncthreads();
    }
    __shared__ unsigned long long s_key[16];
    const int *last = row[(L - 1) & 1];
    unsigned long long key = ~0ull;
    for (int p = t_; p < W; p += 1024) {
        const unsigned long long kk = ((unsigned long long)(unsigned)__hip_atomic_load(last + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) << 32) | (unsigned)p;
        key = kk < key ? kk : key;
    }
    for (int d = 32; d > 0; d >>= 1) {
        const unsigned long long o = __shfl_xor(key, d, 64);
        key = o < key ? o : key;
    }
    if ((t_ & 63) == 0) s_key[t_ >> 6] = key;
    __syncthreads();
    if (t_ == 0) {
        for (int w = 1; w < 16; w++) key = s_key[w] < key ? s_key[w] : key;
        a.end[q] = (int)(key & 0xffffffffu);
    }
}

// ---- backtrace: chunks of SEAM_TR steps, the reachable cone of predecessor bytes staged in LDS -------------------------------------------------------
__global__ __launch_bounds__(256) void k_seam_trace(SeamArgs a)
{
    __shared__ uint8_t s_pred[SEAM_TR][2 * SEAM_TR + 4];
    __shared__ int s_pos[SEAM_TR];
    __shared__ int s_p;
    const int q = blockIdx.x, t_ = threadIdx.x;
    const SeamPlan P = seam_plan(a);
    int *s = a.s + (q ? a.r : 0);
    const int L = P.L[q];
    if (!P.ex[q]) {
        for (int t = t_; t < L; t += 256) s[t] = -1;
        return;
    }
    const int W = P.W[q], lo = P.lo[q];
    const uint8_t *PR = a.P[q];
    const size_t pitch = (size_t)a.pitch;
    if (t_ == 0) s_p = a.end[q];
    __syncthreads();
    for (int t1 = L - 1; t1 >= 0; t1 -= SEAM_TR) {
        const int t0 = max(t1 - SEAM_TR + 1, 0), n = t1 - t0 + 1;
        const int p = s_p;
        const int w0 = max(p - SEAM_TR, 0), w1 = min(p + SEAM_TR, W - 1), nw = w1 - w0 + 1;      // step t is at most t1 - t positions away from p
        for (int e = t_; e < n * nw; e += 256) {
            const int y = e / nw, x = e - y * nw;
            s_pred[y][x] = PR[(size_t)(t0 + y) * pitch + w0 + x];
        }
        __syncthreads();
        if (t_ == 0) {
            int pp = p;
            for (int y = n - 1; y >= 0; y--) {
                s_pos[y] = pp;
                if (t0 + y > 0) pp += (int)s_pred[y][pp - w0] - 1;                            // (row 0 has no predecessor)
            }
            s_p = pp;
        }
        __syncthreads();
        for (int y = t_; y < n; y += 256) s[t0 + y] = lo + s_pos[y];
        __syncthreads();
    }
}

// ---- label and apply -------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool seam_a_side(const SeamPlan &P, const int *s, int r, int i, int j)
{
    bool side = false;
    if (P.ex[0]) { const int sv = s[i]; side = P.alow[0] ? j < sv : j > sv; }
    if (P.ex[1]) { const int sh = s[r + j]; side = side || (P.alow[1] ? i < sh : i > sh); }
    return side;
}
template <class Src>
__global__ __launch_bounds__(256) void k_seam_label(Src S, SeamArgs a, uint8_t *label)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= a.c || i >= a.r) return;
    const SeamPlan P = seam_plan(a);
    label[(size_t)i * a.c + j] = S.av(i, j) && seam_a_side(P, a.s, a.r, i, j);
}
__global__ __launch_bounds__(256) void k_seam_apply_i64(SeamI64 S, SeamArgs a, uint8_t *out)
{
    const int j = blockIdx.x * 256 + threadIdx.x, i = blockIdx.y;
    if (j >= a.c || i >= a.r) return;
    const SeamPlan P = seam_plan(a);
    const bool refused = !a.hostkind && a.mode[5];
    const bool lab = S.av(i, j) && seam_a_side(P, a.s, a.r, i, j);
    for (int k = 0; k < S.ch; k++) {
        int a1, b1;
        S.ab(i, j, k, a1, b1);
        out[((size_t)i * a.c + j) * S.ch + k] = refused ? 0 : (uint8_t)(lab ? a1 : b1);
    }
}
// the grid covers the tile rectangle (th x tw at canvas (y0, x0)): ROI pixels labelled A keep the canvas, every other pixel takes the tile, and
// every pixel of the rectangle becomes valid
__global__ __launch_bounds__(256) void k_seam_apply_canvas(SeamCanvas S, SeamArgs a, uint8_t *pix, uint8_t *mask, int y0, int x0, int th, int tw)
{
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= tw || y >= th) return;
    const size_t co = (size_t)(y0 + y) * S.ccols + x0 + x;
    const int i = y0 + y - S.ry0, j = x0 + x - S.rx0;
    bool keep = false;
    if (i >= 0 && i < a.r && j >= 0 && j < a.c && mask[co]) keep = seam_a_side(seam_plan(a), a.s, a.r, i, j);
    if (!keep)
        for (int k = 0; k < S.ch; k++) pix[co * S.ch + k] = S.tile[((size_t)y * tw + x) * S.ch + k];
    mask[co] = 1;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
// the register path's cap (VFSMS_SEAM_REG_CAP lowers it, 0 = wide kernel only: tests, A/B runs)
static int seam_kcap()
{
    const char *env = getenv("VFSMS_SEAM_REG_CAP");
    return env ? std::min(std::max(atoi(env), 0), SEAM_KMAX) : SEAM_KMAX;
}

// scratch layout.  wmax: an upper bound of the positions of a seam of this region (min(r, c) for a strip the host decided on, the widest arm of
// the four corner picks when the host evaluated them, max(r, c) otherwise).  It sizes the planes' pitch only: K = the register path's
// positions per lane AT that bound, and the kernels pick their own K <= it from the seam's real width (64 K_device <= pitch either way)
struct SeamRun { SeamArgs a; uint8_t *label; int K; };
static int seam_setup(vfsms_ctx *ctx, int hostkind, int r, int c, int dx, int dy, const int *mode, int wmax, bool want_label, SeamRun *R)
{
    if ((long long)5100 * std::max(r, c) > 0x7fffffffLL) { vfsms_set_error("fuse_seam: region too long for int32 cumulative costs (5100 * max(r, c) > 2^31 - 1)"); return VFSMS_ERR_BAD_ARG; }
    R->a.kcap = seam_kcap();
    R->K = seam_k(wmax, R->a.kcap);
    const size_t pitch = R->K ? (size_t)64 * R->K : (((size_t)wmax + 63) & ~(size_t)63);
    const bool v = hostkind != 2, h = hostkind != 1;          // which seams can exist
    size_t off = 0;
    auto take = [&](size_t n) { const size_t o = off; off += (n + 255) & ~(size_t)255; return o; };
    const size_t oE0 = take(v ? (size_t)r * pitch * 2 : 0), oE1 = take(h ? (size_t)c * pitch * 2 : 0);
    const size_t oP0 = take(v ? (size_t)r * pitch : 0), oP1 = take(h ? (size_t)c * pitch : 0);
    const size_t oS = take(sizeof(int) * ((size_t)r + c)), oEnd = take(sizeof(int) * 2);
    const size_t oWide = take(R->K ? 0 : sizeof(int) * 4 * pitch), oLab = take(want_label ? (size_t)r * c : 0);
    TRY(ctx->seam_scratch.reserve(off, ctx->stream));
    char *base = ctx->seam_scratch.as<char>();
    SeamArgs &a = R->a;
    a.hostkind = hostkind; a.r = r; a.c = c; a.dx = dx; a.dy = dy; a.mode = mode;
    a.E[0] = (uint16_t *)(base + oE0); a.E[1] = (uint16_t *)(base + oE1);
    a.P[0] = (uint8_t *)(base + oP0); a.P[1] = (uint8_t *)(base + oP1);
    a.pitch = (int)pitch; a.s = (int *)(base + oS); a.end = (int *)(base + oEnd); a.wide = (int *)(base + oWide);
    R->label = (uint8_t *)(base + oLab);
    return VFSMS_OK;
}
static int seam_solve(vfsms_ctx *ctx, const SeamRun &R)
{
    const SeamArgs &a = R.a;
    {
        ProfScope ps(ctx, "seam_dp");
        // each seam is solved by exactly one of the two kernels (seam_k of its real width); the wide one is only launched where the bound admits it
        if (a.kcap >= 4) hipLaunchKernelGGL(k_seam_dp, dim3(2), dim3(64), 0, ctx->stream, a);
        if (!R.K) hipLaunchKernelGGL(k_seam_dp_wide, dim3(2), dim3(1024), 0, ctx->stream, a);
    }
    {
        ProfScope ps(ctx, "seam_trace");
        hipLaunchKernelGGL(k_seam_trace, dim3(2), dim3(256), 0, ctx->stream, a);
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// The placement's ROI cut along its seam between the canvas and the tile, the tile pasted around it.  hostkind / mode as SeamArgs.  blend 0:
// none, 1: the label plane into the pyramid blend with `levels`.  Enqueue only; the caller marks the rectangle in the canvas's list.
int seam_fuse_canvas(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, int hostkind, const int *mode, int wmax,
                     int blend, int levels)
{
    const int r = p.r(), c = p.c();
    SeamRun R;
    TRY(seam_setup(ctx, hostkind, r, c, p.dx, p.dy, mode, wmax, blend != 0, &R));
    const SeamCanvas S = {cv->pix.as<uint8_t>(), cv->mask.as<uint8_t>(), cv->cols, cv->ch, p.ry0, p.rx0, d_tile, p.w, p.ry0 - p.y0, p.rx0 - p.x0};
    const dim3 rgrid((c + 255) / 256, r);
    {
        ProfScope ps(ctx, "seam_energy");
        hipLaunchKernelGGL(k_seam_energy<SeamCanvas>, rgrid, dim3(256), 0, ctx->stream, S, R.a, cv->ch);
    }
    TRY(seam_solve(ctx, R));
    if (blend) {
        {
            ProfScope ps(ctx, "seam_apply");
            hipLaunchKernelGGL(k_seam_label<SeamCanvas>, rgrid, dim3(256), 0, ctx->stream, S, R.a, R.label);
        }
        SeamGeom G = {4, r, c, p.dx, p.dy};
        G.label = R.label;
        return mb_blend_canvas(ctx, cv, d_tile, p, G, levels);
    }
    ProfScope ps(ctx, "seam_apply");
    hipLaunchKernelGGL(k_seam_apply_canvas, dim3((p.w + 255) / 256, p.h), dim3(256), 0, ctx->stream, S, R.a, cv->pix.as<uint8_t>(), cv->mask.as<uint8_t>(), p.y0, p.x0, p.h, p.w);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// int64 regions (device) -> u8 [r][c][ch] (device) and, when d_seam is given, the r + c seam entries; mode[]: the ramp kernel's status ints
int seam_fuse_i64(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, int ch, int dx, int dy, const int *mode,
                  int blend, int levels, uint8_t *d_out, int32_t *d_seam)
{
    SeamRun R;
    TRY(seam_setup(ctx, 0, r, c, dx, dy, mode, std::max(r, c), blend != 0, &R));
    const SeamI64 S = {dA, dB, c, ch};
    const dim3 rgrid((c + 255) / 256, r);
    {
        ProfScope ps(ctx, "seam_energy");
        hipLaunchKernelGGL(k_seam_energy<SeamI64>, rgrid, dim3(256), 0, ctx->stream, S, R.a, ch);
    }
    TRY(seam_solve(ctx, R));
    if (d_seam) HIP_TRY(hipMemcpyAsync(d_seam, R.a.s, sizeof(int32_t) * ((size_t)r + c), hipMemcpyDeviceToDevice, ctx->stream));
    if (blend) {
        {
            ProfScope ps(ctx, "seam_apply");
            hipLaunchKernelGGL(k_seam_label<SeamI64>, rgrid, dim3(256), 0, ctx->stream, S, R.a, R.label);
        }
        SeamGeom G = {4, r, c, dx, dy};
        G.label = R.label;
        return mb_blend_i64(ctx, dA, dB, r, c, ch, G, levels, d_out);
    }
    ProfScope ps(ctx, "seam_apply");
    hipLaunchKernelGGL(k_seam_apply_i64, rgrid, dim3(256), 0, ctx->stream, S, R.a, d_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
