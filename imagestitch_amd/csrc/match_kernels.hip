// match_kernels.hip -- brute-force matchers + ratio test + mode vote for gfx950.
//
// Replaces BFMatcher("BruteForce").knnMatch(k=2) + ratio filter (ImageUtility.py:288-296; DLL twin
// appendix/myGpuFeatures.cpp:160-173), BFMatcher("BruteForce-Hamming").match (ImageUtility.py:297-302)
// and Method.getOffsetByMode (ImageUtility.py:139-178).
//
// BF-L2 layout (CDNA4-native, not a warp-tiled GEMM): every lane OWNS two query descriptors in VGPRs
// (2 x 64 floats, packed so the inner loop is v_pk_add/v_pk_mul on both queries at once); train
// descriptors are wave-uniform and stream through the scalar data path (s_load) -- no LDS traffic, no
// cross-lane reduction in the hot loop: each lane keeps its own running best / second best.  Trains are
// split across blockIdx.y so that a single ROI pair still fills 256 CUs; the partial 2-NN lists are
// merged (ascending train order, ties keep the lower index) by k_merge_ratio.
// Distances: float accumulation in the 4-wide order of normL2Sqr_, sqrt per candidate exactly when the
// squared distance can still change the top-2 (comparisons happen in the sqrt domain like OpenCV's).
#include "common.h"
#include <algorithm>
#include <stdlib.h>
#include <math.h>

typedef float float2v __attribute__((ext_vector_type(2)));
typedef const float __attribute__((address_space(4))) cfloat;   // AMDGPU constant address space
typedef float f16v __attribute__((ext_vector_type(16)));

// hand-placed scalar loads (hipcc adds no waits for asm, cdna_hip_programming.md section 5.7): the wait takes the
// destination tuple as an in/out operand so every use of the data is ordered behind it.
#define SLOAD16(dst, ptr) asm volatile("s_load_dwordx16 %0, %1, 0x0" : "=s"(dst) : "s"(ptr))
// prefetch into dst while `live` (the tuple about to be consumed) is threaded through, which pins the issue point
// of the load in front of the VALU work on `live`
#define SLOAD16_BEFORE(dst, ptr, live) asm volatile("s_load_dwordx16 %0, %2, 0x0" : "=s"(dst), "+s"(live) : "s"(ptr))
#define SWAIT(dst) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(dst))
#define SWAIT2(d0, d1) asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d0), "+s"(d1))
#define BF_CHUNK(buf, base)                                                                    \
    _Pragma("unroll") for (int d = 0; d < 16; d += 4) {                                        \
        float2v e0 = qv[base + d + 0] - buf[d + 0];                                            \
        float2v e1 = qv[base + d + 1] - buf[d + 1];                                            \
        float2v e2 = qv[base + d + 2] - buf[d + 2];                                            \
        float2v e3 = qv[base + d + 3] - buf[d + 3];                                            \
        acc += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;                                          \
    }

__device__ __forceinline__ void knn_update(float dsq, int j, float &b1, float &b2, int &i1, float &b1sq, float &b2sq)
{
    if (dsq < b2sq) {
        float d = sqrtf(dsq);
        if (d < b1) { b2 = b1; b2sq = b1sq; b1 = d; b1sq = dsq; i1 = j; }
        else if (d < b2) { b2 = d; b2sq = dsq; }
    }
}

// DIM = 64: two queries per lane (packed).  block = 256 threads = 4 waves x 128 queries.
__global__ __launch_bounds__(256) void k_bf_l2_d64(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.z];
    // device-side counts are wave-uniform: pin them to SGPRs so loop bounds and train addresses stay scalar
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * 512 + wave * 128;
    if (q0 >= nq) return;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int chunk = (nt + nsplit - 1) / nsplit;
    const int t0 = sp * chunk, t1 = min(nt, t0 + chunk);
    const int qa = q0 + lane, qb = q0 + 64 + lane;
    const float *__restrict__ pa = J.q + (size_t)min(qa, nq - 1) * 64;
    const float *__restrict__ pb = J.q + (size_t)min(qb, nq - 1) * 64;
    float2v qv[64];
#pragma unroll
    for (int d = 0; d < 64; d += 4) {
        float4 va = *reinterpret_cast<const float4 *>(pa + d);
        float4 vb = *reinterpret_cast<const float4 *>(pb + d);
        qv[d + 0] = (float2v){va.x, vb.x}; qv[d + 1] = (float2v){va.y, vb.y};
        qv[d + 2] = (float2v){va.z, vb.z}; qv[d + 3] = (float2v){va.w, vb.w};
    }
    float b1a = INFINITY, b2a = INFINITY, b1sa = INFINITY, b2sa = INFINITY; int i1a = -1;
    float b1b = INFINITY, b2b = INFINITY, b1sb = INFINITY, b2sb = INFINITY; int i1b = -1;
    // Train descriptors were written by an earlier kernel and are read-only here and wave-uniform: they are
    // streamed through the scalar data path, 16 floats (one s_load_dwordx16) at a time, double-buffered by hand:
    // the load of chunk c+1 is issued before the 48 packed VALU ops on chunk c, so its latency is covered.
    // (hipcc places s_waitcnt lgkmcnt(0) right behind every scalar load it schedules itself; SMEM returns out
    // of order, so the only safe wait is 0 and it must sit BEFORE the next prefetch is issued.)
    const float *T = J.t;
    if (t0 < t1) {
        // half-train granularity: 2 x s_load_dwordx16 per wait, 96 packed VALU ops of cover for each prefetch
        f16v a0, a1, b0, b1;
        const float *first = T + (size_t)t0 * 64;
        SLOAD16(a0, first); SLOAD16(a1, first + 16);
        for (int j = t0; j < t1; j++) {
            const float *tn = T + (size_t)min(j + 1, t1 - 1) * 64;      // next train (clamped: harmless re-read)
            float2v acc = (float2v){0.f, 0.f};
            SWAIT2(a0, a1);
            SLOAD16_BEFORE(b0, T + (size_t)j * 64 + 32, a0); SLOAD16_BEFORE(b1, T + (size_t)j * 64 + 48, a1);
            BF_CHUNK(a0, 0);
            BF_CHUNK(a1, 16);
            SWAIT2(b0, b1);
            SLOAD16_BEFORE(a0, tn, b0); SLOAD16_BEFORE(a1, tn + 16, b1);
            BF_CHUNK(b0, 32);
            BF_CHUNK(b1, 48);
            knn_update(acc.x, j, b1a, b2a, i1a, b1sa, b2sa);
            knn_update(acc.y, j, b1b, b2b, i1b, b1sb, b2sb);
        }
        SWAIT2(a0, a1);                                                  // drain the last prefetch
    }
    const size_t o = (size_t)sp * J.capq;
    if (qa < nq) { J.p_d1[o + qa] = b1a; J.p_d2[o + qa] = b2a; J.p_i1[o + qa] = i1a; }
    if (qb < nq) { J.p_d1[o + qb] = b1b; J.p_d2[o + qb] = b2b; J.p_i1[o + qb] = i1b; }
}

// generic DIM (multiple of 4, <= 128): one query per lane.  block = 256 threads = 256 queries.
template <int DIM>
__global__ __launch_bounds__(256) void k_bf_l2_gen(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.z];
    // device-side counts are wave-uniform: pin them to SGPRs so loop bounds and train addresses stay scalar
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int q0 = blockIdx.x * 256;
    if (q0 >= nq) return;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int chunk = (nt + nsplit - 1) / nsplit;
    const int t0 = sp * chunk, t1 = min(nt, t0 + chunk);
    const int qa = q0 + threadIdx.x;
    const float *__restrict__ pa = J.q + (size_t)min(qa, nq - 1) * DIM;
    float qv[DIM];
#pragma unroll
    for (int d = 0; d < DIM; d++) qv[d] = pa[d];
    float b1 = INFINITY, b2 = INFINITY, b1s = INFINITY, b2s = INFINITY; int i1 = -1;
    const float *__restrict__ T = J.t;
    for (int j = t0; j < t1; j++) {
        const float *__restrict__ tr = T + (size_t)j * DIM;
        float acc = 0.f;
#pragma unroll
        for (int d = 0; d < DIM; d += 4) {
            float e0 = qv[d] - tr[d], e1 = qv[d + 1] - tr[d + 1], e2 = qv[d + 2] - tr[d + 2], e3 = qv[d + 3] - tr[d + 3];
            acc += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
        }
        knn_update(acc, j, b1, b2, i1, b1s, b2s);
    }
    const size_t o = (size_t)sp * J.capq;
    if (qa < nq) { J.p_d1[o + qa] = b1; J.p_d2[o + qa] = b2; J.p_i1[o + qa] = i1; }
}

// ---------------------------------------------------------------------------------------------------
// Exact matrix-core 2-NN for 128-d descriptors with integer elements 0..255 (the fused SIFT attempt path).
//
// Every element k_sift_describe writes is an integer 0..255, so a squared distance is an integer <= 128 * 255^2 = 8 323 200 < 2^24:
// float accumulation gives it exactly in any order, and so does |q'|^2 + |t'|^2 - 2 q'.t' in int32 with q' = q - 128, t' = t - 128 (the
// shift cancels in q - t; |q'|^2 <= 2^21, |q'.t'| <= 2^21).  The dot products run on v_mfma_i32_16x16x64_i8; the float of the integer
// distance IS the dsq k_bf_l2_gen<128> forms, and it goes through the same knn_update (sqrtf, strict <), so (i1, d1, d2) come out
// bit for bit -- no verification pass.
// k_pack_i8_d128 writes a strip's rows once (per strip, not per job).  k_bf_i8_d128: a wave keeps 64 queries as the B operands of four
// 16-column tiles (8 x 4 VGPRs) and streams 16-train tiles as the A operand straight from memory (the four waves of a workgroup
// walk the same trains, 2 KB a tile); lane l then holds, for query column l & 15, the trains 4 (l >> 4) .. + 3 of the tile.  A lane
// compares the integer score |t'|^2 - 2 q'.t' with its own integer threshold (second best so far - |q'|^2) and only enters knn_update
// for a train that beats it.  A lane sees its trains in ascending order, so its list is the reference's over its subset; the four
// lanes of a query column are merged by (distance, index), which is what the ascending scan gives over the union; train splits are
// whole ranges, merged by k_merge_ratio in ascending order as for every other kernel here.
// ---------------------------------------------------------------------------------------------------
typedef int i4v __attribute__((ext_vector_type(4)));

// one workgroup per 64 rows of a strip, 4 lanes per row; rows at and beyond the strip's count (up to the 64-row tile) become zero rows
// with the norm BFI_PAD_NORM
__global__ __launch_bounds__(256) void k_pack_i8_d128(const PackJob *jobs)
{
    const PackJob J = jobs[blockIdx.y];
    const int n = *J.n_ptr, r0 = blockIdx.x * 64;
    if (r0 >= n) return;
    const int row = r0 + (threadIdx.x >> 2), part = threadIdx.x & 3;
    int nrm = 0;
    unsigned w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = 0;
    if (row < n) {
        const float4 *src = (const float4 *)(J.src + (size_t)row * 128 + part * 32);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float4 v = src[i];
            const int a = (int)v.x - 128, b = (int)v.y - 128, c = (int)v.z - 128, d = (int)v.w - 128;
            nrm += a * a + b * b + c * c + d * d;
            w[i] = (unsigned)(a & 255) | ((unsigned)(b & 255) << 8) | ((unsigned)(c & 255) << 16) | ((unsigned)(d & 255) << 24);
        }
    }
    nrm += __shfl_xor(nrm, 1, 64);
    nrm += __shfl_xor(nrm, 2, 64);
    uint4 *dst = (uint4 *)(J.dst + (size_t)row * 128 + part * 32);
    dst[0] = make_uint4(w[0], w[1], w[2], w[3]);
    dst[1] = make_uint4(w[4], w[5], w[6], w[7]);
    if (part == 0) J.nrm[row] = row < n ? nrm : BFI_PAD_NORM;
}

__device__ __forceinline__ void knn_merge(float &b1, float &b2, int &i1, float ob1, float ob2, int oi1)
{
    if (ob1 < b1 || (ob1 == b1 && (unsigned)oi1 < (unsigned)i1)) { b2 = fminf(ob2, b1); b1 = ob1; i1 = oi1; }
    else b2 = fminf(b2, ob1);
}

// block = 256 threads = 4 waves x 64 queries; grid (query blocks, train splits, jobs)
__global__ __launch_bounds__(256) void k_bf_i8_d128(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.z];
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int lane = threadIdx.x & 63, c = lane & 15, g = lane >> 4;
    const int qw = blockIdx.x * 256 + (threadIdx.x >> 6) * 64;
    if (qw >= nq) return;
    // whole 16-train tiles per split
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int tiles = (nt + 15) >> 4, tchunk = (tiles + nsplit - 1) / nsplit;
    const int t0 = sp * tchunk * 16, t1 = min(tiles * 16, t0 + tchunk * 16);
    i4v qb[4][2];
    int qn[4], thr[4], i1[4];
    float b1[4], b2[4], b1s[4], b2s[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int q = qw + 16 * u + c;                                  // < sift_pad_rows(nq): packed (zero) rows exist up to there
        const i4v *qp = (const i4v *)(J.q8 + (size_t)q * 128);
        qb[u][0] = qp[g]; qb[u][1] = qp[4 + g];
        qn[u] = J.qn2[q];
        thr[u] = 0x7fffffff; i1[u] = -1;
        b1[u] = b2[u] = b1s[u] = b2s[u] = INFINITY;
    }
    for (int jt = t0; jt < t1; jt += 16) {
        const i4v *tp = (const i4v *)(J.t8 + (size_t)(jt + c) * 128);
        const i4v a0 = tp[g], a1 = tp[4 + g];
        const i4v tn = *(const i4v *)(J.tn2 + jt + 4 * g);
        const int j0 = jt + 4 * g;
#pragma unroll
        for (int u = 0; u < 4; u++) {
            i4v acc = {0, 0, 0, 0};
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, qb[u][0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, qb[u][1], acc, 0, 0, 0);
            const int s0 = tn[0] - 2 * acc[0], s1 = tn[1] - 2 * acc[1], s2 = tn[2] - 2 * acc[2], s3 = tn[3] - 2 * acc[3];
            if (min(min(s0, s1), min(s2, s3)) < thr[u]) {
                // ascending train order; a padded row (j >= nt) never counts
                if (s0 < thr[u] && j0 < nt) knn_update((float)(s0 + qn[u]), j0, b1[u], b2[u], i1[u], b1s[u], b2s[u]);
                if (s1 < thr[u] && j0 + 1 < nt) knn_update((float)(s1 + qn[u]), j0 + 1, b1[u], b2[u], i1[u], b1s[u], b2s[u]);
                if (s2 < thr[u] && j0 + 2 < nt) knn_update((float)(s2 + qn[u]), j0 + 2, b1[u], b2[u], i1[u], b1s[u], b2s[u]);
                if (s3 < thr[u] && j0 + 3 < nt) knn_update((float)(s3 + qn[u]), j0 + 3, b1[u], b2[u], i1[u], b1s[u], b2s[u]);
                thr[u] = b2s[u] == INFINITY ? 0x7fffffff : (int)b2s[u] - qn[u];
            }
        }
    }
    const size_t o = (size_t)sp * J.capq;
#pragma unroll
    for (int u = 0; u < 4; u++) {
        float B1 = b1[u], B2 = b2[u]; int I1 = i1[u];
#pragma unroll
        for (int d = 16; d <= 32; d <<= 1) {
            const float ob1 = __shfl_xor(B1, d, 64), ob2 = __shfl_xor(B2, d, 64);
            const int oi1 = __shfl_xor(I1, d, 64);
            knn_merge(B1, B2, I1, ob1, ob2, oi1);
        }
        const int q = qw + 16 * u + c;
        if (g == 0 && q < nq) { J.p_d1[o + q] = B1; J.p_d2[o + q] = B2; J.p_i1[o + q] = I1; }
    }
}

// ---------------------------------------------------------------------------------------------------
// MFMA candidate filter + exact verification (DIM = 64, descriptors of norm <= 1: the fused SURF attempt path).
//
// The 2-NN of a query under the reference's float arithmetic are, with a wide safety margin, among the trains whose
// f32-MFMA score  s(q,t) = |t|^2 - 2 q.t  (= d^2 - |q|^2 up to ~1e-5) lies within BFM_MARGIN of the second best
// score.  k_bf_mfma_d64 streams 32-train tiles against 64 resident queries per wave on v_mfma_f32_32x32x2_f32
// (K = 64 + one augmented step that adds |t|^2, so the accumulator IS the score) and appends to a small per-lane list
// every train whose score is within the margin of the lane's RUNNING second best -- a superset of the final
// candidates, since a running second best over a prefix of half the trains can only be larger than the final one.
// k_bf_verify_d64 then evaluates exactly those few trains (~10 per list) with the arithmetic of k_bf_l2_d64 (4-wide
// float accumulation, sqrt-domain compares, ties keep the lower index) -- the MFMA decides which distances get
// computed, never what they are.  A list that overflows makes its query fall back to the exhaustive exact scan.
// ---------------------------------------------------------------------------------------------------
#define BFM_CAPL 32
#define BFM_MARGIN 1e-3f        // >= 40x the worst-case |score - (d_ref^2 - |q|^2)| for K = 65, |q|,|t| <= 1
#define BFM_FAR 1e30f

struct BfmState { float m1, m2, thr; int cnt; };

__device__ __forceinline__ void bfm_warm(const f16v &acc, BfmState &S)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float v = acc[i];
        S.m2 = fminf(S.m2, fmaxf(S.m1, v));
        S.m1 = fminf(S.m1, v);
    }
}
__device__ __forceinline__ void bfm_scan(const f16v &acc, BfmState &S, int row0, uint2 *list, size_t pitch, bool update)
{
#pragma unroll
    for (int i = 0; i < 16; i++) {
        const float v = acc[i];
        if (v <= S.thr && v < 1e29f) {
            if (S.cnt < BFM_CAPL) list[S.cnt * pitch] = make_uint2(__float_as_uint(v), (unsigned)(row0 + (i & 3) + 8 * (i >> 2)));
            S.cnt++;
            if (update) {
                S.m2 = fminf(S.m2, fmaxf(S.m1, v));
                S.m1 = fminf(S.m1, v);
                S.thr = S.m2 + BFM_MARGIN;
            }
        }
    }
}

__global__ __launch_bounds__(256, 2) void k_bf_mfma_d64(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.z];
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = (blockIdx.x * 4 + wave) * 64;
    if (q0 >= nq) return;
    const int nsplit = gridDim.y, sp = blockIdx.y;
    const int ntiles = (nt + 31) >> 5;
    const int tchunk = (ntiles + nsplit - 1) / nsplit;
    const int tile0 = sp * tchunk, tile1 = min(ntiles, tile0 + tchunk);
    const int col = lane & 31, half = lane >> 5;
    // B operand: lane (col, half) supplies query q0 + 32*qt + col, dims 32*half + s at k-step s (the k order is a
    // permutation of the dims, the same one for A and B); scaled by -2 (exact) so the accumulator holds -2 q.t
    float bq0[32], bq1[32];
    {
        const float4 *p0 = reinterpret_cast<const float4 *>(J.q + (size_t)min(q0 + col, nq - 1) * 64 + 32 * half);
        const float4 *p1 = reinterpret_cast<const float4 *>(J.q + (size_t)min(q0 + 32 + col, nq - 1) * 64 + 32 * half);
#pragma unroll
        for (int s4 = 0; s4 < 8; s4++) {
            const float4 u = p0[s4], v = p1[s4];
            bq0[4 * s4 + 0] = -2.f * u.x; bq0[4 * s4 + 1] = -2.f * u.y; bq0[4 * s4 + 2] = -2.f * u.z; bq0[4 * s4 + 3] = -2.f * u.w;
            bq1[4 * s4 + 0] = -2.f * v.x; bq1[4 * s4 + 1] = -2.f * v.y; bq1[4 * s4 + 2] = -2.f * v.z; bq1[4 * s4 + 3] = -2.f * v.w;
        }
    }
    const float baug = half == 0 ? 1.f : 0.f;
    const bool va = q0 + col < nq, vb = q0 + 32 + col < nq;
    BfmState Sa = {INFINITY, INFINITY, INFINITY, 0}, Sb = {INFINITY, INFINITY, INFINITY, 0};
    // lists are stored [list][entry][query] (query fastest): the 32 lanes of a half append to neighbouring addresses and
    // the verifier, one thread per query, reads them coalesced
    const size_t pitch = (size_t)J.capq;
    const int lst = sp * 2 + half;
    uint2 *lista = J.c_ent + (size_t)lst * BFM_CAPL * pitch + (q0 + col), *listb = lista + 32;
    const float *T = J.t;
    for (int pass = 0; pass < 2; pass++) {          // pass 0: first tile only, to seed the running second best
        const int tend = pass == 0 ? min(tile0 + 1, tile1) : tile1;
        float4 an[8];
        if (tile0 < tend) {
            const float4 *pn = reinterpret_cast<const float4 *>(T + (size_t)min(tile0 * 32 + col, nt - 1) * 64 + 32 * half);
#pragma unroll
            for (int s4 = 0; s4 < 8; s4++) an[s4] = pn[s4];
        }
        for (int tl = tile0; tl < tend; tl++) {
            float a[32];
#pragma unroll
            for (int s4 = 0; s4 < 8; s4++) { a[4 * s4] = an[s4].x; a[4 * s4 + 1] = an[s4].y; a[4 * s4 + 2] = an[s4].z; a[4 * s4 + 3] = an[s4].w; }
            if (tl + 1 < tend) {                    // prefetch the next train tile behind this tile's MFMAs
                const float4 *pn = reinterpret_cast<const float4 *>(T + (size_t)min((tl + 1) * 32 + col, nt - 1) * 64 + 32 * half);
#pragma unroll
                for (int s4 = 0; s4 < 8; s4++) an[s4] = pn[s4];
            }
            // |t|^2 of this lane's train row: half sums met across the two lane halves (a + b == b + a, so both agree)
            float part = 0.f;
#pragma unroll
            for (int s = 0; s < 32; s++) part += a[s] * a[s];
            const float tnorm = part + __shfl_xor(part, 32, 64);
            const float aaug = half == 0 ? (tl * 32 + col < nt ? tnorm : BFM_FAR) : 0.f;
            f16v acc0 = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}, acc1 = acc0;
#pragma unroll
            for (int s = 0; s < 32; s++) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], bq1[s], acc1, 0, 0, 0);
            }
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(aaug, baug, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(aaug, baug, acc1, 0, 0, 0);
            if (pass == 0) {
                bfm_warm(acc0, Sa); bfm_warm(acc1, Sb);
            } else {
                const int row0 = tl * 32 + 4 * half;
                // the seed tile is already part of the running statistics: list its candidates without counting them twice
                bfm_scan(acc0, Sa, row0, lista, pitch, tl != tile0); bfm_scan(acc1, Sb, row0, listb, pitch, tl != tile0);
            }
        }
        if (pass == 0) {
            Sa.thr = va ? Sa.m2 + BFM_MARGIN : -INFINITY;      // lanes of queries beyond nq never append
            Sb.thr = vb ? Sb.m2 + BFM_MARGIN : -INFINITY;
        }
    }
    if (va) J.c_cnt[(size_t)lst * pitch + q0 + col] = Sa.cnt;
    if (vb) J.c_cnt[(size_t)lst * pitch + q0 + 32 + col] = Sb.cnt;
}

// ---------------------------------------------------------------------------------------------------
// The same filter on the 16-bit matrix pipe (16x the f32-MFMA rate) with fp16 operands: every descriptor element is stored once as
// fp16 (round to nearest even; queries pre-scaled by -2, exact) and q.t is ONE v_mfma_f32_32x32x16_f16 product per 16 dims with
// f32 accumulation.  |t|^2 enters as the INITIAL VALUE of the accumulator (the C operand of the first k-step), as the f32 that
// k_bf_split16 sums: it costs no matrix instruction and no rounding of its own.  The scores only select WHICH distances the verifier
// computes exactly.
//
// Error of a score against the exact s = |t|^2 - 2 q.t of the float descriptors (norms^2 <= 1.0001: bf_l2_host checks, SURF's are
// L2-normalised), BFM_F16_ERR:
//   - relative: fp16 keeps 11 significand bits, unit roundoff u = 2^-11; a product of two rounded elements is off by at most
//     ((1 + u)^2 - 1) |a b| (the 22-bit product itself is exact in f32), and sum |2 q_i t_i| <= 2 |q||t| (Cauchy-Schwarz):
//     2 ((1 + 2^-11)^2 - 1) * 1.0001                                                                               = 1.9538e-3
//   - absolute: an element below fp16's normal range (|x| < 2^-14 = 6.1e-5, subnormals and zero) is off by up to half the subnormal
//     spacing, eta = 2^-25, instead of u |x|; a'b' - ab = (a' - a) b' + a (b' - b) adds eta (|b'| + |a|) <= 3 eta per term with
//     |t_i| <= 1, |2 q_i| <= 2: 64 * 3 * 2^-25                                                                        = 5.8e-6
//   - f32 accumulation of the 64 product slots onto the initial value: partial sums stay below 2 |q||t| + |t|^2 <= 3.01, one
//     rounding of at most 2^-23 relative per slot (2^-24 if the pipe rounds to nearest; the bound does not rely on it):
//     64 * 2^-23 * 3.01                                                                                              = 2.30e-5
//   - the initial value: |t|^2 summed in f32 by k_bf_split16 (64 additions, <= 64 * 2^-24 * 1.0001)                   = 3.8e-6
//   total 1.986e-3 <= BFM_F16_ERR = 2.0e-3.  tests/test_bf_filter_norm_init_host.py emulates the scores in numpy and checks the
//   bound (tests/test_bf_fp16_host.py: the same for the hi + lo norm slot of the previous form, whose total was 1.987e-3).
//
// k_bf_split16 writes the operands once per ROI.  Queries (each wave loads its 64 once): row = [dims 0-31 | dims 32-63].  Trains
// (every wave streams all of them) are stored in MFMA FRAGMENT order: per 32-train tile four 1 KB fragments -- k-steps 0..3 -- each
// holding the 16 bytes of lane 0, lane 1, ... lane 63, so that one load instruction of a wave reads 8 consecutive cache lines instead
// of one line per lane (the row-major layout kept the texture-address path, not the matrix pipe, busy: 64 lines per load), and behind
// them the tile's 32 |t|^2 as f32 (128 bytes).
// ---------------------------------------------------------------------------------------------------
#define BF16_ROW 64                  // uint16 per query row: 2 x 32 fp16
#define BF16_FRAGS 4                 // dimension fragments per train tile, 64 lanes x 8 fp16 each
#define BF16_TILE (BF16_FRAGS * 64 + 8)    // 16-byte units per train tile: the fragments + 32 f32 |t|^2 (4.125 KB)
#define BFM_F16_ERR 2.0e-3f          // >= |fp16 score - exact score|, derived above
typedef _Float16 h8v __attribute__((ext_vector_type(8)));

// one thread per (descriptor row, 32-dim half); grid (ceil(cap / 128), 2 [q | t], jobs)
__global__ __launch_bounds__(256) void k_bf_split16(const MatchDev *jobs, float scale_q)
{
    const MatchDev &J = jobs[blockIdx.z];
    const bool is_t = blockIdx.y == 1;
    const int n = is_t ? *J.nt_ptr : *J.nq_ptr;
    const int row = blockIdx.x * 128 + (threadIdx.x >> 1), half = threadIdx.x & 1;
    if (row >= n) return;
    const float *src = (is_t ? J.t : J.q) + (size_t)row * 64 + 32 * half;
    const float sc = is_t ? 1.f : scale_q;                      // queries carry the factor -2 (exact; |x| <= 2.0001, no overflow)
    float part = 0.f;
    h8v el[4];
#pragma unroll
    for (int d = 0; d < 32; d++) {
        const float x = src[d];
        part += x * x;
        el[d >> 3][d & 7] = (_Float16)(x * sc);                 // v_cvt_f16_f32: round to nearest even, subnormals kept
    }
    if (is_t) {
        h8v *tile = reinterpret_cast<h8v *>(J.t16) + (size_t)(row >> 5) * BF16_TILE;
        h8v *dst = tile + (row & 31) + 32 * half;
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++) dst[s4 * 64] = el[s4];
        // |t|^2: the f32 sum of the two halves (a + b == b + a: either thread holds the same value), behind the tile's fragments
        const float tot = part + __shfl_xor(part, 1, 64);
        if (half == 0) reinterpret_cast<float *>(tile + BF16_FRAGS * 64)[row & 31] = tot;
    } else {
        h8v *dst = reinterpret_cast<h8v *>(J.q16 + (size_t)row * BF16_ROW + 32 * half);
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++) dst[s4] = el[s4];
    }
}

// Two launches over the same four k-steps per tile, the first one starting from |t|^2, so both see the SAME scores (same
// instructions in the same order).  PASS 0 (bounds): a branch-free running (best, second best) per lane, written per (list, query);
// m2(q), the second best over all lists, is >= the second smallest fp16 score of the query.  PASS 1 (candidates): a train is listed
// when its score is <= thr(q) = m2(q) + 2 BFM_F16_ERR + BFM_MARGIN, known BEFORE the sweep -- a handful per query instead of the
// ~2 ln(n) records per list that a running threshold admits, so the append branch is almost never taken (one min3 tree + one ballot
// per accumulator decides).
// Superset: write S for exact scores, s for fp16 scores, |s - S| <= E = BFM_F16_ERR, and S2 / s2 for the second smallest of each
// over the trains.  The two trains of smallest s have S <= s2 + E, so S2 <= s2 + E.  The reference's float distances order the
// trains like S up to its own rounding, which BFM_MARGIN covers 40-fold: a train that can come out best or second best has
// S <= S2 + BFM_MARGIN, hence s <= S2 + BFM_MARGIN + E <= s2 + 2 E + BFM_MARGIN <= thr(q).  Every such train is listed; the verifier
// applies the same window around the s2 it reads back from the lists (they hold the two smallest scores, so that s2 is the true one).
// Pass 0 visits only every BFM_P0_STRIDE-th tile of a chunk, and its last: m2(q) is then the second smallest over a subset of the
// trains, hence still >= s2 -- thr(q) only grows, pass 1 lists more.
// (The split-bf16 form of rounds 2-6 -- hi.hi + hi.lo + lo.hi, 13 k-steps and nine fragments in pass 1 -- and its switch that skipped
//  the correction k-steps per tile, 8 % slower, are gone: profiles/r06_ab_bf_skip.txt)
#ifndef BFM_P0_STRIDE
#define BFM_P0_STRIDE 2           // 1, 2 or 4: pass 0 sweeps tiles tile0, tile0 + stride, ... and the chunk's last (profiles/r10_ab_bf_trim.txt)
#endif
#define BFM_WINDOW (2.f * BFM_F16_ERR + BFM_MARGIN)      // what a listed fp16 score may lie above the second-best fp16 score (superset argument above)
#define GASM __attribute__((address_space(1)))
typedef GASM const h8v *g_cs8v;
typedef float f2v __attribute__((ext_vector_type(2)));

#ifdef VFSMS_DESC_TIMING
// debug build: per-wave cycles of the filter sweeps, [pass][0 prologue, 1 barrier wait, 2 fetch issue, 3 LDS reads + MFMAs + minimum tree, 4 append, 5 whole kernel, 6 waves]
__device__ unsigned long long g_bf_cycles[2][8];
extern "C" int vfsms_debug_bf_cycles(unsigned long long *out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bf_cycles), sizeof(unsigned long long) * 16) == hipSuccess ? 0 : -3; }
#define BT_DECL unsigned long long _bt[5] = {0, 0, 0, 0, 0}, _bt0 = clock64(), _btl = _bt0
#define BT_MARK(ph) do { const unsigned long long _n = clock64(); _bt[ph] += _n - _btl; _btl = _n; } while (0)
#define BT_FLUSH(pass) do { if ((threadIdx.x & 63) == 0) { for (int _q = 0; _q < 5; _q++) atomicAdd(&g_bf_cycles[pass][_q], _bt[_q]); \
        atomicAdd(&g_bf_cycles[pass][5], clock64() - _bt0); atomicAdd(&g_bf_cycles[pass][6], 1ull); } } while (0)
#else
#define BT_DECL do {} while (0)
#define BT_MARK(ph) do {} while (0)
#define BT_FLUSH(pass) do {} while (0)
#endif
template <int PASS>
__global__ __launch_bounds__(256, 3) void k_bf_mfma16_d64(const MatchDev *jobs, int qblocks, int nsplit, int njobs)
{
    static_assert(BFM_P0_STRIDE == 1 || BFM_P0_STRIDE == 2 || BFM_P0_STRIDE == 4, "BFM_P0_STRIDE is 1, 2 or 4");
    // a (job, train chunk) and its 0.3 MB of split descriptors stay on one XCD (xcd_roi_map): every query block of the unit re-reads them
    unsigned unit, qb;
    xcd_roi_map(blockIdx.x, (unsigned)qblocks, (unsigned)(nsplit * njobs), unit, qb);
    const int sp = (int)(unit % (unsigned)nsplit);
    const MatchDev &J = jobs[unit / (unsigned)nsplit];
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if ((int)qb * 256 >= nq) return;                    // (whole workgroup)
    BT_DECL;
    const int q0 = ((int)qb * 4 + wave) * 64;
    const bool live = q0 < nq;                           // a wave beyond nq still stages train tiles and keeps the barriers
    const int ntiles = (nt + 31) >> 5;
    const int tchunk = (ntiles + nsplit - 1) / nsplit;
    const int tile0 = sp * tchunk, tile1 = min(ntiles, tile0 + tchunk);
    // the sweep's k-th tile: pass 1 takes every tile of the chunk; pass 0 every STRIDE-th and, whatever the stride, the last one -- no
    // tile twice ((nvis - 2) * STRIDE < tile1 - 1 - tile0), and a chunk of one or two tiles is swept whole, so a query has two scores
    // whenever it has two trains
    constexpr int STRIDE = PASS == 0 ? BFM_P0_STRIDE : 1;
    const int nvis = tile1 > tile0 ? (tile1 - tile0 - 1 + STRIDE - 1) / STRIDE + 1 : 0;
    auto tile_of = [&](int k) { return min(tile0 + k * STRIDE, tile1 - 1); };
    const int col = lane & 31, half = lane >> 5;
    // B operands (queries, resident): per 16-dim step s the lane's 8 values of dims 32*half + 8*s .. + 7
    h8v bh0[4], bh1[4];
    {
        g_cs8v p0 = (g_cs8v)(J.q16 + (size_t)min(q0 + col, nq - 1) * BF16_ROW + 32 * half);
        g_cs8v p1 = (g_cs8v)(J.q16 + (size_t)min(q0 + 32 + col, nq - 1) * BF16_ROW + 32 * half);
#pragma unroll
        for (int s4 = 0; s4 < 4; s4++) { bh0[s4] = p0[s4]; bh1[s4] = p1[s4]; }
    }
    // Train tiles go through LDS: the four waves of a workgroup sweep the SAME tiles (for different queries), so one cooperative
    // copy per tile replaces four sets of per-wave loads, and the operands arrive by ds_read_b128 instead of waiting on L2.  The
    // waves meet once per UNIT of BFM_UNIT tiles (they sit on four SIMDs, each shared with other workgroups: every meeting waits
    // for the slowest): two buffers of one unit each.
    constexpr int BFM_UNIT = 2;                          // train tiles per meeting (four in pass 0 -- twice the bytes in flight -- changed nothing)
    __shared__ h8v stage[2][BFM_UNIT][BF16_TILE];
    g_cs8v T = (g_cs8v)J.t16;                            // tile * BF16_TILE: four fragments of 64 lanes, then 32 f32 |t|^2 (k_bf_split16)
    // A tile is ONE lane-linear block in global memory (k_bf_split16 writes it in fragment order) and the same block in LDS, so the
    // copy is LDS-DMA: wave w issues global_load_lds_dwordx4 for the 1 KB fragment w, and lanes 0-7 of wave 0 one more for the 128
    // bytes of |t|^2 -- one or two instructions per tile and wave, no staging registers, no ds_write pass.  Unit u + 1 is requested
    // right behind the barrier that frees its buffer and has the whole of unit u's MFMAs to land.  (profiles/r06_glds_probe.txt: the
    // instruction takes 4-byte-aligned global addresses and partial EXEC, and writes LDS only for the lanes that are on.)
    const int wv_u = __builtin_amdgcn_readfirstlane(wave);
    auto glds16 = [&](g_cs8v src, const h8v *dst) {
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)src, (__attribute__((address_space(3))) void *)dst, 16, 0, 0);
    };
    const int nunits = (nvis + BFM_UNIT - 1) / BFM_UNIT;
    auto fetch = [&](int unit, int b) {
#pragma unroll
        for (int u = 0; u < BFM_UNIT; u++) {
            g_cs8v pn = T + (size_t)tile_of(min(unit * BFM_UNIT + u, nvis - 1)) * BF16_TILE;
            glds16(pn + 64 * wv_u + lane, &stage[b][u][64 * wv_u]);
            if (wv_u == 0 && lane < 8) glds16(pn + BF16_FRAGS * 64 + lane, &stage[b][u][BF16_FRAGS * 64]);
        }
    };
    if (nunits > 0) fetch(0, 0);
    // Pin the query operands as "defined here": the compiler otherwise carries their load waits into the tile loop as in-order
    // vmcnt counts, which also drain the train prefetch issued at the top of every iteration (a full L2 round trip per tile).
#pragma unroll
    for (int s4 = 0; s4 < 4; s4++) asm volatile("" : "+v"(bh0[s4]), "+v"(bh1[s4]));
    const bool va = q0 + col < nq, vb = q0 + 32 + col < nq;
    const size_t pitch = (size_t)J.capq;
    const int lst = sp * 2 + half, nl = 2 * nsplit;
    float m1a = INFINITY, m2a = INFINITY, m1b = INFINITY, m2b = INFINITY;       // PASS 0: running best / second best
    float thra = -INFINITY, thrb = -INFINITY;                                  // PASS 1: fixed thresholds (lanes beyond nq never append)
    int cnta = 0, cntb = 0;
    if (PASS == 1) {
        GASM const f2v *B = (GASM const f2v *)J.c_m12;
        float a1 = INFINITY, a2 = INFINITY, b1 = INFINITY, b2 = INFINITY;
        for (int L0 = 0; L0 < nl; L0 += 4) {                  // four lists per round trip (the loop was one dependent load per list)
            f2v ua[4], ub[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const size_t row = (size_t)min(L0 + k, nl - 1) * pitch;
                ua[k] = B[row + min(q0 + col, nq - 1)]; ub[k] = B[row + min(q0 + 32 + col, nq - 1)];
            }
#pragma unroll
            for (int k = 0; k < 4; k++) {
                if (L0 + k >= nl) break;
                a2 = fminf(fminf(a2, ua[k].y), fmaxf(a1, ua[k].x)); a1 = fminf(a1, ua[k].x);
                b2 = fminf(fminf(b2, ub[k].y), fmaxf(b1, ub[k].x)); b1 = fminf(b1, ub[k].x);
            }
        }
        if (va) thra = a2 + BFM_WINDOW;
        if (vb) thrb = b2 + BFM_WINDOW;
    }
    // (global address space: a generic pointer makes the append a flat_store, which the compiler orders behind every LDS-DMA in flight)
    GASM unsigned long long *lista = (GASM unsigned long long *)J.c_ent + (size_t)lst * BFM_CAPL * pitch + (q0 + col), *listb = lista + 32;   // uint2 (score bits, train) as one 64-bit word
    BT_MARK(0);
    for (int unit = 0; unit < nunits; unit++) {
        const int b = unit & 1;
        // this wave's LDS-DMA of the unit has landed (hipcc 7.2 does NOT put this wait in front of the barrier by itself: the ISA showed
        // `s_waitcnt lgkmcnt(0); s_barrier` only) -- behind the barrier every wave's has
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        BT_MARK(1);
        if (unit + 1 < nunits) fetch(unit + 1, b ^ 1);
        BT_MARK(2);
        if (!live) continue;
#pragma unroll
        for (int u = 0; u < BFM_UNIT; u++) {
            if (unit * BFM_UNIT + u >= nvis) break;
            const int tl = tile_of(unit * BFM_UNIT + u);
            const h8v *st = stage[b][u];
            // both accumulators of a lane hold the train rows 4 * half + (i & 3) + 8 * (i >> 2): one set of 16 |t|^2 (four ds_read_b128,
            // the same address across a lane half) starts both
            const float4 *tn = reinterpret_cast<const float4 *>(st + BF16_FRAGS * 64) + half;
            f16v cinit;
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const float4 n4 = tn[2 * j];
                cinit[4 * j] = n4.x; cinit[4 * j + 1] = n4.y; cinit[4 * j + 2] = n4.z; cinit[4 * j + 3] = n4.w;
            }
            const h8v at0 = st[lane];                // fragment s = the lane's dims 8s .. 8s + 7
            f16v acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(at0, bh0[0], cinit, 0, 0, 0);       // |t|^2 - 2 q.t, dims of k-step 0
            f16v acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(at0, bh1[0], cinit, 0, 0, 0);
#pragma unroll
            for (int s = 1; s < 4; s++) {
                const h8v at = st[s * 64 + lane];
                acc0 = __builtin_amdgcn_mfma_f32_32x32x16_f16(at, bh0[s], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x16_f16(at, bh1[s], acc1, 0, 0, 0);
            }
            if (tl * 32 + 31 >= nt) {                // train rows beyond nt never qualify (k_bf_split16 writes nothing for them)
#pragma unroll
                for (int i = 0; i < 16; i++) {
                    const bool past = tl * 32 + 4 * half + (i & 3) + 8 * (i >> 2) >= nt;
                    acc0[i] = past ? BFM_FAR : acc0[i]; acc1[i] = past ? BFM_FAR : acc1[i];
                }
            }
            if (PASS == 0) {
                // A lane's 16 scores of an accumulator belong to ONE query.  Only their minimum enters the running (best, second best): the
                // second smallest of a SUBSET of the scores (one per tile and lane) is >= the true second smallest, so thr(q) stays an upper
                // bound -- exact unless a query's two nearest trains share a tile and a lane half (15 / nt of the queries; pass 1 then lists a
                // few more candidates for them) -- and the sweep costs 11 VALU operations per accumulator instead of 48 (it was VALU-bound).
                float ta = fminf(fminf(acc0[0], acc0[1]), fminf(acc0[2], acc0[3])), tb = fminf(fminf(acc1[0], acc1[1]), fminf(acc1[2], acc1[3]));
#pragma unroll
                for (int i = 4; i < 16; i += 3) {
                    ta = fminf(ta, fminf(acc0[i], fminf(acc0[i + 1], acc0[i + 2])));
                    tb = fminf(tb, fminf(acc1[i], fminf(acc1[i + 1], acc1[i + 2])));
                }
                m2a = fminf(m2a, fmaxf(m1a, ta)); m1a = fminf(m1a, ta);
                m2b = fminf(m2b, fmaxf(m1b, tb)); m1b = fminf(m1b, tb);
            } else {
                const int row0 = tl * 32 + 4 * half;
#pragma unroll
                for (int h = 0; h < 2; h++) {
                    const f16v &acc = h == 0 ? acc0 : acc1;
                    const float thr = h == 0 ? thra : thrb;
                    // minima of the value groups {0..3}, {4..6}, {7..9}, {10..12}, {13..15}: the append walks only the groups that hold a hit
                    // (one or two values of the 16, as a rule), in ascending order -- the lists are the ones a full walk writes
                    float gm[5];
                    gm[0] = fminf(fminf(acc[0], acc[1]), fminf(acc[2], acc[3]));
#pragma unroll
                    for (int g = 1; g < 5; g++) gm[g] = fminf(acc[3 * g + 1], fminf(acc[3 * g + 2], acc[3 * g + 3]));
                    const float mn = fminf(fminf(gm[0], fminf(gm[1], gm[2])), fminf(gm[3], gm[4]));
                    const bool some = __any(mn <= thr);
                    BT_MARK(3);
                    if (some) {
                        GASM unsigned long long *list = h == 0 ? lista : listb;
                        int cnt = h == 0 ? cnta : cntb;
#pragma unroll
                        for (int g = 0; g < 5; g++) {
                            if (!__any(gm[g] <= thr)) continue;
#pragma unroll
                            for (int i = (g == 0 ? 0 : 3 * g + 1); i < (g == 0 ? 4 : 3 * g + 4); i++) {
                                const float v = acc[i];
                                if (v <= thr && v < 1e29f) {
                                    if (cnt < BFM_CAPL) list[cnt * pitch] = (unsigned long long)__float_as_uint(v) | ((unsigned long long)(unsigned)(row0 + (i & 3) + 8 * (i >> 2)) << 32);
                                    cnt++;
                                }
                            }
                        }
                        if (h == 0) cnta = cnt; else cntb = cnt;
                        BT_MARK(4);
                    }
                }
            }
            if (PASS == 0) BT_MARK(3);
        }
    }
    BT_FLUSH(PASS);
    if (PASS == 0) {
        GASM f2v *B = (GASM f2v *)J.c_m12;
        if (va) B[(size_t)lst * pitch + q0 + col] = f2v{m1a, m2a};
        if (vb) B[(size_t)lst * pitch + q0 + 32 + col] = f2v{m1b, m2b};
    } else {
        if (va) J.c_cnt[(size_t)lst * pitch + q0 + col] = cnta;
        if (vb) J.c_cnt[(size_t)lst * pitch + q0 + 32 + col] = cntb;
    }
}

// One THREAD per query (no cross-lane traffic; list reads are coalesced across the queries of a wave).  Sweep 1 takes
// the second smallest score S2 over the query's lists (the lists hold the true 2-NN, so S2 bounds their scores up to the
// MFMA rounding); sweep 2 parks the entries within `window` of S2 in a per-thread LDS column -- BFM_MARGIN for the f32 filter, whose
// scores are within ~1e-5 of the exact ones, BFM_WINDOW = 2 BFM_F16_ERR + BFM_MARGIN for the fp16 filter, whose listed scores carry
// their own error (superset argument at k_bf_mfma16_d64) --; the exact distances are then evaluated hit by hit, all lanes in step, with the arithmetic of k_bf_l2_d64 and
// the semantics of knn_update over ascending train indices (best = lowest index among the smallest sqrt-domain
// distances; second = next smallest value), which is order-independent in this form.
#define BFV_HITS 12
#ifdef VFSMS_DESC_TIMING
__device__ unsigned g_bfv_stats[4];        // debug build: [0] queries, [1] queries with an overflowed list, [2] list entries read, [3] exact evaluations
extern "C" int vfsms_debug_bfv_stats(unsigned *out) { return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_bfv_stats), sizeof(unsigned) * 4) == hipSuccess ? 0 : -3; }
#define BFV_STAT(i, v) atomicAdd(&g_bfv_stats[i], (unsigned)(v))
#else
#define BFV_STAT(i, v) do {} while (0)
#endif
__device__ __forceinline__ void bfv_exact(const float *__restrict__ Qr, const float *__restrict__ T, int idx, float &B1, float &B2, int &I1)
{
    const float4 *tr = reinterpret_cast<const float4 *>(T + (size_t)idx * 64);
    const float4 *qr = reinterpret_cast<const float4 *>(Qr);
    float acc = 0.f;
#pragma unroll
    for (int d4 = 0; d4 < 16; d4++) {
        const float4 tv = tr[d4], qv = qr[d4];
        const float e0 = qv.x - tv.x, e1 = qv.y - tv.y, e2 = qv.z - tv.z, e3 = qv.w - tv.w;
        acc += e0 * e0 + e1 * e1 + e2 * e2 + e3 * e3;
    }
    const float d = sqrtf(acc);
    if (d < B1 || (d == B1 && idx < I1)) { B2 = B1; B1 = d; I1 = idx; }
    else B2 = fminf(B2, d);
}

__global__ __launch_bounds__(256) void k_bf_verify_d64(const MatchDev *jobs, int cns, float window)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    if ((int)(blockIdx.x * 256) >= nq) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const bool live = q < nq;
    const int nl = 2 * cns;
    const size_t pitch = (size_t)J.capq;
    __shared__ int hits[BFV_HITS][256];
    float s1 = INFINITY, s2 = INFINITY; bool overflow = false;
    if (live)
        for (int L = 0; L < nl; L++) {
            const int c = J.c_cnt[(size_t)L * pitch + q];
            overflow = overflow || c > BFM_CAPL;
            BFV_STAT(2, min(c, BFM_CAPL));
            const uint2 *e = J.c_ent + (size_t)L * BFM_CAPL * pitch + q;
            for (int k = 0; k < min(c, BFM_CAPL); k++) {
                const float v = __uint_as_float(e[k * pitch].x);
                s2 = fminf(s2, fmaxf(s1, v));
                s1 = fminf(s1, v);
            }
        }
    const float cut = s2 + window;
    if (live) { BFV_STAT(0, 1); BFV_STAT(1, overflow ? 1 : 0); }
    const float *Qr = J.q + (size_t)min(q, nq - 1) * 64;
    float B1 = INFINITY, B2 = INFINITY; int I1 = -1;
    int nh = 0;
    if (live && !overflow)
        for (int L = 0; L < nl; L++) {
            const int c = min(J.c_cnt[(size_t)L * pitch + q], BFM_CAPL);
            const uint2 *e = J.c_ent + (size_t)L * BFM_CAPL * pitch + q;
            for (int k = 0; k < c; k++) {
                const uint2 ev = e[k * pitch];
                if (__uint_as_float(ev.x) <= cut) {
                    if (nh < BFV_HITS) hits[nh++][threadIdx.x] = (int)ev.y;
                    else bfv_exact(Qr, J.t, (int)ev.y, B1, B2, I1);      // more near-ties than slots: evaluate in place
                }
            }
        }
    if (live) BFV_STAT(3, nh);
    int maxh = nh;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) maxh = max(maxh, __shfl_xor(maxh, d, 64));
    for (int k = 0; k < maxh; k++)
        if (k < nh) bfv_exact(Qr, J.t, hits[k][threadIdx.x], B1, B2, I1);
    // A list overflowed (a query with dozens of trains inside the margin, e.g. an all-zero descriptor): exhaustive exact scan of
    // all trains for that query, shared by the 64 lanes of its wave and merged with the same first-index / second-value rule.
    {
        const int lane = threadIdx.x & 63;
        unsigned long long om = __ballot(live && overflow);
        while (om) {
            const int src = __ffsll((long long)om) - 1;
            om &= om - 1;
            const int qo = __shfl(q, src, 64);
            const float *Qo = J.q + (size_t)qo * 64;
            float b1 = INFINITY, b2 = INFINITY; int i1 = -1;
            for (int j = lane; j < nt; j += 64) bfv_exact(Qo, J.t, j, b1, b2, i1);
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) {
                const float ob1 = __shfl_xor(b1, d, 64), ob2 = __shfl_xor(b2, d, 64);
                const int oi1 = __shfl_xor(i1, d, 64);
                if (ob1 < b1 || (ob1 == b1 && oi1 >= 0 && (i1 < 0 || oi1 < i1))) { b2 = fminf(b1, ob2); b1 = ob1; i1 = oi1; }
                else b2 = fminf(b2, ob1);
            }
            if (lane == src) { B1 = b1; B2 = b2; I1 = i1; }
        }
    }
    if (live) { J.p_d1[q] = B1; J.p_d2[q] = B2; J.p_i1[q] = I1; }
}

// merge the per-split 2-NN lists, apply the ratio test (Python double arithmetic on float32 distances,
// ImageUtility.py:294) and compute the vote of ImageUtility.py:153-161 for surviving matches.
__global__ __launch_bounds__(256) void k_merge_ratio(const MatchDev *jobs, double ratio, int do_ratio)
{
    const MatchDev &J = jobs[blockIdx.y];
    // device-side counts are wave-uniform: pin them to SGPRs so loop bounds and train addresses stay scalar
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    float B1 = INFINITY, B2 = INFINITY; int I1 = -1;
    for (int s = 0; s < J.nsplit; s++) {
        const size_t o = (size_t)s * J.capq + q;
        float d = J.p_d1[o]; int i = J.p_i1[o];
        if (i >= 0) {
            if (d < B1) { B2 = B1; B1 = d; I1 = i; } else if (d < B2) { B2 = d; }
            float e = J.p_d2[o];
            if (e < B1) { B2 = B1; B1 = e; } else if (e < B2) { B2 = e; }
        }
    }
    J.d1[q] = B1; J.d2[q] = B2; J.i1[q] = I1;
    if (!do_ratio) return;
    int ok = (I1 >= 0) && (nt >= 2) && ((double)B1 < (double)B2 * ratio);
    int vote = 0;
    if (ok && J.kq) {
        // ptA = (kpsA[q][1], kpsA[q][0]); dx = int(ptA[0]-ptB[0]) (float32 subtract, trunc toward zero)
        float ay = J.kq[2 * q + 1], ax = J.kq[2 * q];
        float by = J.kt[2 * I1 + 1], bx = J.kt[2 * I1];
        int dx = (int)(ay - by), dy = (int)(ax - bx);
        vote = !(dx == 0 && dy == 0);
        J.votes[2 * (size_t)(J.capq + q)] = dx;             // staging area: second half of the votes buffer
        J.votes[2 * (size_t)(J.capq + q) + 1] = dy;
    }
    J.match_flag[q] = ok | (vote << 1);
}

__device__ __forceinline__ int wave_incl_scan_i(int v)
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        int n = __shfl_up(v, d, 64);
        if (lane >= d) v += n;
    }
    return v;
}

// order-preserving compaction of matches and of non-(0,0) votes: one 1024-thread workgroup per job
__global__ __launch_bounds__(1024) void k_match_scan(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.x];
    const int nq = *J.nq_ptr;
    __shared__ int wsum_m[16], wsum_v[16];
    __shared__ int carry_m, carry_v;
    if (threadIdx.x == 0) { carry_m = 0; carry_v = 0; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int base = 0; base < nq; base += 1024) {
        const int q = base + threadIdx.x;
        const int f = (q < nq) ? J.match_flag[q] : 0;
        const int fm = f & 1, fv = (f >> 1) & 1;
        const int im = wave_incl_scan_i(fm), iv = wave_incl_scan_i(fv);
        if (lane == 63) { wsum_m[wid] = im; wsum_v[wid] = iv; }
        __syncthreads();
        int om = carry_m, ov = carry_v;
        for (int k = 0; k < wid; k++) { om += wsum_m[k]; ov += wsum_v[k]; }
        if (fm && !J.pairs_given) {
            const int pos = om + im - 1;
            J.pairs[2 * (size_t)pos] = J.i1[q];              // (trainIdx, queryIdx)
            J.pairs[2 * (size_t)pos + 1] = q;
        }
        if (fv) {
            const int pos = ov + iv - 1;
            J.votes[2 * (size_t)pos] = J.votes[2 * (size_t)(J.capq + q)];
            J.votes[2 * (size_t)pos + 1] = J.votes[2 * (size_t)(J.capq + q) + 1];
        }
        __syncthreads();
        if (threadIdx.x == 1023) { carry_m = om + im; carry_v = ov + iv; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { J.mcount[0] = carry_m; J.mcount[1] = carry_v; J.mcount[2] = 0; J.mcount[3] = 0; }
}

// votes from an explicit (trainIdx, queryIdx) list (per-operator entry points vfsms_mode_offset, vfsms_consensus_offset)
__global__ __launch_bounds__(256) void k_votes_from_pairs(const MatchDev *jobs, int m)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const int tr = J.pairs[2 * k], q = J.pairs[2 * k + 1];
    float ay = J.kq[2 * q + 1], ax = J.kq[2 * q];
    float by = J.kt[2 * tr + 1], bx = J.kt[2 * tr];
    int dx = (int)(ay - by), dy = (int)(ax - bx);
    J.votes[2 * (size_t)(J.capq + k)] = dx;
    J.votes[2 * (size_t)(J.capq + k) + 1] = dy;
    J.match_flag[k] = 1 | ((!(dx == 0 && dy == 0)) << 1);
}

// Compaction + mode vote + result record of one job in ONE 1024-thread workgroup (round 2: k_match_scan + k_mode_count + k_mode_final): after the order-preserving compaction every vote (dx, dy) is inserted into an LDS hash table
// (linear probing on the packed 32-bit key; per slot a count and the smallest vote index), then the slots bid (count, -first index):
// the most frequent tuple, ties to the first inserted -- Method.getOffsetByMode's dict order + stable sort (ImageUtility.py:165-168) --
// in O(M) instead of the O(M^2) equality count (100 us per launch on SURF batches, 230 us on ORB's 5000 unconditional votes).
#define MODE_SLOTS 8192
#define MODE_HASH_MAX 5600         // votes per pass of the table (ORB votes 5000 times: one pass); more are dealt to several passes
// three uint32[8192] tables = 96 KB of static LDS: this kernel needs gfx950's 160 KB per CU (the library is gfx950-only: README, Makefile);
// a 64 KB-LDS target would have to shrink MODE_SLOTS and run more passes (MODE_HASH_MAX)
static_assert(3 * MODE_SLOTS * sizeof(uint32_t) <= 160 * 1024 - 16 * 1024, "k_scan_mode's hash tables are sized for the 160 KB LDS of gfx950");
__global__ __launch_bounds__(1024) void k_scan_mode(const MatchDev *jobs, int offset_evaluate)
{
    const MatchDev &J = jobs[blockIdx.x];
    const int nq = *J.nq_ptr;
    __shared__ int wsum_m[16], wsum_v[16];
    __shared__ int carry_m, carry_v;
    __shared__ uint32_t hkey[MODE_SLOTS], hcnt[MODE_SLOTS], hfirst[MODE_SLOTS];
    __shared__ unsigned long long best;
    if (threadIdx.x == 0) { carry_m = 0; carry_v = 0; best = 0ull; }
    for (int s = threadIdx.x; s < MODE_SLOTS; s += 1024) { hkey[s] = 0u; hcnt[s] = 0u; hfirst[s] = 0xFFFFFFFFu; }
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int base = 0; base < nq; base += 1024) {
        const int q = base + threadIdx.x;
        const int f = (q < nq) ? J.match_flag[q] : 0;
        const int fm = f & 1, fv = (f >> 1) & 1;
        const int im = wave_incl_scan_i(fm), iv = wave_incl_scan_i(fv);
        if (lane == 63) { wsum_m[wid] = im; wsum_v[wid] = iv; }
        __syncthreads();
        int om = carry_m, ov = carry_v;
        for (int k = 0; k < wid; k++) { om += wsum_m[k]; ov += wsum_v[k]; }
        if (fm && !J.pairs_given) {
            const int pos = om + im - 1;
            J.pairs[2 * (size_t)pos] = J.i1[q];              // (trainIdx, queryIdx)
            J.pairs[2 * (size_t)pos + 1] = q;
        }
        if (fv) {
            const int pos = ov + iv - 1;
            J.votes[2 * (size_t)pos] = J.votes[2 * (size_t)(J.capq + q)];
            J.votes[2 * (size_t)pos + 1] = J.votes[2 * (size_t)(J.capq + q) + 1];
        }
        __syncthreads();
        if (threadIdx.x == 1023) { carry_m = om + im; carry_v = ov + iv; }
        __syncthreads();
    }
    const int nm = carry_m, nv = carry_v;
    if (threadIdx.x == 0) { J.mcount[0] = nm; J.mcount[1] = nv; J.mcount[2] = 0; J.mcount[3] = 0; }
    __threadfence_block();
    __syncthreads();
    // insert: key = (dx + 32768) << 16 | (dy + 32768); offsets beyond +-32767 px cannot occur (tiles are <= 8192 px).
    // More votes than one table takes (configs[4]: 37 k keypoints per 819 x 4096 strip leave 6-9 k matches; round 4 sent those
    // through an O(M^2) equality count, 25 ms per launch): the votes are dealt to P passes by a second hash of the key -- equal tuples meet in
    // one pass, every pass fills a cleared table and bids (count, -first index) into `best`, so the winner is still the most frequent tuple,
    // ties to the first inserted (ImageUtility.py:165-168).
    const int P = (nv + MODE_HASH_MAX - 1) / MODE_HASH_MAX;
    for (int pass = 0; pass < P; pass++) {
        if (pass > 0) {
            __syncthreads();
            for (int s = threadIdx.x; s < MODE_SLOTS; s += 1024) { hkey[s] = 0u; hcnt[s] = 0u; hfirst[s] = 0xFFFFFFFFu; }
            __syncthreads();
        }
        for (int i = threadIdx.x; i < nv; i += 1024) {
            const int dx = J.votes[2 * (size_t)i], dy = J.votes[2 * (size_t)i + 1];
            const uint32_t key = ((uint32_t)(dx + 32768) << 16) | ((uint32_t)(dy + 32768) & 0xffffu);
            if (P > 1 && (int)(((key ^ (key >> 15)) * 0x9E3779B1u >> 8) % (uint32_t)P) != pass) continue;
            uint32_t h = (key * 2654435761u) >> 19;             // 13 bits
            for (;;) {
                const uint32_t old = atomicCAS(&hkey[h], 0u, key);
                if (old == 0u || old == key) { atomicAdd(&hcnt[h], 1u); atomicMin(&hfirst[h], (uint32_t)i); break; }
                h = (h + 1) & (MODE_SLOTS - 1);
            }
        }
        __syncthreads();
        unsigned long long mine = 0ull;
        for (int s = threadIdx.x; s < MODE_SLOTS; s += 1024)
            if (hcnt[s]) {
                const unsigned long long bid = ((unsigned long long)hcnt[s] << 32) | (unsigned long long)(0xFFFFFFFFu - hfirst[s]);
                mine = bid > mine ? bid : mine;
            }
        for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_down(mine, d, 64); mine = o > mine ? o : mine; }
        if (lane == 0 && mine) atomicMax(&best, mine);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int status = 0, dx = 0, dy = 0, votes = 0;
        if (nm > 0) {
            if (nv == 0) { votes = 1; }                      // dxList.append(0); dyList.append(0)
            else {
                votes = (int)(best >> 32);
                const unsigned idx = 0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull);
                dx = J.votes[2 * (size_t)idx]; dy = J.votes[2 * (size_t)idx + 1];
            }
            status = votes >= offset_evaluate;
        }
        *reinterpret_cast<unsigned long long *>(J.mcount + 2) = best;
        J.result[0] = status; J.result[1] = dx; J.result[2] = dy; J.result[3] = votes;
        J.result[4] = *J.nq_ptr; J.result[5] = *J.nt_ptr; J.result[6] = nm; J.result[7] = 0;
    }
}

// ---------------------------------------------------------------------------------------------------
// Hamming 1-NN for a batch of jobs + votes (BFMatcher("BruteForce-Hamming").match, ImageUtility.py:297-302)
// ---------------------------------------------------------------------------------------------------
// lanes own queries (8 dwords in VGPRs), trains stream through the scalar path like the L2 matcher
typedef const uint32_t __attribute__((address_space(4))) cu32c;
// trains are split over blockIdx.z (ascending ranges); per-split first minima land in p_d1 / p_i1 and are merged in split order
__global__ __launch_bounds__(256) void k_bf_hamming_jobs(const MatchDev *jobs)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int nq = __builtin_amdgcn_readfirstlane(*J.nq_ptr), nt = __builtin_amdgcn_readfirstlane(*J.nt_ptr);
    if ((int)(blockIdx.x * 256) >= nq) return;
    const int q = blockIdx.x * 256 + threadIdx.x;
    const uint32_t *pq = reinterpret_cast<const uint32_t *>(J.q) + (size_t)min(max(q, 0), nq - 1) * 8;
    uint32_t v[8];
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = pq[k];
    const int nsplit = gridDim.z, sp = blockIdx.z;
    const int chunk = (nt + nsplit - 1) / nsplit;
    const int t0 = sp * chunk, t1 = min(nt, t0 + chunk);
    int best = 0x7fffffff, bi = -1;
    cu32c *T = (cu32c *)(uintptr_t)J.t;
    for (int j = t0; j < t1; j++) {
        cu32c *tr = T + (size_t)j * 8;
        int d = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) d += __popc(v[k] ^ tr[k]);
        if (d < best) { best = d; bi = j; }              // first minimum wins
    }
    if (q >= nq) return;
    J.p_d1[(size_t)sp * J.capq + q] = (float)best; J.p_i1[(size_t)sp * J.capq + q] = bi;
}

__global__ __launch_bounds__(256) void k_hamming_merge(const MatchDev *jobs, int nsplit, int max_dist)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int nq = *J.nq_ptr;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    int best = 0x7fffffff, bi = -1;
    for (int s = 0; s < nsplit; s++) {
        const int i = J.p_i1[(size_t)s * J.capq + q];
        const int d = i >= 0 ? (int)J.p_d1[(size_t)s * J.capq + q] : 0x7fffffff;
        if (d < best) { best = d; bi = i; }              // splits are ascending train ranges: the first minimum still wins
    }
    J.i1[q] = bi; J.d1[q] = (float)best; J.d2[q] = 0.f;
    int ok = bi >= 0 && (max_dist < 0 || best < max_dist);
    int vote = 0;
    if (ok && J.kq) {
        float ay = J.kq[2 * q + 1], ax = J.kq[2 * q];
        float by = J.kt[2 * bi + 1], bx = J.kt[2 * bi];
        int dx = (int)(ay - by), dy = (int)(ax - bx);
        vote = !(dx == 0 && dy == 0);
        J.votes[2 * (size_t)(J.capq + q)] = dx;
        J.votes[2 * (size_t)(J.capq + q) + 1] = dy;
    }
    J.match_flag[q] = ok | (vote << 1);
}

// ---------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------
// The one place that knows a match job's device arrays: a counting walk gives their bytes, a carving walk the arrays (api.hip: match_run_layout)
void match_layout(ArenaWalk &a, MatchDev *m, int capq, int dim, int nsplit)
{
    m->capq = capq; m->dim = dim; m->nsplit = nsplit;
    m->p_d1 = a.take<float>((size_t)capq * nsplit);
    m->p_d2 = a.take<float>((size_t)capq * nsplit);
    m->p_i1 = a.take<int>((size_t)capq * nsplit);
    m->d1 = a.take<float>(capq);
    m->d2 = a.take<float>(capq);
    m->i1 = a.take<int>(capq);
    m->match_flag = a.take<int>(capq);
    m->match_pos = a.take<int>(capq);
    m->pairs = a.take<int32_t>(2 * (size_t)capq);
    m->votes = a.take<int32_t>(4 * (size_t)capq);
    m->mcount = a.take<int>(16);
    m->vsum = a.take<unsigned long long>(8);
    m->result = a.take<int32_t>(16);              // a run points the job at its row of the run's result block instead (api.hip)
}

// largest squared row norm of an n x 64 array (one wave per row): decides whether host-supplied descriptors qualify
// for the MFMA-filtered search, whose margin is absolute and assumes norms <= 1
__global__ __launch_bounds__(256) void k_max_norm2_d64(const float *a, int n, unsigned *out)
{
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float v = a[(size_t)row * 64 + lane];
    float s = v * v;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) atomicMax(out, __float_as_uint(s == s ? s : INFINITY));   // non-negative floats order like their bits; NaN -> inf
}

int launch_max_norm2_d64(vfsms_ctx *ctx, const float *a, int n, unsigned *d_out)
{
    if (n > 0) hipLaunchKernelGGL(k_max_norm2_d64, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, a, n, d_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// The device arrays of a job's MFMA candidate filter, likewise
void match_filter_layout(ArenaWalk &a, MatchDev *m, int capq, int capt, int cns)
{
    m->c_ent = a.take<uint2>((size_t)capq * cns * 2 * BFM_CAPL);
    m->c_cnt = a.take<int>((size_t)capq * cns * 2);
    m->q16 = a.take<unsigned short>(BF16_ROW * (size_t)capq);
    m->t16 = (unsigned short *)a.take<h8v>(BF16_TILE * ((size_t)capt / 32 + 1));      // whole 32-train tiles
    m->c_m12 = a.take<float2>((size_t)capq * cns * 2);
}

static bool bf_f32_filter()
{
    static const bool v = getenv("VFSMS_BF_F32FILTER") && atoi(getenv("VFSMS_BF_F32FILTER")) != 0;
    return v;
}

// MFMA-filtered exact 2-NN for 64-d descriptors of norm <= 1 (jobs of a filtered MatchPlan: nsplit == 1 plus match_filter_layout).
// Default: fp16 filter on the 16-bit matrix pipe; VFSMS_BF_F32FILTER=1 keeps round 1's f32-MFMA filter.
int launch_bf_l2_filtered(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int capt, int cns)
{
    if (njobs <= 0 || capq <= 0) return VFSMS_OK;
    {
        ProfScope ps(ctx, "bf_mfma");
        if (bf_f32_filter())
            hipLaunchKernelGGL(k_bf_mfma_d64, dim3((capq + 255) / 256, cns, njobs), dim3(256), 0, ctx->stream, d_jobs);
        else {
            hipLaunchKernelGGL(k_bf_split16, dim3((std::max(capq, capt) + 127) / 128, 2, njobs), dim3(256), 0, ctx->stream, d_jobs, -2.f);
            const int qblocks = (capq + 255) / 256;
            hipLaunchKernelGGL(k_bf_mfma16_d64<0>, dim3((unsigned)qblocks * cns * njobs), dim3(256), 0, ctx->stream, d_jobs, qblocks, cns, njobs);
            hipLaunchKernelGGL(k_bf_mfma16_d64<1>, dim3((unsigned)qblocks * cns * njobs), dim3(256), 0, ctx->stream, d_jobs, qblocks, cns, njobs);
        }
    }
    {
        ProfScope ps(ctx, "bf_verify");
        hipLaunchKernelGGL(k_bf_verify_d64, dim3((capq + 255) / 256, njobs), dim3(256), 0, ctx->stream, d_jobs, cns, bf_f32_filter() ? BFM_MARGIN : BFM_WINDOW);
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

int launch_bf_l2(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit, int dim)
{
    if (njobs <= 0 || capq <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "bf_l2");
    if (dim == 64) {
        hipLaunchKernelGGL(k_bf_l2_d64, dim3((capq + 511) / 512, nsplit, njobs), dim3(256), 0, ctx->stream, d_jobs);
    } else if (dim == 128) {
        hipLaunchKernelGGL(k_bf_l2_gen<128>, dim3((capq + 255) / 256, nsplit, njobs), dim3(256), 0, ctx->stream, d_jobs);
    } else if (dim == 32) {
        hipLaunchKernelGGL(k_bf_l2_gen<32>, dim3((capq + 255) / 256, nsplit, njobs), dim3(256), 0, ctx->stream, d_jobs);
    } else {
        vfsms_set_error("bf_l2: descriptor dim %d unsupported (64, 128, 32)", dim);
        return VFSMS_ERR_UNSUPPORTED;
    }
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

int launch_pack_i8_d128(vfsms_ctx *ctx, const PackJob *d_jobs, int njobs, int max_rows)
{
    if (njobs <= 0 || max_rows <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "pack_i8");
    hipLaunchKernelGGL(k_pack_i8_d128, dim3((max_rows + 63) / 64, njobs), dim3(256), 0, ctx->stream, d_jobs);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// integer 2-NN of jobs whose q8 / t8 / qn2 / tn2 were packed by k_pack_i8_d128 (jobs carved with the same nsplit)
int launch_bf_i8_d128(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit)
{
    if (njobs <= 0 || capq <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "bf_i8");
    hipLaunchKernelGGL(k_bf_i8_d128, dim3((capq + 255) / 256, nsplit, njobs), dim3(256), 0, ctx->stream, d_jobs);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// compaction + vote + result record.  Mode: one workgroup per job (k_scan_mode).  Consensus (Method.offsetCaculate = "ransac"):
// the same order-preserving compaction (k_match_scan), then support + pick (consensus_kernels.hip)
static int launch_vote_tail(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int estimator, int tol, int offset_evaluate)
{
    if (estimator == VFSMS_OFFSET_CONSENSUS) {
        hipLaunchKernelGGL(k_match_scan, dim3(njobs), dim3(1024), 0, ctx->stream, d_jobs);
        HIP_TRY(hipGetLastError());
        return launch_consensus(ctx, d_jobs, njobs, capq, tol, offset_evaluate);
    }
    hipLaunchKernelGGL(k_scan_mode, dim3(njobs), dim3(1024), 0, ctx->stream, d_jobs, offset_evaluate);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// the context's acceptance check behind the vote of the fused paths (vfsms_ctx_set_offset_verifier); off: nothing is launched
static int verify_tail(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs)
{
    if (ctx->offset_verifier != VFSMS_VERIFY_NCC) return VFSMS_OK;
    return launch_verify(ctx, d_jobs, njobs, ctx->verify_threshold, ctx->verify_min_pixels);
}

// The one tail behind every search, and behind pairs that were given (common.h: MatchTailKind); capq: the largest query set, or pair list
int launch_match_tail(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, const MatchTail &tail)
{
    if (njobs <= 0) return VFSMS_OK;
    const dim3 per_query((capq + 255) / 256, njobs);
    if (tail.kind == TAIL_VOTE) {
        {
            ProfScope ps(ctx, "vote");
            if (!tail.merged) hipLaunchKernelGGL(k_merge_ratio, per_query, dim3(256), 0, ctx->stream, d_jobs, tail.ratio, 1);
            TRY(launch_vote_tail(ctx, d_jobs, njobs, capq, ctx->offset_estimator, ctx->offset_tol, tail.offset_evaluate));
        }
        return verify_tail(ctx, d_jobs, njobs);
    }
    if (tail.kind == TAIL_GIVEN_PAIRS) {
        if (capq > 0) hipLaunchKernelGGL(k_votes_from_pairs, per_query, dim3(256), 0, ctx->stream, d_jobs, capq);
        return launch_vote_tail(ctx, d_jobs, njobs, capq, tail.estimator, tail.tol, tail.offset_evaluate);
    }
    const int pairs = tail.kind == TAIL_PAIRS;                // TAIL_KNN: the merge without the ratio test
    if (!tail.merged) hipLaunchKernelGGL(k_merge_ratio, per_query, dim3(256), 0, ctx->stream, d_jobs, tail.ratio, pairs);
    if (pairs) hipLaunchKernelGGL(k_match_scan, dim3(njobs), dim3(1024), 0, ctx->stream, d_jobs);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

// Hamming search over nsplit train ranges + merge of jobs carved with that nsplit: i1 / d1, match flags and (jobs with keypoints) votes
int launch_bf_hamming(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int nsplit, int max_dist)
{
    if (njobs <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "bf_hamming");
    hipLaunchKernelGGL(k_bf_hamming_jobs, dim3((capq + 255) / 256, njobs, nsplit), dim3(256), 0, ctx->stream, d_jobs);
    hipLaunchKernelGGL(k_hamming_merge, dim3((capq + 255) / 256, njobs), dim3(256), 0, ctx->stream, d_jobs, nsplit, max_dist);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
