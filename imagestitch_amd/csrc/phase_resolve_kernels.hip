// phase_resolve_kernels.hip -- Stitcher.phaseResolve = "ncc" for gfx950: the K largest peaks of the FP64 correlation surface of
// phase_kernels.hip, every circular reading of each scored by the overlap correlation of verify_kernels.hip, the best one kept.
//
// Specification: tests/phase_resolve_ref.py.  The device's transforms round differently from pocketfft, so the peak LIST equals the
// reference's where the reference's own peak values are a relative gap apart; everything behind the list is integer sums and the fixed
// float64 tail of verify_math.h, and equals the reference bit for bit.
//
//   k_phase_peaks        (row blocks x jobs)   -> per-block top-K lists of the peaks of PEAK_ROWS stored rows (+ one halo row above and below,
//                                                 circular); the surface is read once from HBM but for those two rows, every load coalesced
//   k_phase_peaks_merge  (one wave per job)    -> the job's K peaks {value, row-major index in the ORIGINAL orientation} (a tail kernel: no
//                                                 hand-off between workgroups inside a launch)
//   k_phase_cand_sums    (row blocks x 4 K x jobs) -> Sa, Sb, Saa, Sbb, Sab of every kept reading over the RAW u8 strips; the row body is
//                                                 k_verify_ncc's (overlap_rows_sums of overlap_sums.h)
//   k_phase_cand_pick    (one lane per job)    -> scores, the winner, the attempt row, the candidate table, the peak positions
// All on the context's stream, no host synchronisation; scratch from the arena; profiler stage "phase_resolve".
#include "common.h"
#include "overlap_sums.h"
#include "phase_resolve_math.h"
#include <algorithm>

#define PEAK_ROWS 16          // stored rows of a k_phase_peaks workgroup: 18 rows read for 16 (12 % over one pass)
#define PEAK_T 256
#define PR_K VFSMS_PHASE_MAX_PEAKS

// the order of the peak list: value descending, then index ascending; an absent record (idx < 0) comes last
__device__ __forceinline__ bool peak_before(const PhasePeak &a, const PhasePeak &b)
{
    if (a.idx < 0) return false;
    if (b.idx < 0) return true;
    return a.v > b.v || (a.v == b.v && a.idx < b.idx);
}

// a sorted list of PR_K records in registers (every index is a compile-time constant after unrolling)
struct PeakList {
    PhasePeak e[PR_K];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int i = 0; i < PR_K; i++) { e[i].v = 0.0; e[i].idx = -1; }
    }
    __device__ __forceinline__ void insert(PhasePeak c)
    {
        if (!peak_before(c, e[PR_K - 1])) return;
#pragma unroll
        for (int i = 0; i < PR_K; i++)
            if (peak_before(c, e[i])) { const PhasePeak t = e[i]; e[i] = c; c = t; }
    }
    __device__ __forceinline__ void pop()
    {
#pragma unroll
        for (int i = 0; i + 1 < PR_K; i++) e[i] = e[i + 1];
        e[PR_K - 1].v = 0.0; e[PR_K - 1].idx = -1;
    }
};

__device__ __forceinline__ PhasePeak wave_first(PhasePeak p)
{
    for (int d = 32; d > 0; d >>= 1) {
        PhasePeak o;
        o.v = __shfl_xor(p.v, d, 64); o.idx = __shfl_xor(p.idx, d, 64);
        if (peak_before(o, p)) p = o;
    }
    return p;                                             // the same record on every lane
}

// RE: the planes of a chunk as k_phase_rows_inv / rocFFT's inverse leave them: job j at RE + j SM SN, stored row-major SM x SN.  tr: the planes
// hold the transposed problem (stored row = original column), so element (sr, sc) is original (sc, sr) and the original surface is SN x SM.
// The eight circular neighbours of an element are the same set in both orientations; what differs is which of them PRECEDE it in the
// original's row-major order, so every index is formed in the original orientation.
__global__ __launch_bounds__(PEAK_T) void k_phase_peaks(const double *__restrict__ RE, int SM, int SN, int tr, int K, PhasePeak *__restrict__ partial)
{
    const double *R = RE + (size_t)blockIdx.y * SM * SN;
    const int y0 = blockIdx.x * PEAK_ROWS;
    const int rows = min(PEAK_ROWS, SM - y0);
    const long long oN = tr ? SM : SN;                    // row length of the original surface
    PeakList L; L.clear();
    for (int x = threadIdx.x; x < SN; x += PEAK_T) {
        const int xl = x == 0 ? SN - 1 : x - 1, xr = x == SN - 1 ? 0 : x + 1;
        int yu = y0 == 0 ? SM - 1 : y0 - 1;               // the stored row above the current one
        const double *pu = R + (size_t)yu * SN, *pc = R + (size_t)y0 * SN;
        double u0 = pu[xl], u1 = pu[x], u2 = pu[xr];
        double c0 = pc[xl], c1 = pc[x], c2 = pc[xr];
        for (int r = 0; r < rows; r++) {
            const int y = y0 + r, yd = y == SM - 1 ? 0 : y + 1;
            const double *pd = R + (size_t)yd * SN;
            const double d0 = pd[xl], d1 = pd[x], d2 = pd[xr];
            const double v = c1;
            if (v >= u0 && v >= u1 && v >= u2 && v >= c0 && v >= c2 && v >= d0 && v >= d1 && v >= d2) {
                const long long ip = tr ? (long long)x * oN + y : (long long)y * oN + x;
                // strictly greater than the neighbours of smaller original index (a neighbour that IS the element, in a surface of one or
                // two rows or columns, has the same index and passes)
                const int ys[3] = {yu, y, yd}, xs[3] = {xl, x, xr};
                const double nb[3][3] = {{u0, u1, u2}, {c0, c1, c2}, {d0, d1, d2}};
                bool ok = true;
#pragma unroll
                for (int i = 0; i < 3; i++)
#pragma unroll
                    for (int j = 0; j < 3; j++) {
                        const long long iq = tr ? (long long)xs[j] * oN + ys[i] : (long long)ys[i] * oN + xs[j];
                        if (iq < ip && !(v > nb[i][j])) ok = false;
                    }
                if (ok) { PhasePeak c; c.v = v; c.idx = ip; L.insert(c); }
            }
            u0 = c0; u1 = c1; u2 = c2; c0 = d0; c1 = d1; c2 = d2; yu = y;
        }
    }
    // K rounds: the first record of the workgroup among the heads of the threads' lists; its owner pops it
    __shared__ PhasePeak sm[PEAK_T / 64];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    PhasePeak *out = partial + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * K;
    for (int k = 0; k < K; k++) {
        const PhasePeak w = wave_first(L.e[0]);
        if (lane == 0) sm[wid] = w;
        __syncthreads();
        PhasePeak b = sm[0];
#pragma unroll
        for (int q = 1; q < PEAK_T / 64; q++) if (peak_before(sm[q], b)) b = sm[q];
        if (b.idx >= 0 && L.e[0].idx == b.idx) L.pop();   // indices are unique: exactly one owner
        if (threadIdx.x == 0) out[k] = b;
        __syncthreads();
    }
}

// partial: [job][nblk][K] -> peaks: [job][K]
__global__ __launch_bounds__(64) void k_phase_peaks_merge(const PhasePeak *__restrict__ partial, int nblk, int K, PhasePeak *__restrict__ peaks)
{
    const PhasePeak *P = partial + (size_t)blockIdx.x * nblk * K;
    PeakList L; L.clear();
    for (int e = threadIdx.x; e < nblk * K; e += 64) L.insert(P[e]);
    for (int k = 0; k < K; k++) {
        const PhasePeak b = wave_first(L.e[0]);
        if (b.idx >= 0 && L.e[0].idx == b.idx) L.pop();
        if (threadIdx.x == 0) peaks[(size_t)blockIdx.x * K + k] = b;
    }
}

int launch_phase_peaks(vfsms_ctx *ctx, const double *RE, int njobs, int SM, int SN, int tr, int K, PhasePeak *partial, PhasePeak *peaks)
{
    if (njobs <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "phase_resolve");
    const int nblk = phase_peaks_blocks(SM);
    hipLaunchKernelGGL(k_phase_peaks, dim3(nblk, njobs), dim3(PEAK_T), 0, ctx->stream, RE, SM, SN, tr, K, partial);
    hipLaunchKernelGGL(k_phase_peaks_merge, dim3(njobs), dim3(64), 0, ctx->stream, (const PhasePeak *)partial, nblk, K, peaks);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
int phase_peaks_blocks(int SM) { return (SM + PEAK_ROWS - 1) / PEAK_ROWS; }

// ---- the candidates' sums ------------------------------------------------------------------------------------------------------------
#define CAND_WG 32           // row blocks per candidate at most: 128 waves, a wave per overlap row

// grid (row blocks, 4 K candidates, jobs).  A wave per overlap row (overlap_rows_sums).  sums: [job][4 K][5] uint64, zeroed by the launcher.
__global__ __launch_bounds__(256) void k_phase_cand_sums(const PhaseJobHost *__restrict__ jobs, const PhasePeak *__restrict__ peaks, int K, int oM, int oN,
                                                          int h, int w, unsigned long long *__restrict__ sums)
{
    const int job = blockIdx.z, cand = blockIdx.y;
    const long long pidx = peaks[(size_t)job * K + (cand >> 2)].idx;
    const PhaseCand C = phase_candidate(pidx, cand & 3, oM, oN, h, w);
    if (!C.kept) return;
    const int dx = __builtin_amdgcn_readfirstlane(C.dx), dy = __builtin_amdgcn_readfirstlane(C.dy);
    const Overlap o = verify_overlap(h, w, dx, dy);
    if (o.r1 <= o.r0 || o.c1 <= o.c0) return;
    const PhaseJobHost J = jobs[job];
    overlap_rows_sums(J.a, J.sa, J.b, J.sb, o, dx, dy, sums + ((size_t)job * 4 * K + cand) * 5);
}

// rows: [job][VFSMS_ATTEMPT_INTS]; cands: [job][4 K][4] = {dx, dy, fixed score, shared pixels}; peaks_out: [job][K][2] = {uy, ux}
__global__ __launch_bounds__(64) void k_phase_cand_pick(const PhasePeak *__restrict__ peaks, int njobs, int K, int oM, int oN, int h, int w,
                                                         const unsigned long long *__restrict__ sums, double threshold, int min_pixels,
                                                         int32_t *__restrict__ rows, int32_t *__restrict__ cands, int32_t *__restrict__ peaks_out)
{
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j >= njobs) return;
    int best = -1, bdx = 0, bdy = 0, bfx = 0;
    double bscore = 0.0;
    for (int c = 0; c < 4 * K; c++) {
        const long long pidx = peaks[(size_t)j * K + (c >> 2)].idx;
        const PhaseCand C = phase_candidate(pidx, c & 3, oM, oN, h, w);
        int32_t *o = cands + ((size_t)j * 4 * K + c) * 4;
        if ((c & 3) == 0) {
            int32_t *po = peaks_out + ((size_t)j * K + (c >> 2)) * 2;
            po[0] = C.present ? (int)(pidx / oN) : -1;
            po[1] = C.present ? (int)(pidx % oN) : -1;
        }
        o[0] = C.dx; o[1] = C.dy; o[2] = 0; o[3] = 0;
        if (!C.kept) continue;
        long long N;
        const double score = overlap_score(h, w, C.dx, C.dy, sums + ((size_t)j * 4 * K + c) * 5, min_pixels, &N);
        const int fx = verify_fixed(score);
        o[2] = fx; o[3] = (int32_t)N;
        if (best < 0 || score > bscore) { best = c; bscore = score; bdx = C.dx; bdy = C.dy; bfx = fx; }
    }
    int32_t *r = rows + (size_t)j * VFSMS_ATTEMPT_INTS;
    r[0] = (best >= 0 && bscore >= threshold) ? 1 : 0;
    r[1] = bdx; r[2] = bdy; r[3] = 0; r[4] = 1; r[5] = 1; r[6] = best >= 0 ? best : 0; r[7] = bfx;
}

size_t phase_resolve_sums_bytes(int njobs, int K) { return sizeof(unsigned long long) * 5 * 4 * (size_t)K * (size_t)njobs; }

// njobs jobs of one strip shape h x w whose peaks (original surface oM x oN) are on the device; d_jobs: their strips
int launch_phase_resolve(vfsms_ctx *ctx, const PhaseJobHost *d_jobs, const PhasePeak *d_peaks, int njobs, int K, int oM, int oN, int h, int w,
                         double threshold, int min_pixels, unsigned long long *d_sums, int32_t *d_rows, int32_t *d_cands, int32_t *d_peaks_out)
{
    if (njobs <= 0) return VFSMS_OK;
    ProfScope ps(ctx, "phase_resolve");
    HIP_TRY(hipMemsetAsync(d_sums, 0, phase_resolve_sums_bytes(njobs, K), ctx->stream));
    const int part = 16384;                               // jobs per launch (grid z holds 65535)
    const int gx = std::max(1, std::min(CAND_WG, (std::max(h, 1) + 3) / 4));
    for (int k0 = 0; k0 < njobs; k0 += part) {
        const int c = std::min(part, njobs - k0);
        hipLaunchKernelGGL(k_phase_cand_sums, dim3(gx, 4 * K, c), dim3(256), 0, ctx->stream, d_jobs + k0, d_peaks + (size_t)k0 * K, K, oM, oN, h, w,
                           d_sums + (size_t)k0 * 4 * K * 5);
    }
    hipLaunchKernelGGL(k_phase_cand_pick, dim3((njobs + 63) / 64), dim3(64), 0, ctx->stream, d_peaks, njobs, K, oM, oN, h, w,
                       (const unsigned long long *)d_sums, threshold, min_pixels, d_rows, d_cands, d_peaks_out);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
