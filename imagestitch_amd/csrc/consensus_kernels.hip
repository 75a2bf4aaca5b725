// consensus_kernels.hip -- the consensus offset estimator of Method.offsetCaculate = "ransac" for gfx950.
//
// Specification: tests/consensus_ref.py (the device equals it bit for bit).  A one-point translation model evaluated over EVERY
// hypothesis, so it is deterministic: the support of vote k is the number of votes j (the non-(0,0) votes the mode votes over, in match
// order) with |dx_j - dx_k| <= t and |dy_j - dy_k| <= t; the winner is the smallest k of largest support; the offset is the lower median
// of the winner's inliers, per axis.  At t = 0 this is Method.getOffsetByMode exactly (k_scan_mode).
//
// Runs after k_match_scan (match_kernels.hip), which compacted the votes to votes[0, 2 nv) and wrote mcount = {nm, nv}:
//   k_consensus_support  (hypothesis blocks x jobs) -> support[k] in the staging half of votes (free after the compaction)
//   k_consensus_pick     (one workgroup per job)    -> result[8] and mcount in k_scan_mode's layout
// Grids are sized by capacity and the counts are read on the device: no host synchronisation inside a batch.
#include "common.h"
#include <algorithm>

#define CONS_HYP 64          // hypotheses per workgroup: one per lane; the workgroup's four waves split the candidate votes between them
#define CONS_TILE 2048       // packed candidate votes per LDS tile (8 KB)

// k_scan_mode's key: (dx + 32768) << 16 | (dy + 32768).  Offsets beyond +-32767 px cannot occur (tiles are <= 8192 px).
__device__ __forceinline__ uint32_t cons_key(int dx, int dy)
{
    return ((uint32_t)(dx + 32768) << 16) | ((uint32_t)(dy + 32768) & 0xffffu);
}

// 1 when the packed vote lies in the window whose lower corner is (lx, ly) in key coordinates (non-short-circuit: no branch per key)
__device__ __forceinline__ int cons_hit(uint32_t key, int lx, int ly, uint32_t span)
{
    return (int)(((key >> 16) - (uint32_t)lx) <= span) & (int)(((key & 0xffffu) - (uint32_t)ly) <= span);
}

// O(nv^2) on purpose: exact for every nv with one code path (a hash would deal neighbouring tuples to different passes).  Every lane holds
// one hypothesis in registers; the job's votes stream through LDS as packed keys and every lane of a wave reads the same word (a
// broadcast, no bank conflicts).  The window test is two unsigned compares on the packed halves: (key_x - (x_k - t)) <= 2t.
__global__ __launch_bounds__(256) void k_consensus_support(const MatchDev *jobs, int tol)
{
    const MatchDev &J = jobs[blockIdx.y];
    const int nv = __builtin_amdgcn_readfirstlane(J.mcount[1]);
    __shared__ __attribute__((aligned(16))) uint32_t tile[CONS_TILE];
    __shared__ int part[4][CONS_HYP];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int2 *votes = reinterpret_cast<const int2 *>(J.votes);
    int *support = J.votes + 2 * (size_t)J.capq;
    const uint32_t span = 2u * (uint32_t)tol;
    for (int h0 = blockIdx.x * CONS_HYP; h0 < nv; h0 += gridDim.x * CONS_HYP) {
        const int k = h0 + lane;
        int lx = 0, ly = 0;                               // lower window corner in key coordinates; lanes past nv count nothing they keep
        if (k < nv) { const int2 v = votes[k]; lx = v.x + 32768 - tol; ly = v.y + 32768 - tol; }
        int cnt = 0;
        for (int base = 0; base < nv; base += CONS_TILE) {
            const int n = min(CONS_TILE, nv - base), n16 = (n + 15) & ~15;
            __syncthreads();                                // the previous tile is consumed
            for (int i = threadIdx.x; i < n16; i += 256) {
                // key 0 is (-32768, -32768): outside every window of a representable vote, so it pads the tile to whole uint4 quarters
                uint32_t key = 0u;
                if (i < n) { const int2 v = votes[base + i]; key = cons_key(v.x, v.y); }
                tile[i] = key;
            }
            __syncthreads();
            const int q4 = n16 >> 4;                         // uint4 words per wave
            const uint4 *t4 = reinterpret_cast<const uint4 *>(tile) + wid * q4;
            for (int i = 0; i < q4; i++) {
                const uint4 w = t4[i];
                cnt += cons_hit(w.x, lx, ly, span) + cons_hit(w.y, lx, ly, span) + cons_hit(w.z, lx, ly, span) + cons_hit(w.w, lx, ly, span);
            }
        }
        part[wid][lane] = cnt;
        __syncthreads();
        if (wid == 0 && k < nv) support[k] = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    }
}

// winner by bid (support << 32) | ~k (largest support, then smallest k) -- wave reduction + LDS atomicMax -- then 2t + 1-bin LDS
// histograms of the winner's inliers per axis give the lower medians (element (n - 1) / 2 of the ascending inliers) exactly.
__global__ __launch_bounds__(1024) void k_consensus_pick(const MatchDev *jobs, int tol, int offset_evaluate)
{
    const MatchDev &J = jobs[blockIdx.x];
    const int nm = J.mcount[0], nv = J.mcount[1];
    const int2 *votes = reinterpret_cast<const int2 *>(J.votes);
    const int *support = J.votes + 2 * (size_t)J.capq;
    __shared__ unsigned long long best;
    __shared__ int hx[2 * VFSMS_CONSENSUS_MAX_TOL + 1], hy[2 * VFSMS_CONSENSUS_MAX_TOL + 1];
    const int nb = 2 * tol + 1, lane = threadIdx.x & 63;
    if (threadIdx.x == 0) best = 0ull;
    for (int b = threadIdx.x; b < nb; b += 1024) { hx[b] = 0; hy[b] = 0; }
    __syncthreads();
    unsigned long long mine = 0ull;
    for (int k = threadIdx.x; k < nv; k += 1024) {
        const unsigned long long bid = ((unsigned long long)(uint32_t)support[k] << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)k);
        mine = bid > mine ? bid : mine;
    }
    for (int d = 32; d > 0; d >>= 1) { const unsigned long long o = __shfl_down(mine, d, 64); mine = o > mine ? o : mine; }
    if (lane == 0 && mine) atomicMax(&best, mine);
    __syncthreads();
    const unsigned long long win = best;
    int cx = 0, cy = 0;
    if (nv > 0) { const int2 v = votes[0xFFFFFFFFu - (uint32_t)(win & 0xFFFFFFFFull)]; cx = v.x; cy = v.y; }
    for (int k = threadIdx.x; k < nv; k += 1024) {
        const int2 v = votes[k];
        const int ex = v.x - cx + tol, ey = v.y - cy + tol;
        if ((uint32_t)ex < (uint32_t)nb && (uint32_t)ey < (uint32_t)nb) { atomicAdd(&hx[ex], 1); atomicAdd(&hy[ey], 1); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int status = 0, dx = 0, dy = 0, count = 0;
        if (nm > 0) {
            if (nv == 0) { count = 1; }                      // the mode's dxList.append(0); dyList.append(0)
            else {
                count = (int)(win >> 32);                    // = the inliers the histograms hold
                const int r = (count - 1) / 2;
                int b = 0, c = 0;
                for (; b < nb; b++) { c += hx[b]; if (c > r) break; }
                dx = cx - tol + b;
                for (b = 0, c = 0; b < nb; b++) { c += hy[b]; if (c > r) break; }
                dy = cy - tol + b;
            }
            status = count >= offset_evaluate;
        }
        J.mcount[0] = nm; J.mcount[1] = nv;
        *reinterpret_cast<unsigned long long *>(J.mcount + 2) = win;
        J.result[0] = status; J.result[1] = dx; J.result[2] = dy; J.result[3] = count;
        J.result[4] = *J.nq_ptr; J.result[5] = *J.nt_ptr; J.result[6] = nm; J.result[7] = 0;
    }
}

// support + pick of njobs jobs whose votes k_match_scan has compacted.  The support grid is capacity-sized (capq >= every job's nv) and
// capped by job count so that a large batch does not launch hypothesis blocks no job can fill; the blocks stride over the hypotheses.
int launch_consensus(vfsms_ctx *ctx, const MatchDev *d_jobs, int njobs, int capq, int tol, int offset_evaluate)
{
    if (njobs <= 0) return VFSMS_OK;
    if (tol < 0 || tol > VFSMS_CONSENSUS_MAX_TOL) { vfsms_set_error("consensus: tolerance %d outside 0..%d", tol, VFSMS_CONSENSUS_MAX_TOL); return VFSMS_ERR_BAD_ARG; }
    const int need = std::max(1, (capq + CONS_HYP - 1) / CONS_HYP);
    const int gx = std::min(need, std::max(4, 4096 / njobs));
    hipLaunchKernelGGL(k_consensus_support, dim3(gx, njobs), dim3(256), 0, ctx->stream, d_jobs, tol);
    hipLaunchKernelGGL(k_consensus_pick, dim3(njobs), dim3(1024), 0, ctx->stream, d_jobs, tol, offset_evaluate);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
