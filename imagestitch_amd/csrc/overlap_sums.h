// overlap_sums.h -- the device parts shared by the kernels that sum over the pixels two images share under an offset: verify_kernels.hip,
// phase_resolve_kernels.hip (both: a wave per overlap row, overlap_rows_sums), adjust_kernels.hip and exposure_kernels.hip (both: 16-byte
// chunks of B rows with column masks; byte_mask, range_bits, load_partner).  All four end in wg_add_u64.  Every sum is an exact integer,
// so the reduction order is free; what turns sums into a score is in verify_math.h.
#pragma once
#include "verify_math.h"

// ---- a workgroup's sums -> memory --------------------------------------------------------------------------------------------------------
// v: NQ 64-bit lane sums of a workgroup of NWAVES waves, which reaches this call as a whole.  Shuffle down, lane 0 to LDS, one barrier, then
// thread q < nlive adds the waves' sums of v[q] and issues ONE atomic add to dst[q] -- none when the sum is 0 (dst starts cleared).
// The LDS array is the helper's: one call per kernel.
template <int NQ, int NWAVES>
__device__ __forceinline__ void wg_add_u64(const unsigned long long (&v)[NQ], unsigned long long *dst, int nlive = NQ)
{
    __shared__ unsigned long long part[NWAVES][NQ];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        unsigned long long x = v[q];
        for (int d = 32; d > 0; d >>= 1) x += __shfl_down(x, d, 64);
        if (lane == 0) part[wid][q] = x;
    }
    __syncthreads();
    if ((int)threadIdx.x < nlive) {
        unsigned long long x = 0ull;
#pragma unroll
        for (int k = 0; k < NWAVES; k++) x += part[k][threadIdx.x];
        if (x) atomicAdd(dst + threadIdx.x, x);
    }
}

// ---- the five sums, four byte pairs at a time ----------------------------------------------------------------------------------------------
struct Sums5 { uint32_t a, b, aa, bb, ab; };
__device__ __forceinline__ void acc4(uint32_t a, uint32_t b, Sums5 &s)
{
    s.a = __builtin_amdgcn_sad_u8(a, 0u, s.a);
    s.b = __builtin_amdgcn_sad_u8(b, 0u, s.b);
    s.aa = __builtin_amdgcn_udot4(a, a, s.aa, false);
    s.bb = __builtin_amdgcn_udot4(b, b, s.bb, false);
    s.ab = __builtin_amdgcn_udot4(a, b, s.ab, false);
}

// ---- a wave per overlap row --------------------------------------------------------------------------------------------------------------
// Sa, Sb, Saa, Sbb, Sab over the overlap o = verify_overlap(h, w, dx, dy) (not empty) of strips A and B (strides sa, sb), added to out5[0..4].
// For a workgroup of 4 waves; blockIdx.x of gridDim.x row blocks share the rows.  Strip B's row is cut at its 16-byte boundaries: the body
// is read as aligned uint4, the partner bytes of strip A (shifted by dy and by the strips' own column offsets inside their tiles, so at any
// byte alignment) as the five aligned dwords around them, funnel-shifted into place; heads and tails (< 16 bytes each) are single bytes on
// the first lanes.  Per-row sums are 32-bit (a lane sees at most w / 64 + 30 pixels of a row: 65025 * 158 at w = 8192), the running sums 64-bit.
__device__ __forceinline__ void overlap_rows_sums(const uint8_t *A, int sa, const uint8_t *B, int sb, Overlap o, int dx, int dy, unsigned long long *out5)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int L = o.c1 - o.c0;
    unsigned long long t[5] = {0ull, 0ull, 0ull, 0ull, 0ull};
    for (int r = o.r0 + (int)blockIdx.x * 4 + wid; r < o.r1; r += (int)gridDim.x * 4) {
        const uint8_t *pb = B + (size_t)r * sb + o.c0;
        const uint8_t *pa = A + (size_t)(r + dx) * sa + (o.c0 + dy);
        const int head = min(L, (int)((16u - (unsigned)((uintptr_t)pb & 15u)) & 15u));
        const int nb = (L - head) >> 4, tail = L - head - (nb << 4);
        Sums5 s = {0u, 0u, 0u, 0u, 0u};
        const unsigned m = (unsigned)((uintptr_t)(pa + head) & 3u);          // the same for every chunk of the row
        for (int k = lane; k < nb; k += 64) {
            const uint4 b = *reinterpret_cast<const uint4 *>(pb + head + 16 * (size_t)k);
            const uint32_t *a4 = reinterpret_cast<const uint32_t *>(pa + head + 16 * (size_t)k - m);
            const uint32_t d0 = a4[0], d1 = a4[1], d2 = a4[2], d3 = a4[3], d4 = m ? a4[4] : 0u;   // a4[4] holds bytes of the chunk when m != 0
            acc4(__builtin_amdgcn_alignbyte(d1, d0, m), b.x, s);
            acc4(__builtin_amdgcn_alignbyte(d2, d1, m), b.y, s);
            acc4(__builtin_amdgcn_alignbyte(d3, d2, m), b.z, s);
            acc4(__builtin_amdgcn_alignbyte(d4, d3, m), b.w, s);
        }
        int e = -1;                                       // head byte `lane`, tail byte `lane - 32`
        if (lane < head) e = lane;
        else if (lane >= 32 && lane - 32 < tail) e = head + (nb << 4) + lane - 32;
        if (e >= 0) acc4((uint32_t)pa[e], (uint32_t)pb[e], s);
        t[0] += s.a; t[1] += s.b; t[2] += s.aa; t[3] += s.bb; t[4] += s.ab;
    }
    wg_add_u64<5, 4>(t, out5);
}

// ---- 16-byte chunks with column masks ------------------------------------------------------------------------------------------------------
// bit b of a nibble -> byte b of a dword (0xff / 0x00)
__device__ __forceinline__ uint32_t byte_mask(uint32_t nib) { return ((nib * 0x00204081u) & 0x01010101u) * 0xffu; }
// the bits p of [0, n) whose column x0 + p lies in [c0, c1)
__device__ __forceinline__ uint32_t range_bits(int x0, int c0, int c1, int n)
{
    const int lo = min(max(c0 - x0, 0), n), hi = min(max(c1 - x0, 0), n);
    return hi > lo ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
}
// The 4 NQ bytes of a row of A from address `pa` on as NQ dwords: the NQ + 1 aligned dwords around them, funnel-shifted by pa's alignment.
// `ca` is the column of pa[0], the row's columns are [0, w) (a caller that needs fewer bytes passes the end of what it needs for w); an
// aligned dword is loaded only when it holds at least one of them, else it reads as 0 -- so no load leaves the page of a valid byte.
template <int NQ>
__device__ __forceinline__ void load_partner(uintptr_t pa, int ca, int w, uint32_t e[NQ])
{
    const unsigned m = (unsigned)(pa & 3u);
    const uint32_t *a4 = reinterpret_cast<const uint32_t *>(pa - m);
    const int cq = ca - (int)m;
    uint32_t d[NQ + 1];
#pragma unroll
    for (int q = 0; q < NQ + 1; q++) d[q] = (cq + 4 * q + 3 >= 0 && cq + 4 * q < w) ? a4[q] : 0u;
#pragma unroll
    for (int q = 0; q < NQ; q++) e[q] = __builtin_amdgcn_alignbyte(d[q + 1], d[q], m);
}
