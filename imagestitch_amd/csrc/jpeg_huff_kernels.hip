// jpeg_huff_kernels.hip -- the entropy decode of a baseline JPEG file on the device (Method.jpegDecoder = "device-entropy"; specified by
// tests/jpeg_huff_ref.py).  The host has scanned the file for its markers (vfsms_jpeg_scan, csrc/jpeg_host.cpp): what arrives is the scan
// record of csrc/jpeg_huff_core.h -- tables, the unstuffed stream cut into restart segments, every segment cut into subsequences of sub_bits.
// A file without restart markers is ONE serial bit stream; it is decoded by self-synchronisation (Klein & Wiseman; Weissenberger & Schmidt):
//
//   k_huff_sync    one thread per subsequence decodes it from a guess -- (its first bit, block 0, coefficient 0); the first of a segment from
//                  the truth (0, 0, 0) -- to its end and records its exit state, the blocks it closed and its DC sums
//   k_huff_round   Jacobi repair round r: a thread whose predecessor's exit of round r - 1 differs from its own entry takes that state and
//                  decodes again; flags[r] = something changed.  A round whose predecessor changed nothing returns at once, so rounds are
//                  launched in batches without the host in between; the last launch only compares (repair = 0).  The fixed point is the
//                  sequential decode; a wrong decoder usually falls in step at the next end-of-block, so a few rounds do
//   k_huff_scan    one workgroup: per segment the exclusive prefix sums of the blocks closed and of the DC sums per component -> every
//                  subsequence's first block and DC predictors
//   k_huff_write   the decode once more from the now-true entry states, storing every coefficient at (component grid, block, natural index)
//                  of the zeroed coefficient buffer -- the layout of vfsms_jpeg_coefficients -- and raising the damage flags
//
// A file is untrusted input: every loop is bounded before launch (a subsequence's bits, the round count, ceil(nsub / 1024) chunks of the scan),
// no workgroup waits for another, every stream read is clamped to its segment (jh_peek32), every store is checked against the segment's block
// count, the grid and index 63 first.  The step and the subsequence decode are csrc/jpeg_huff_core.h, the code tools/jpeg_huff_host.cpp runs
// on the host.  Kept from the first shape: tables in LDS (a 9-bit look-up, then the maxcode walk), state in registers.  Not kept: the stream
// staged in LDS -- a thread keeps its stream words in registers and asks for the next one a word ahead (jh_peek32), so the load is off the
// path from one symbol to the next.
#include "common.h"
#include "jpeg_huff_core.h"
#include <memory>

#define JH_WG 64
#define JH_SCAN_WG 1024

struct JpegHuffDev {
    const uint8_t *rec;                 // the scan record
    JpegScanHeader H;
    JpegHuffState *entry;               // [nsub]
    JpegHuffSubOut *res[2];             // [nsub] each: round r reads res[r & 1], writes res[(r + 1) & 1]
    uint32_t *base;                     // [nsub]: the first block of the subsequence, counted in its segment
    uint32_t *dcbase;                   // [3 * nsub]: the DC predictors it starts from
    uint32_t *flags;                    // [rounds + 1], then the damage bits
};

__device__ __forceinline__ void jh_stage_tables(const JpegHuffDev &D, uint32_t *lds)
{
    const uint32_t *src = (const uint32_t *)(D.rec + D.H.off_tables);
    const int n = 2 * D.H.ncomp * (int)(sizeof(JpegHuffTable) / 4);
    for (int k = threadIdx.x; k < n; k += blockDim.x) lds[k] = src[k];
    __syncthreads();
}
struct JhSub { JpegHuffBits bits; uint32_t start, end, seg, first, limit; bool last; };
__device__ __forceinline__ JhSub jh_sub(const JpegHuffDev &D, uint32_t i)
{
    const uint32_t *subseg = (const uint32_t *)(D.rec + D.H.off_subseg);
    const JpegHuffSeg *segs = (const JpegHuffSeg *)(D.rec + D.H.off_seg);
    JhSub s; s.seg = min(subseg[i], (uint32_t)D.H.nseg - 1);
    const JpegHuffSeg S = segs[s.seg];
    s.bits.words = (const uint32_t *)(D.rec + D.H.off_stream + S.byte_off);
    s.bits.nwords = (S.byte_count + 3) >> 2; s.bits.nbits = S.byte_count * 8;
    if ((size_t)S.byte_off + 4 * (size_t)s.bits.nwords > D.H.stream_bytes) { s.bits.nwords = 0; s.bits.nbits = 0; }      // (a record that lies about itself reads nothing)
    s.first = i - S.sub0;
    s.start = min(s.first * (uint32_t)D.H.sub_bits, s.bits.nbits);
    s.end = min(s.start + (uint32_t)D.H.sub_bits, s.bits.nbits);
    s.last = i + 1 == (uint32_t)D.H.nsub || subseg[i + 1] != s.seg;
    s.limit = jh_segment_blocks(D.H, S.first_mcu);
    return s;
}

__global__ __launch_bounds__(JH_WG) void k_huff_sync(JpegHuffDev D)
{
    __shared__ uint32_t lds[6 * sizeof(JpegHuffTable) / 4];
    jh_stage_tables(D, lds);
    const uint32_t i = blockIdx.x * JH_WG + threadIdx.x;
    if (i >= (uint32_t)D.H.nsub) return;
    const JhSub s = jh_sub(D, i);
    JpegHuffState e; e.p = s.start; e.cz = 0;
    JpegHuffNoSink sink; unsigned damage = 0;
    D.entry[i] = e;
    D.res[0][i] = jh_decode_sub(s.bits, (const JpegHuffTable *)lds, D.H.blocks_per_mcu, e, s.end, 0u, 0xFFFFFFFFu, sink, &damage);
}

__global__ __launch_bounds__(JH_WG) void k_huff_round(JpegHuffDev D, int r, int repair)
{
    if (r > 0 && D.flags[r - 1] == 0) return;                    // the round before changed nothing: the fixed point stands
    __shared__ uint32_t lds[6 * sizeof(JpegHuffTable) / 4];
    const uint32_t i = blockIdx.x * JH_WG + threadIdx.x;
    const bool live = i < (uint32_t)D.H.nsub;
    const JpegHuffSubOut *in = D.res[r & 1]; JpegHuffSubOut *out = D.res[(r + 1) & 1];
    JhSub s; JpegHuffSubOut mine; JpegHuffState prev;
    bool stale = false;
    if (live) {
        s = jh_sub(D, i);
        mine = in[i];
        if (s.first > 0) { prev = in[i - 1].exit; stale = !jh_same(prev, D.entry[i]); }
    }
    if (!__syncthreads_or(stale)) {                              // a workgroup in step: nothing to stage, nothing to decode
        if (live && repair) out[i] = mine;
        return;
    }
    if (repair) jh_stage_tables(D, lds);
    if (!live) return;
    if (stale) {
        atomicOr(&D.flags[r], 1u);
        if (repair) {
            JpegHuffNoSink sink; unsigned damage = 0;
            D.entry[i] = prev;
            mine = jh_decode_sub(s.bits, (const JpegHuffTable *)lds, D.H.blocks_per_mcu, prev, s.end, 0u, 0xFFFFFFFFu, sink, &damage);
        }
    }
    if (repair) out[i] = mine;
}

// per segment: base[i] = the blocks closed by the segment's subsequences in front of i, dcbase[3 i + k] = their DC sums of component k
__global__ __launch_bounds__(JH_SCAN_WG) void k_huff_scan(JpegHuffDev D, int which)
{
    __shared__ uint32_t sv[2][4][JH_SCAN_WG];
    __shared__ uint32_t sf[2][JH_SCAN_WG];
    __shared__ uint32_t carry[4];
    const JpegHuffSubOut *res = D.res[which & 1];
    const uint32_t *subseg = (const uint32_t *)(D.rec + D.H.off_subseg);
    const JpegHuffSeg *segs = (const JpegHuffSeg *)(D.rec + D.H.off_seg);
    const uint32_t n = (uint32_t)D.H.nsub, t = threadIdx.x;
    if (t < 4) carry[t] = 0;
    __syncthreads();
    for (uint32_t c0 = 0; c0 < n; c0 += JH_SCAN_WG) {            // ceil(nsub / 1024) chunks
        const uint32_t i = c0 + t;
        uint32_t v[4] = {0, 0, 0, 0}, head = 0;
        if (i < n) {
            const JpegHuffSubOut o = res[i];
            v[0] = o.blocks; v[1] = o.dc[0]; v[2] = o.dc[1]; v[3] = o.dc[2];
            head = segs[min(subseg[i], (uint32_t)D.H.nseg - 1)].sub0 == i;
        }
        const uint32_t own[4] = {v[0], v[1], v[2], v[3]};
        if (t == 0 && !head) for (int k = 0; k < 4; k++) v[k] += carry[k];       // the chunk goes on inside a segment
        int cur = 0;
        for (int k = 0; k < 4; k++) sv[0][k][t] = v[k];
        sf[0][t] = head;
        __syncthreads();
        for (uint32_t d = 1; d < JH_SCAN_WG; d <<= 1) {           // inclusive segmented scan, ten steps
            uint32_t f = sf[cur][t];
            for (int k = 0; k < 4; k++) v[k] = sv[cur][k][t];
            if (t >= d && !f) {
                for (int k = 0; k < 4; k++) v[k] += sv[cur][k][t - d];
                f = sf[cur][t - d];
            }
            for (int k = 0; k < 4; k++) sv[cur ^ 1][k][t] = v[k];
            sf[cur ^ 1][t] = f;
            cur ^= 1;
            __syncthreads();
        }
        if (i < n) {
            D.base[i] = v[0] - own[0];
            for (int k = 0; k < 3; k++) D.dcbase[3 * (size_t)i + k] = v[k + 1] - own[k + 1];
        }
        __syncthreads();
        if (t == JH_SCAN_WG - 1) for (int k = 0; k < 4; k++) carry[k] = v[k];
        __syncthreads();
    }
}

// zig-zag position -> natural (row-major) position
__constant__ uint8_t c_jh_natural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                         35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
struct JhStore {
    int16_t *coef[3];                           // a component's blocks (null: not wanted)
    JpegHuffPlace place;
    uint32_t block0;                            // the segment's first block in scan order
    uint32_t pred0, pred1, pred2;               // the DC predictors (selected, not indexed: they stay in registers)
    __device__ __forceinline__ void operator()(uint32_t blk, int zi, int value, int comp)
    {
        if (zi == 0) {
            pred0 += comp == 0 ? (uint32_t)value : 0u; pred1 += comp == 1 ? (uint32_t)value : 0u; pred2 += comp == 2 ? (uint32_t)value : 0u;
            value = (int)(int16_t)(uint16_t)(comp == 0 ? pred0 : comp == 1 ? pred1 : pred2);
        }
        int16_t *dst = comp == 0 ? coef[0] : comp == 1 ? coef[1] : coef[2];
        uint32_t b;
        if ((unsigned)zi > 63u || !dst || !jh_place(place, block0 + blk, comp, &b)) return;
        dst[(size_t)b * 64 + c_jh_natural[zi]] = (int16_t)value;
    }
};

__global__ __launch_bounds__(JH_WG) void k_huff_write(JpegHuffDev D, JhStore proto)
{
    __shared__ uint32_t lds[6 * sizeof(JpegHuffTable) / 4];
    jh_stage_tables(D, lds);
    const uint32_t i = blockIdx.x * JH_WG + threadIdx.x;
    if (i >= (uint32_t)D.H.nsub) return;
    const JhSub s = jh_sub(D, i);
    const uint32_t base = D.base[i];
    if (base >= s.limit) return;                                 // the segment's blocks were complete in front of this subsequence: leftover bits
    const JpegHuffSeg *segs = (const JpegHuffSeg *)(D.rec + D.H.off_seg);
    JhStore sink = proto;
    sink.block0 = segs[s.seg].first_mcu * (uint32_t)D.H.blocks_per_mcu;
    sink.pred0 = D.dcbase[3 * (size_t)i]; sink.pred1 = D.dcbase[3 * (size_t)i + 1]; sink.pred2 = D.dcbase[3 * (size_t)i + 2];
    unsigned damage = 0;
    const JpegHuffSubOut o = jh_decode_sub(s.bits, (const JpegHuffTable *)lds, D.H.blocks_per_mcu, D.entry[i], s.end, base, s.limit, sink, &damage);
    if (o.exit.p > s.bits.nbits) damage |= JH_DAMAGE_BITS;                               // a symbol read beyond the segment's end
    if (s.last && base + o.blocks < s.limit) damage |= JH_DAMAGE_BITS;                   // the bits ran out in front of the blocks
    if (damage) atomicOr(D.flags, damage);
}

// ---- the host side ---------------------------------------------------------------------------------------------------------------------------
static size_t jh_up(size_t v) { return (v + 255) & ~(size_t)255; }
static int jh_rounds(const JpegScanHeader &H, int max_rounds) { return max_rounds < 0 || max_rounds > H.nsub ? H.nsub : max_rounds; }
size_t jpeg_huff_work_bytes(const JpegScanHeader &H, int max_rounds)
{
    const size_t n = (size_t)H.nsub;
    return jh_up(n * sizeof(JpegHuffState)) + 2 * jh_up(n * sizeof(JpegHuffSubOut)) + jh_up(n * 4) + jh_up(n * 12) + jh_up(((size_t)jh_rounds(H, max_rounds) + 2) * 4);
}

// The decode of a scan record that lies on the device at d_rec (H: its header, the host's copy) into d_coef -- per wanted component its blocks,
// 64 int16 each in natural order, back to back: the block part of vfsms_jpeg_coefficients' layout (luma_only: component 0 alone).  d_work:
// jpeg_huff_work_bytes() of device memory.  h_flags: (rounds + 2) uint32 of host memory the flags are read back to (pinned, for true DMA).
// Stream-ordered, but it WAITS on `sync` twice or more: for the round flags, a batch of rounds at a time, and for the damage flags.
// max_rounds < 0: as many as there are subsequences (always enough).  VFSMS_ERR_UNSUPPORTED: the rounds ran out (nothing is decoded into
// d_coef then); VFSMS_ERR_BAD_ARG: the true decode met damage (tests/jpeg_huff_ref.py).  *rounds_used: the rounds that changed something.
// prof: the context whose profiler books the stages "jpeg_entropy_sync / _rounds / _scan / _write" (its stream must be `stream`), or NULL.
int jpeg_huff_decode_device(hipStream_t stream, hipEvent_t sync, const JpegScanHeader &H, const uint8_t *d_rec, uint8_t *d_work, uint32_t *h_flags,
                            int max_rounds, int luma_only, int16_t *d_coef, int *rounds_used, vfsms_ctx *prof)
{
    if (H.nsub < 1 || H.nseg < 1 || H.ncomp < 1 || H.ncomp > 3 || (H.blocks_per_mcu != 1 && H.blocks_per_mcu != 6) || H.sub_bits < 64) {
        vfsms_set_error("jpeg_huff: not a scan record"); return VFSMS_ERR_BAD_ARG;
    }
    JhStore S; memset(&S, 0, sizeof(S));
    if (!jh_place_from_header(H, &S.place)) { vfsms_set_error("jpeg_huff: the record's grids do not fit its frame"); return VFSMS_ERR_BAD_ARG; }
    const size_t n = (size_t)H.nsub;
    const int rounds = jh_rounds(H, max_rounds);
    JpegHuffDev D; D.rec = d_rec; D.H = H;
    uint8_t *w = d_work;
    D.entry = (JpegHuffState *)w; w += jh_up(n * sizeof(JpegHuffState));
    D.res[0] = (JpegHuffSubOut *)w; w += jh_up(n * sizeof(JpegHuffSubOut));
    D.res[1] = (JpegHuffSubOut *)w; w += jh_up(n * sizeof(JpegHuffSubOut));
    D.base = (uint32_t *)w; w += jh_up(n * 4);
    D.dcbase = (uint32_t *)w; w += jh_up(n * 12);
    D.flags = (uint32_t *)w;
    const size_t flag_bytes = ((size_t)rounds + 2) * 4;
    const dim3 grid((unsigned)((n + JH_WG - 1) / JH_WG)), wg(JH_WG);
    // (the stage split of the bare operator: the profiler belongs to the context thread, the fills pass no context)
    std::unique_ptr<ProfScope> ps;
#define JH_MARK(name) do { ps.reset(); if (prof) ps.reset(new ProfScope(prof, name)); } while (0)
    JH_MARK("jpeg_entropy_sync");
    HIP_TRY(hipMemsetAsync(D.flags, 0, flag_bytes, stream));
    hipLaunchKernelGGL(k_huff_sync, grid, wg, 0, stream, D);
    HIP_TRY(hipGetLastError());
    JH_MARK("jpeg_entropy_rounds");
    // rounds 0 .. rounds - 1 repair, round `rounds` only compares; four launches, then a look at the flags
    int used = -1;
    for (int r = 0; r <= rounds && used < 0; ) {
        const int stop = r + 4 < rounds + 1 ? r + 4 : rounds + 1;
        for (; r < stop; r++) { hipLaunchKernelGGL(k_huff_round, grid, wg, 0, stream, D, r, r < rounds ? 1 : 0); HIP_TRY(hipGetLastError()); }
        HIP_TRY(hipMemcpyAsync(h_flags, D.flags, (size_t)stop * 4, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipEventRecord(sync, stream));
        HIP_TRY(hipEventSynchronize(sync));
        for (int k = 0; k < stop; k++) if (h_flags[k] == 0) { used = k; break; }
    }
    ps.reset();
    if (used < 0) { vfsms_set_error("jpeg_huff: the decoders are not in step after %d repair rounds", rounds); return VFSMS_ERR_UNSUPPORTED; }
    if (rounds_used) *rounds_used = used;
    D.flags += rounds + 1;                                       // the damage bits
    JH_MARK("jpeg_entropy_scan");
    hipLaunchKernelGGL(k_huff_scan, dim3(1), dim3(JH_SCAN_WG), 0, stream, D, used);
    HIP_TRY(hipGetLastError());
    JH_MARK("jpeg_entropy_write");
    size_t total = 0;
    for (int k = 0; k < (luma_only ? 1 : H.ncomp); k++) { S.coef[k] = d_coef + total; total += (size_t)S.place.blocks[k] * 64; }
    HIP_TRY(hipMemsetAsync(d_coef, 0, total * 2, stream));
    hipLaunchKernelGGL(k_huff_write, grid, wg, 0, stream, D, S);
    HIP_TRY(hipGetLastError());
    ps.reset();
    HIP_TRY(hipMemcpyAsync(h_flags, D.flags, 4, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipEventRecord(sync, stream));
    HIP_TRY(hipEventSynchronize(sync));
#undef JH_MARK
    if (h_flags[0]) {
        vfsms_set_error("jpeg_huff: damaged entropy-coded data (%s%s%s)", h_flags[0] & JH_DAMAGE_CODE ? "undefined code " : "",
                        h_flags[0] & JH_DAMAGE_INDEX ? "coefficient beyond 63 " : "", h_flags[0] & JH_DAMAGE_BITS ? "bits exhausted" : "");
        return VFSMS_ERR_BAD_ARG;
    }
    return VFSMS_OK;
}
