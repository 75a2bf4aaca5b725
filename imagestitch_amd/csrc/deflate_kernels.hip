// deflate_kernels.hip -- the lossless tile coder of Method.pyramidCompression = "deflate-device" (TIFF compression 8, Predictor = 2), specified
// by tests/deflate_ref.py; the coder's rules (tokens, code lengths, frame) are csrc/deflate_core.h's, shared with a host program.
//
// A tile is tile x tile x ch predicted bytes, cut into chunks of DFL_THREADS x DFL_PER_THREAD bytes: one workgroup a chunk, DFL_PER_THREAD
// consecutive bytes a thread.  The passes of a call, all tiles of all levels at once:
//   predict    pixels -> predicted bytes (B G R flip, zero padding, horizontal differencing) in scratch; per chunk its first and last run
//              boundary; per tile the two Adler sums
//   runs       per tile, over its chunks: the last boundary in front of every chunk (forward) and the first behind it (backward)
//   symbols    every byte knows its run's start and end, hence its token: the 286-bin histogram per tile (LDS bins, merged once a workgroup)
//   codes      one wave a tile: code lengths, codes, the stream's size; then a scan across tiles for the offsets, which go to the host
//   count      the bits of every chunk's tokens, then a scan inside the tile
//   write      every chunk knows its bit offset: its tokens are composed into whole words in LDS and stored; only a chunk's first and last
//              word meet a neighbour's and are merged into the zeroed payload by an atomic OR.  The frame (zlib header, block header, end of
//              block, Adler-32) is one wave a tile.
#include "common.h"
#include "deflate_core.h"

#define DFL_THREADS 256
#define DFL_PER_THREAD 16
#define DFL_CHUNK (DFL_THREADS * DFL_PER_THREAD)
#define DFL_MAX_TILE 4096                   // tile x tile x 3 bytes at 15 bits each stay inside 32 bits
#define DFL_ROW 288                         // entries a tile in hist, lens and table (286, padded)
#define DFL_CHUNK_WORDS (DFL_CHUNK * DFL_MAX_BITS / 32 + 4)     // a chunk's tokens, at most 15 bits a byte and one match's tail more, from any bit of a word

namespace {

// the predicted byte b of tile (job J, row ty, column tx): sample (r, col, c) of the tile minus its left neighbour in the tile row; samples
// beyond the level are 0
__device__ __forceinline__ int dfl_raw(const DflJobDev &J, int bgr, int ch, int y, int x, int c)
{
    if (y >= J.rows || x >= J.cols) return 0;
    const unsigned long long at = (unsigned long long)(y - J.src_row0) * J.pitch + (unsigned long long)x * ch + (bgr ? ch - 1 - c : c);
    return at < J.src_bytes ? J.src[at] : 0;
}
__device__ __forceinline__ int dfl_pred_byte(const DflArgs &A, const DflJobDev &J, int y0, int x0, int b)
{
    const int rowbytes = A.tile * A.ch, r = b / rowbytes, i = b - r * rowbytes, col = i / A.ch, c = i - col * A.ch;
    const int v = dfl_raw(J, A.bgr, A.ch, y0 + r, x0 + col, c);
    return col ? (v - dfl_raw(J, A.bgr, A.ch, y0 + r, x0 + col - 1, c)) & 255 : v;
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}
// the sum over the workgroup's DFL_THREADS threads, in every thread
__device__ __forceinline__ unsigned long long block_sum(unsigned long long v, unsigned long long *lds)
{
    v = wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < DFL_THREADS / 64; w++) t += lds[w];
    return t;
}
// max over the threads in front of this one (and `init`), min over the threads behind it (and `init`)
__device__ __forceinline__ int block_max_before(int v, int init, int *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int s = 1; s < 64; s <<= 1) { const int t = __shfl_up(inc, s, 64); if (lane >= s) inc = max(inc, t); }
    __syncthreads();
    if (lane == 63) lds[wave] = inc;
    __syncthreads();
    int before = __shfl_up(inc, 1, 64);
    if (lane == 0) before = init;
    before = max(before, init);
    for (int w = 0; w < wave; w++) before = max(before, lds[w]);
    return before;
}
__device__ __forceinline__ int block_min_behind(int v, int init, int *lds)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
    for (int s = 1; s < 64; s <<= 1) { const int t = __shfl_down(inc, s, 64); if (lane + s < 64) inc = min(inc, t); }
    __syncthreads();
    if (lane == 0) lds[wave] = inc;
    __syncthreads();
    int behind = __shfl_down(inc, 1, 64);
    if (lane == 63) behind = init;
    behind = min(behind, init);
    for (int w = wave + 1; w < DFL_THREADS / 64; w++) behind = min(behind, lds[w]);
    return behind;
}

// the thread's DFL_PER_THREAD predicted bytes from scratch and the mask of the run boundaries among them (bit i: byte i differs from the byte
// in front of it, or is the tile's first); b0 < nbytes
__device__ __forceinline__ unsigned dfl_load(const uint8_t *pred, int b0, int d[DFL_PER_THREAD])
{
    const uint4 q = *(const uint4 *)(pred + b0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) d[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
    unsigned mask = 0;
    int prev = b0 ? pred[b0 - 1] : -1;
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) { mask |= (unsigned)(d[i] != prev) << i; prev = d[i]; }
    return mask;
}

// The tokens of the thread's bytes (every thread of the workgroup calls this; threads beyond the tile get DFL_NONE): the boundary in front of
// the thread's bytes by a forward scan over the workgroup from the chunk's `reach`, the one behind them by a backward scan
__device__ __forceinline__ void dfl_chunk_tokens(const DflArgs &A, long long tile, int chunk, int *lds, int tok[DFL_PER_THREAD])
{
    const int b0 = chunk * DFL_CHUNK + (int)threadIdx.x * DFL_PER_THREAD;
    const bool live = b0 < A.nbytes;
    int d[DFL_PER_THREAD];
    unsigned mask = 0;
    if (live) mask = dfl_load(A.pred + (size_t)tile * A.nbytes, b0, d);
    const int2 reach = A.reach[tile * A.nchunks + chunk];
    const int last = mask ? b0 + 31 - __builtin_clz(mask) : -1, first = mask ? b0 + __builtin_ctz(mask) : 0x7fffffff;
    int start = block_max_before(last, reach.x, lds);
    int behind = block_min_behind(first, reach.y, lds);
    int end[DFL_PER_THREAD];
#pragma unroll
    for (int i = DFL_PER_THREAD - 1; i >= 0; i--) { end[i] = behind; if (mask >> i & 1) behind = b0 + i; }
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) {
        if (mask >> i & 1) start = b0 + i;
        tok[i] = live ? dfl_token(b0 + i - start, end[i] - start, d[i]) : DFL_NONE;
    }
}

// ---- predict ---------------------------------------------------------------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_predict(const DflArgs A)
{
    __shared__ int s_first, s_last;
    __shared__ unsigned long long s_sum[DFL_THREADS / 64];
    const long long blk = blockIdx.x, tile = blk / A.nchunks;
    const int chunk = (int)(blk - tile * A.nchunks);
    int j = 0;
    while (j + 1 < A.n_jobs && tile >= A.job[j + 1].first_tile) j++;
    const DflJobDev &J = A.job[j];
    const long long t = tile - J.first_tile;
    const int y0 = J.row0 + (int)(t / J.ntx) * A.tile, x0 = (int)(t % J.ntx) * A.tile;
    if (threadIdx.x == 0) { s_first = 0x7fffffff; s_last = -1; }
    __syncthreads();
    const int b0 = chunk * DFL_CHUNK + (int)threadIdx.x * DFL_PER_THREAD;
    unsigned long long sa = 0, sb = 0;
    if (b0 < A.nbytes) {
        // the 16 bytes lie in one tile row (its bytes are a multiple of 16)
        const int rowbytes = A.tile * CH, r = b0 / rowbytes, i0 = b0 - r * rowbytes;
        int prev = b0 ? dfl_pred_byte(A, J, y0, x0, b0 - 1) : -1;
        uint32_t w[4] = {0, 0, 0, 0};
        unsigned mask = 0;
#pragma unroll
        for (int i = 0; i < DFL_PER_THREAD; i++) {
            const int col = (i0 + i) / CH, c = (i0 + i) - col * CH;
            const int v = dfl_raw(J, A.bgr, CH, y0 + r, x0 + col, c);
            const int p = col ? (v - dfl_raw(J, A.bgr, CH, y0 + r, x0 + col - 1, c)) & 255 : v;
            w[i >> 2] |= (uint32_t)p << (8 * (i & 3));
            mask |= (unsigned)(p != prev) << i; prev = p;
            sa += (unsigned)p; sb += (unsigned long long)(A.nbytes - (b0 + i)) * (unsigned)p;
        }
        *(uint4 *)(A.pred + (size_t)tile * A.nbytes + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        if (mask) { atomicMin(&s_first, b0 + __builtin_ctz(mask)); atomicMax(&s_last, b0 + 31 - __builtin_clz(mask)); }
    }
    sa = block_sum(sa, s_sum);
    sb = block_sum(sb, s_sum);
    if (threadIdx.x == 0) {
        A.bounds[blk] = make_int2(s_first, s_last);
        atomicAdd(&A.adler[2 * tile], (uint32_t)(sa % DFL_ADLER_MOD));
        atomicAdd(&A.adler[2 * tile + 1], (uint32_t)(sb % DFL_ADLER_MOD));
    }
}

// ---- runs: reach[chunk] = (the last boundary in the chunks in front, the first boundary in the chunks behind or nbytes), one workgroup a tile ----
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_runs(const DflArgs A)
{
    __shared__ int lds[DFL_THREADS / 64];
    __shared__ int s_carry;
    const long long tile = blockIdx.x;
    const int2 *bounds = A.bounds + tile * A.nchunks;
    int2 *reach = A.reach + tile * A.nchunks;
    if (threadIdx.x == 0) s_carry = -1;
    __syncthreads();
    for (int base = 0; base < A.nchunks; base += DFL_THREADS) {
        const int c = base + (int)threadIdx.x, carry = s_carry;
        const int v = c < A.nchunks ? bounds[c].y : -1;
        const int before = block_max_before(v, carry, lds);
        if (c < A.nchunks) reach[c].x = before;
        __syncthreads();
        if (threadIdx.x == DFL_THREADS - 1) s_carry = max(before, v);
        __syncthreads();
    }
    if (threadIdx.x == 0) s_carry = A.nbytes;
    __syncthreads();
    for (int top = A.nchunks; top > 0; top -= DFL_THREADS) {
        const int c = top - DFL_THREADS + (int)threadIdx.x, carry = s_carry;
        const int v = c >= 0 ? bounds[c].x : 0x7fffffff;
        const int behind = block_min_behind(v, carry, lds);
        if (c >= 0) reach[c].y = behind;
        __syncthreads();
        if (threadIdx.x == 0) s_carry = min(behind, v);
        __syncthreads();
    }
}

// ---- symbols ---------------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_symbols(const DflArgs A)
{
    __shared__ int lds[DFL_THREADS / 64];
    __shared__ uint32_t bins[DFL_SYMS];
    const long long blk = blockIdx.x, tile = blk / A.nchunks;
    const int chunk = (int)(blk - tile * A.nchunks);
    for (int s = threadIdx.x; s < DFL_SYMS; s += DFL_THREADS) bins[s] = 0;
    int tok[DFL_PER_THREAD];
    dfl_chunk_tokens(A, tile, chunk, lds, tok);                // (its barriers stand between the zeroing and the counting)
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) if (tok[i] != DFL_NONE) atomicAdd(&bins[dfl_token_symbol(tok[i])], 1u);
    __syncthreads();
    for (int s = threadIdx.x; s < DFL_SYMS; s += DFL_THREADS) if (bins[s]) atomicAdd(&A.hist[tile * DFL_ROW + s], bins[s]);
}

// ---- codes: one wave a tile ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_deflate_codes(const DflArgs A)
{
    __shared__ uint32_t counts[DFL_SYMS], first[DFL_MAX_BITS + 1];
    __shared__ uint8_t lens[DFL_SYMS];
    __shared__ DflBuild build;
    __shared__ int s_deepest;
    const long long tile = blockIdx.x;
    uint32_t *hist = A.hist + tile * DFL_ROW;
    const int lane = threadIdx.x;
    if (lane == 0) hist[DFL_END] = 1;
    for (int s = lane; s < DFL_SYMS; s += 64) counts[s] = s == DFL_END ? 1u : hist[s];
    __syncthreads();
    // the end of block and at least one literal: two symbols or more.  Ranks and leaf depths are position-local, one symbol a lane and step;
    // the merge of the two queues is one lane's
    for (;;) {
        if (lane == 0) { build.n = dfl_used(counts); s_deepest = 0; }
        for (int s = lane; s < DFL_SYMS; s += 64) { lens[s] = 0; if (counts[s]) build.order[dfl_rank(counts, s)] = (uint16_t)s; }
        __syncthreads();
        if (lane == 0) dfl_merge(&build, counts);
        __syncthreads();
        for (int k = lane; k < build.n; k += 64) {
            const int d = dfl_leaf_depth(&build, k);
            lens[build.order[k]] = (uint8_t)(d > 255 ? 255 : d);
            atomicMax(&s_deepest, d);
        }
        __syncthreads();
        if (s_deepest <= DFL_MAX_BITS) break;
        for (int s = lane; s < DFL_SYMS; s += 64) dfl_halve(counts, s);
        __syncthreads();
    }
    for (int s = lane; s < DFL_SYMS; s += 64) counts[s] = s == DFL_END ? 1u : hist[s];       // the tokens' own counts again
    if (lane == 0) dfl_code_starts(lens, first);
    __syncthreads();
    for (int s = lane; s < DFL_SYMS; s += 64) {
        const uint32_t e = dfl_code_entry(lens, first, s);
        A.lens[tile * DFL_ROW + s] = lens[s]; A.table[tile * DFL_ROW + s] = e;
    }
    if (lane == 0) {
        const unsigned long long bits = dfl_block_bits(counts, lens);
        A.sizes[tile] = (uint32_t)dfl_stream_bytes(bits);
        A.eob[tile] = DFL_HEAD_BITS + bits - lens[DFL_END];
    }
}

// offs[0 .. n] = the exclusive scan of sizes[0 .. n): one workgroup, 1024 elements a step
__global__ void __launch_bounds__(1024) k_deflate_scan(const uint32_t *sizes, int n, unsigned long long *offs)
{
    __shared__ unsigned long long part[1024];
    __shared__ unsigned long long carry;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 1024) {
        const int e = base + tid;
        const unsigned long long v = e < n ? sizes[e] : 0;
        part[tid] = v;
        __syncthreads();
        for (int s = 1; s < 1024; s <<= 1) {
            const unsigned long long t = tid >= s ? part[tid - s] : 0;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (e < n) offs[e] = carry + part[tid] - v;
        __syncthreads();
        if (tid == 1023) carry += part[1023];
        __syncthreads();
    }
    if (tid == 0) offs[n] = carry;
}

// ---- count: chunk_bits[chunk] = the bits of its tokens; then, one workgroup a tile, where they start among the tile's tokens -------------------------
__device__ __forceinline__ void dfl_table_load(const DflArgs &A, long long tile, uint32_t *table)
{
    for (int s = threadIdx.x; s < DFL_SYMS; s += DFL_THREADS) table[s] = A.table[tile * DFL_ROW + s];
}
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_count(const DflArgs A)
{
    __shared__ int lds[DFL_THREADS / 64];
    __shared__ unsigned long long s_sum[DFL_THREADS / 64];
    __shared__ uint32_t table[DFL_SYMS];
    const long long blk = blockIdx.x, tile = blk / A.nchunks;
    const int chunk = (int)(blk - tile * A.nchunks);
    dfl_table_load(A, tile, table);
    int tok[DFL_PER_THREAD];
    dfl_chunk_tokens(A, tile, chunk, lds, tok);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) if (tok[i] != DFL_NONE) { int n; dfl_token_bits(tok[i], table, &n); bits += (unsigned)n; }
    const unsigned long long total = block_sum(bits, s_sum);
    if (threadIdx.x == 0) A.chunk_bits[blk] = (uint32_t)total;
}
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_chunk_scan(const DflArgs A)
{
    __shared__ uint32_t part[DFL_THREADS];
    __shared__ uint32_t carry;
    uint32_t *bits = A.chunk_bits + (long long)blockIdx.x * A.nchunks;
    const int tid = threadIdx.x;
    if (tid == 0) carry = 0;
    __syncthreads();
    for (int base = 0; base < A.nchunks; base += DFL_THREADS) {
        const int e = base + tid;
        const uint32_t v = e < A.nchunks ? bits[e] : 0;
        part[tid] = v;
        __syncthreads();
        for (int s = 1; s < DFL_THREADS; s <<= 1) {
            const uint32_t t = tid >= s ? part[tid - s] : 0;
            __syncthreads();
            part[tid] += t;
            __syncthreads();
        }
        if (e < A.nchunks) bits[e] = carry + part[tid] - v;
        __syncthreads();
        if (tid == DFL_THREADS - 1) carry += part[DFL_THREADS - 1];
        __syncthreads();
    }
}

// ---- write -------------------------------------------------------------------------------------------------------------------------------------------
// `nbits` bits (first bit lowest, at most 32) at bit `at` of the payload, merged into the zeroed words
__device__ __forceinline__ void dfl_or_bits(const DflArgs &A, unsigned long long at, uint32_t value, int nbits)
{
    const unsigned long long word = at >> 5; const int sh = (int)(at & 31);
    if (word + (sh + nbits > 32) >= A.out_words) { *A.err = 1; return; }
    atomicOr(&A.out[word], value << sh);
    if (sh + nbits > 32) atomicOr(&A.out[word + 1], value >> (32 - sh));
}
__global__ void __launch_bounds__(DFL_THREADS) k_deflate_write(const DflArgs A)
{
    __shared__ int lds[DFL_THREADS / 64];
    __shared__ unsigned long long s_sum[DFL_THREADS / 64];
    __shared__ uint32_t table[DFL_SYMS];
    __shared__ uint32_t words[DFL_CHUNK_WORDS];
    __shared__ uint32_t s_wave[DFL_THREADS / 64];
    const long long blk = blockIdx.x, tile = blk / A.nchunks;
    const int chunk = (int)(blk - tile * A.nchunks);
    dfl_table_load(A, tile, table);
    for (int k = threadIdx.x; k < DFL_CHUNK_WORDS; k += DFL_THREADS) words[k] = 0;
    int tok[DFL_PER_THREAD];
    dfl_chunk_tokens(A, tile, chunk, lds, tok);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) if (tok[i] != DFL_NONE) { int n; dfl_token_bits(tok[i], table, &n); bits += (unsigned)n; }
    // where the thread's bits start in the chunk: a scan over the workgroup
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = bits;
    for (int s = 1; s < 64; s <<= 1) { const unsigned t = __shfl_up(inc, s, 64); if (lane >= s) inc += t; }
    if (lane == 63) s_wave[wave] = inc;
    const unsigned long long total = block_sum(bits, s_sum);                              // (its barriers publish s_wave)
    unsigned before = inc - bits;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    const unsigned long long at = A.offs[tile] * 8 + DFL_HEAD_BITS + A.chunk_bits[blk];     // the chunk's first bit in the payload
    const int shift = (int)(at & 31);
    // whole words are composed in registers and merged into the chunk's words in LDS
    unsigned long long acc = 0;
    unsigned pos = (unsigned)shift + before, word = pos >> 5;
    int fill = (int)(pos & 31);
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) {
        if (tok[i] == DFL_NONE) continue;
        int n;
        const uint32_t v = dfl_token_bits(tok[i], table, &n);
        acc |= (unsigned long long)v << fill; fill += n;
        if (fill >= 32) { atomicOr(&words[word++], (uint32_t)acc); acc >>= 32; fill -= 32; }
    }
    if (fill > 0 && (uint32_t)acc) atomicOr(&words[word], (uint32_t)acc);
    __syncthreads();
    // the chunk's words leave: those it shares with a neighbour (its first and last, when they are partial) by an atomic OR
    const unsigned span = (unsigned)shift + (unsigned)total, nwords = (span + 31) >> 5;
    const unsigned long long word0 = at >> 5;
    for (unsigned k = threadIdx.x; k < nwords; k += DFL_THREADS) {
        if (word0 + k >= A.out_words) { *A.err = 1; continue; }
        const bool whole = (k > 0 || shift == 0) && (k + 1 < nwords || (span & 31) == 0);
        if (whole) A.out[word0 + k] = words[k];
        else if (words[k]) atomicOr(&A.out[word0 + k], words[k]);
    }
}

// the frame of a tile, one wave: every lane runs the frame's fields and writes every 64th
struct DflFramePut {
    const DflArgs &A; unsigned long long at; int lane, k;
    __device__ __forceinline__ void operator()(uint32_t value, int nbits)
    {
        if ((k++ & 63) == lane) dfl_or_bits(A, at, value, nbits);
        at += (unsigned)nbits;
    }
};
__global__ void __launch_bounds__(64) k_deflate_frame(const DflArgs A)
{
    const long long tile = blockIdx.x;
    const unsigned long long first = A.offs[tile] * 8, end = A.offs[tile + 1] * 8;
    DflFramePut put = {A, first, (int)threadIdx.x, 0};
    dfl_head(A.lens + tile * DFL_ROW, put);
    if (threadIdx.x == 0) {
        const uint32_t e = A.table[tile * DFL_ROW + DFL_END];
        dfl_or_bits(A, first + A.eob[tile], e >> 4, (int)(e & 15));
        const uint32_t a = (1u + A.adler[2 * tile]) % DFL_ADLER_MOD, b = ((uint32_t)(A.nbytes % DFL_ADLER_MOD) + A.adler[2 * tile + 1]) % DFL_ADLER_MOD;
        const uint32_t sum = dfl_adler(a, b);
        for (int k = 0; k < 4; k++) dfl_or_bits(A, end - 32 + 8 * k, (sum >> (24 - 8 * k)) & 255, 8);        // big-endian
    }
}

// the scratch of a call carved from s->meta; everything a pass accumulates into (adler, hist, err) lies in front, in `zero` bytes
size_t deflate_carve(char *base, size_t n_tiles, size_t n_chunks, DflArgs *a, size_t *zero)
{
    size_t at = 0;
    auto take = [&](size_t bytes) { char *p = base ? base + at : nullptr; at = (at + bytes + 255) & ~(size_t)255; return p; };
    a->err = (int *)take(sizeof(int));
    a->adler = (uint32_t *)take(n_tiles * 8);
    a->hist = (uint32_t *)take(n_tiles * DFL_ROW * 4);
    *zero = at;
    a->lens = (uint8_t *)take(n_tiles * DFL_ROW);
    a->table = (uint32_t *)take(n_tiles * DFL_ROW * 4);
    a->sizes = (uint32_t *)take(n_tiles * 4);
    a->offs = (unsigned long long *)take((n_tiles + 1) * 8);
    a->eob = (unsigned long long *)take(n_tiles * 8);
    a->bounds = (int2 *)take(n_chunks * 8);
    a->reach = (int2 *)take(n_chunks * 8);
    a->chunk_bits = (uint32_t *)take(n_chunks * 4);
    return at;
}

}  // namespace

int deflate_check_tile_geometry(const char *who, int tile, int ch)
{
    if (ch != 1 && ch != 3) { vfsms_set_error("%s: 1 or 3 channels, got %d", who, ch); return VFSMS_ERR_BAD_ARG; }
    if (tile <= 0 || tile % 16) { vfsms_set_error("%s: the tile must be a positive multiple of 16, got %d", who, tile); return VFSMS_ERR_BAD_ARG; }
    if (tile > DFL_MAX_TILE) { vfsms_set_error("%s: the tile is at most %d, got %d", who, DFL_MAX_TILE, tile); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}

// Counting half: the tile rows of `n_jobs` levels (api.hip has checked the tile and the jobs) are predicted into s->pred, tile after tile in job
// order; histograms, codes, sizes and ONE scan over all tiles follow, and the tiles' offsets (tile_offs[0 .. n_tiles], the last being the total)
// come to the host with `d_flag` (an int on the device, may be NULL) in *flag.  The predicted bytes hold everything the streams need: the
// caller may move the pixels afterwards.  Synchronises the stream.
int deflate_tiles_count_device(vfsms_ctx *ctx, DeflateScratch *s, const JpegTileJob *jobs, int n_jobs, int ch, int bgr, int tile, const int *d_flag, int *flag,
                               DeflateTilesRun *run)
{
    DflArgs &a = run->a;
    a = DflArgs();
    long long n_tiles = 0;
    for (int j = 0; j < n_jobs; j++) {
        const JpegTileJob &J = jobs[j];
        const int ntx = (J.cols + tile - 1) / tile;
        a.job[j] = {J.src, (unsigned long long)J.src_bytes, (unsigned long long)J.pitch, J.src_row0, J.rows, J.cols, J.row0, ntx, n_tiles};
        n_tiles += (long long)J.tile_rows * ntx;
    }
    // (a grid takes 2^24 workgroups of 256 threads)
    const long long nbytes = (long long)tile * tile * ch, nchunks = (nbytes + DFL_CHUNK - 1) / DFL_CHUNK;
    if (n_tiles < 1 || n_tiles > 0x7fffffff || n_tiles * nchunks > 0xffffff) { vfsms_set_error("deflate tiles: %lld tiles of %lld chunks are more than one call takes", n_tiles, nchunks); return VFSMS_ERR_BAD_ARG; }
    a.n_jobs = n_jobs; a.tile = tile; a.ch = ch; a.bgr = bgr && ch == 3; a.nbytes = (int)nbytes; a.nchunks = (int)nchunks; a.n_tiles = (int)n_tiles;
    const size_t n_chunks = (size_t)(n_tiles * nchunks);
    size_t zero = 0;
    DflArgs probe;
    TRY(s->meta.reserve(deflate_carve(nullptr, (size_t)n_tiles, n_chunks, &probe, &zero), ctx->stream));
    deflate_carve(s->meta.as<char>(), (size_t)n_tiles, n_chunks, &a, &zero);
    TRY(s->pred.reserve((size_t)n_tiles * (size_t)nbytes, ctx->stream));
    a.pred = s->pred.as<uint8_t>();
    const unsigned grid = (unsigned)n_chunks;
    {
        ProfScope ps(ctx, "deflate.symbols");
        HIP_TRY(hipMemsetAsync(s->meta.as<void>(), 0, zero, ctx->stream));
        if (ch == 3) hipLaunchKernelGGL(k_deflate_predict<3>, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
        else hipLaunchKernelGGL(k_deflate_predict<1>, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_runs, dim3((unsigned)n_tiles), dim3(DFL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_symbols, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "deflate.codes");
        hipLaunchKernelGGL(k_deflate_codes, dim3((unsigned)n_tiles), dim3(64), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(1024), 0, ctx->stream, a.sizes, (int)n_tiles, a.offs);
        HIP_TRY(hipGetLastError());
    }
    run->tile_offs.resize((size_t)n_tiles + 1);
    HIP_TRY(hipMemcpyAsync(run->tile_offs.data(), a.offs, ((size_t)n_tiles + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (d_flag) HIP_TRY(hipMemcpyAsync(flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// Writing half: the streams the counting half measured into `out` on the host (cap >= run->tile_offs[n_tiles], checked by the caller): the
// chunks' bit counts and their scan, one writing pass into the zeroed payload, one copy.  Synchronises the stream.
int deflate_tiles_write_device(vfsms_ctx *ctx, DeflateScratch *s, const DeflateTilesRun *run, uint8_t *out)
{
    DflArgs a = run->a;
    const size_t total = (size_t)run->tile_offs[(size_t)a.n_tiles], padded = (total + 15) & ~(size_t)15;
    TRY(s->out.reserve(padded, ctx->stream));
    a.out = s->out.as<uint32_t>(); a.out_words = padded / 4;
    const unsigned grid = (unsigned)((size_t)a.n_tiles * a.nchunks);
    int err = 0;
    {
        ProfScope ps(ctx, "deflate.write");
        HIP_TRY(hipMemsetAsync(a.out, 0, padded, ctx->stream));
        hipLaunchKernelGGL(k_deflate_count, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_chunk_scan, dim3((unsigned)a.n_tiles), dim3(DFL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_write, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_deflate_frame, dim3((unsigned)a.n_tiles), dim3(64), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "deflate.copy");
        HIP_TRY(hipMemcpyAsync(&err, a.err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out, s->out.as<uint8_t>(), total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!err) return VFSMS_OK;
    vfsms_set_error("deflate tiles: the coded tiles outgrew the %zu bytes counted for them", total);
    return VFSMS_ERR_CAPACITY;
}
