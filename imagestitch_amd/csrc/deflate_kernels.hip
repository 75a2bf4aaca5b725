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
//
// The passes behind predict take byte strings, not tiles: the PNG coder at the end of this file (Method.pngEncoder = "device") runs them over
// the segments of a PNG, whose last string is shorter than the others (dfl_string_len; the bytes behind a string's end are dead) and whose frame
// is a chunk of its own (A.png: the stream's size and the bit its tokens start at, A.head_bits).  deflate_symbol_passes, deflate_code_passes
// and deflate_write_passes are those passes.
#include "common.h"
#include "png_core.h"                       // (on deflate_core.h)

#define DFL_THREADS 256
#define DFL_PER_THREAD 16
#define DFL_CHUNK (DFL_THREADS * DFL_PER_THREAD)
#define DFL_MAX_TILE 4096                   // tile x tile x 3 bytes at 15 bits each stay inside 32 bits
#define DFL_ROW 288                         // entries a tile in hist, lens and table (286, padded)
#define DFL_CHUNK_WORDS (DFL_CHUNK * DFL_MAX_BITS / 32 + 4)     // a chunk's tokens, at most 15 bits a byte and one match's tail more, from any bit of a word

namespace {

// the live bytes of string `tile`: all strings of a call are `len` bytes long but the last, which may be shorter (a PNG's last segment); the
// bytes behind them, up to the stride A.nbytes, are dead: no token, no boundary, nothing in the histogram or the Adler sums
__device__ __forceinline__ int dfl_string_len(const DflArgs &A, long long tile) { return tile == A.n_tiles - 1 ? A.last_len : A.len; }

__device__ __forceinline__ unsigned long long dfl_wave_sum(unsigned long long v)
{
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_down(v, s, 64);
    return v;
}
// the sum over the workgroup's DFL_THREADS threads, in every thread
__device__ __forceinline__ unsigned long long dfl_block_sum(unsigned long long v, unsigned long long *lds)
{
    v = dfl_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    unsigned long long t = 0;
    for (int w = 0; w < DFL_THREADS / 64; w++) t += lds[w];
    return t;
}

// `nbits` bits (first bit lowest, at most 32) at bit `at` of the payload, merged into the zeroed words
__device__ __forceinline__ void dfl_or_bits(const DflArgs &A, unsigned long long at, uint32_t value, int nbits)
{
    const unsigned long long word = at >> 5; const int sh = (int)(at & 31);
    if (word + (sh + nbits > 32) >= A.out_words) { *A.err = 1; return; }
    atomicOr(&A.out[word], value << sh);
    if (sh + nbits > 32) atomicOr(&A.out[word + 1], value >> (32 - sh));
}
// the frame of a string, one wave: every lane runs the frame's fields and writes every 64th
struct DflFramePut {
    const DflArgs &A; unsigned long long at; int lane, k;
    __device__ __forceinline__ void operator()(uint32_t value, int nbits)
    {
        if ((k++ & 63) == lane) dfl_or_bits(A, at, value, nbits);
        at += (unsigned)nbits;
    }
};

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
// in front of it, or is the string's first); b0 < len, the string's live bytes
__device__ __forceinline__ unsigned dfl_load(const uint8_t *pred, int b0, int len, int d[DFL_PER_THREAD])
{
    const uint4 q = *(const uint4 *)(pred + b0);
    const uint32_t w[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) d[i] = (w[i >> 2] >> (8 * (i & 3))) & 255;
    unsigned mask = 0;
    int prev = b0 ? pred[b0 - 1] : -1;
#pragma unroll
    for (int i = 0; i < DFL_PER_THREAD; i++) { mask |= (unsigned)(d[i] != prev) << i; prev = d[i]; }
    if (len - b0 < DFL_PER_THREAD) mask &= (1u << (len - b0)) - 1u;             // (the bytes behind the string's end are dead)
    return mask;
}

// The tokens of the thread's bytes (every thread of the workgroup calls this; threads beyond the tile get DFL_NONE): the boundary in front of
// the thread's bytes by a forward scan over the workgroup from the chunk's `reach`, the one behind them by a backward scan
__device__ __forceinline__ void dfl_chunk_tokens(const DflArgs &A, long long tile, int chunk, int *lds, int tok[DFL_PER_THREAD])
{
    const int b0 = chunk * DFL_CHUNK + (int)threadIdx.x * DFL_PER_THREAD;
    const int len = dfl_string_len(A, tile);
    const bool live = b0 < len;
    int d[DFL_PER_THREAD];
    unsigned mask = 0;
    if (live) mask = dfl_load(A.pred + (size_t)tile * A.nbytes, b0, len, d);
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
        tok[i] = live && b0 + i < len ? dfl_token(b0 + i - start, end[i] - start, d[i]) : DFL_NONE;
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
    sa = dfl_block_sum(sa, s_sum);
    sb = dfl_block_sum(sb, s_sum);
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
    if (threadIdx.x == 0) s_carry = dfl_string_len(A, tile);
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
        A.sizes[tile] = (uint32_t)(A.png ? png_chunk_bytes(bits) : dfl_stream_bytes(bits));
        A.eob[tile] = (unsigned)A.head_bits + bits - lens[DFL_END];
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
    const unsigned long long total = dfl_block_sum(bits, s_sum);
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
    const unsigned long long total = dfl_block_sum(bits, s_sum);                              // (its barriers publish s_wave)
    unsigned before = inc - bits;
    for (int w = 0; w < wave; w++) before += s_wave[w];
    const unsigned long long at = A.offs[tile] * 8 + (unsigned)A.head_bits + A.chunk_bits[blk];     // the chunk's first bit in the payload
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

// the frame of a tile, one wave
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

// ==== the PNG coder of Method.pngEncoder = "device" around those passes, specified by tests/png_ref.py; the rules (filters, cost, frame, CRC step
// and join, Adler join) are csrc/png_core.h's, shared with a host program ====
//
// A band of rows is cut into segments of `segment_rows` rows; a segment's byte string is its rows' filter types and filtered bytes, 1 + cols x ch
// a row, and becomes one IDAT chunk that holds one dynamic block and an empty stored block, so the chunks of all bands concatenate into one
// deflate stream.  The passes of a call, all segments of the band at once:
//   choose     one workgroup a row: the five filters' sums of absolutes from the row and the RAW row above, read from the image; the type of the
//              smallest sum (ties to the lowest) goes to a table
//   filter     takes predict's place: one workgroup a chunk of a segment's string, DFL_PER_THREAD output bytes a thread, indexed by the output
//              byte (rows are 1 + cols x ch bytes: a thread's bytes straddle rows and filter bytes); per chunk its first and last run
//              boundary, per segment the two Adler sums.  The bytes behind the last segment's end are dead
//   symbols, codes, count, write: deflate_kernels.hip's
//   frame      one wave a segment: length and "IDAT", the block's header with BFINAL = 0, the end of block, and FF FF of the empty stored block
//   crc        one workgroup a segment over tag + data: every thread the raw remainder of a span, joined by products with powers of x
// the image and the band; types[nrows]: the band's filter types; sums[2 a segment]: sum d and sum (len - position) d, every chunk's share
// reduced modulo 65521
struct PngArgs {
    const uint8_t *pix; unsigned long long pitch; int rows, cols, ch, bgr, row0, nrows, seg_rows, rowbytes;
    uint8_t *types; unsigned long long *sums;
    PngCrcPowers pw;
};

// byte i (file order: R G B) of the image's row y; 0 left of the row and above the image
template <int CH> __device__ __forceinline__ int png_raw(const PngArgs &P, int y, int i)
{
    if (y < 0 || i < 0) return 0;
    const int col = i / CH, c = i - col * CH;
    return P.pix[(unsigned long long)y * P.pitch + (unsigned)(col * CH + (P.bgr ? CH - 1 - c : c))];
}
// byte i of row y under filter `type`
template <int CH> __device__ __forceinline__ int png_filtered(const PngArgs &P, int type, int y, int i)
{
    return png_filter(type, png_raw<CH>(P, y, i), png_raw<CH>(P, y, i - CH), png_raw<CH>(P, y - 1, i), png_raw<CH>(P, y - 1, i - CH));
}
// byte i of the string row of band row r: its filter type, then its filtered bytes
template <int CH> __device__ __forceinline__ int png_string_byte(const PngArgs &P, int r, int i)
{
    const int type = P.types[r];
    return i == 0 ? type : png_filtered<CH>(P, type, P.row0 + r, i - 1);
}

// ---- choose ----------------------------------------------------------------------------------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(DFL_THREADS) k_png_choose(const PngArgs P)
{
    __shared__ unsigned long long s_sum[DFL_THREADS / 64];
    const int r = blockIdx.x, y = P.row0 + r, n = P.cols * CH;
    unsigned cost[PNG_TYPES] = {0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < n; i += DFL_THREADS) {
        const int x = png_raw<CH>(P, y, i), a = png_raw<CH>(P, y, i - CH), b = png_raw<CH>(P, y - 1, i), c = png_raw<CH>(P, y - 1, i - CH);
#pragma unroll
        for (int t = 0; t < PNG_TYPES; t++) cost[t] += (unsigned)png_cost(png_filter(t, x, a, b, c));
    }
    // (a row's cost is at most 128 x 3 x 2^22 < 2^31)
#pragma unroll
    for (int t = 0; t < PNG_TYPES; t++) cost[t] = (unsigned)dfl_block_sum(cost[t], s_sum);
    if (threadIdx.x == 0) P.types[r] = (uint8_t)png_choose(cost);
}

// ---- filter: the segment's string to scratch, as k_deflate_predict leaves a tile's ---------------------------------------------------------------
template <int CH>
__global__ void __launch_bounds__(DFL_THREADS) k_png_filter(const DflArgs A, const PngArgs P)
{
    __shared__ int s_first, s_last;
    __shared__ unsigned long long s_sum[DFL_THREADS / 64];
    const long long blk = blockIdx.x, seg = blk / A.nchunks;
    const int chunk = (int)(blk - seg * A.nchunks), len = dfl_string_len(A, seg);
    if (threadIdx.x == 0) { s_first = 0x7fffffff; s_last = -1; }
    __syncthreads();
    const int b0 = chunk * DFL_CHUNK + (int)threadIdx.x * DFL_PER_THREAD;
    unsigned long long sa = 0, sb = 0;
    if (b0 < A.nbytes) {                                          // (the stride is whole threads: dead bytes are stored as 0)
        uint32_t w[4] = {0, 0, 0, 0};
        unsigned mask = 0;
        if (b0 < len) {
            const int rb = P.rowbytes, r0 = (int)seg * P.seg_rows;
            int r = b0 / rb, i = b0 - r * rb;
            int prev = -1;
            if (b0) prev = i ? png_string_byte<CH>(P, r0 + r, i - 1) : png_string_byte<CH>(P, r0 + r - 1, rb - 1);
#pragma unroll
            for (int k = 0; k < DFL_PER_THREAD; k++) {
                if (b0 + k < len) {
                    const int p = png_string_byte<CH>(P, r0 + r, i);
                    w[k >> 2] |= (uint32_t)p << (8 * (k & 3));
                    mask |= (unsigned)(p != prev) << k; prev = p;
                    sa += (unsigned)p; sb += (unsigned long long)(len - (b0 + k)) * (unsigned)p;
                    if (++i == rb) { i = 0; r++; }
                }
            }
        }
        *(uint4 *)(A.pred + (size_t)seg * A.nbytes + b0) = make_uint4(w[0], w[1], w[2], w[3]);
        if (mask) { atomicMin(&s_first, b0 + __builtin_ctz(mask)); atomicMax(&s_last, b0 + 31 - __builtin_clz(mask)); }
    }
    sa = dfl_block_sum(sa, s_sum);
    sb = dfl_block_sum(sb, s_sum);
    if (threadIdx.x == 0) {
        A.bounds[blk] = make_int2(s_first, s_last);
        if (sa) atomicAdd(&P.sums[2 * seg], sa % DFL_ADLER_MOD);
        if (sb) atomicAdd(&P.sums[2 * seg + 1], sb % DFL_ADLER_MOD);
    }
}

// ---- frame: one wave a segment ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_png_frame(const DflArgs A)
{
    const long long seg = blockIdx.x;
    const unsigned long long first = A.offs[seg] * 8, end = A.offs[seg + 1] * 8;
    DflFramePut put = {A, first, (int)threadIdx.x, 0};
    png_chunk_head(A.offs[seg + 1] - A.offs[seg], put);
    dfl_block_head(A.lens + seg * DFL_ROW, put, 0u);
    if (threadIdx.x == 0) {
        const uint32_t e = A.table[seg * DFL_ROW + DFL_END];
        dfl_or_bits(A, first + A.eob[seg], e >> 4, (int)(e & 15));
        dfl_or_bits(A, end - 48, 0xffffu, 16);                    // 00 00 FF FF in front of the CRC: the zeros are the payload's own
    }
}

// ---- crc: one workgroup a segment, behind the writing passes ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(DFL_THREADS) k_png_crc(const DflArgs A, const PngArgs P)
{
    __shared__ uint32_t tab[256];
    __shared__ uint32_t s_part[DFL_THREADS / 64];
    const long long seg = blockIdx.x;
    const unsigned long long begin = A.offs[seg] + 4, stop = A.offs[seg + 1] - 4;     // tag + data
    if (stop > A.out_words * 4 || stop + 4 > A.out_words * 4) { if (threadIdx.x == 0) *A.err = 1; return; }
    const uint8_t *bytes = (const uint8_t *)A.out;
    tab[threadIdx.x] = png_crc_byte(0u, threadIdx.x);
    __syncthreads();
    const uint32_t n = (uint32_t)(stop - begin), span = (n + DFL_THREADS - 1) / DFL_THREADS;
    const uint32_t s0 = threadIdx.x * span, m = s0 < n ? (n - s0 < span ? n - s0 : span) : 0u;
    uint32_t r = 0;
    for (uint32_t k = 0; k < m; k++) r = tab[(r ^ bytes[begin + s0 + k]) & 255u] ^ (r >> 8);
    // the span's share of the chunk's remainder: what lies behind it multiplies it by x^8 a byte
    if (m) r = png_gf_mul(r, png_xpow8(&P.pw, n - s0 - m));
    for (int s = 32; s >= 1; s >>= 1) r ^= __shfl_down(r, s, 64);
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = r;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t raw = 0;
        for (int w = 0; w < DFL_THREADS / 64; w++) raw ^= s_part[w];
        const uint32_t crc = png_crc_finish(&P.pw, raw, n);
        uint8_t *o = (uint8_t *)A.out + stop;
        for (int k = 0; k < 4; k++) o[k] = (uint8_t)(crc >> (24 - 8 * k));
    }
}

}  // namespace

// the scratch of a call carved from s->meta; everything a pass accumulates into (adler, hist, err) lies in front, in `zero` bytes
static size_t deflate_carve(char *base, size_t n_tiles, size_t n_chunks, DflArgs *a, size_t *zero)
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

// The passes over the byte strings of a call, enqueued (the strings lie in a.pred with every chunk's bounds, as predict leaves them): the runs
// across chunks and the histograms; the codes, the streams' sizes and their offsets; the tokens' bits per chunk, their scan and the writing pass
// into the zeroed payload.  The frame around the tokens is the caller's
static int deflate_symbol_passes(vfsms_ctx *ctx, const DflArgs &a)
{
    hipLaunchKernelGGL(k_deflate_runs, dim3((unsigned)a.n_tiles), dim3(DFL_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_deflate_symbols, dim3((unsigned)((size_t)a.n_tiles * a.nchunks)), dim3(DFL_THREADS), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
static int deflate_code_passes(vfsms_ctx *ctx, const DflArgs &a)
{
    hipLaunchKernelGGL(k_deflate_codes, dim3((unsigned)a.n_tiles), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_deflate_scan, dim3(1), dim3(1024), 0, ctx->stream, a.sizes, a.n_tiles, a.offs);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}
static int deflate_write_passes(vfsms_ctx *ctx, const DflArgs &a)
{
    const unsigned grid = (unsigned)((size_t)a.n_tiles * a.nchunks);
    hipLaunchKernelGGL(k_deflate_count, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_deflate_chunk_scan, dim3((unsigned)a.n_tiles), dim3(DFL_THREADS), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_deflate_write, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a);
    HIP_TRY(hipGetLastError());
    return VFSMS_OK;
}

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
    a.len = a.last_len = (int)nbytes; a.head_bits = DFL_HEAD_BITS; a.png = 0;
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
        TRY(deflate_symbol_passes(ctx, a));
    }
    {
        ProfScope ps(ctx, "deflate.codes");
        TRY(deflate_code_passes(ctx, a));
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
    int err = 0;
    {
        ProfScope ps(ctx, "deflate.write");
        HIP_TRY(hipMemsetAsync(a.out, 0, padded, ctx->stream));
        TRY(deflate_write_passes(ctx, a));
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

// ---- PNG ---------------------------------------------------------------------------------------------------------------------------------------
int png_check_geometry(const char *who, int segment_rows, int rows, int cols, int ch)
{
    if (ch != 1 && ch != 3) { vfsms_set_error("%s: 1 or 3 channels, got %d", who, ch); return VFSMS_ERR_BAD_ARG; }
    if (rows < 1 || cols < 1) { vfsms_set_error("%s: an image has at least one row and one column, got %d x %d", who, rows, cols); return VFSMS_ERR_BAD_ARG; }
    if (segment_rows < 1 || segment_rows > PNG_MAX_SEGMENT_ROWS) { vfsms_set_error("%s: segment_rows must be 1..%d, got %d", who, PNG_MAX_SEGMENT_ROWS, segment_rows); return VFSMS_ERR_BAD_ARG; }
    if (!png_segment_fits(segment_rows, 1 + (long long)cols * ch)) {
        vfsms_set_error("%s: a segment of %d rows of %lld bytes is more than the coder's 32-bit bit counts take", who, segment_rows, 1 + (long long)cols * ch);
        return VFSMS_ERR_BAD_ARG;
    }
    return VFSMS_OK;
}

// api.hip has checked the geometry and the band (row0 a multiple of segment_rows; nrows too unless the band ends the image)
int png_encode_band_device(vfsms_ctx *ctx, DeflateScratch *s, const uint8_t *pix, int rows, int cols, int ch, size_t pitch, int bgr, int row0, int nrows,
                           int segment_rows, uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler, const int *d_flag, int *flag)
{
    const long long rowbytes = 1 + (long long)cols * ch, n_seg = ((long long)nrows + segment_rows - 1) / segment_rows;
    const long long len = rowbytes * (segment_rows < nrows ? segment_rows : nrows), last_len = rowbytes * (nrows - (n_seg - 1) * segment_rows);
    const long long stride = (len + 15) & ~15ll, nchunks = (stride + DFL_CHUNK - 1) / DFL_CHUNK;
    // (a grid takes 2^24 workgroups of 256 threads)
    if (n_seg * nchunks > 0xffffff) { vfsms_set_error("png: %lld segments of %lld chunks are more than one call takes", n_seg, nchunks); return VFSMS_ERR_BAD_ARG; }
    DflArgs a = DflArgs();
    a.ch = ch; a.bgr = bgr && ch == 3; a.nbytes = (int)stride; a.nchunks = (int)nchunks; a.n_tiles = (int)n_seg;
    a.len = (int)len; a.last_len = (int)last_len; a.head_bits = PNG_HEAD_BITS; a.png = 1;
    PngArgs p = {pix, (unsigned long long)pitch, rows, cols, ch, a.bgr, row0, nrows, segment_rows, (int)rowbytes, nullptr, nullptr, {}};
    png_crc_powers(&p.pw);
    const size_t n_chunks = (size_t)(n_seg * nchunks);
    size_t zero = 0;
    DflArgs probe;
    TRY(s->meta.reserve(deflate_carve(nullptr, (size_t)n_seg, n_chunks, &probe, &zero), ctx->stream));
    deflate_carve(s->meta.as<char>(), (size_t)n_seg, n_chunks, &a, &zero);
    const size_t sums_bytes = (size_t)n_seg * 16;
    TRY(s->png.reserve(sums_bytes + (size_t)nrows, ctx->stream));
    p.sums = s->png.as<unsigned long long>(); p.types = s->png.as<uint8_t>() + sums_bytes;
    TRY(s->pred.reserve((size_t)n_seg * (size_t)stride, ctx->stream));
    a.pred = s->pred.as<uint8_t>();
    const unsigned grid = (unsigned)n_chunks;
    {
        ProfScope ps(ctx, "png.choose");
        HIP_TRY(hipMemsetAsync(s->meta.as<void>(), 0, zero, ctx->stream));
        HIP_TRY(hipMemsetAsync(p.sums, 0, sums_bytes, ctx->stream));
        if (ch == 3) hipLaunchKernelGGL(k_png_choose<3>, dim3((unsigned)nrows), dim3(DFL_THREADS), 0, ctx->stream, p);
        else hipLaunchKernelGGL(k_png_choose<1>, dim3((unsigned)nrows), dim3(DFL_THREADS), 0, ctx->stream, p);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "png.filter");
        if (ch == 3) hipLaunchKernelGGL(k_png_filter<3>, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a, p);
        else hipLaunchKernelGGL(k_png_filter<1>, dim3(grid), dim3(DFL_THREADS), 0, ctx->stream, a, p);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "png.symbols");
        TRY(deflate_symbol_passes(ctx, a));
    }
    {
        ProfScope ps(ctx, "png.codes");
        TRY(deflate_code_passes(ctx, a));
    }
    std::vector<unsigned long long> offs((size_t)n_seg + 1), sums((size_t)n_seg * 2);
    HIP_TRY(hipMemcpyAsync(offs.data(), a.offs, offs.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(sums.data(), p.sums, sums_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (d_flag) HIP_TRY(hipMemcpyAsync(flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    const size_t total = (size_t)offs[(size_t)n_seg];
    *nbytes = total;
    uint32_t sum = 1;                                               // (the Adler-32 of nothing)
    for (long long g = 0; g < n_seg; g++) {
        const unsigned long long n = (unsigned long long)(g == n_seg - 1 ? last_len : len);
        sum = png_adler_combine(sum, png_adler_of_sums(sums[2 * g], sums[2 * g + 1], n), n);
    }
    *adler = sum;
    if (!out || cap < total) { vfsms_set_error("png: the band takes %zu bytes, the buffer holds %zu", total, out ? cap : (size_t)0); return VFSMS_ERR_CAPACITY; }
    const size_t padded = (total + 15) & ~(size_t)15;
    TRY(s->out.reserve(padded, ctx->stream));
    a.out = s->out.as<uint32_t>(); a.out_words = padded / 4;
    int err = 0;
    {
        ProfScope ps(ctx, "png.write");
        HIP_TRY(hipMemsetAsync(a.out, 0, padded, ctx->stream));
        TRY(deflate_write_passes(ctx, a));
        hipLaunchKernelGGL(k_png_frame, dim3((unsigned)n_seg), dim3(64), 0, ctx->stream, a);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "png.crc");
        hipLaunchKernelGGL(k_png_crc, dim3((unsigned)n_seg), dim3(DFL_THREADS), 0, ctx->stream, a, p);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, "png.copy");
        HIP_TRY(hipMemcpyAsync(&err, a.err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out, s->out.as<uint8_t>(), total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!err) return VFSMS_OK;
    vfsms_set_error("png: the coded segments outgrew the %zu bytes counted for them", total);
    return VFSMS_ERR_CAPACITY;
}
