// The lossless tile coder of Method.pyramidCompression = "deflate-device" as plain C++ that compiles for the host and for the device: the
// length-symbol table, the position-local token rule, the code-length construction and the bits of a tile's frame.
// csrc/deflate_kernels.hip calls it from its kernels, tools/deflate_core_host_check.cpp from a host program that codes a tile serially (and
// under sanitizers).  Specified by tests/deflate_ref.py.  No allocation, no recursion, every loop bounded by its arguments.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define DFL_HD __host__ __device__ __forceinline__
#else
#define DFL_HD inline
#endif

#define DFL_SYMS 286                    // literal/length symbols (HLIT = 29)
#define DFL_END 256
#define DFL_MAX_BITS 15
#define DFL_MAX_MATCH 258
#define DFL_HEAD_BITS (16 + 3 + 5 + 5 + 4 + 19 * 3 + (DFL_SYMS + 1) * 4)      // 78 01, the block's header, the 286 + 1 lengths: 1238 bits in front of the tokens
#define DFL_ADLER_MOD 65521u

// ---- tokens ---------------------------------------------------------------------------------------------------------------------------------
// a token: a literal byte 0..255, a match of length L at distance 1 as 256 + L (259..514), or DFL_NONE for a byte inside a match
#define DFL_NONE (-1)
// the symbol of a match length 3..258 with its extra bits (RFC 1951, 3.2.5)
DFL_HD int dfl_len_symbol(int L, int *extra_bits, int *extra_val)
{
    // the table in closed form: symbols 257..264 are the lengths 3..10; from 265 on four symbols share each power of two of L - 3, with
    // e = 1..5 extra bits: base 11, 13, 15, 17 | 19, 23, 27, 31 | 35, 43, 51, 59 | 67, 83, 99, 115 | 131, 163, 195, 227; 285 is 258 alone
    *extra_bits = 0; *extra_val = 0;
    if (L == DFL_MAX_MATCH) return 285;
    if (L < 11) return 254 + L;
    const int x = L - 3, e = 29 - __builtin_clz((unsigned)x), q = (x >> e) & 3;
    *extra_bits = e; *extra_val = x - ((4 + q) << e);
    return 261 + 4 * e + q;
}
// the byte `value` at offset o of a run of n equal bytes: the first byte of a run is a literal; of the n - 1 behind it every 258 are one match
// while at least 3 are left, and what is left (0..2 bytes) are literals
DFL_HD int dfl_token(int o, int n, int value)
{
    if (o == 0) return value;
    const int m = (o - 1) / DFL_MAX_MATCH, i = (o - 1) - m * DFL_MAX_MATCH;
    const int left = n - 1 - DFL_MAX_MATCH * m;
    const int L = left < DFL_MAX_MATCH ? left : DFL_MAX_MATCH;
    if (L < 3) return value;
    return i == 0 ? 256 + L : DFL_NONE;
}
DFL_HD int dfl_token_symbol(int tok) { int eb, ev; return tok < 256 ? tok : dfl_len_symbol(tok - 256, &eb, &ev); }
// the bits a symbol's occurrences take beyond its code: the extra bits and the one distance bit of a match
DFL_HD int dfl_symbol_tail_bits(int s)
{
    if (s <= 256) return 0;
    if (s < 265 || s == 285) return 1;
    return ((s - 261) >> 2) + 1;
}

// ---- code lengths -------------------------------------------------------------------------------------------------------------------------------
// Huffman lengths by the two-queue construction: leaves ordered by (count, symbol); at equal weight a leaf goes before an internal node,
// internal nodes in creation order.  A code deeper than 15 bits: every non-zero count becomes (c + 1) >> 1 and the build runs again.
struct DflBuild {
    int n;                                          // used symbols
    uint16_t order[DFL_SYMS];                       // ascending by (count, symbol)
    uint32_t weight[2 * DFL_SYMS - 1];
    uint16_t parent[2 * DFL_SYMS - 1];              // leaves 0 .. n - 1 in `order`, internal nodes n .. 2 n - 2 in creation order, the last the root
};
// where symbol s stands among the used symbols (position-local: the device ranks all symbols at once)
DFL_HD int dfl_rank(const uint32_t *counts, int s)
{
    int r = 0;
    const uint32_t c = counts[s];
    for (int t = 0; t < DFL_SYMS; t++) r += counts[t] != 0 && (counts[t] < c || (counts[t] == c && t < s));
    return r;
}
DFL_HD int dfl_used(const uint32_t *counts) { int n = 0; for (int t = 0; t < DFL_SYMS; t++) n += counts[t] != 0; return n; }
// w->order and w->n (>= 2) are set: the tree, by merging the two lightest of the next leaf and the next internal node n - 1 times
DFL_HD void dfl_merge(DflBuild *w, const uint32_t *counts)
{
    const int n = w->n;
    for (int k = 0; k < n; k++) w->weight[k] = counts[w->order[k]];
    int li = 0, ii = n;                             // the next leaf, the next internal node
    for (int node = n; node < 2 * n - 1; node++) {
        uint32_t sum = 0;
        for (int two = 0; two < 2; two++) {
            int pick;
            if (li < n && (ii >= node || w->weight[li] <= w->weight[ii])) pick = li++; else pick = ii++;
            w->parent[pick] = (uint16_t)node;
            sum += w->weight[pick];
        }
        w->weight[node] = sum;
    }
}
// the depth of leaf k of the merged tree: the nodes above it (position-local: the device walks all leaves at once)
DFL_HD int dfl_leaf_depth(const DflBuild *w, int k)
{
    int d = 0;
    for (int node = k; node != 2 * w->n - 2; node = w->parent[node]) d++;
    return d;
}
// w->order and w->n are set: the lengths of all 286 symbols; returns the deepest
DFL_HD int dfl_build(DflBuild *w, const uint32_t *counts, uint8_t *lens)
{
    for (int s = 0; s < DFL_SYMS; s++) lens[s] = 0;
    if (w->n == 0) return 0;
    if (w->n == 1) { lens[w->order[0]] = 1; return 1; }
    dfl_merge(w, counts);
    int deepest = 0;
    for (int k = 0; k < w->n; k++) {
        const int d = dfl_leaf_depth(w, k);
        lens[w->order[k]] = (uint8_t)(d > 255 ? 255 : d);
        if (d > deepest) deepest = d;
    }
    return deepest;
}
DFL_HD void dfl_halve(uint32_t *counts, int s) { if (counts[s]) counts[s] = (counts[s] + 1) >> 1; }

// the whole construction, serially: counts[286] (changed when the limit is hit) -> lens[286]; returns how often the counts were halved;
// *unlimited = the deepest code of the first build
DFL_HD int dfl_code_lengths(uint32_t *counts, uint8_t *lens, DflBuild *w, int *unlimited)
{
    for (int halvings = 0;; halvings++) {
        w->n = dfl_used(counts);
        for (int s = 0; s < DFL_SYMS; s++) if (counts[s]) w->order[dfl_rank(counts, s)] = (uint16_t)s;
        const int deepest = dfl_build(w, counts, lens);
        if (halvings == 0 && unlimited) *unlimited = deepest;
        if (deepest <= DFL_MAX_BITS) return halvings;
        for (int s = 0; s < DFL_SYMS; s++) dfl_halve(counts, s);
    }
}

// ---- codes and the bits of a tile -----------------------------------------------------------------------------------------------------------------
// the low `nbits` (0..16) bits of code, first bit last
DFL_HD uint32_t dfl_reverse(uint32_t code, int nbits)
{
    uint32_t r = code & 0xffffu;
    r = ((r & 0x5555u) << 1) | ((r >> 1) & 0x5555u);
    r = ((r & 0x3333u) << 2) | ((r >> 2) & 0x3333u);
    r = ((r & 0x0f0fu) << 4) | ((r >> 4) & 0x0f0fu);
    r = ((r & 0x00ffu) << 8) | (r >> 8);
    return r >> (16 - nbits);
}
// canonical codes as RFC 1951, 3.2.2 assigns them.  first[b], b = 1 .. 15: the first code of length b
DFL_HD void dfl_code_starts(const uint8_t *lens, uint32_t *first)
{
    uint32_t count[DFL_MAX_BITS + 1] = {};
    for (int s = 0; s < DFL_SYMS; s++) if (lens[s]) count[lens[s]]++;
    uint32_t code = 0;
    first[0] = 0;
    for (int b = 1; b <= DFL_MAX_BITS; b++) { code = (code + count[b - 1]) << 1; first[b] = code; }
}
// symbol s's table entry, (the code, first bit lowest) << 4 | length: its code is the first of its length plus the symbols of that length
// in front of it (position-local: the device codes all symbols at once)
DFL_HD uint32_t dfl_code_entry(const uint8_t *lens, const uint32_t *first, int s)
{
    const int len = lens[s];
    if (!len) return 0;
    uint32_t code = first[len];
    for (int t = 0; t < s; t++) code += lens[t] == len;
    return (dfl_reverse(code, len) << 4) | (uint32_t)len;
}
DFL_HD void dfl_codes(const uint8_t *lens, uint32_t *table)
{
    uint32_t first[DFL_MAX_BITS + 1];
    dfl_code_starts(lens, first);
    for (int s = 0; s < DFL_SYMS; s++) table[s] = dfl_code_entry(lens, first, s);
}
// a token's bits, first bit lowest: its code, and for a match its extra bits and the distance code 0 (at most 15 + 5 + 1 bits)
DFL_HD uint32_t dfl_token_bits(int tok, const uint32_t *table, int *nbits)
{
    if (tok < 256) { const uint32_t e = table[tok]; *nbits = (int)(e & 15); return e >> 4; }
    int eb, ev;
    const uint32_t e = table[dfl_len_symbol(tok - 256, &eb, &ev)];
    const int len = (int)(e & 15);
    *nbits = len + eb + 1;
    return (e >> 4) | ((uint32_t)ev << len);
}
// the bits of the tokens counted in hist[286] (end of block included) under `lens`
DFL_HD unsigned long long dfl_block_bits(const uint32_t *hist, const uint8_t *lens)
{
    unsigned long long bits = 0;
    for (int s = 0; s < DFL_SYMS; s++) bits += (unsigned long long)hist[s] * (unsigned)(lens[s] + dfl_symbol_tail_bits(s));
    return bits;
}
// a tile's stream: 78 01, the block (header, tokens, end of block, zero bits up to a byte), the Adler-32 of the predicted bytes
DFL_HD unsigned long long dfl_stream_bytes(unsigned long long block_bits) { return (DFL_HEAD_BITS + block_bits + 7) / 8 + 4; }
// the DFL_HEAD_BITS bits in front of the tokens through put(value, nbits) (first bit lowest, at most 8 bits a call): the zlib header; BFINAL = 1,
// BTYPE = 2, HLIT = 29, HDIST = 0, HCLEN = 15; the code-length code lengths 4 for 0..15 and 0 for 16, 17, 18 (sent in RFC 1951's order 16, 17,
// 18, 0, 8, ...), under which symbol s is the 4-bit code s; the 286 lengths and the one distance length 1
// (dfl_block_head: the block's header alone, with BFINAL = `bfinal`: a block of png_core.h's segments is not final)
template <class Put> DFL_HD void dfl_block_head(const uint8_t *lens, Put &put, unsigned bfinal)
{
    put(bfinal, 1); put(2u, 2); put(29u, 5); put(0u, 5); put(15u, 4);
    for (int k = 0; k < 19; k++) put(k < 3 ? 0u : 4u, 3);
    for (int s = 0; s < DFL_SYMS; s++) put(dfl_reverse(lens[s], 4), 4);
    put(dfl_reverse(1, 4), 4);
}
template <class Put> DFL_HD void dfl_head(const uint8_t *lens, Put &put)
{
    put(0x78u, 8); put(0x01u, 8);
    dfl_block_head(lens, put, 1u);
}
// running Adler-32 sums of bytes d[0 .. n) of a string of `total` bytes, d[0] at position `at`: a += sum d, b += sum (total - position) d; the
// caller reduces modulo 65521 (b grows by at most 255 * total a byte) and adds the string's own 1 and `total`
DFL_HD uint32_t dfl_adler(uint32_t a, uint32_t b) { return (b % DFL_ADLER_MOD) << 16 | (a % DFL_ADLER_MOD); }
