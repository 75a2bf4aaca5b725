// The PNG coder of Method.pngEncoder = "device" as plain C++ that compiles for the host and for the device, on top of deflate_core.h (tokens,
// code lengths, codes): the Paeth predictor, the five filters and a byte's cost, a segment's frame (chunk head, block head with BFINAL = 0, the
// empty stored block behind the end of block), the CRC-32 step with the product that joins spans, and the Adler-32 of two strings joined.
// csrc/deflate_kernels.hip calls it from its kernels, tools/png_core_host_check.cpp from a host program that codes an image serially (and under
// sanitizers).  Specified by tests/png_ref.py.  No allocation, no recursion, every loop bounded by its arguments.
#pragma once
#include "deflate_core.h"

#define PNG_MAX_SEGMENT_ROWS 4096
#define PNG_TYPES 5
// a segment's chunk in front of its tokens: the length and "IDAT" (64 bits), then the block's header without the zlib header
#define PNG_HEAD_BITS (64 + DFL_HEAD_BITS - 16)
#define PNG_CRC_POLY 0xEDB88320u

// ---- filters ------------------------------------------------------------------------------------------------------------------------------------
// the first of a (left), b (above), c (above left) nearest to a + b - c
DFL_HD int png_paeth(int a, int b, int c)
{
    const int p = a + b - c;
    const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pc = p > c ? p - c : c - p;
    if (pa <= pb && pa <= pc) return a;
    return pb <= pc ? b : c;
}
// the byte x under filter `type` (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth)
DFL_HD int png_filter(int type, int x, int a, int b, int c)
{
    const int pred = type == 0 ? 0 : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : png_paeth(a, b, c);
    return (x - pred) & 255;
}
// |v| as a signed byte; 128 costs 128
DFL_HD int png_cost(int v) { return v < 256 - v ? v : 256 - v; }
// the type of the smallest cost, ties to the lowest
DFL_HD int png_choose(const unsigned *cost)
{
    int best = 0;
    for (int t = 1; t < PNG_TYPES; t++) if (cost[t] < cost[best]) best = t;
    return best;
}
// whether `segment_rows` rows of rowbytes = 1 + cols * ch bytes are a segment the coder takes: its bits at 15 a byte fit 32 bits
DFL_HD int png_segment_fits(int segment_rows, long long rowbytes)
{
    return segment_rows >= 1 && segment_rows <= PNG_MAX_SEGMENT_ROWS && (unsigned long long)segment_rows * (unsigned long long)rowbytes * DFL_MAX_BITS <= 0xffffffffull;
}

// ---- a segment's chunk ----------------------------------------------------------------------------------------------------------------------------
// length, "IDAT", the block (header, tokens, end of block), three zero bits (an empty stored block, not final), zero bits up to the byte,
// 00 00 FF FF, the CRC-32
DFL_HD unsigned long long png_chunk_bytes(unsigned long long block_bits) { return (PNG_HEAD_BITS + block_bits + 3 + 7) / 8 + 4 + 4; }
// the 64 bits in front of the block through put(value, nbits) (first bit lowest, at most 8 bits a call), given the chunk's bytes
template <class Put> DFL_HD void png_chunk_head(unsigned long long chunk_bytes, Put &put)
{
    const uint32_t n = (uint32_t)(chunk_bytes - 12);
    put(n >> 24, 8); put((n >> 16) & 255, 8); put((n >> 8) & 255, 8); put(n & 255, 8);
    put('I', 8); put('D', 8); put('A', 8); put('T', 8);
}

// ---- CRC-32 (zlib's: reflected, bit 31 of a value is x^0) -------------------------------------------------------------------------------------------
// the raw remainder after one more byte (no initial or final complement)
DFL_HD uint32_t png_crc_byte(uint32_t r, uint32_t byte)
{
    r ^= byte;
    for (int k = 0; k < 8; k++) r = (r >> 1) ^ (PNG_CRC_POLY & (0u - (r & 1u)));
    return r;
}
// a * b in GF(2)[x] / P: 32 steps of shift and xor
DFL_HD uint32_t png_gf_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 0; i < 32; i++) {
        p ^= b & (0u - ((a >> (31 - i)) & 1u));
        b = (b >> 1) ^ (PNG_CRC_POLY & (0u - (b & 1u)));
    }
    return p;
}
// pow8[k] = x^(8 * 2^k), k = 0 .. 31
struct PngCrcPowers { uint32_t pow8[32]; };
DFL_HD void png_crc_powers(PngCrcPowers *t)
{
    t->pow8[0] = 0x00800000u;
    for (int k = 1; k < 32; k++) t->pow8[k] = png_gf_mul(t->pow8[k - 1], t->pow8[k - 1]);
}
// x^(8 n)
DFL_HD uint32_t png_xpow8(const PngCrcPowers *t, uint32_t n)
{
    uint32_t r = 0x80000000u;
    for (int k = 0; n; k++, n >>= 1) if (n & 1u) r = png_gf_mul(r, t->pow8[k]);
    return r;
}
// the raw remainder of A || B from those of A and B: raw(A) x^(8 |B|) + raw(B)
DFL_HD uint32_t png_crc_join(const PngCrcPowers *t, uint32_t ra, uint32_t rb, uint32_t len_b) { return png_gf_mul(ra, png_xpow8(t, len_b)) ^ rb; }
// zlib's crc32 of n bytes from their raw remainder: the initial complement travels through n bytes, the final one is applied
DFL_HD uint32_t png_crc_finish(const PngCrcPowers *t, uint32_t raw, uint32_t n) { return raw ^ png_gf_mul(0xffffffffu, png_xpow8(t, n)) ^ 0xffffffffu; }

// ---- Adler-32 ----------------------------------------------------------------------------------------------------------------------------------------
// of A || B from those of A and B and B's length
DFL_HD uint32_t png_adler_combine(uint32_t a1, uint32_t a2, unsigned long long len2)
{
    const unsigned long long M = DFL_ADLER_MOD, rem = len2 % M;
    const unsigned long long s1 = a1 & 0xffffu, s2 = a1 >> 16, t1 = a2 & 0xffffu, t2 = a2 >> 16;
    const unsigned long long lo = (s1 + t1 + M - 1) % M, hi = (s2 + t2 + rem * s1 + M * M - rem) % M;
    return (uint32_t)(hi << 16 | lo);
}
// of a string of n bytes from its sums a = sum d, b = sum (n - position) d (any size: reduced here)
DFL_HD uint32_t png_adler_of_sums(unsigned long long a, unsigned long long b, unsigned long long n)
{
    return dfl_adler((uint32_t)((1 + a % DFL_ADLER_MOD) % DFL_ADLER_MOD), (uint32_t)((n % DFL_ADLER_MOD + b % DFL_ADLER_MOD) % DFL_ADLER_MOD));
}
