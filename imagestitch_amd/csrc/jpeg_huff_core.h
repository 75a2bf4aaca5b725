// The entropy decoder of Method.jpegDecoder = "device-entropy" as plain C++ that compiles for the host and for the device: the decode step and
// the decode of one subsequence.  csrc/jpeg_huff_kernels.hip calls it from its kernels, tools/jpeg_huff_host.cpp from a host program that runs
// the same rounds serially (and under sanitizers), vfsms_jpeg_scan (csrc/jpeg_host.cpp) builds the tables and the scan record with it.
// Specified by tests/jpeg_huff_ref.py.  No allocation, no recursion, every loop bounded by its arguments.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define JH_HD __host__ __device__ __forceinline__
#else
#define JH_HD inline
#endif

// ---- the scan record: what vfsms_jpeg_scan writes and the device reads (every offset a multiple of 4 bytes from the record's start) --------
#define JH_LOOK_BITS 9
struct JpegHuffTable {                  // one Huffman table, ready to decode with
    uint16_t look[1 << JH_LOOK_BITS];   // the next 9 bits -> (length << 8) | symbol for codes of up to 9 bits, 0: a longer code, or none
    int32_t maxcode[17];                // [l], l = 1..16: the largest code of length l, -1 when there is none
    int32_t valoff[17];                 // [l]: index into vals of the first symbol of length l, minus its code
    uint8_t vals[256];
    uint8_t counts[16];                 // as in the file's DHT segment; sum = the number of symbols
};
struct JpegHuffSeg { uint32_t byte_off, byte_count, first_mcu, sub0; };   // a restart interval: its bytes in the stream (byte_off a multiple of 4,
                                                                         // padded with FF to one), its first MCU, its first subsequence
struct JpegScanHeader {
    int32_t h, w, ncomp, grid6[6];
    int32_t restart_interval, nseg, nsub, mcus, blocks_per_mcu, sub_bits;
    uint32_t stream_bytes;              // the unstuffed stream, segment padding included
    uint32_t off_quant;                 // uint16[64] natural order per component (VFSMS_JPEG_COEF_TABLE_BYTES each)
    uint32_t off_tables;                // JpegHuffTable[2 * ncomp]: component k's DC table at 2 k, its AC table at 2 k + 1
    uint32_t off_stream, off_seg;       // bytes; JpegHuffSeg[nseg]
    uint32_t off_subseg;                // uint32[nsub]: the segment of every subsequence
    uint32_t total_bytes;
};
#define JH_DAMAGE_CODE 1                // a bit pattern that is no code of its table
#define JH_DAMAGE_INDEX 2               // a coefficient position beyond 63
#define JH_DAMAGE_BITS 4                // a segment's bits exhausted before its blocks are complete

// counts[16] + values -> the table.  False for counts that are no prefix code (a code that does not fit its length, more than 256 symbols)
inline bool jh_build_table(const uint8_t counts[16], const uint8_t *values, JpegHuffTable *t)
{
    memset(t, 0, sizeof(*t));
    unsigned code = 0, k = 0;
    for (int l = 1; l <= 16; l++) {
        t->maxcode[l] = -1; t->valoff[l] = 0;
        const unsigned n = counts[l - 1];
        if (n) {
            if (k + n > 256 || code + n > (1u << l)) return false;
            t->valoff[l] = (int32_t)k - (int32_t)code;
            for (unsigned i = 0; i < n; i++, code++, k++) {
                t->vals[k] = values[k];
                if (l <= JH_LOOK_BITS)
                    for (unsigned f = code << (JH_LOOK_BITS - l); f < ((code + 1) << (JH_LOOK_BITS - l)); f++) t->look[f] = (uint16_t)((l << 8) | values[k]);
            }
            t->maxcode[l] = (int32_t)code - 1;
        }
        code <<= 1;
    }
    memcpy(t->counts, counts, 16);
    return true;
}

// ---- the bit reader: a segment as big-endian dwords; nwords = its padded length.  Every read is clamped to the segment: a word beyond it
// reads as all ones, and so do the FF bytes the scan pads the last word with ------------------------------------------------------------------
struct JpegHuffBits { const uint32_t *words; uint32_t nwords, nbits; };
JH_HD uint32_t jh_bswap(uint32_t v) { return (v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24); }
JH_HD uint32_t jh_word(const JpegHuffBits &B, uint32_t i) { return i < B.nwords ? jh_bswap(B.words[i]) : 0xFFFFFFFFu; }
// A decoder reads its stream front to back and a step moves it by fewer than 32 bits, so the words are kept in registers: w0, w1 hold the
// 64 bits from word wi on, w2 is word wi + 2, asked for one word ahead -- its load is off the path from one symbol to the next
struct JpegHuffWindow { uint32_t wi, w0, w1, w2; };
JH_HD void jh_window_open(const JpegHuffBits &B, uint32_t p, JpegHuffWindow &W)
{
    W.wi = p >> 5; W.w0 = jh_word(B, W.wi); W.w1 = jh_word(B, W.wi + 1); W.w2 = jh_word(B, W.wi + 2);
}
// the 32 bits from position p on
JH_HD uint32_t jh_peek32(const JpegHuffBits &B, JpegHuffWindow &W, uint32_t p)
{
    const uint32_t t = p >> 5;
    if (t != W.wi) {
        if (t == W.wi + 1) { W.wi = t; W.w0 = W.w1; W.w1 = W.w2; W.w2 = jh_word(B, t + 2); }
        else jh_window_open(B, p, W);
    }
    return (uint32_t)(((((uint64_t)W.w0) << 32) | W.w1) >> (32 - (p & 31)));
}

struct JpegHuffState { uint32_t p, cz; };             // bit position in the segment; (block in MCU << 8) | coefficient index
JH_HD bool jh_same(const JpegHuffState &a, const JpegHuffState &b) { return a.p == b.p && a.cz == b.cz; }
struct JpegHuffStep { int zi, value; bool coef, closed; unsigned damage; };

// the decode step (tests/jpeg_huff_ref.py: step).  v: the 32 bits from s.p on; dc / ac: the tables of the block s.cz >> 8.  Total: defined for
// every bit pattern and state
JH_HD JpegHuffStep jh_step(uint32_t v, const JpegHuffTable *dc, const JpegHuffTable *ac, int blocks_per_mcu, JpegHuffState &s)
{
    JpegHuffStep r; r.zi = 0; r.value = 0; r.coef = false; r.closed = false; r.damage = 0;
    int z = (int)(s.cz & 255u); unsigned c = s.cz >> 8;
    const JpegHuffTable *T = z == 0 ? dc : ac;
    unsigned len, sym;
    const unsigned e = T->look[v >> (32 - JH_LOOK_BITS)];
    if (e) { len = e >> 8; sym = e & 255u; }
    else {
        len = 16; sym = 0; r.damage = JH_DAMAGE_CODE;
        for (int l = JH_LOOK_BITS + 1; l <= 16; l++) {
            const int32_t code = (int32_t)(v >> (32 - l));
            if (code <= T->maxcode[l]) { len = (unsigned)l; sym = T->vals[(unsigned)(T->valoff[l] + code) & 255u]; r.damage = 0; break; }
        }
    }
    const unsigned size = sym & 15u;
    int x = 0;
    if (size) {
        x = (int)((v << len) >> (32 - size));
        if (x < (1 << (size - 1))) x -= (1 << size) - 1;
    }
    s.p += len + size;
    if (z == 0) { r.coef = true; r.zi = 0; r.value = x; z = 1; }
    else {
        const int run = (int)(sym >> 4);
        if (size == 0) {
            if (run == 15) { z += 16; if (z > 63) { r.damage |= JH_DAMAGE_INDEX; r.closed = true; } }
            else r.closed = true;
        } else {
            z += run;
            if (z > 63) { r.damage |= JH_DAMAGE_INDEX; r.closed = true; }
            else { r.coef = true; r.zi = z; r.value = x; z++; r.closed = z == 64; }
        }
    }
    if (r.closed) { c = c + 1 == (unsigned)blocks_per_mcu ? 0 : c + 1; z = 0; }
    s.cz = (c << 8) | (unsigned)z;
    return r;
}

// what a subsequence leaves behind: its exit state, the blocks it closed and the sum of the DC differences it decoded, per component
struct JpegHuffSubOut { JpegHuffState exit; uint32_t blocks; uint32_t dc[3]; };

JH_HD int jh_comp_of(int blocks_per_mcu, unsigned c) { return blocks_per_mcu == 1 || c < 4 ? 0 : (int)c - 3; }

// Decode from `entry` until the position reaches `end` (a symbol that straddles the end is finished) or `block_limit` blocks counted from
// `block0` are complete.  tables: [2 * component + (0: DC, 1: AC)].  sink(block, zi, value, component) sees every coefficient, the DC ones as
// DIFFERENCES; *damage collects the damage bits of the steps taken.  At most end - entry.p steps: every step consumes a bit.
template <class Sink>
JH_HD JpegHuffSubOut jh_decode_sub(const JpegHuffBits &B, const JpegHuffTable *tables, int blocks_per_mcu, JpegHuffState entry, uint32_t end,
                                   uint32_t block0, uint32_t block_limit, Sink &sink, unsigned *damage)
{
    JpegHuffSubOut o; o.exit = entry; o.blocks = 0; o.dc[0] = o.dc[1] = o.dc[2] = 0;
    uint32_t blk = block0;
    JpegHuffWindow W; jh_window_open(B, entry.p, W);
    while (o.exit.p < end && blk < block_limit) {
        const int comp = jh_comp_of(blocks_per_mcu, o.exit.cz >> 8);
        const JpegHuffStep r = jh_step(jh_peek32(B, W, o.exit.p), tables + 2 * comp, tables + 2 * comp + 1, blocks_per_mcu, o.exit);
        *damage |= r.damage;
        if (r.coef) {
            if (r.zi == 0) {                                     // (selects, not an index: the sums stay in registers)
                const uint32_t v = (uint32_t)r.value;
                o.dc[0] += comp == 0 ? v : 0u; o.dc[1] += comp == 1 ? v : 0u; o.dc[2] += comp == 2 ? v : 0u;
            }
            sink(blk, r.zi, r.value, comp);
        }
        if (r.closed) { blk++; o.blocks++; }
    }
    return o;
}
struct JpegHuffNoSink { JH_HD void operator()(uint32_t, int, int, int) const {} };

// where a block of the scan lies: g = its number in scan order (MCU after MCU; a 4:2:0 MCU is four luma blocks, Cb, Cr) -> its index on its
// component's block-row-major grid.  False for a block beyond the scan or the grid: nothing is stored then
struct JpegHuffPlace { uint32_t blocks[3]; int bcols[3]; int bpm, gray_cols; uint32_t nblocks; };
JH_HD bool jh_place(const JpegHuffPlace &P, uint32_t g, int comp, uint32_t *b)
{
    if (g >= P.nblocks) return false;
    if (P.bpm == 1) *b = (g / (uint32_t)P.gray_cols) * (uint32_t)P.bcols[0] + g % (uint32_t)P.gray_cols;
    else {
        const uint32_t m = g / 6u, c = g - 6u * m, my = m / (uint32_t)P.bcols[1], mx = m - my * (uint32_t)P.bcols[1];
        *b = c < 4 ? (2 * my + (c >> 1)) * (uint32_t)P.bcols[0] + 2 * mx + (c & 1) : m;
    }
    return *b < (comp == 0 ? P.blocks[0] : comp == 1 ? P.blocks[1] : P.blocks[2]);
}
// the record's grids against its frame: what jh_place relies on
inline bool jh_place_from_header(const JpegScanHeader &H, JpegHuffPlace *P)
{
    memset(P, 0, sizeof(*P));
    for (int k = 0; k < H.ncomp && k < 3; k++) { P->bcols[k] = H.grid6[2 * k + 1]; P->blocks[k] = (uint32_t)H.grid6[2 * k] * (uint32_t)H.grid6[2 * k + 1]; }
    P->bpm = H.blocks_per_mcu; P->gray_cols = (H.w + 7) / 8; P->nblocks = (uint32_t)H.mcus * (uint32_t)H.blocks_per_mcu;
    if (H.h < 1 || H.w < 1 || P->gray_cols > P->bcols[0]) return false;
    if (H.blocks_per_mcu == 6)
        return H.ncomp == 3 && P->bcols[0] == 2 * P->bcols[1] && P->bcols[2] == P->bcols[1] && H.mcus == H.grid6[2] * H.grid6[3] && H.grid6[0] == 2 * H.grid6[2] && H.grid6[4] == H.grid6[2];
    return H.blocks_per_mcu == 1 && (long long)H.mcus <= (long long)P->gray_cols * H.grid6[0];
}
// a segment's blocks: the MCUs of its restart interval, the last one cut at the frame's end
JH_HD uint32_t jh_segment_blocks(const JpegScanHeader &H, uint32_t first_mcu)
{
    const uint32_t mcus = (uint32_t)H.mcus, m0 = first_mcu < mcus ? first_mcu : mcus;
    const uint32_t nm = H.restart_interval && (uint32_t)H.restart_interval < mcus - m0 ? (uint32_t)H.restart_interval : mcus - m0;
    return nm * (uint32_t)H.blocks_per_mcu;
}
