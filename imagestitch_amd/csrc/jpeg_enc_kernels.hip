// jpeg_enc_kernels.hip -- the baseline JPEG encoder on the device (Method.jpegEncoder = "device"; specified by tests/jpeg_enc_ref.py, whose
// files at one restart interval are libjpeg's byte for byte).  A band of canvas rows (or a staged image) leaves the device as its
// entropy-coded bytes instead of its pixels.  Profile stages "jpeg_encode.transform", "jpeg_encode.entropy", "jpeg_encode.copy".
//
//   k_jpeg_transform   one workgroup per strip of an MCU row (16 colour MCUs / 96 gray MCUs = 96 blocks of 8 x 8): the strip's rows are read
//                      with aligned dword loads into LDS, then colour conversion (jccolor.c), edge replication, the 2 x 2 chroma box
//                      (jcsample.c), jfdctint.c's two passes (8 lanes per block) and jcdctmgr.c's quantisation, all in 32-bit integers,
//                      and the quantised int16 coefficients leave in zigzag order, MCU-major, as 16-byte stores
//   k_jpeg_entropy     one LANE per restart interval runs jchuff.c's coder over the interval's coefficients (the DC predictor starts at 0 and
//                      is carried inside the lane, so intervals share nothing).  Twice: <false> counts the interval's exact bytes (stuffed
//                      0x00s and the RSTn marker included), k_jpeg_scan turns the counts into offsets, <true> writes.  A wave's 64 intervals
//                      are one contiguous range of the output: the lanes put their bytes into an LDS window over that range and the wave
//                      flushes the window with 16-byte stores (the bytes a window shares with its neighbours' 16-byte units go out one by one)
// The sizes are exact, so the output buffer is allocated after the counting pass and cannot overflow; the writing pass still takes its
// capacity and raises a flag instead of storing beyond it.
// Tile order (the TILES instantiations; Method.pyramidCompression = "jpeg", specified by tests/tiff_jpeg_ref.py): the same two kernels over the
// tiles of a pyramid level, every tile an image of its own -- edges replicated, its prefix (SOI .. SOS) in front and EOI behind -- so that
// a band leaves as finished tile streams.  Profile stages "pyramid_jpeg.transform", ".entropy", ".copy".
#include "common.h"
#include <string.h>

namespace {

constexpr int JE_BLOCKS = 96;            // 8 x 8 blocks per workgroup of the transform
constexpr int JE_ROWB = 768;             // bytes of a strip row: 256 B G R pixels or 768 gray ones
constexpr int JE_PITCH = JE_ROWB + 16;   // LDS pitch of a raw row
constexpr int JE_WINDOW = 32768;         // LDS bytes over a wave's output range (k_jpeg_entropy<true>)

__constant__ uint8_t c_zigzag_of[64] = {  // natural position -> zigzag index
    0, 1, 5, 6, 14, 15, 27, 28, 2, 4, 7, 13, 16, 26, 29, 42, 3, 8, 12, 17, 25, 30, 41, 43, 9, 11, 18, 24, 31, 40, 44, 53,
    10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38, 46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K (jchuff.c: jpeg_make_c_derived_tbl of the standard tables): code << 5 | length per symbol; [0] luminance, [1] chrominance
struct HuffTables { uint32_t dc[2][12]; uint32_t ac[2][256]; };
__constant__ HuffTables c_huff;

// quantisation: q (natural order) and ceil(2^32 / (8 q)).  (n * recip) >> 32 == n / (8 q) for every n < 2^32 / (8 q): the product's excess
// over n * 2^32 / (8 q) is below n, hence below 2^32 / (8 q), which cannot carry the quotient over.  n = |coefficient| + 4 q < 2^17 here
// (jfdctint.c's outputs are below 2^16) and 8 q <= 2040, so the condition holds with room to spare
struct JpegQuant { uint32_t recip[2][64]; uint8_t q[2][64]; };

struct JpegXformArgs {
    const uint8_t *src; size_t src_bytes;   // the image the rows belong to (its first byte is 256-byte aligned) and its size
    size_t pitch;                           // bytes between rows
    int rows, cols;                         // image size
    int row0;                               // first row of the band (a multiple of the MCU height)
    int mw;                                 // MCUs per row
    int bgr;                                // colour: B G R (else R G B)
    int16_t *coef;                          // [band MCU][blocks per MCU][64]
    JpegQuant qt;
    // tile order (k_jpeg_transform<.., true>): the image is a pyramid level cut into tm x tm MCU tiles, ntx of them in a row; `mw` is the
    // tile-padded MCU count ntx * tm, row0 a multiple of the tile side, and row y of the level lies at src + (y - src_row0) * pitch
    int src_row0;
    int tm, ntx;
    long long mcu_base;                     // MCUs in front of this launch's first tile in `coef`
};

// the aligned dword at byte `a` of the image, bytes beyond its end read as 0
__device__ inline uint32_t je_dword(const uint8_t *src, size_t a, size_t total)
{
    if (a + 4 <= total) return *(const uint32_t *)(src + a);
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) if (a + k < total) v |= (uint32_t)src[a + k] << (8 * k);
    return v;
}

__device__ inline int je_descale(int x, int n) { return (x + (1 << (n - 1))) >> n; }

// jfdctint.c, one pass over d[0..7]; FIRST: the row pass (results scaled up by PASS1_BITS)
template <bool FIRST>
__device__ inline void je_fdct8(int *d)
{
    constexpr int CB = 13, PB = 2, SH = FIRST ? CB - PB : CB + PB;
    const int t0 = d[0] + d[7], t7 = d[0] - d[7], t1 = d[1] + d[6], t6 = d[1] - d[6];
    const int t2 = d[2] + d[5], t5 = d[2] - d[5], t3 = d[3] + d[4], t4 = d[3] - d[4];
    const int t10 = t0 + t3, t13 = t0 - t3, t11 = t1 + t2, t12 = t1 - t2;
    if (FIRST) { d[0] = (t10 + t11) << PB; d[4] = (t10 - t11) << PB; }
    else { d[0] = je_descale(t10 + t11, PB); d[4] = je_descale(t10 - t11, PB); }
    int z1 = (t12 + t13) * 4433;
    d[2] = je_descale(z1 + t13 * 6270, SH);
    d[6] = je_descale(z1 - t12 * 15137, SH);
    z1 = t4 + t7; int z2 = t5 + t6, z3 = t4 + t6, z4 = t5 + t7;
    const int z5 = (z3 + z4) * 9633;
    const int a4 = t4 * 2446, a5 = t5 * 16819, a6 = t6 * 25172, a7 = t7 * 12299;
    z1 *= -7373; z2 *= -20995; z3 = z3 * -16069 + z5; z4 = z4 * -3196 + z5;
    d[7] = je_descale(a4 + z1 + z3, SH);
    d[5] = je_descale(a5 + z2 + z4, SH);
    d[3] = je_descale(a6 + z2 + z3, SH);
    d[1] = je_descale(a7 + z1 + z4, SH);
}

// jccolor.c: 16-bit fixed point
__device__ inline int je_y(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }
__device__ inline int je_cb(int r, int g, int b) { return (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16; }
__device__ inline int je_cr(int r, int g, int b) { return (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16; }

// COLOR: 16 MCUs of 16 x 16 (Y00 Y01 Y10 Y11 Cb Cr); else 96 MCUs of one 8 x 8 block.  grid: (strips of an MCU row, MCU rows of the band)
// TILES: every tile is an image of its own (tests/tiff_jpeg_ref.py).  The MCU grid is the tile grid's, so MCU rows and columns may lie wholly
// beyond the level: source rows and columns are clamped to the level's last (a strip that starts beyond the last column holds that column
// alone), there are no dummy blocks, and an MCU goes to [tile in the row of tiles][MCU row in tile][MCU column in tile]
template <bool COLOR, bool TILES>
__global__ void __launch_bounds__(256) k_jpeg_transform(const JpegXformArgs a)
{
    constexpr int CH = COLOR ? 3 : 1, MCU = COLOR ? 16 : 8, MPW = COLOR ? 16 : 96, BPM = COLOR ? 6 : 1, SW = JE_ROWB / CH;
    constexpr int RAW = MCU * JE_PITCH > JE_BLOCKS * 128 ? MCU * JE_PITCH : JE_BLOCKS * 128;
    __shared__ __attribute__((aligned(16))) uint8_t raw[RAW];                 // the strip's rows; later the quantised coefficients (12288 bytes)
    __shared__ __attribute__((aligned(16))) uint8_t yp[COLOR ? 16 * 256 : 16];
    __shared__ __attribute__((aligned(16))) uint8_t cbcr[COLOR ? 2 * 8 * 128 : 16];
    __shared__ __attribute__((aligned(16))) int16_t ws[JE_BLOCKS * 64];
    const int tid = threadIdx.x;
    const int mx0 = blockIdx.x * MPW, my = blockIdx.y;
    const int x0 = mx0 * MCU, y0 = a.row0 + my * MCU;
    const int nvalid = min(MPW, a.mw - mx0);                                  // MCUs of this strip
    const int sx0 = TILES ? min(x0, a.cols - 1) : x0;                         // the strip's first source column
    const int nb = (min(sx0 + SW, a.cols) - sx0) * CH;                        // bytes of a strip row that exist
    const int nrow = TILES ? MCU : min(MCU, a.rows - y0);                     // rows that exist (TILES: every row, clamped when it is loaded)

    // ---- the rows into LDS: dword d of a row = bytes [4 d, 4 d + 4) of the strip row, from the two aligned dwords that hold them
    {
        const int nd = (nb + 3) >> 2;
        for (int e = tid; e < nrow * (JE_ROWB / 4); e += 256) {
            const int r = e / (JE_ROWB / 4), d = e % (JE_ROWB / 4);
            if (d >= nd) continue;
            const int sr = TILES ? min(y0 + r, a.rows - 1) - a.src_row0 : y0 + r;
            const size_t g = (size_t)sr * a.pitch + (size_t)sx0 * CH + 4 * (size_t)d;
            const size_t al = g & ~(size_t)3;
            const int sh = (int)(g & 3) * 8;
            uint32_t v = je_dword(a.src, al, a.src_bytes);
            if (sh) v = (v >> sh) | (je_dword(a.src, al + 4, a.src_bytes) << (32 - sh));
            *(uint32_t *)(raw + r * JE_PITCH + 4 * d) = v;
        }
    }
    __syncthreads();

    // ---- samples: Y (and the 2 x 2 chroma box) of the 16 x 256 strip, columns clamped to the image (the right edge repeats), rows likewise
    if (COLOR) {
        const int xmax = a.cols - 1 - sx0;                                    // last column that exists, strip-relative
        const int cj_last = ((a.rows + 1) >> 1) - 1;                          // last chroma row the image has (jcprepct.c: rows repeat to an even count first)
        const int ro = a.bgr ? 2 : 0, bo = a.bgr ? 0 : 2;
        for (int q = tid; q < 8 * 128; q += 256) {
            const int qy = q >> 7, qx = q & 127;
            const int xa = min(2 * qx, xmax) * 3, xb = min(2 * qx + 1, xmax) * 3;
            const int ra = min(2 * qy, nrow - 1), rb = min(2 * qy + 1, nrow - 1);
            const uint8_t *pa = raw + ra * JE_PITCH, *pb = raw + rb * JE_PITCH;
            yp[(2 * qy) * 256 + 2 * qx] = (uint8_t)je_y(pa[xa + ro], pa[xa + 1], pa[xa + bo]);
            yp[(2 * qy) * 256 + 2 * qx + 1] = (uint8_t)je_y(pa[xb + ro], pa[xb + 1], pa[xb + bo]);
            yp[(2 * qy + 1) * 256 + 2 * qx] = (uint8_t)je_y(pb[xa + ro], pb[xa + 1], pb[xa + bo]);
            yp[(2 * qy + 1) * 256 + 2 * qx + 1] = (uint8_t)je_y(pb[xb + ro], pb[xb + 1], pb[xb + bo]);
            // chroma row j of the image is the box of rows 2 j, 2 j + 1 (the last row repeated when there is no 2 j + 1); below the image's
            // last chroma row that row repeats
            const int j = min((y0 >> 1) + qy, cj_last);
            const int ca = TILES ? 2 * qy : min(2 * j, a.rows - 1) - y0, cb_ = TILES ? 2 * qy + 1 : min(2 * j + 1, a.rows - 1) - y0;
            const uint8_t *ua = raw + ca * JE_PITCH, *ub = raw + cb_ * JE_PITCH;
            const int bias = 1 + (qx & 1);
            const int sb = je_cb(ua[xa + ro], ua[xa + 1], ua[xa + bo]) + je_cb(ua[xb + ro], ua[xb + 1], ua[xb + bo]) +
                           je_cb(ub[xa + ro], ub[xa + 1], ub[xa + bo]) + je_cb(ub[xb + ro], ub[xb + 1], ub[xb + bo]);
            const int sr = je_cr(ua[xa + ro], ua[xa + 1], ua[xa + bo]) + je_cr(ua[xb + ro], ua[xb + 1], ua[xb + bo]) +
                           je_cr(ub[xa + ro], ub[xa + 1], ub[xa + bo]) + je_cr(ub[xb + ro], ub[xb + 1], ub[xb + bo]);
            cbcr[qy * 128 + qx] = (uint8_t)((sb + bias) >> 2);
            cbcr[1024 + qy * 128 + qx] = (uint8_t)((sr + bias) >> 2);
        }
        __syncthreads();
    }

    // ---- pass 1: the rows of every block (8 lanes per block)
    for (int t = tid; t < JE_BLOCKS * 8; t += 256) {
        const int blk = t >> 3, r = t & 7;
        int d[8];
        if (COLOR) {
            const int m = blk / 6, b = blk % 6;
            const uint8_t *p = b < 4 ? yp + ((b >> 1) * 8 + r) * 256 + m * 16 + (b & 1) * 8 : cbcr + (b - 4) * 1024 + r * 128 + m * 8;
            const uint2 v = *(const uint2 *)p;
            for (int k = 0; k < 4; k++) { d[k] = (int)((v.x >> (8 * k)) & 255) - 128; d[4 + k] = (int)((v.y >> (8 * k)) & 255) - 128; }
        } else {
            const uint8_t *p = raw + min(r, nrow - 1) * JE_PITCH;
            const int xmax = a.cols - 1 - sx0;
            for (int k = 0; k < 8; k++) d[k] = (int)p[min(blk * 8 + k, xmax)] - 128;
        }
        je_fdct8<true>(d);
        int16_t *w = ws + blk * 64 + r * 8;
        for (int k = 0; k < 8; k++) w[k] = (int16_t)d[k];
    }
    __syncthreads();

    // ---- pass 2: the columns, quantised, to their zigzag places
    int16_t *out = (int16_t *)raw;
    for (int t = tid; t < JE_BLOCKS * 8; t += 256) {
        const int blk = t >> 3, c = t & 7;
        const int tab = COLOR && blk % 6 >= 4;
        int d[8];
        for (int k = 0; k < 8; k++) d[k] = ws[blk * 64 + k * 8 + c];
        je_fdct8<false>(d);
        for (int k = 0; k < 8; k++) {
            const int pos = k * 8 + c;
            const uint32_t n = (uint32_t)abs(d[k]) + 4u * a.qt.q[tab][pos];
            const int mag = (int)__umulhi(n, a.qt.recip[tab][pos]);
            out[blk * 64 + c_zigzag_of[pos]] = (int16_t)(d[k] < 0 ? -mag : mag);
        }
    }
    __syncthreads();

    // ---- jccoefct.c: the Y blocks of an MCU that lie beyond the image's block grid carry no AC and the DC of the block in front of them
    if (COLOR && !TILES) {
        const int bw = (a.cols + 7) >> 3, bh = (a.rows + 7) >> 3;
        const int by0 = y0 >> 3;
        if (tid < nvalid && ((mx0 + tid) * 2 + 1 >= bw || by0 + 1 >= bh)) {
            int16_t *m = out + tid * 6 * 64;
            const bool col_dummy = (mx0 + tid) * 2 + 1 >= bw, row_dummy = by0 + 1 >= bh;
            if (col_dummy) { for (int k = 1; k < 64; k++) m[64 + k] = 0; m[64] = m[0]; }
            if (row_dummy) {
                for (int k = 1; k < 64; k++) { m[128 + k] = 0; m[192 + k] = 0; }
                m[128] = m[64]; m[192] = m[64];
            } else if (col_dummy) { for (int k = 1; k < 64; k++) m[192 + k] = 0; m[192] = m[128]; }
        }
        __syncthreads();
    }

    // ---- out: the strip's MCUs are consecutive in the coefficient array; in tile order every MCU has its own place
    if (TILES) {
        const uint4 *s = (const uint4 *)out;
        for (int e = tid; e < nvalid * BPM * 8; e += 256) {
            const int m = e / (BPM * 8), q = e % (BPM * 8);
            const int mx = mx0 + m;
            const size_t dm = (size_t)a.mcu_base + (((size_t)(my / a.tm) * a.ntx + mx / a.tm) * a.tm + my % a.tm) * a.tm + mx % a.tm;
            ((uint4 *)(a.coef + dm * BPM * 64))[q] = s[e];
        }
    } else {
        uint4 *dst = (uint4 *)(a.coef + ((size_t)my * a.mw + mx0) * BPM * 64);
        const uint4 *s = (const uint4 *)out;
        for (int e = tid; e < nvalid * BPM * 8; e += 256) dst[e] = s[e];
    }
}

struct JpegEntropyArgs {
    const int16_t *coef;                    // [band MCU][blocks per MCU][64]
    int n_mcu;                              // MCUs of the band
    int interval;                           // MCUs per restart interval
    int n_int;                              // intervals of the band
    int first_int;                          // the band's first interval, counted from the start of the image (RSTn numbering)
    int last_marker;                        // an RSTn follows the band's last interval too (the band is not the image's last)
    int bpm;                                // blocks per MCU: 6 (Y Y Y Y Cb Cr) or 1
    uint32_t *sizes;                        // [n_int] bytes of every interval, marker included
    const unsigned long long *offs;         // [n_int + 1] their exclusive scan
    uint8_t *out; unsigned long long cap;   // the output stream and its capacity
    int *err;                               // set when the stream would not fit `cap`
    // tile order (k_jpeg_entropy<.., true>): `ipt` intervals per tile; a tile's first interval is preceded by the tile prefix (SOI, SOF0,
    // DRI, SOS: the same bytes for every tile of a file), its last is followed by EOI instead of an RSTn, and RSTn counts within the tile
    int ipt;
    int plen; uint8_t prefix[44];
};

// one lane's coder
template <bool WRITE>
struct JeLane {
    unsigned long long acc = 0; int nbits = 0; bool stuff = false;
    unsigned long long pos, wend; uint8_t *win; unsigned long long wbeg;
    __device__ inline void put(uint32_t b) { if (WRITE) win[pos - wbeg] = (uint8_t)b; pos++; }
    // whole bytes out of the accumulator, 0xFF followed by 0x00; false: the window is full
    __device__ inline bool drain()
    {
        for (;;) {
            if (stuff) { if (WRITE && pos >= wend) return false; put(0); stuff = false; }
            if (nbits < 8) return true;
            if (WRITE && pos >= wend) return false;
            const uint32_t b = (uint32_t)(acc >> (nbits - 8)) & 255u;
            nbits -= 8;
            put(b);
            stuff = b == 255u;
        }
    }
    __device__ inline void bits(uint32_t v, int n) { acc = (acc << n) | v; nbits += n; }
};

// WRITE = false: sizes[i] = the bytes of interval i.  WRITE = true: the bytes, at offs[i].  One wave per workgroup, one lane per interval
// TILES: the tile streams of tests/tiff_jpeg_ref.py back to back in interval order, so a tile's stream starts at offs[its first interval]
template <bool WRITE, bool TILES>
__global__ void __launch_bounds__(64) k_jpeg_entropy(const JpegEntropyArgs a)
{
    __shared__ __attribute__((aligned(16))) uint8_t win[WRITE ? JE_WINDOW : 16];
    __shared__ uint8_t pre[TILES ? 64 : 1];
    const int lane = threadIdx.x;
    if (TILES) { pre[lane] = lane < a.plen ? a.prefix[lane] : 0; __syncthreads(); }
    const int i0 = blockIdx.x * 64, i = i0 + lane;
    const bool live = i < a.n_int;
    const int m0 = live ? i * a.interval : 0;
    const int nblk = live ? (min(m0 + a.interval, a.n_mcu) - m0) * a.bpm : 0;
    const int16_t *cf = a.coef + (size_t)m0 * a.bpm * 64;
    const int it = TILES ? i % a.ipt : 0;                                      // the interval within its tile
    const bool marker = TILES ? live : live && (i + 1 < a.n_int || a.last_marker);
    const uint32_t rst = TILES ? (it + 1 == a.ipt ? 0xFFD9u : 0xFFD0u | (uint32_t)(it & 7)) : 0xFFD0u | (uint32_t)((a.first_int + i) & 7);

    JeLane<WRITE> L;
    L.win = win;
    unsigned long long B0 = 0, B1 = 0;
    if (WRITE) {
        const int i1 = min(i0 + 64, a.n_int);
        B0 = a.offs[i0]; B1 = a.offs[i1];
        L.pos = live ? a.offs[i] : B1;
    } else L.pos = 0;
    const unsigned long long A0 = B0 & ~15ull;
    const int rounds = WRITE ? (int)((B1 - A0 + JE_WINDOW - 1) / JE_WINDOW) : 1;

    // the coder's place: block, coefficient, zero run, predictors; stage -1 the tile prefix, 0 coding, 1 padded, 2 marker bytes, 3 done
    int blk = 0, k = 0, run = 0, pred[3] = {0, 0, 0}, stage = live ? 0 : 3, rawn = 0;
    if (TILES && live && it == 0) { stage = -1; rawn = a.plen; }
    uint4 v8 = make_uint4(0, 0, 0, 0);

    for (int round = 0; round < rounds; round++) {
        L.wbeg = A0 + (unsigned long long)round * JE_WINDOW;
        L.wend = WRITE ? L.wbeg + JE_WINDOW : ~0ull;
        while (stage < 3) {
            if (TILES && stage < 0) {                                         // the prefix: bytes as they are, like the marker's
                while (rawn > 0 && !(WRITE && L.pos >= L.wend)) { L.put(pre[a.plen - rawn]); rawn--; }
                if (rawn > 0) break;
                stage = 0;
                continue;
            }
            if (stage == 2) {                                                 // the marker: two bytes as they are
                while (rawn > 0 && !(WRITE && L.pos >= L.wend)) { L.put((rst >> (8 * (rawn - 1))) & 255u); rawn--; }
                if (rawn > 0) break;
                stage = 3;
                break;
            }
            if (!L.drain()) break;
            if (stage == 1) { rawn = marker ? 2 : 0; stage = 2; continue; }
            if (blk == nblk) {                                                // the interval's last byte is filled up with 1-bits
                if (L.nbits) { const int pad = 8 - L.nbits; L.bits((1u << pad) - 1u, pad); }
                stage = 1;
                continue;
            }
            if ((k & 7) == 0) v8 = *(const uint4 *)(cf + (size_t)blk * 64 + k);
            const uint32_t w = (k & 4) ? ((k & 2) ? v8.w : v8.z) : ((k & 2) ? v8.y : v8.x);
            int c = (int)(int16_t)(uint16_t)(w >> ((k & 1) * 16));
            const int comp = a.bpm == 1 ? 0 : (blk % 6 < 4 ? 0 : blk % 6 - 3);
            const int tab = comp > 0;
            if (k == 0) {                                                     // DC: the difference to the component's previous block
                const int diff = c - pred[comp];
                pred[comp] = c;
                const int mag = abs(diff);
                const int s = mag ? 32 - __clz(mag) : 0;
                const uint32_t h = c_huff.dc[tab][s];
                L.bits(h >> 5, (int)(h & 31));
                if (s) L.bits((uint32_t)(diff < 0 ? diff - 1 : diff) & ((1u << s) - 1u), s);
                k = 1; run = 0;
                continue;
            }
            if (c == 0) {
                run++;
                if (k == 63) { const uint32_t h = c_huff.ac[tab][0]; L.bits(h >> 5, (int)(h & 31)); k = 0; blk++; }      // end of block
                else k++;
                continue;
            }
            if (run >= 16) { const uint32_t h = c_huff.ac[tab][0xF0]; L.bits(h >> 5, (int)(h & 31)); run -= 16; continue; }  // ZRL, same coefficient again
            {
                const int mag = abs(c);
                const int s = 32 - __clz(mag);
                const uint32_t h = c_huff.ac[tab][(run << 4) | s];
                L.bits(h >> 5, (int)(h & 31));
                L.bits((uint32_t)(c < 0 ? c - 1 : c) & ((1u << s) - 1u), s);
                run = 0;
                if (k == 63) { k = 0; blk++; } else k++;
            }
        }
        if (WRITE) {
            __syncthreads();
            // the window's part of this wave's range [B0, B1): whole 16-byte units as one store, the units it shares with a neighbour by bytes
            const unsigned long long gb = max(L.wbeg, B0), ge = min(L.wend, B1);
            for (int u = lane; u < JE_WINDOW / 16; u += 64) {
                const unsigned long long g = L.wbeg + 16ull * u;
                if (g + 16 <= gb || g >= ge) continue;
                if (g + 16 > a.cap) { if (ge > a.cap) *a.err = 1; for (int q = 0; q < 16; q++) if (g + q >= gb && g + q < ge && g + q < a.cap) a.out[g + q] = win[16 * u + q]; continue; }
                if (g >= gb && g + 16 <= ge) *(uint4 *)(a.out + g) = *(const uint4 *)(win + 16 * u);
                else for (int q = 0; q < 16; q++) if (g + q >= gb && g + q < ge) a.out[g + q] = win[16 * u + q];
            }
            __syncthreads();
        }
    }
    if (!WRITE && live) a.sizes[i] = (uint32_t)L.pos;
}

// offs[0 .. n] = the exclusive scan of sizes[0 .. n): one workgroup, 1024 elements a step
__global__ void __launch_bounds__(1024) k_jpeg_scan(const uint32_t *sizes, int n, unsigned long long *offs)
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

void huff_derive(const uint8_t *bits, const uint8_t *vals, uint32_t *table)
{
    uint32_t code = 0; int k = 0;
    for (int len = 1; len <= 16; len++) {
        for (int j = 0; j < bits[len - 1]; j++) table[vals[k++]] = (code++ << 5) | (uint32_t)len;
        code <<= 1;
    }
}

// tile_offs[t] = offs[t * ipt], t = 0 .. n_tiles: where every tile's stream starts, and the total
__global__ void __launch_bounds__(256) k_jpeg_tile_offsets(const unsigned long long *offs, int ipt, int n_tiles, unsigned long long *tile_offs)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t <= n_tiles) tile_offs[t] = offs[(size_t)t * ipt];
}

// the Annex K tables in constant memory, once per process and device
int huff_tables_up(vfsms_ctx *ctx)
{
    static bool tables_up = false;                                            // (per process: one device image of the library per device in use)
    static int tables_dev = -1;
    if (!tables_up || tables_dev != ctx->device) {
        HuffTables h; memset(&h, 0, sizeof(h));
        for (int t = 0; t < 2; t++) {
            uint32_t dc[256]; memset(dc, 0, sizeof(dc));
            huff_derive(jpeg_std_huff_bits(0, t), jpeg_std_huff_vals(0, t), dc);
            memcpy(h.dc[t], dc, sizeof(h.dc[t]));
            huff_derive(jpeg_std_huff_bits(1, t), jpeg_std_huff_vals(1, t), h.ac[t]);
        }
        HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(c_huff), &h, sizeof(h)));
        tables_up = true; tables_dev = ctx->device;
    }
    return VFSMS_OK;
}

void quant_args(int quality, JpegQuant *qt)
{
    uint8_t q[2][64];
    jpeg_quant_tables(quality, q);
    for (int t = 0; t < 2; t++) for (int k = 0; k < 64; k++) {
        qt->q[t][k] = q[t][k];
        qt->recip[t][k] = (uint32_t)((((unsigned long long)1 << 32) + 8ull * q[t][k] - 1) / (8ull * q[t][k]));
    }
}

// the `sizes` scratch of a call: the intervals' sizes, their offsets (the last being the total) and the error word of the writing pass; in
// tile order the tiles' offsets behind them
struct JpegSizes { uint32_t *sizes; unsigned long long *offs; int *err; unsigned long long *toffs; };
int sizes_carve(vfsms_ctx *ctx, JpegScratch *s, size_t n_int, size_t n_tiles, JpegSizes *z)
{
    const size_t o_offs = (n_int * 4 + 255) & ~(size_t)255, o_err = o_offs + (n_int + 1) * 8;
    const size_t o_toffs = (o_err + sizeof(int) + 255) & ~(size_t)255;
    TRY(s->sizes.reserve(o_toffs + (n_tiles + 1) * 8, ctx->stream));
    char *at = s->sizes.as<char>();
    *z = {(uint32_t *)at, (unsigned long long *)(at + o_offs), (int *)(at + o_err), (unsigned long long *)(at + o_toffs)};
    return VFSMS_OK;
}

// the arguments of a counting pass (the writing half adds `out`); band order: ipt = 0 and no prefix
JpegEntropyArgs entropy_args(const JpegScratch *s, uint32_t *d_sizes, unsigned long long *d_offs, int *d_err, int n_mcu, int interval, int n_int,
                             int first_int, int last_marker, int bpm, int ipt, const uint8_t *prefix, int plen)
{
    JpegEntropyArgs e;
    e.coef = s->coef.as<int16_t>(); e.n_mcu = n_mcu; e.interval = interval; e.n_int = n_int; e.first_int = first_int; e.last_marker = last_marker;
    e.bpm = bpm; e.sizes = d_sizes; e.offs = d_offs; e.out = nullptr; e.cap = 0; e.err = d_err;
    e.ipt = ipt; e.plen = plen; memset(e.prefix, 0, sizeof(e.prefix)); if (plen) memcpy(e.prefix, prefix, (size_t)plen);
    return e;
}

// Writing half of both orders: the `total` bytes that the counting pass `e` measured into `out` on the host (the caller has checked its
// capacity): one writing pass, one copy.  Synchronises the stream.
template <bool TILES>
int entropy_write(vfsms_ctx *ctx, JpegScratch *s, JpegEntropyArgs e, unsigned long long total, uint8_t *out)
{
    TRY(s->out.reserve(((size_t)total + 15) & ~(size_t)15, ctx->stream));
    e.out = s->out.as<uint8_t>(); e.cap = s->out.bytes();
    int err = 0;
    {
        ProfScope ps(ctx, TILES ? "pyramid_jpeg.entropy" : "jpeg_encode.entropy");
        HIP_TRY(hipMemsetAsync(e.err, 0, sizeof(int), ctx->stream));
        hipLaunchKernelGGL((k_jpeg_entropy<true, TILES>), dim3((unsigned)((e.n_int + 63) / 64)), dim3(64), 0, ctx->stream, e);
        HIP_TRY(hipGetLastError());
    }
    {
        ProfScope ps(ctx, TILES ? "pyramid_jpeg.copy" : "jpeg_encode.copy");
        HIP_TRY(hipMemcpyAsync(&err, e.err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(out, s->out.as<uint8_t>(), (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (!err) return VFSMS_OK;
    if (TILES) vfsms_set_error("jpeg tiles: the coded tiles outgrew the %zu bytes counted for them", s->out.bytes());
    else vfsms_set_error("jpeg_encode: the coded band outgrew the %zu bytes counted for it", s->out.bytes());
    return VFSMS_ERR_CAPACITY;
}

}  // namespace

// The entropy-coded bytes of rows [row0, row0 + nrows) of the rows x cols x ch image at d_img (256-byte aligned, `pitch` bytes a row) into
// `out` on the host.  api.hip has checked the band contract: row0 is a multiple of the MCU height, the MCUs in front of the band are whole
// intervals and so are the band's own unless it ends at the last row.  *nbytes = the size, also on VFSMS_ERR_CAPACITY (nothing is copied
// then).  Synchronises the stream.
int jpeg_encode_band_device(vfsms_ctx *ctx, JpegScratch *s, const uint8_t *d_img, int rows, int cols, int ch, size_t pitch, int bgr,
                            int row0, int nrows, int quality, int interval, uint8_t *out, size_t cap, size_t *nbytes)
{
    TRY(huff_tables_up(ctx));
    const int mcu = ch == 3 ? 16 : 8, bpm = ch == 3 ? 6 : 1;
    const int mw = (cols + mcu - 1) / mcu;
    const int mrows = (nrows + mcu - 1) / mcu;
    const long long n_mcu = (long long)mw * mrows;
    const int n_int = (int)((n_mcu + interval - 1) / interval);
    const bool last = row0 + nrows >= rows;

    TRY(s->coef.reserve((size_t)n_mcu * bpm * 128, ctx->stream));
    JpegSizes z;
    TRY(sizes_carve(ctx, s, (size_t)n_int, 0, &z));

    JpegXformArgs x;
    x.src = d_img; x.src_bytes = (size_t)rows * pitch; x.pitch = pitch; x.rows = rows; x.cols = cols; x.row0 = row0; x.mw = mw; x.bgr = bgr;
    x.coef = s->coef.as<int16_t>();
    x.src_row0 = 0; x.tm = 0; x.ntx = 0; x.mcu_base = 0;
    quant_args(quality, &x.qt);
    {
        ProfScope ps(ctx, "jpeg_encode.transform");
        const int mpw = ch == 3 ? 16 : 96;
        const dim3 grid((unsigned)((mw + mpw - 1) / mpw), (unsigned)mrows);
        if (ch == 3) hipLaunchKernelGGL((k_jpeg_transform<true, false>), grid, dim3(256), 0, ctx->stream, x);
        else hipLaunchKernelGGL((k_jpeg_transform<false, false>), grid, dim3(256), 0, ctx->stream, x);
        HIP_TRY(hipGetLastError());
    }
    const JpegEntropyArgs e = entropy_args(s, z.sizes, z.offs, z.err, (int)n_mcu, interval, n_int, (int)(((long long)(row0 / mcu) * mw) / interval), last ? 0 : 1, bpm, 0, nullptr, 0);
    unsigned long long total = 0;
    {
        ProfScope ps(ctx, "jpeg_encode.entropy");
        hipLaunchKernelGGL((k_jpeg_entropy<false, false>), dim3((unsigned)((n_int + 63) / 64)), dim3(64), 0, ctx->stream, e);
        hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(1024), 0, ctx->stream, z.sizes, n_int, z.offs);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(&total, z.offs + n_int, sizeof(total), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *nbytes = (size_t)total;
    if (!out || cap < total) { vfsms_set_error("jpeg_encode: the band takes %llu bytes, the buffer holds %zu", total, out ? cap : (size_t)0); return VFSMS_ERR_CAPACITY; }
    return entropy_write<false>(ctx, s, e, total, out);
}

// ---- tile order: the JPEG tiles of a pyramidal TIFF (Method.pyramidCompression = "jpeg"; specified by tests/tiff_jpeg_ref.py) ---------------
// Counting half: the tile rows of `n_jobs` levels (api.hip has checked tile, interval and the jobs) are transformed into s->coef, tile after
// tile in job order, one launch per job; ONE counting pass and ONE scan over all their intervals follow, and the tiles' offsets
// (tile_offs[0 .. n_tiles], the last being the total) come to the host with `d_flag` (an int on the device, may be NULL) in *flag.
// Synchronises the stream.
int jpeg_tiles_count_device(vfsms_ctx *ctx, JpegScratch *s, const JpegTileJob *jobs, int n_jobs, int ch, int bgr, int tile, int quality, int restart_mcus,
                            int interval, const int *d_flag, int *flag, JpegTilesRun *run)
{
    TRY(huff_tables_up(ctx));
    const int mcu = ch == 3 ? 16 : 8, bpm = ch == 3 ? 6 : 1, tm = tile / mcu, mpt = tm * tm, ipt = mpt / interval;
    long long n_tiles = 0;
    for (int j = 0; j < n_jobs; j++) n_tiles += (long long)jobs[j].tile_rows * ((jobs[j].cols + tile - 1) / tile);
    const long long n_mcu = n_tiles * mpt, n_int = n_tiles * ipt;
    if (n_tiles < 1 || n_int > 0x7fffffff - 64 || n_mcu > 0x7fffffff) { vfsms_set_error("jpeg tiles: %lld tiles of %d intervals are more than one call takes", n_tiles, ipt); return VFSMS_ERR_BAD_ARG; }
    run->n_tiles = (int)n_tiles; run->n_int = (int)n_int; run->ipt = ipt; run->interval = interval; run->bpm = bpm;
    run->plen = jpeg_tile_prefix(tile, ch, restart_mcus, run->prefix);

    TRY(s->coef.reserve((size_t)n_mcu * bpm * 128, ctx->stream));
    JpegSizes z;
    TRY(sizes_carve(ctx, s, (size_t)n_int, (size_t)n_tiles, &z));
    run->d_sizes = z.sizes; run->d_offs = z.offs; run->d_err = z.err;

    {
        ProfScope ps(ctx, "pyramid_jpeg.transform");
        JpegXformArgs x;
        quant_args(quality, &x.qt);
        x.coef = s->coef.as<int16_t>(); x.bgr = bgr; x.tm = tm;
        long long base = 0;
        const int mpw = ch == 3 ? 16 : 96;
        for (int j = 0; j < n_jobs; j++) {
            const JpegTileJob &J = jobs[j];
            x.src = J.src; x.src_bytes = J.src_bytes; x.pitch = J.pitch; x.rows = J.rows; x.cols = J.cols; x.row0 = J.row0; x.src_row0 = J.src_row0;
            x.ntx = (J.cols + tile - 1) / tile; x.mw = x.ntx * tm; x.mcu_base = base;
            const dim3 grid((unsigned)((x.mw + mpw - 1) / mpw), (unsigned)(J.tile_rows * tm));
            if (ch == 3) hipLaunchKernelGGL((k_jpeg_transform<true, true>), grid, dim3(256), 0, ctx->stream, x);
            else hipLaunchKernelGGL((k_jpeg_transform<false, true>), grid, dim3(256), 0, ctx->stream, x);
            base += (long long)J.tile_rows * x.ntx * mpt;
        }
        HIP_TRY(hipGetLastError());
    }
    const JpegEntropyArgs e = entropy_args(s, z.sizes, z.offs, z.err, (int)n_mcu, interval, (int)n_int, 0, 0, bpm, ipt, run->prefix, run->plen);
    {
        ProfScope ps(ctx, "pyramid_jpeg.entropy");
        hipLaunchKernelGGL((k_jpeg_entropy<false, true>), dim3((unsigned)((n_int + 63) / 64)), dim3(64), 0, ctx->stream, e);
        hipLaunchKernelGGL(k_jpeg_scan, dim3(1), dim3(1024), 0, ctx->stream, run->d_sizes, (int)n_int, run->d_offs);
        hipLaunchKernelGGL(k_jpeg_tile_offsets, dim3((unsigned)((n_tiles + 256) / 256)), dim3(256), 0, ctx->stream, run->d_offs, ipt, (int)n_tiles, z.toffs);
        HIP_TRY(hipGetLastError());
    }
    run->tile_offs.resize((size_t)n_tiles + 1);
    HIP_TRY(hipMemcpyAsync(run->tile_offs.data(), z.toffs, ((size_t)n_tiles + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (d_flag) HIP_TRY(hipMemcpyAsync(flag, d_flag, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// Writing half: the streams the counting half measured into `out` on the host (cap >= run->tile_offs[n_tiles], checked by the caller).
// Synchronises the stream.
int jpeg_tiles_write_device(vfsms_ctx *ctx, JpegScratch *s, const JpegTilesRun *run, uint8_t *out)
{
    const JpegEntropyArgs e = entropy_args(s, run->d_sizes, run->d_offs, run->d_err, run->n_int * run->interval, run->interval, run->n_int, 0, 0, run->bpm, run->ipt, run->prefix, run->plen);
    return entropy_write<true>(ctx, s, e, run->tile_offs[(size_t)run->n_tiles], out);
}
