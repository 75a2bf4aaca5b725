// jpeg_huff_host.cpp -- the entropy decoder of Method.jpegDecoder = "device-entropy" as a host program: vfsms_jpeg_scan (csrc/jpeg_host.cpp)
// and then the rounds of csrc/jpeg_huff_kernels.hip over the same csrc/jpeg_huff_core.h, one "thread" after the other -- sync, Jacobi repair
// rounds on two result buffers, the segmented prefix sums, the write pass with its damage flags.  No GPU, no HIP runtime at work, no
// libvfsms.  Built plain it is what tests/test_jpeg_huff_host.py holds to tests/jpeg_huff_ref.py; built with -fsanitize=address,undefined it
// is how untrusted files meet this code before a device does.
//
//     jpeg_huff_host FILE.jpg OUT.bin [max_rounds = -1 [sub_bits = VFSMS_JPEG_HUFF_SUB_BITS]]
//
// Writes the layout of vfsms_jpeg_coefficients to OUT.bin and prints "rc=0 rounds=R nsub=N nseg=S"; a refusal prints "rc=-N ..." and
// writes nothing.  The exit status is 0 either way: a refusal is an answer.
#include "common.h"
#include "jpeg_huff_core.h"
#include <stdarg.h>
#include <stdio.h>
#include <vector>

static char g_error[512];
void vfsms_set_error(const char *fmt, ...)
{
    va_list ap; va_start(ap, fmt); vsnprintf(g_error, sizeof(g_error), fmt, ap); va_end(ap);
}

static const uint8_t kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                     35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct Sub { JpegHuffBits bits; uint32_t start, end, seg, first, limit; bool last; };
static Sub sub_of(const JpegScanHeader &H, const uint8_t *rec, uint32_t i)
{
    const uint32_t *subseg = (const uint32_t *)(rec + H.off_subseg);
    const JpegHuffSeg *segs = (const JpegHuffSeg *)(rec + H.off_seg);
    Sub s; s.seg = subseg[i];
    const JpegHuffSeg S = segs[s.seg];
    s.bits.words = (const uint32_t *)(rec + H.off_stream + S.byte_off);
    s.bits.nwords = (S.byte_count + 3) >> 2; s.bits.nbits = S.byte_count * 8;
    s.first = i - S.sub0;
    s.start = s.first * (uint32_t)H.sub_bits < s.bits.nbits ? s.first * (uint32_t)H.sub_bits : s.bits.nbits;
    s.end = s.start + (uint32_t)H.sub_bits < s.bits.nbits ? s.start + (uint32_t)H.sub_bits : s.bits.nbits;
    s.last = i + 1 == (uint32_t)H.nsub || subseg[i + 1] != s.seg;
    s.limit = jh_segment_blocks(H, S.first_mcu);
    return s;
}

struct Store {
    std::vector<int16_t> *coef; size_t comp_off[3];
    JpegHuffPlace place; uint32_t block0; uint32_t pred[3];
    void operator()(uint32_t blk, int zi, int value, int comp)
    {
        if (zi == 0) { pred[comp] += (uint32_t)value; value = (int)(int16_t)(uint16_t)pred[comp]; }
        uint32_t b;
        if ((unsigned)zi > 63u || !jh_place(place, block0 + blk, comp, &b)) return;
        coef->at(comp_off[comp] + (size_t)b * 64 + kNatural[zi]) = (int16_t)value;
    }
};

int main(int argc, char **argv)
{
    if (argc < 3) { fprintf(stderr, "usage: %s FILE.jpg OUT.bin [max_rounds [sub_bits]]\n", argv[0]); return 2; }
    int max_rounds = argc > 3 ? atoi(argv[3]) : -1;
    const int sub_bits = argc > 4 ? atoi(argv[4]) : VFSMS_JPEG_HUFF_SUB_BITS;
    FILE *f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
    std::vector<uint8_t> file;
    uint8_t buf[65536]; size_t got;
    while ((got = fread(buf, 1, sizeof(buf), f)) > 0) file.insert(file.end(), buf, buf + got);
    fclose(f);
    size_t bound = 0, rec_bytes = 0;
    int rc = jpeg_scan_host(file.data(), file.size(), sub_bits, nullptr, 0, &bound);
    std::vector<uint8_t> recv;
    if (rc == VFSMS_ERR_CAPACITY) { recv.resize(bound); rc = jpeg_scan_host(file.data(), file.size(), sub_bits, recv.data(), bound, &rec_bytes); }
    if (rc != VFSMS_OK) { printf("rc=%d scan: %s\n", rc, g_error); return 0; }
    recv.resize(rec_bytes);                                      // (exactly the record: a read beyond it is a sanitizer finding)
    const uint8_t *rec = recv.data();
    JpegScanHeader H; memcpy(&H, rec, sizeof(H));
    const JpegHuffTable *tables = (const JpegHuffTable *)(rec + H.off_tables);
    const uint32_t n = (uint32_t)H.nsub;
    if (max_rounds < 0 || max_rounds > H.nsub) max_rounds = H.nsub;
    // k_huff_sync
    std::vector<JpegHuffState> entry(n);
    std::vector<JpegHuffSubOut> res[2] = {std::vector<JpegHuffSubOut>(n), std::vector<JpegHuffSubOut>(n)};
    JpegHuffNoSink nosink; unsigned ignored = 0;
    for (uint32_t i = 0; i < n; i++) {
        const Sub s = sub_of(H, rec, i);
        entry[i].p = s.start; entry[i].cz = 0;
        res[0][i] = jh_decode_sub(s.bits, tables, H.blocks_per_mcu, entry[i], s.end, 0u, 0xFFFFFFFFu, nosink, &ignored);
    }
    // k_huff_round: rounds 0 .. max_rounds - 1 repair, round max_rounds only compares
    int used = -1;
    for (int r = 0; r <= max_rounds && used < 0; r++) {
        const bool repair = r < max_rounds;
        const std::vector<JpegHuffSubOut> &in = res[r & 1]; std::vector<JpegHuffSubOut> &out = res[(r + 1) & 1];
        bool changed = false;
        for (uint32_t i = 0; i < n; i++) {
            const Sub s = sub_of(H, rec, i);
            JpegHuffSubOut mine = in[i];
            if (s.first > 0 && !jh_same(in[i - 1].exit, entry[i])) {
                changed = true;
                if (repair) { entry[i] = in[i - 1].exit; mine = jh_decode_sub(s.bits, tables, H.blocks_per_mcu, entry[i], s.end, 0u, 0xFFFFFFFFu, nosink, &ignored); }
            }
            if (repair) out[i] = mine;
        }
        if (!changed) used = r;
    }
    if (used < 0) { printf("rc=%d not in step after %d rounds nsub=%u nseg=%d\n", VFSMS_ERR_UNSUPPORTED, max_rounds, n, H.nseg); return 0; }
    // k_huff_scan
    const std::vector<JpegHuffSubOut> &fin = res[used & 1];
    std::vector<uint32_t> base(n), dcbase(3 * (size_t)n);
    uint32_t run[4] = {0, 0, 0, 0};
    for (uint32_t i = 0; i < n; i++) {
        if (sub_of(H, rec, i).first == 0) run[0] = run[1] = run[2] = run[3] = 0;
        base[i] = run[0]; for (int k = 0; k < 3; k++) dcbase[3 * (size_t)i + k] = run[k + 1];
        run[0] += fin[i].blocks; for (int k = 0; k < 3; k++) run[k + 1] += fin[i].dc[k];
    }
    // k_huff_write
    Store S; memset((void *)&S, 0, sizeof(S));
    if (!jh_place_from_header(H, &S.place)) { printf("rc=%d the record's grids do not fit its frame\n", VFSMS_ERR_BAD_ARG); return 0; }
    size_t total = 0;
    for (int k = 0; k < H.ncomp; k++) { S.comp_off[k] = total; total += (size_t)S.place.blocks[k] * 64; }
    std::vector<int16_t> coef(total, 0);
    S.coef = &coef;
    unsigned damage = 0;
    const JpegHuffSeg *segs = (const JpegHuffSeg *)(rec + H.off_seg);
    for (uint32_t i = 0; i < n; i++) {
        const Sub s = sub_of(H, rec, i);
        if (base[i] >= s.limit) continue;
        S.block0 = segs[s.seg].first_mcu * (uint32_t)H.blocks_per_mcu;
        for (int k = 0; k < 3; k++) S.pred[k] = dcbase[3 * (size_t)i + k];
        unsigned d = 0;
        const JpegHuffSubOut o = jh_decode_sub(s.bits, tables, H.blocks_per_mcu, entry[i], s.end, base[i], s.limit, S, &d);
        if (o.exit.p > s.bits.nbits) d |= JH_DAMAGE_BITS;
        if (s.last && base[i] + o.blocks < s.limit) d |= JH_DAMAGE_BITS;
        damage |= d;
    }
    if (damage) { printf("rc=%d damage=%u rounds=%d nsub=%u nseg=%d\n", VFSMS_ERR_BAD_ARG, damage, used, n, H.nseg); return 0; }
    FILE *o = fopen(argv[2], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    fwrite(rec + H.off_quant, 1, (size_t)H.ncomp * VFSMS_JPEG_COEF_TABLE_BYTES, o);
    fwrite(coef.data(), 2, coef.size(), o);
    fclose(o);
    printf("rc=0 rounds=%d nsub=%u nseg=%d\n", used, n, H.nseg);
    return 0;
}
