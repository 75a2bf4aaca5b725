// png_core_host_check.cpp -- csrc/png_core.h (on csrc/deflate_core.h), the rules of the PNG coder (Method.pngEncoder = "device"), as the plain
// host C++ it is: the lines the kernels of csrc/deflate_kernels.hip compile, run serially over one image, for a sanitizer build that needs neither
// the HIP runtime nor libvfsms.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I imagestitch_amd/csrc \
//       tools/png_core_host_check.cpp -o /tmp/pchc && /tmp/pchc case0.bin out0.bin [case1.bin out1.bin ...]
// (tests/test_png_device_host.py does this and compares every output with tests/png_ref.py.)  Per case the input file holds, little-endian,
// uint32 rows, cols, ch, segment_rows and the rows x cols x ch samples in the file's channel order; the output file holds the `rows` filter
// types as bytes; uint32 the Adler-32 of all filtered bytes (the segments' own, joined); uint32 n, and per segment uint32 m and the m bytes of
// its IDAT chunk, length and CRC-32 included.
#include "png_core.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

struct BitSink {
    std::vector<uint8_t> out; unsigned long long at = 0;
    void operator()(uint32_t value, int nbits)
    {
        for (int b = 0; b < nbits; b++, at++) {
            if (at / 8 >= out.size()) out.push_back(0);
            out[at / 8] |= (uint8_t)(((value >> b) & 1u) << (at & 7));
        }
    }
};

static bool read_file(const char *path, std::vector<uint8_t> *data)
{
    FILE *f = fopen(path, "rb");
    if (!f) return false;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), f)) > 0) data->insert(data->end(), buf, buf + n);
    fclose(f);
    return true;
}
static void put32(std::vector<uint8_t> *o, uint32_t v) { for (int k = 0; k < 4; k++) o->push_back((uint8_t)(v >> (8 * k))); }
static uint32_t get32(const uint8_t *p) { return p[0] | p[1] << 8 | p[2] << 16 | (uint32_t)p[3] << 24; }

// the chunk of the filtered bytes d[0 .. n): the device's passes, serially
static int code_segment(const char *in, const uint8_t *d, int n, const PngCrcPowers *pw, std::vector<uint8_t> *chunk)
{
    std::vector<int> start(n), end(n);
    for (int p = 0; p < n; p++) start[p] = p && d[p] == d[p - 1] ? start[p - 1] : p;
    for (int p = n - 1; p >= 0; p--) end[p] = p + 1 < n && d[p] == d[p + 1] ? end[p + 1] : p + 1;
    std::vector<int> toks;
    uint32_t hist[DFL_SYMS] = {}, counts[DFL_SYMS];
    for (int p = 0; p < n; p++) {
        const int t = dfl_token(p - start[p], end[p] - start[p], d[p]);
        if (t == DFL_NONE) continue;
        toks.push_back(t);
        hist[dfl_token_symbol(t)]++;
    }
    hist[DFL_END] = 1;
    memcpy(counts, hist, sizeof(hist));
    uint8_t lens[DFL_SYMS];
    uint32_t table[DFL_SYMS];
    DflBuild build;
    dfl_code_lengths(counts, lens, &build, nullptr);
    dfl_codes(lens, table);
    const unsigned long long bits = dfl_block_bits(hist, lens), bytes = png_chunk_bytes(bits);
    BitSink sink;
    png_chunk_head(bytes, sink);
    dfl_block_head(lens, sink, 0u);
    if (sink.at != PNG_HEAD_BITS) { fprintf(stderr, "%s: the head took %llu bits\n", in, sink.at); return 1; }
    for (int t : toks) { int nb; const uint32_t v = dfl_token_bits(t, table, &nb); sink(v, nb); }
    sink(table[DFL_END] >> 4, (int)(table[DFL_END] & 15));
    if (sink.at != PNG_HEAD_BITS + bits) { fprintf(stderr, "%s: %llu bits written, %llu counted\n", in, sink.at, PNG_HEAD_BITS + bits); return 1; }
    sink(0u, 3);
    *chunk = sink.out;
    chunk->push_back(0); chunk->push_back(0); chunk->push_back(0xff); chunk->push_back(0xff);
    if (chunk->size() + 4 != bytes) { fprintf(stderr, "%s: %zu bytes written, %llu counted\n", in, chunk->size() + 4, bytes); return 1; }
    // the CRC-32 of tag + data as the device forms it: raw remainders of short spans, joined, the complements folded in once
    const uint32_t len = (uint32_t)chunk->size() - 4, span = 7;
    uint32_t raw = 0;
    for (uint32_t s0 = 0; s0 < len; s0 += span) {
        const uint32_t m = len - s0 < span ? len - s0 : span;
        uint32_t r = 0;
        for (uint32_t k = 0; k < m; k++) r = png_crc_byte(r, (*chunk)[4 + s0 + k]);
        raw = png_crc_join(pw, raw, r, m);
    }
    const uint32_t crc = png_crc_finish(pw, raw, len);
    for (int k = 0; k < 4; k++) chunk->push_back((uint8_t)(crc >> (24 - 8 * k)));
    return 0;
}

static int one_case(const char *in, const char *outp, const PngCrcPowers *pw)
{
    std::vector<uint8_t> f;
    if (!read_file(in, &f) || f.size() < 16) { fprintf(stderr, "%s: no case\n", in); return 1; }
    const long long rows = get32(&f[0]), cols = get32(&f[4]), ch = get32(&f[8]), S = get32(&f[12]);
    if (rows < 1 || cols < 1 || (ch != 1 && ch != 3) || rows > 65536 || cols > 65536 || !png_segment_fits((int)S, 1 + cols * ch) || (long long)f.size() != 16 + rows * cols * ch) {
        fprintf(stderr, "%s: not a case\n", in); return 1;
    }
    const uint8_t *img = &f[16];
    const int rb = (int)(cols * ch), bpp = (int)ch;
    auto raw = [&](long long y, int i) { return y < 0 || i < 0 ? 0 : (int)img[y * rb + i]; };
    std::vector<uint8_t> types((size_t)rows), filt((size_t)rows * (rb + 1));
    for (long long y = 0; y < rows; y++) {
        unsigned cost[PNG_TYPES] = {};
        for (int i = 0; i < rb; i++)
            for (int t = 0; t < PNG_TYPES; t++) cost[t] += (unsigned)png_cost(png_filter(t, raw(y, i), raw(y, i - bpp), raw(y - 1, i), raw(y - 1, i - bpp)));
        const int t = png_choose(cost);
        types[(size_t)y] = (uint8_t)t;
        uint8_t *o = &filt[(size_t)y * (rb + 1)];
        o[0] = (uint8_t)t;
        for (int i = 0; i < rb; i++) o[1 + i] = (uint8_t)png_filter(t, raw(y, i), raw(y, i - bpp), raw(y - 1, i), raw(y - 1, i - bpp));
    }
    std::vector<uint8_t> o(types);
    std::vector<std::vector<uint8_t>> chunks;
    uint32_t adler = 1;
    for (long long y0 = 0; y0 < rows; y0 += S) {
        const long long nr = rows - y0 < S ? rows - y0 : S, n = nr * (rb + 1);
        const uint8_t *d = &filt[(size_t)y0 * (rb + 1)];
        unsigned long long a = 0, b = 0;
        for (long long p = 0; p < n; p++) { a += d[p]; b += (unsigned long long)(n - p) * d[p]; }
        adler = png_adler_combine(adler, png_adler_of_sums(a, b, (unsigned long long)n), (unsigned long long)n);
        chunks.emplace_back();
        if (code_segment(in, d, (int)n, pw, &chunks.back())) return 1;
    }
    put32(&o, adler);
    put32(&o, (uint32_t)chunks.size());
    for (const auto &c : chunks) { put32(&o, (uint32_t)c.size()); o.insert(o.end(), c.begin(), c.end()); }
    FILE *fo = fopen(outp, "wb");
    if (!fo || fwrite(o.data(), 1, o.size(), fo) != o.size()) { fprintf(stderr, "%s: cannot write\n", outp); if (fo) fclose(fo); return 1; }
    fclose(fo);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s case.bin out.bin [case.bin out.bin ...]\n", argv[0]); return 2; }
    PngCrcPowers pw;
    png_crc_powers(&pw);
    // the Paeth predictor against its definition over all (a, b, c)
    for (int a = 0; a < 256; a += 5) for (int b = 0; b < 256; b += 3) for (int c = 0; c < 256; c++) {
        const int p = a + b - c, pa = abs(p - a), pb = abs(p - b), pc = abs(p - c), m = pa < pb ? (pa < pc ? pa : pc) : (pb < pc ? pb : pc);
        const int want = pa == m ? a : pb == m ? b : c;
        if (png_paeth(a, b, c) != want) { fprintf(stderr, "paeth(%d, %d, %d)\n", a, b, c); return 1; }
    }
    for (int k = 1; k + 1 < argc; k += 2) if (one_case(argv[k], argv[k + 1], &pw)) return 1;
    printf("png_core_host_check: %d cases ok\n", (argc - 1) / 2);
    return 0;
}
