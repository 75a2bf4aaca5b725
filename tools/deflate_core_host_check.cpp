// deflate_core_host_check.cpp -- csrc/deflate_core.h, the rules of the lossless tile coder (Method.pyramidCompression = "deflate-device"), as the
// plain host C++ it is: the lines the kernels of csrc/deflate_kernels.hip compile, run serially over one tile's predicted bytes, for a
// sanitizer build that needs neither the HIP runtime nor libvfsms.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -I imagestitch_amd/csrc \
//       tools/deflate_core_host_check.cpp -o /tmp/dchc && /tmp/dchc case0.bin out0.bin [case1.bin out1.bin ...]
// (tests/test_deflate_host.py does this and compares every output with tests/deflate_ref.py.)  Per case the input file holds the predicted
// bytes of a tile; the output file holds, little-endian: uint32 n, the n tokens as int32 (a literal byte, or 256 + the match length); the 286
// code lengths as bytes; uint32 how often the counts were halved, uint32 the deepest code of the unlimited build; uint32 m, the m bytes of the
// zlib stream.
#include "deflate_core.h"
#include <stdio.h>
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

static int one_case(const char *in, const char *outp)
{
    std::vector<uint8_t> d;
    if (!read_file(in, &d) || d.empty() || d.size() > 0x7fffffff / DFL_MAX_BITS) { fprintf(stderr, "%s: no tile\n", in); return 1; }
    const int n = (int)d.size();
    // run start and run end of every byte: the forward and the backward scan of the device, serially
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
    int unlimited = 0;
    const int halvings = dfl_code_lengths(counts, lens, &build, &unlimited);
    dfl_codes(lens, table);
    // the stream, and its size as the device learns it: from the histogram alone
    BitSink sink;
    dfl_head(lens, sink);
    if (sink.at != DFL_HEAD_BITS) { fprintf(stderr, "%s: the head took %llu bits\n", in, sink.at); return 1; }
    for (int t : toks) { int nb; const uint32_t v = dfl_token_bits(t, table, &nb); sink(v, nb); }
    sink(table[DFL_END] >> 4, (int)(table[DFL_END] & 15));
    const unsigned long long bits = dfl_block_bits(hist, lens);
    if (sink.at != DFL_HEAD_BITS + bits) { fprintf(stderr, "%s: %llu bits written, %llu counted\n", in, sink.at, DFL_HEAD_BITS + bits); return 1; }
    // the Adler sums as the device forms them: partial sums of d and of (n - position) d, reduced chunk by chunk
    uint32_t sa = 0, sb = 0;
    for (int c0 = 0; c0 < n; c0 += 4096) {
        unsigned long long a = 0, b = 0;
        for (int p = c0; p < n && p < c0 + 4096; p++) { a += d[p]; b += (unsigned long long)(n - p) * d[p]; }
        sa = (sa + (uint32_t)(a % DFL_ADLER_MOD)) % DFL_ADLER_MOD; sb = (sb + (uint32_t)(b % DFL_ADLER_MOD)) % DFL_ADLER_MOD;
    }
    const uint32_t sum = dfl_adler((1u + sa) % DFL_ADLER_MOD, ((uint32_t)(n % DFL_ADLER_MOD) + sb) % DFL_ADLER_MOD);
    std::vector<uint8_t> stream = sink.out;
    for (int k = 0; k < 4; k++) stream.push_back((uint8_t)(sum >> (24 - 8 * k)));
    if (stream.size() != dfl_stream_bytes(bits)) { fprintf(stderr, "%s: %zu bytes written, %llu counted\n", in, stream.size(), dfl_stream_bytes(bits)); return 1; }

    std::vector<uint8_t> o;
    put32(&o, (uint32_t)toks.size());
    for (int t : toks) put32(&o, (uint32_t)t);
    o.insert(o.end(), lens, lens + DFL_SYMS);
    put32(&o, (uint32_t)halvings); put32(&o, (uint32_t)unlimited);
    put32(&o, (uint32_t)stream.size());
    o.insert(o.end(), stream.begin(), stream.end());
    FILE *f = fopen(outp, "wb");
    if (!f || fwrite(o.data(), 1, o.size(), f) != o.size()) { fprintf(stderr, "%s: cannot write\n", outp); if (f) fclose(f); return 1; }
    fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc < 3 || (argc - 1) % 2) { fprintf(stderr, "usage: %s tile.bin out.bin [tile.bin out.bin ...]\n", argv[0]); return 2; }
    // the length symbols against RFC 1951's table
    static const int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    static const int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int L = 3; L <= DFL_MAX_MATCH; L++) {
        int k = 28;
        while (base[k] > L) k--;
        int eb, ev;
        const int s = dfl_len_symbol(L, &eb, &ev);
        if (s != 257 + k || eb != extra[k] || ev != L - base[k] || dfl_symbol_tail_bits(s) != extra[k] + 1) { fprintf(stderr, "length %d: symbol %d, %d extra bits of value %d\n", L, s, eb, ev); return 1; }
    }
    for (int k = 1; k + 1 < argc; k += 2) if (one_case(argv[k], argv[k + 1])) return 1;
    printf("deflate_core_host_check: %d cases ok\n", (argc - 1) / 2);
    return 0;
}
