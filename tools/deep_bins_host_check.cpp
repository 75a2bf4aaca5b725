// deep_bins_host_check.cpp -- the bin table of the 16-bit mosaic gather (csrc/deep_bins.h) against a brute-force intersection, as a program
// of its own for the host sanitizers (no GPU, no HIP runtime, no libvfsms):
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I imagestitch_amd/csrc tools/deep_bins_host_check.cpp -o deep_bins_host_check
// Random layouts (tiles of mixed shapes, nested, repeated, touching the canvas's edges), every band of a few band heights, the ragged last
// one and bands no tile touches included: each block's list must be exactly the tiles whose rectangle meets the block, ascending.
#include "deep_bins.h"
#include <stdio.h>
#include <stdlib.h>
#include <random>

static int fail(const char *what, int layout, int row0, int b)
{
    printf("deep_bins_host_check: FAILED (%s) layout %d row0 %d block %d\n", what, layout, row0, b);
    return 1;
}

int main()
{
    std::mt19937 rng(20240611u);
    auto pick = [&](int lo, int hi) { return lo + (int)(rng() % (unsigned)(hi - lo + 1)); };
    long long checked = 0;
    for (int layout = 0; layout < 160; layout++) {
        const int rows = pick(1, 300), cols = pick(1, 1500), n = pick(1, 24);
        std::vector<DeepRect> T(n);
        for (int t = 0; t < n; t++) {
            if (t && pick(0, 5) == 0) { T[t] = T[pick(0, t - 1)]; continue; }      // the same position twice
            const int h = pick(1, rows), w = pick(1, cols);
            T[t] = DeepRect{pick(0, rows - h), pick(0, cols - w), h, w};
        }
        const int bands[4] = {1, 7, 64, rows};
        for (int bi = 0; bi < 4; bi++) {
            const int band = bands[bi] < rows ? bands[bi] : rows;
            for (int row0 = 0; row0 < rows; row0 += band) {
                const int nrows = row0 + band <= rows ? band : rows - row0;
                DeepBins B;
                if (!deep_bins_build(T.data(), n, cols, row0, nrows, (size_t)1 << 24, &B)) return fail("refused", layout, row0, -1);
                if (B.nby != (nrows + DEEP_BIN_H - 1) / DEEP_BIN_H || B.nbx != (cols + DEEP_BIN_W - 1) / DEEP_BIN_W) return fail("grid", layout, row0, -1);
                if (B.start.size() != (size_t)B.nby * B.nbx + 1 || B.start[0] != 0 || B.start.back() != B.list.size()) return fail("csr", layout, row0, -1);
                for (int by = 0; by < B.nby; by++)
                    for (int bx = 0; bx < B.nbx; bx++) {
                        const int b = by * B.nbx + bx;
                        const long long ya = (long long)row0 + by * DEEP_BIN_H, yb = ya + DEEP_BIN_H < (long long)row0 + nrows ? ya + DEEP_BIN_H : (long long)row0 + nrows;
                        const long long xa = (long long)bx * DEEP_BIN_W, xb = xa + DEEP_BIN_W < cols ? xa + DEEP_BIN_W : cols;
                        std::vector<uint32_t> want;
                        for (int t = 0; t < n; t++)
                            if (T[t].y0 < yb && (long long)T[t].y0 + T[t].h > ya && T[t].x0 < xb && (long long)T[t].x0 + T[t].w > xa) want.push_back((uint32_t)t);
                        if (B.start[b + 1] < B.start[b] || B.start[b + 1] - B.start[b] != want.size()) return fail("count", layout, row0, b);
                        for (size_t k = 0; k < want.size(); k++)
                            if (B.list[B.start[b] + k] != want[k]) return fail("list", layout, row0, b);
                        checked++;
                    }
            }
        }
    }
    // the refusal: more entries than the caller allows leaves nothing to use, and says so
    {
        DeepRect big{0, 0, 4096, 4096};
        DeepBins B;
        if (deep_bins_build(&big, 1, 4096, 0, 4096, 100, &B)) return fail("cap", -1, 0, -1);
        if (!deep_bins_build(&big, 1, 4096, 0, 4096, 4096, &B) || B.list.size() != 128u * 16u) return fail("cap2", -1, 0, -1);
    }
    // coordinates at the top of the int range: a band that ends at row 2^31 - 1
    {
        DeepRect far{2147483647 - 40, 0, 40, 10};
        DeepBins B;
        if (!deep_bins_build(&far, 1, 10, 2147483647 - 64, 64, 1 << 20, &B) || B.nby != 2 || B.list.size() != 2u) return fail("far", -1, 0, -1);
    }
    printf("deep_bins_host_check: %lld blocks ok\n", checked);
    return 0;
}
