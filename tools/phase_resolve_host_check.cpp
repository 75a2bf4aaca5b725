// phase_resolve_host_check.cpp -- the host-side pieces of Stitcher.phaseResolve = "ncc" (csrc/phase_resolve_math.h: the circular readings
// of a peak and the argument rules of the entry points) exercised as the plain C++ they are, for a sanitizer build:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I imagestitch_amd/csrc tools/phase_resolve_host_check.cpp -o /tmp/prhc && /tmp/prhc
// Walks every peak position of a set of surfaces (even, odd, padded, one row, production size), checks each reading against the rule
// restated independently, that every present peak keeps at least one reading, and the bounds of the tables an entry point fills.
#include "phase_resolve_math.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>

static int optimal(int n)
{
    for (int m = n;; m++) { int k = m; while (k % 2 == 0) k /= 2; while (k % 3 == 0) k /= 3; while (k % 5 == 0) k /= 5; if (k == 1) return m; }
}

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

int main()
{
    const int shapes[][2] = {{48, 160}, {160, 48}, {45, 75}, {49, 97}, {1, 1}, {1, 7}, {7, 1}, {2, 2}, {409, 2048}, {2048, 409}, {387, 2584}};
    long long readings = 0;
    for (auto &s : shapes) {
        const int h = s[0], w = s[1], M = optimal(h), N = optimal(w);
        for (int K = 1; K <= VFSMS_PHASE_MAX_PEAKS; K += 7) {
            std::vector<int32_t> cands((size_t)4 * K * 4), pk((size_t)2 * K);           // the tables of one job, exactly sized
            const long long step = (long long)M * N > 200000 ? 37 : 1;
            for (long long idx = 0; idx < (long long)M * N; idx += step) {
                int kept = 0;
                for (int k = 0; k < K; k++) {
                    const long long id = k == 0 ? idx : -1;                              // the other peaks absent
                    for (int pos = 0; pos < 4; pos++) {
                        const PhaseCand c = phase_candidate(id, pos, M, N, h, w);
                        int32_t *o = &cands[((size_t)4 * k + pos) * 4];
                        o[0] = c.dx; o[1] = c.dy; o[2] = 0; o[3] = c.kept;
                        if (k > 0) { CHECK(!c.present && !c.kept && c.dx == 0 && c.dy == 0); continue; }
                        const int uy = (int)(idx / N), ux = (int)(idx % N);
                        CHECK(c.present && c.dx == uy - ((pos & 1) ? M : 0) && c.dy == ux - ((pos & 2) ? N : 0));
                        CHECK(c.kept == (abs(c.dx) < h && abs(c.dy) < w));
                        CHECK(((c.dx % M) + M) % M == uy && ((c.dy % N) + N) % N == ux);
                        kept += c.kept; readings++;
                    }
                    pk[2 * k] = id < 0 ? -1 : (int)(id / N); pk[2 * k + 1] = id < 0 ? -1 : (int)(id % N);
                }
                CHECK(kept >= 1);                                                        // M < 2 h and N < 2 w
            }
        }
        CHECK(!phase_candidate((long long)M * N, 0, M, N, h, w).present && !phase_candidate(-1, 3, M, N, h, w).present);
    }
    CHECK(phase_resolve_params_ok(1, -1.0, 0) && phase_resolve_params_ok(8, 1.0, 1 << 30) && phase_resolve_params_ok(2, 0.5, 4096));
    CHECK(!phase_resolve_params_ok(0, 0.5, 0) && !phase_resolve_params_ok(9, 0.5, 0) && !phase_resolve_params_ok(-3, 0.5, 0));
    CHECK(!phase_resolve_params_ok(2, 1.0000001, 0) && !phase_resolve_params_ok(2, -1.5, 0) && !phase_resolve_params_ok(2, NAN, 0) && !phase_resolve_params_ok(2, INFINITY, 0));
    CHECK(!phase_resolve_params_ok(2, 0.5, -1));
    CHECK(phase_resolver_ok(0) && phase_resolver_ok(1) && !phase_resolver_ok(2) && !phase_resolver_ok(-1));
    printf("phase_resolve_host_check: %lld readings ok\n", readings);
    return 0;
}
