// arena_layout_host_check.cpp -- every arena record's layout function (csrc/arena_walk.h, the X_layout functions of csrc/common.h) walked
// as the plain host C++ it is, for a sanitizer build linked against the built library, so that the REAL layout functions run:
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -I imagestitch_amd/csrc tools/arena_layout_host_check.cpp -o /tmp/alhc -L imagestitch_amd/lib -lvfsms \
//       -Wl,-rpath,$PWD/imagestitch_amd/lib -Wl,-rpath,/opt/rocm/lib && /tmp/alhc
// (the sanitizer runtimes are linked into the program, so it runs as it is, with nothing preloaded; tests/test_arena_layout_host.py does this)
// No GPU, and no HIP runtime at work: a context here is its arena, a DevBuf whose allocation is hip_host_stubs.h's malloc.  For every record and shape: the counting walk gives
// `bytes`; a carve into exactly `bytes` succeeds, ends at `bytes` and leaves every pointer inside the buffer; a carve into
// bytes - 256 latches ok == false and ctx_arena_commit answers VFSMS_ERR_CAPACITY without moving the arena.
// Left out: the rocFFT path of phase_layout (a shape phase_own_shape refuses) -- its work buffer size comes from a rocFFT plan, which
// needs a device; its counting and carving halves are the same function as the LDS path's, and its peak lists are checked here.
#include "hip_host_stubs.h"
#include "common.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <functional>
#include <vector>

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s [%s]\n", __FILE__, __LINE__, #c, g_what); return 1; } } while (0)
static const char *g_what = "";
static int g_records = 0;
typedef std::vector<const void *> Ptrs;

// layout(a, p): the record's layout function over walk a, then every device pointer it set appended to p
// distinct: no two of the listed pointers may be equal (a record whose list names no array twice)
static int check_record(const char *what, const std::function<void(ArenaWalk &, Ptrs &)> &layout, bool distinct = false)
{
    g_what = what;
    ArenaWalk c; Ptrs p;
    layout(c, p);
    CHECK(c.ok && c.base == nullptr && c.off > 0 && !p.empty());
    for (const void *q : p) CHECK(q == nullptr);                       // a counting walk hands out nothing to dereference
    const size_t bytes = c.off;
    vfsms_ctx ctx, small;
    CHECK(ctx.arena.reserve(bytes, nullptr) == VFSMS_OK && small.arena.reserve(bytes > 256 ? bytes - 256 : bytes - 1, nullptr) == VFSMS_OK);
    const char *buf = ctx.arena.as<char>();
    ArenaWalk a = ctx_arena_walk(&ctx);
    p.clear();
    layout(a, p);
    CHECK(a.ok && a.off == bytes);
    CHECK(ctx_arena_commit(&ctx, a, what) == VFSMS_OK && ctx.arena_off == bytes);
    for (const void *q : p) CHECK(q != nullptr && (const char *)q >= buf && (const char *)q < buf + bytes);
    if (distinct) for (size_t i = 0; i < p.size(); i++) for (size_t j = 0; j < i; j++) CHECK(p[i] != p[j]);
    ArenaWalk s = ctx_arena_walk(&small);
    p.clear();
    layout(s, p);
    CHECK(!s.ok && s.off <= small.arena.bytes());
    CHECK(ctx_arena_commit(&small, s, what) == VFSMS_ERR_CAPACITY && small.arena_off == 0);
    g_records++;
    return 0;
}

static void list(Ptrs &p, const RoiDev &r, int nlayers)
{
    for (const void *q : {(const void *)r.sum, (const void *)r.pair, (const void *)r.icarry, (const void *)r.cand, (const void *)r.kps, (const void *)r.patch,
                          (const void *)r.keep_pos, (const void *)r.order, (const void *)r.kps_xy, (const void *)r.desc, (const void *)r.kps_out}) p.push_back(q);
    for (int l = 0; l < nlayers; l++) p.push_back(r.det[l]);
}
static void list(Ptrs &p, const MatchDev &m, bool filter)
{
    for (const void *q : {(const void *)m.p_d1, (const void *)m.p_d2, (const void *)m.p_i1, (const void *)m.d1, (const void *)m.d2, (const void *)m.i1,
                          (const void *)m.match_flag, (const void *)m.match_pos, (const void *)m.pairs, (const void *)m.votes, (const void *)m.mcount,
                          (const void *)m.vsum, (const void *)m.result}) p.push_back(q);
    if (filter) for (const void *q : {(const void *)m.c_ent, (const void *)m.c_cnt, (const void *)m.q16, (const void *)m.t16, (const void *)m.c_m12}) p.push_back(q);
}
static void list(Ptrs &p, const OrbDev &r, int nlevels, int first_level)
{
    for (int l = 0; l < nlevels; l++) {
        if (l != first_level) p.push_back(r.lv[l]);
        p.push_back(r.bl[l]); p.push_back(r.score[l]); p.push_back(r.nms[l]);
    }
    for (const void *q : {(const void *)r.hist, (const void *)r.k1_xy, (const void *)r.k1_resp, (const void *)r.k2_xy, (const void *)r.k2_resp, (const void *)r.k2_angle,
                          (const void *)r.kps_xy, (const void *)r.desc, (const void *)r.kps_out}) p.push_back(q);
}
static void list(Ptrs &p, const EnhJob &J) { p.push_back(J.dst); p.push_back(J.hist); p.push_back(J.lut); }

static void orb_caps(const vfsms_orb_params &P, int *c1, int *c2, int *c)      // api.hip's default capacities
{
    const float f = 1.f / P.scale_factor;
    const int q0 = (int)lrintf(P.n_features * (1 - f) / (1 - powf(f, (float)P.n_levels)));
    *c1 = 4 * q0 + 2048; *c2 = 2 * q0 + 1024; *c = 2 * P.n_features + 2048;
}

static int check_walker()
{
    g_what = "walker";
    char buf[1024];
    ArenaWalk a{buf, 3, sizeof(buf)};                                   // an unaligned start
    CHECK(a.take<char>(1, 1) == buf + 3 && a.off == 4);
    CHECK(a.take<char>(2, 1) == buf + 4 && a.off == 6);
    CHECK((char *)a.take<int>(1, 4) == buf + 8 && a.off == 12);
    CHECK((char *)a.take<int>(0, 4) == buf + 12 && a.off == 16);        // a zero count takes one element
    CHECK(a.take<char>(5) == buf + 256 && a.off == 261);
    a.pad();
    CHECK(a.ok && a.off == 512);
    CHECK((char *)a.take<double>(64) == buf + 512 && a.off == 1024 && a.ok);      // to the last byte
    CHECK(a.take<char>(1, 1) == nullptr && !a.ok && a.off == 1024);     // the first request that does not fit latches ...
    CHECK(a.take<char>(0, 1) == nullptr && !a.ok && a.off == 1024);
    ArenaWalk b{buf, 0, 300};
    CHECK(b.take<char>(1) == buf && b.take<char>(64) == nullptr && !b.ok && b.off == 1);      // ... the aligned start lies behind the limit
    CHECK(b.take<char>(1, 1) == nullptr && b.off == 1);                 // ... and a later, smaller request that would fit gets nothing
    b.pad();
    CHECK(!b.ok && b.off == 1);
    ArenaWalk c;                                                        // counting: no limit, but no product that wraps
    CHECK(c.take<double>(7) == nullptr && c.ok && c.off == 56);
    CHECK(c.take<double>(SIZE_MAX / 4) == nullptr && !c.ok && c.off == 56);
    ArenaWalk d;
    CHECK(d.take<char>(SIZE_MAX - 100, 1) == nullptr && d.ok && d.off == SIZE_MAX - 100);
    CHECK(d.take<char>(1) == nullptr && !d.ok && d.off == SIZE_MAX - 100);        // rounding the offset up would wrap
    ArenaWalk e;
    CHECK(e.take<uint16_t>(SIZE_MAX / 2 + 2) == nullptr && !e.ok && e.off == 0);
    return 0;
}

int main()
{
    if (check_walker()) return 1;
    char what[256];
    // SURF ROI (h, w, cap): default 4 octaves x (3 + 2) layers -- at (7, 9) and (1, 1) the coarse layers have zero cells
    const int surf_shapes[][4] = {{1, 1, 1, 0}, {7, 9, 1, 0}, {37, 41, 64, 0}, {409, 2048, 6000, 0}, {409, 2048, 6000, 1}};
    for (auto &s : surf_shapes) {
        const vfsms_surf_params P = {100.f, 4, 3, s[3], 0};
        snprintf(what, sizeof(what), "SURF ROI %d x %d cap %d extended %d", s[0], s[1], s[2], s[3]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { RoiDev r; surf_roi_layout(a, &r, nullptr, s[1], s[0], s[1], s[2], &P); list(p, r, 20); })) return 1;
        snprintf(what, sizeof(what), "describe work list capsum %d", s[2]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { DescWork W; surf_describe_layout(a, &W, s[2]); p.insert(p.end(), {W.tickets, W.plan, W.rec_big, W.rec_small}); })) return 1;
    }
    // match job (capq, nsplit) and its filter (capq, capt, cns): both sides of the 32-train tile
    const int match_shapes[][2] = {{1, 1}, {6000, 8}};
    for (auto &s : match_shapes) {
        snprintf(what, sizeof(what), "match %d x %d", s[0], s[1]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { MatchDev m = {}; match_layout(a, &m, s[0], 64, s[1]); list(p, m, false); }, true)) return 1;
        // a run of this one job, exhaustive plan: the job's count plus the run's result row (the job's `result` points there) and its uploaded record
        const MatchPlan P = {false, s[1], 0};
        MatchJob J = {}; J.capq = J.capt = s[0];
        snprintf(what, sizeof(what), "match run of one, %d x %d", s[0], s[1]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { MatchRun run; match_run_layout(a, &run, &J, 1, 64, P); p.push_back(run.dM); list(p, run.M[0], false); }, true)) return 1;
        ArenaWalk c, r; MatchDev m; MatchRun run;
        c.take<int32_t>(VFSMS_ATTEMPT_INTS); match_layout(c, &m, s[0], 64, s[1]); c.take<MatchDev>(1);
        match_run_layout(r, &run, &J, 1, 64, P);
        CHECK(r.ok && r.off == c.off);
    }
    const int filter_shapes[][3] = {{1, 1, 1}, {256, 31, 1}, {256, 32, 2}, {257, 33, 4}};
    for (auto &s : filter_shapes) {
        snprintf(what, sizeof(what), "match + filter %d, %d, %d", s[0], s[1], s[2]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { MatchDev m = {}; match_layout(a, &m, s[0], 64, 1); match_filter_layout(a, &m, s[0], s[1], s[2]); list(p, m, true); }, true)) return 1;
        snprintf(what, sizeof(what), "filter %d, %d, %d", s[0], s[1], s[2]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { MatchDev m = {}; match_filter_layout(a, &m, s[0], s[1], s[2]); p.insert(p.end(), {m.c_ent, m.c_cnt, m.q16, m.t16, m.c_m12}); }, true)) return 1;
        // a run of this one job, filtered plan, answers for itself: exactly enough, then 256 bytes short
        const MatchPlan P = {true, 1, s[2]};
        MatchJob J = {}; J.capq = s[0]; J.capt = s[1];
        snprintf(what, sizeof(what), "filtered match run of one, %d, %d, %d", s[0], s[1], s[2]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { MatchRun run; match_run_layout(a, &run, &J, 1, 64, P); p.push_back(run.dM); list(p, run.M[0], true); }, true)) return 1;
        ArenaWalk c; MatchRun run;
        match_run_layout(c, &run, &J, 1, 64, P);
        const size_t bytes = c.off;
        vfsms_ctx ctx, small;
        CHECK(ctx.arena.reserve(bytes, nullptr) == VFSMS_OK && small.arena.reserve(bytes - 256, nullptr) == VFSMS_OK);
        ArenaWalk a = ctx_arena_walk(&ctx), b = ctx_arena_walk(&small);
        match_run_layout(a, &run, &J, 1, 64, P);
        CHECK(ctx_arena_commit(&ctx, a, what) == VFSMS_OK && ctx.arena_off == bytes && run.M[0].c_m12 != nullptr && run.dM != nullptr);
        match_run_layout(b, &run, &J, 1, 64, P);
        CHECK(ctx_arena_commit(&small, b, what) == VFSMS_ERR_CAPACITY && small.arena_off == 0);
    }
    // ORB ROI
    const int orb_shapes[][4] = {{31, 31, 8, 5000}, {64, 2048, 8, 5000}, {31, 31, 1, 5000}, {64, 2048, 8, 1}, {64, 2048, 1, 1}};
    for (auto &s : orb_shapes) {
        const vfsms_orb_params P = {s[3], 1.2f, s[2], 31, 0, 2, 0, 31, 20};
        int c1, c2, c;
        orb_caps(P, &c1, &c2, &c);
        snprintf(what, sizeof(what), "ORB ROI %d x %d, %d levels, %d features", s[0], s[1], s[2], s[3]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { OrbDev r; orb_roi_layout(a, &r, nullptr, s[1], s[0], s[1], &P, c1, c2, c); list(p, r, s[2], 0); })) return 1;
    }
    // enhancement job (mode, grid) at 10 x 13 (no grid divides it) and a strip
    const int enh_shapes[][2] = {{1, 0}, {2, 1}, {2, 5}, {2, 64}};
    for (auto &s : enh_shapes) for (auto &hw : {std::make_pair(10, 13), std::make_pair(409, 2048)}) {
        snprintf(what, sizeof(what), "enhance %d x %d mode %d grid %d", hw.first, hw.second, s[0], s[1]);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { EnhJob J; enhance_layout(a, &J, nullptr, hw.second, hw.first, hw.second, s[0], s[1]); list(p, J); })) return 1;
        g_what = what;
        ArenaWalk c; EnhJob J;
        enhance_layout(c, &J, nullptr, hw.second, hw.first, hw.second, s[0], s[1]);
        CHECK(enhance_scratch_bytes(hw.first, hw.second, s[0], s[1]) == c.off);
        CHECK(J.eh >= hw.first && J.ew >= hw.second && (s[0] != 2 || (J.eh % s[1] == 0 && J.ew % s[1] == 0)));
    }
    // phase batch, LDS path: (160, 48) takes the transposed orientation; nb on both sides of the chunk (32); with and without a sink
    const int phase_shapes[][2] = {{48, 160}, {160, 48}, {409, 2048}};
    for (auto &s : phase_shapes) for (int nb : {1, 33}) for (int K : {0, 1, 8}) {
        snprintf(what, sizeof(what), "phase %d x %d, %d jobs, K %d", s[0], s[1], nb, K);
        int32_t info[8];
        CHECK(vfsms_phase_plan(s[0], s[1], info) == VFSMS_OK && info[0] == 1 && info[1] == (s[0] == 160));      // the LDS path, transposed or not
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                PhaseScratch sc;
                if (phase_layout(nullptr, a, &sc, s[0], s[1], nb, K) != VFSMS_OK) a.ok = false;
                p.insert(p.end(), {sc.RE, sc.FQ, sc.CP, sc.partial, sc.jobs});
                if (info[1]) p.push_back(sc.TB);
                if (K) p.push_back(sc.ppart);
            })) return 1;
        if (K && check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                PhaseResolveDev d; PhaseScratch sc;
                phase_resolve_layout(a, &d, nb, K);
                if (phase_layout(nullptr, a, &sc, s[0], s[1], nb, K) != VFSMS_OK) a.ok = false;
                p.insert(p.end(), {d.out3, d.peaks, d.sums, d.jobs, sc.RE, sc.FQ, sc.CP, sc.partial, sc.jobs, sc.ppart});
            })) return 1;
    }
    // phase peaks: also of a shape the LDS transforms refuse (rows of 9000 points)
    for (auto &s : {std::make_pair(48, 160), std::make_pair(160, 48), std::make_pair(9000, 9000)}) for (int nb : {1, 33}) for (int K : {1, 8}) {
        snprintf(what, sizeof(what), "phase peaks %d x %d, %d jobs, K %d", s.first, s.second, nb, K);
        int32_t info[8];
        CHECK(vfsms_phase_plan(s.first, s.second, info) == VFSMS_OK && info[0] == (s.first != 9000));
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) { PhaseScratch sc; phase_peaks_layout(a, &sc, s.first, s.second, nb, K); p.push_back(sc.ppart); })) return 1;
        ArenaWalk c; PhaseScratch sc;
        phase_peaks_layout(c, &sc, s.first, s.second, nb, K);
        CHECK(phase_peaks_bytes(s.first, s.second, nb, K) == c.off);
    }
    // runs: 1 source, and 3 sources of two shapes
    const vfsms_surf_params SP = {100.f, 4, 3, 0, 0};
    const vfsms_orb_params OP = {5000, 1.2f, 8, 31, 0, 2, 0, 31, 20};
    const int run_shapes[3][2] = {{409, 2048}, {409, 2048}, {2048, 409}};
    for (int n : {1, 3}) {
        std::vector<SurfSrc> S(n); std::vector<StripTable::Strip> T(n); std::vector<MatchJob> J(n, MatchJob{});
        for (int i = 0; i < n; i++) {
            const int h = run_shapes[i][0], w = run_shapes[i][1], cap = h * w / 24 + 4096;
            S[i] = SurfSrc{nullptr, w, h, w, cap}; T[i] = StripTable::Strip{nullptr, w, h, w};
            J[i].capq = J[i].capt = cap; J[i].row = n - 1 - i;
        }
        for (int mode : {0, 2}) {
            const SurfEnh enh = {mode, 40.0, 5};
            snprintf(what, sizeof(what), "SURF run of %d, enhance %d", n, mode);
            if (check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                    SurfRun run;
                    surf_run_layout(a, &run, S.data(), n, &SP, enh);
                    p.push_back(run.cblock); p.push_back(run.dR);
                    if (mode) p.push_back(run.dE);
                    for (int i = 0; i < n; i++) { list(p, run.R[i], 20); p.push_back(run.R[i].counters); if (mode) list(p, run.E[i]); }
                })) return 1;
        }
        for (int filtered : {0, 1}) {
            const MatchPlan P = {filtered != 0, filtered ? 1 : 4, 2};
            snprintf(what, sizeof(what), "match run of %d, filtered %d", n, filtered);
            if (check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                    MatchRun run;
                    match_run_layout(a, &run, J.data(), n, 64, P);
                    p.push_back(run.dM);                                  // (run.rblock is the result row of the job of row 0)
                    for (int i = 0; i < n; i++) list(p, run.M[i], filtered != 0);
                }, true)) return 1;
        }
        int c1, c2, c;
        orb_caps(OP, &c1, &c2, &c);
        snprintf(what, sizeof(what), "ORB run of %d", n);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                OrbRun run;
                orb_run_layout(a, &run, T.data(), n, &OP, c1, c2, c);
                p.push_back(run.cblock); p.push_back(run.dR);
                for (int i = 0; i < n; i++) { list(p, run.R[i], 8, 0); p.insert(p.end(), {run.R[i].counters, run.R[i].thr1, run.R[i].n1, run.R[i].n2}); }
            })) return 1;
    }
    // SIFT strip block: the plan of an h x w strip at the default 3 layers (sift_kernels.hip: sift_plan), restated
    for (auto &s : {std::make_pair(32, 32), std::make_pair(409, 2048)}) {
        const int L = 3, no = std::max((int)lrint(log((double)std::min(2 * s.first, 2 * s.second)) / log(2.) - 2) + 1, 0);
        size_t pyr = 0; int nslots = 0, R = 2 * s.first, C = 2 * s.second;
        for (int o = 0; o < no; o++) { if (o) { R /= 2; C /= 2; } pyr += (size_t)(2 * L + 5) * R * C; nslots += L * R; }
        snprintf(what, sizeof(what), "SIFT strip %d x %d", s.first, s.second);
        if (check_record(what, [&](ArenaWalk &a, Ptrs &p) {
                SiftStripDev d;
                sift_strip_layout(a, &d, pyr, (size_t)4 * s.first * s.second, nslots);
                p.insert(p.end(), {d.pyr, d.t0, d.t1, d.counts});
            })) return 1;
        ArenaWalk c; SiftStripDev d;
        sift_strip_layout(c, &d, pyr, (size_t)4 * s.first * s.second, nslots);
        g_what = what;
        CHECK(c.off % 256 == 0);                                        // the distance between the blocks of two strips keeps every block aligned
    }
    printf("arena_layout_host_check: %d records ok\n", g_records);
    return 0;
}
