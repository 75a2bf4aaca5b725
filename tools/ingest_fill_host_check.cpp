// ingest_fill_host_check.cpp -- csrc/ingest_fill.h, the transaction behind every vfsms_tile_fill* entry, as the plain host C++ it is, for a
// sanitizer build that links neither the HIP runtime nor libvfsms: the runtime calls are tools/hip_host_stubs.h's, over malloc / free / memcpy.
//   c++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -I imagestitch_amd/csrc tools/ingest_fill_host_check.cpp -o /tmp/ifhc && /tmp/ifhc
// (the sanitizer runtimes are linked into the program, so it runs as it is, with nothing preloaded; tests/test_ingest_fill_host.py does this)
// The orderings a GPU test cannot reach, because they show only when a runtime call fails: the copy stream is quiet before a staging buffer
// goes back to a pool, tiles are never left reserved after work was enqueued on them, and never given up when a file was merely refused.
// fill() below is an entry of api.hip in small -- lookup, host staging, 0 / 1 / 4 device leases, a copy, a body, the end -- and every row of
// the behaviour table is driven through it for begin_one and begin_pair, with a failure injected at each position.  The stubs' probe writes
// the pools' sizes into the log INSIDE every synchronising call: "sync(stream) pools(p,d)" with the sizes of before the fill's leases went back
// is the ordering.  At exit nothing is live; LeakSanitizer agrees or fails the run.
#include "hip_host_stubs.h"
#include "ingest_fill.h"
#include <stdarg.h>
#include <algorithm>
#include <memory>

static char g_err[512] = "";
void vfsms_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_checks = 0;
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "%s:%d: %s\n  (%s)\n", __FILE__, __LINE__, #c, g_what.c_str()); for (auto &l : g_hip.log) fprintf(stderr, "  log: %s\n", l.c_str()); return 1; } } while (0)
static std::string g_what;                                      // the scenario at work, for a failing CHECK
static vfsms_ctx *g_ctx = nullptr;
static void probe_pools() { char b[64]; snprintf(b, sizeof(b), "pools(%zu,%zu)", g_ctx->pin_pool.size(), g_ctx->stage_pool.size()); g_hip.log.push_back(b); }
static std::string pools(size_t p, size_t d) { char b[64]; snprintf(b, sizeof(b), "pools(%zu,%zu)", p, d); return b; }
static long at(const std::string &line) { auto it = std::find(g_hip.log.begin(), g_hip.log.end(), line); return it == g_hip.log.end() ? -1 : (long)(it - g_hip.log.begin()); }
static long count(const char *prefix) { long n = 0; for (auto &l : g_hip.log) n += l.compare(0, strlen(prefix), prefix) == 0; return n; }
// every pooled buffer is one live allocation, no pointer twice: each lease came back exactly once, none was lost
static bool pools_hold_all_live(vfsms_ctx *ctx)
{
    std::vector<uint8_t *> p;
    for (auto &b : ctx->pin_pool) p.push_back(b.ptr);
    for (auto &b : ctx->stage_pool) p.push_back(b.ptr);
    std::sort(p.begin(), p.end());
    return std::adjacent_find(p.begin(), p.end()) == p.end() && (long)p.size() == g_hip.live;
}

// the reserved tiles of the checks: "device" pixels in plain memory, events from the stubs
struct Tiles {
    vfsms_ctx *ctx; std::vector<std::unique_ptr<uint8_t[]>> mem;
    int64_t add(int h, int w, int ch, int fill = 1)
    {
        TileRec t; t.h = h; t.w = w; t.stride = w * ch; t.owned = false; t.pending = true; t.ch = ch; t.bytes = (size_t)h * w * ch; t.fill = fill;
        mem.emplace_back(new uint8_t[t.bytes]()); t.ptr = mem.back().get();
        (void)hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
        const int64_t hd = ctx->next_handle++;
        ctx->tiles[hd] = t;
        return hd;
    }
    void reset(int64_t hd) { if (hd) { TileRec &t = ctx->tiles[hd]; t.fill = 1; t.pending = true; memset(t.ptr, 0, t.bytes); } }
    ~Tiles() { for (auto &kv : ctx->tiles) (void)hipEventDestroy(kv.second.ready); ctx->tiles.clear(); }
};

enum Early { NONE, BEFORE_ENQUEUE, AFTER_ENQUEUE };
struct Shot {
    bool pair; int64_t a, b;           // begin_pair(a, b) or begin_one(a)
    const uint8_t *src; int stride;    // the pixels (nullptr: give up), begin_one's row stride
    int leases;                        // device leases: 0 (the copy goes to the tile itself), 1 or 4
    int bad_format, host_refusal, body_rc;   // codes returned at the three places an entry can stop or fail by itself
    Early early;                       // a return that leaves the object un-finished
};
static int fill(vfsms_ctx *ctx, const Shot &s)
{
    TileFill f(ctx);
    TRY(s.pair ? f.begin_pair(s.a, s.b, "check", !s.src) : f.begin_one(s.a, "check", !s.src));
    if (!s.src) return VFSMS_OK;
    if (s.bad_format) return f.refuse(s.bad_format);
    const size_t n = (size_t)f.h * f.w * f.ch;
    const uint8_t *host;
    if (s.pair) { uint8_t *hb = f.host(n); memcpy(hb, s.src, n); host = hb; }       // a decode into staging
    else host = f.pack(s.src, s.stride, (size_t)f.w * f.ch, f.h);
    if (s.host_refusal) return f.refuse(s.host_refusal);
    uint8_t *d[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < s.leases; k++) d[k] = f.device(n + 16 * (size_t)k);
    if (s.early == BEFORE_ENQUEUE) return VFSMS_ERR_CAPACITY;
    uint8_t *first = s.leases ? d[0] : f.dg ? f.dg : f.dc;
    f.copy(first, host, n);
    if (s.early == AFTER_ENQUEUE) return VFSMS_ERR_CAPACITY;
    bool handed_back = false;
    f.run([&] {
        if (s.body_rc) { handed_back = s.body_rc == VFSMS_ERR_UNSUPPORTED; return s.body_rc; }
        for (int k = 1; k < s.leases; k++) memset(d[k], k, n + 16 * (size_t)k);    // (ASan: every lease is as large as asked for)
        if (s.leases && f.dg) memcpy(f.dg, d[0], n);
        // the gray replication, from the last pixel down: with no lease and no gray tile the plane lies at the start of the colour tile itself
        for (size_t i = f.dc ? n : 0; i-- > 0;) { const uint8_t v = first[i]; for (int c = 0; c < 3; c++) f.dc[3 * i + c] = v; }
        return VFSMS_OK;
    });
    return handed_back ? f.refuse(f.rc) : f.finish();
}

// the injection positions of the failure row; the program prints their number
struct Inject { const char *name, *kind; int nth, min_leases; };
static const Inject POSITIONS[] = { {"first device allocation", "hipMalloc", 1, 1}, {"third device allocation", "hipMalloc", 3, 4}, {"the copy", "copy", 1, 0},
                                    {"the body", nullptr, 0, 0}, {"the event record", "record", 1, 0}, {"the event wait", "wait", 1, 0} };
static const int N_POSITIONS = (int)(sizeof(POSITIONS) / sizeof(POSITIONS[0]));
static const int N_ROWS = 8;                                     // the rows of the behaviour table, row1 .. row8 below

struct Bed {
    vfsms_ctx *ctx; Tiles *T; int64_t one, gray, color; int h, w; std::vector<uint8_t> src3, src1;
    hipStream_t stream() const { return ctx->copy_stream; }
    TileRec &rec(int64_t hd) const { return ctx->tiles.at(hd); }
    // the modes a scenario runs in: begin_one on a 3-channel tile, begin_pair on both tiles, gray alone, colour alone
    struct Mode { const char *name; bool pair; int64_t a, b; };
    std::vector<Mode> modes() const { return { {"one", false, one, 0}, {"pair", true, gray, color}, {"gray", true, gray, 0}, {"colour", true, 0, color} }; }
    Shot shot(const Mode &m, int leases) const { return Shot{m.pair, m.a, m.b, m.pair ? src1.data() : src3.data(), w * 3, leases, 0, 0, 0, NONE}; }
    void fresh(const Mode &m) const { T->reset(m.a); T->reset(m.b); g_hip.log.clear(); g_err[0] = 0; }
    bool tiles_are(const Mode &m, int fill, bool pending) const
    {
        for (int64_t hd : {m.a, m.b}) if (hd && (rec(hd).fill != fill || rec(hd).pending != pending)) return false;
        return true;
    }
    bool pixels_ok(const Mode &m) const
    {
        if (!m.pair) return memcmp(rec(m.a).ptr, src3.data(), src3.size()) == 0;
        if (m.a && memcmp(rec(m.a).ptr, src1.data(), src1.size()) != 0) return false;
        for (size_t i = 0; m.b && i < src1.size(); i++) for (int c = 0; c < 3; c++) if (rec(m.b).ptr[3 * i + c] != src1[i]) return false;
        return true;
    }
};
static std::string what(const char *row, const Bed::Mode &m, int leases, const char *extra = "") { char b[160]; snprintf(b, sizeof(b), "%s, %s, %d leases %s", row, m.name, leases, extra); return b; }

// row 1: unknown handle, wrong channel count, not reserved, sizes differ -> BAD_ARG, tiles untouched, nothing taken
static int row1(const Bed &B)
{
    const int64_t filled = B.T->add(B.h, B.w, 1, 0), other = B.T->add(B.h + 1, B.w, 3);
    const Shot bad[] = { {false, 999, 0, B.src3.data(), B.w * 3, 1}, {false, filled, 0, B.src1.data(), B.w, 1}, {true, 999, B.color, B.src1.data(), 0, 1},
                         {true, B.color, 0, B.src1.data(), 0, 1}, {true, B.gray, B.gray, B.src1.data(), 0, 1}, {true, 0, 0, B.src1.data(), 0, 1},
                         {true, filled, B.color, B.src1.data(), 0, 1}, {true, B.gray, other, B.src1.data(), 0, 1}, {true, 999, 0, nullptr, 0, 0} };
    g_what = "row 1";
    for (const Shot &s : bad) {
        B.fresh({"", true, B.gray, B.color}); B.T->reset(other);
        CHECK(fill(B.ctx, s) == VFSMS_ERR_BAD_ARG && g_err[0] && g_hip.log.empty());
        CHECK(B.tiles_are({"", true, B.gray, B.color}, 1, true) && B.rec(other).fill == 1 && B.rec(filled).fill == 0 && B.rec(filled).pending);
    }
    return 0;
}
// row 2: src == NULL gives the tiles up at once.  row 3: a bad stride or format refuses before anything is taken
static int row2_row3(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) {
        g_what = what("row 2", m, 0);
        B.fresh(m);
        Shot s = B.shot(m, 1); s.src = nullptr;
        CHECK(fill(B.ctx, s) == VFSMS_OK && g_hip.log.empty() && B.tiles_are(m, 2, true));
        CHECK(fill(B.ctx, s) == VFSMS_ERR_BAD_ARG && B.tiles_are(m, 2, true));      // (given up is not reserved)
        g_what = what("row 3", m, 0);
        B.fresh(m);
        s = B.shot(m, 1); s.bad_format = VFSMS_ERR_BAD_ARG;
        CHECK(fill(B.ctx, s) == VFSMS_ERR_BAD_ARG && g_hip.log.empty() && B.tiles_are(m, 1, true));
    }
    return 0;
}
// row 4: the host side refuses the file: the pinned lease goes back, no stream call, the tiles stay reserved.  Also the object dropped
// before anything was enqueued, with device leases held
static int row4(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) for (int code : {VFSMS_ERR_UNSUPPORTED, VFSMS_ERR_BAD_ARG}) for (int pass = 0; pass < 2; pass++) {
        g_what = what("row 4", m, 0, pass ? "warm" : "cold");
        if (!pass) stage_pools_free(B.ctx);
        B.fresh(m);
        Shot s = B.shot(m, 0); s.host_refusal = code;
        CHECK(fill(B.ctx, s) == code && B.tiles_are(m, 1, true));
        CHECK(count("malloc(") == (pass ? 0 : 1) && (long)g_hip.log.size() == (pass ? 0 : 1));        // no sync, no record, no wait
        CHECK(B.ctx->pin_pool.size() == 1 && B.ctx->stage_pool.empty() && pools_hold_all_live(B.ctx));
    }
    for (const Bed::Mode &m : B.modes()) for (int leases : {0, 1, 4}) {
        g_what = what("dropped before the enqueue", m, leases);
        stage_pools_free(B.ctx); B.fresh(m);
        Shot s = B.shot(m, leases); s.early = BEFORE_ENQUEUE;
        CHECK(fill(B.ctx, s) == VFSMS_ERR_CAPACITY && B.tiles_are(m, 1, true));
        CHECK(count("malloc(") == 1 + leases && (long)g_hip.log.size() == 1 + leases);
        CHECK(B.ctx->pin_pool.size() == 1 && (int)B.ctx->stage_pool.size() == leases && pools_hold_all_live(B.ctx));
    }
    return 0;
}
// row 5: the body hands the file back after work was enqueued: the stream is synchronised, THEN the leases go back, the tiles stay reserved
static int row5(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) for (int leases : {1, 4}) for (int pass = 0; pass < 2; pass++) {
        g_what = what("row 5", m, leases, pass ? "warm" : "cold");
        if (!pass) stage_pools_free(B.ctx);
        B.fresh(m);
        Shot s = B.shot(m, leases); s.body_rc = VFSMS_ERR_UNSUPPORTED;
        CHECK(fill(B.ctx, s) == VFSMS_ERR_UNSUPPORTED && B.tiles_are(m, 1, true));
        const long sync = at(stub_name("sync", B.stream()));
        CHECK(sync >= 0 && g_hip.log[sync + 1] == pools(0, 0) && sync + 2 == (long)g_hip.log.size());   // at the sync the leases were still out
        CHECK(count("record(") == 0 && count("wait(") == 0 && count("free(") == 0 && count("malloc(") == (pass ? 0 : 1 + leases));
        CHECK(B.ctx->pin_pool.size() == 1 && (int)B.ctx->stage_pool.size() == leases && pools_hold_all_live(B.ctx));
    }
    return 0;
}
// row 6: no pinned memory: the fill succeeds from pageable memory (or from the caller's own dense rows), the sticky error is taken
static int row6(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) for (int leases : {0, 1, 4}) for (int strided = 0; strided < (m.pair ? 1 : 2); strided++) {
        g_what = what("row 6", m, leases, strided ? "strided" : "dense");
        stage_pools_free(B.ctx); B.fresh(m);
        std::vector<uint8_t> wide((size_t)B.h * (B.w * 3 + 5), 0xEE);
        for (int y = 0; y < B.h; y++) memcpy(&wide[(size_t)y * (B.w * 3 + 5)], &B.src3[(size_t)y * B.w * 3], (size_t)B.w * 3);
        Shot s = B.shot(m, leases);
        if (strided) { s.src = wide.data(); s.stride = B.w * 3 + 5; }
        fail_call("hipHostMalloc", 1);
        CHECK(fill(B.ctx, s) == VFSMS_OK && B.tiles_are(m, 0, false) && B.pixels_ok(m));
        CHECK(!g_hip.fail_kind && at("getlasterror") == 1 && g_hip.sticky == hipSuccess);
        CHECK(count("sync(") == 0 && count("record(") == 1 && count("wait(") == 1);
        CHECK(B.ctx->pin_pool.empty() && (int)B.ctx->stage_pool.size() == leases && pools_hold_all_live(B.ctx));
    }
    return 0;
}
// row 7: a device staging allocation, the copy, the body or an event call fails after the lookup: the stream is synchronised before any
// lease goes back, each goes back once, the tiles are given up.  Also the object dropped after the enqueue
static int row7(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) for (int leases : {0, 1, 4}) for (const Inject &I : POSITIONS) for (int pass = 0; pass < 2; pass++) {
        const bool alloc = I.kind && !strcmp(I.kind, "hipMalloc");
        if (leases < I.min_leases || (alloc && pass)) continue;          // (a warm pool allocates nothing: no allocation to fail)
        g_what = what("row 7", m, leases, I.name);
        if (!pass) stage_pools_free(B.ctx);
        B.fresh(m);
        Shot s = B.shot(m, leases);
        if (I.kind) fail_call(I.kind, I.nth); else s.body_rc = VFSMS_ERR_CAPACITY;
        const int got = alloc ? I.nth - 1 : leases;                      // the device leases the fill holds when it ends
        const int rc = fill(B.ctx, s);
        CHECK(!g_hip.fail_kind && B.tiles_are(m, 2, false));
        if (I.kind) CHECK(rc == VFSMS_ERR_HIP && !strncmp(g_err, "check: ", 7) && strstr(g_err, alloc ? "out of memory" : "unknown error"));
        else CHECK(rc == VFSMS_ERR_CAPACITY);
        const long sync = at(stub_name("sync", B.stream()));
        CHECK(sync >= 0 && g_hip.log[sync + 1] == pools(0, 0) && sync + 2 == (long)g_hip.log.size() && count("sync(") == 1 && count("free(") == 0);
        CHECK(count("record(") == (I.kind && !alloc && strcmp(I.kind, "copy") ? 1 : 0) && count("wait(") == (I.kind && !strcmp(I.kind, "wait") ? 1 : 0));
        CHECK(B.ctx->pin_pool.size() == 1 && (int)B.ctx->stage_pool.size() == got && pools_hold_all_live(B.ctx));
        CHECK(count("malloc(") == (pass ? 0 : 1 + (alloc ? I.nth : leases)));
    }
    for (const Bed::Mode &m : B.modes()) for (int leases : {0, 1, 4}) {
        g_what = what("dropped after the enqueue", m, leases);
        stage_pools_free(B.ctx); B.fresh(m);
        Shot s = B.shot(m, leases); s.early = AFTER_ENQUEUE;
        CHECK(fill(B.ctx, s) == VFSMS_ERR_CAPACITY && B.tiles_are(m, 2, false));
        const long sync = at(stub_name("sync", B.stream()));
        CHECK(sync >= 0 && g_hip.log[sync + 1] == pools(0, 0) && sync + 2 == (long)g_hip.log.size() && count("record(") == 0);
        CHECK(B.ctx->pin_pool.size() == 1 && (int)B.ctx->stage_pool.size() == leases && pools_hold_all_live(B.ctx));
    }
    return 0;
}
// row 8: success: the tiles' event recorded on the copy stream and waited for, THEN the leases back; a second fill reuses them all
static int row8(const Bed &B)
{
    for (const Bed::Mode &m : B.modes()) for (int leases : {0, 1, 4}) for (int pass = 0; pass < 2; pass++) {
        g_what = what("row 8", m, leases, pass ? "warm" : "cold");
        if (!pass) stage_pools_free(B.ctx);
        B.fresh(m);
        CHECK(fill(B.ctx, B.shot(m, leases)) == VFSMS_OK && B.tiles_are(m, 0, false) && B.pixels_ok(m));
        const hipEvent_t ev = B.rec(m.a ? m.a : m.b).ready;
        const long rec = at(stub_name("record", ev)), wait = at(stub_name("wait", ev));
        CHECK(rec >= 0 && wait == rec + 1 && g_hip.log[wait + 1] == pools(0, 0) && wait + 2 == (long)g_hip.log.size());
        CHECK(count("sync(") == 0 && count("free(") == 0 && count("malloc(") == (pass ? 0 : 1 + leases));      // warm: no malloc line
        CHECK(B.ctx->pin_pool.size() == 1 && (int)B.ctx->stage_pool.size() == leases && pools_hold_all_live(B.ctx));
    }
    return 0;
}
// the cap: 65 fills open at once return 65 pinned and 65 device buffers: 64 of each are pooled, one of each is freed
static int cap_check(vfsms_ctx *ctx)
{
    g_what = "the cap";
    stage_pools_free(ctx);
    Tiles T{ctx, {}};
    std::vector<std::unique_ptr<TileFill>> open;
    for (int k = 0; k < 65; k++) {
        open.emplace_back(new TileFill(ctx));
        CHECK(open.back()->begin_one(T.add(2, 3, 1), "cap", false) == VFSMS_OK && open.back()->host(6) && open.back()->device(6));
    }
    g_hip.log.clear();
    CHECK(g_hip.live == 130 && ctx->pin_pool.empty() && ctx->stage_pool.empty());
    for (auto &f : open) CHECK(f->refuse(VFSMS_ERR_UNSUPPORTED) == VFSMS_ERR_UNSUPPORTED);
    CHECK(ctx->pin_pool.size() == 64 && ctx->stage_pool.size() == 64 && count("free(") == 2 && g_hip.log.size() == 2 && pools_hold_all_live(ctx));
    open.clear();                                                // (the destructors of ended fills do nothing)
    CHECK(g_hip.log.size() == 2 && g_hip.live == 128);
    for (auto &kv : ctx->tiles) CHECK(kv.second.fill == 1);
    return 0;
}

static int run()
{
    vfsms_ctx ctx;
    ctx.copy_stream = (hipStream_t)0x3000;
    g_ctx = &ctx; g_hip.probe = probe_pools;
    int bad = 0;
    {
        Tiles T{&ctx, {}};
        Bed B{&ctx, &T, 0, 0, 0, 5, 7, {}, {}};
        B.one = T.add(B.h, B.w, 3); B.gray = T.add(B.h, B.w, 1); B.color = T.add(B.h, B.w, 3);
        for (int i = 0; i < B.h * B.w * 3; i++) B.src3.push_back((uint8_t)(i * 37 + 11));
        for (int i = 0; i < B.h * B.w; i++) B.src1.push_back((uint8_t)(i * 29 + 3));
        bad = row1(B) || row2_row3(B) || row4(B) || row5(B) || row6(B) || row7(B) || row8(B);
    }
    if (!bad) bad = cap_check(&ctx);
    stage_pools_free(&ctx);
    g_hip.probe = nullptr; g_ctx = nullptr;
    return bad;
}

int main()
{
    if (run()) return 1;
    if (g_hip.live != 0 || g_hip.events != 0) { fprintf(stderr, "%ld allocations and %ld events still live\n", g_hip.live, g_hip.events); return 1; }
    printf("ingest_fill_host_check: %d checks ok, %d table rows x %d injection positions\n", g_checks, N_ROWS, N_POSITIONS);
    return 0;
}
