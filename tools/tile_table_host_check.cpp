// tile_table_host_check.cpp -- csrc/tile_table.h, the rules of the context's tile table, as the plain host C++ it is, for a sanitizer build
// that links neither the HIP runtime nor libvfsms: the runtime calls are tools/hip_host_stubs.h's, over malloc / free.
//   c++ -std=c++17 -g -pthread -fsanitize=address,undefined -fno-sanitize-recover=all -static-libasan -static-libubsan -D__HIP_PLATFORM_AMD__ \
//       -I/opt/rocm/include -I imagestitch_amd/csrc tools/tile_table_host_check.cpp -o /tmp/tthc && /tmp/tthc
// (the sanitizer runtimes are linked into the program, so it runs as it is, with nothing preloaded; tests/test_tile_table_host.py does this)
// What a GPU test cannot see is WHEN a refusal comes: whether a call that is refused has already blocked on a decoder thread or made the
// compute stream wait.  sweep() sends every list of 0 .. MAX_LEN of the KINDS below through tile_list under every rule and compares with
// model(), the order of checks written a second time over the KINDS table alone (no TileRec, no map, no sort); the stubs' log says what
// was enqueued.  pool() drives tile_rec, tile_register, tile_find and tile_pool_return with failures injected; at exit nothing is live, and
// LeakSanitizer agrees or fails the run.
#include "hip_host_stubs.h"
#include "tile_table.h"
#include <stdarg.h>
#include <chrono>
#include <thread>

static char g_err[512] = "";
void vfsms_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int g_checks = 0;
static std::string g_what;                                      // the case at work, for a failing CHECK
#define CHECK(c) do { g_checks++; if (!(c)) { fprintf(stderr, "%s:%d: %s\n  (%s; error \"%s\")\n", __FILE__, __LINE__, #c, g_what.c_str(), g_err); for (auto &l : g_hip.log) fprintf(stderr, "  log: %s\n", l.c_str()); return 1; } } while (0)
static long count(const char *prefix) { long n = 0; for (auto &l : g_hip.log) n += l.compare(0, strlen(prefix), prefix) == 0; return n; }
static std::string fmt(const char *f, ...) { char b[256]; va_list ap; va_start(ap, f); vsnprintf(b, sizeof(b), f, ap); va_end(ap); return b; }

// ---- the sweep ------------------------------------------------------------------------------------------------------------------------------
struct Kind { const char *name; int h, w, ch; bool owned, pending; int fill; bool known; };
static const Kind KINDS[] = {
    {"owned a", 16, 24, 1, true, false, 0, true}, {"owned b", 16, 24, 1, true, false, 0, true}, {"owned wider", 16, 25, 1, true, false, 0, true},
    {"owned B G R", 16, 24, 3, true, false, 0, true}, {"owned 4-channel", 16, 24, 4, true, false, 0, true}, {"wrapped", 16, 24, 1, false, false, 0, true},
    {"pending", 16, 24, 1, true, true, 0, true}, {"given up", 16, 24, 1, true, false, 2, true}, {"unknown", 0, 0, 0, false, false, 0, false} };
static const int N_KINDS = (int)(sizeof(KINDS) / sizeof(KINDS[0])), MAX_LEN = 4, PENDING = 6;
struct Range { int lo, hi; bool got; const char *noun; };
static const Range RANGES[] = { {1, 4096, false, "tile"}, {2, 3, true, "plane"} };
static const int N_FLAGS = 4;                                    // gray or B G R, one shape, rewritten, a predicate (refuses B G R tiles)
static bool pred_refuses(int ch) { return ch == 3; }

// the order of tile_table.h, over KINDS: the code, a piece of the message that names the offender, and the kinds whose event is waited for
struct Verdict { int rc; std::string say; std::vector<int> waits; };
static Verdict model(const Range &R, int flags, const int *L, int n)
{
    const bool gray_or_bgr = flags & 1, same_shape = flags & 2, rewritten = flags & 4, pred = flags & 8;
    if (n < R.lo || n > R.hi) return {VFSMS_ERR_BAD_ARG, R.got ? fmt("check: %d..%d tiles, got %d", R.lo, R.hi, n) : fmt("check: %d..%d tiles", R.lo, R.hi), {}};
    for (int i = 0; i < n; i++) if (!KINDS[L[i]].known) return {VFSMS_ERR_BAD_ARG, "check: unknown tile handle", {}};
    for (int i = 0; i < n; i++) {
        const Kind &k = KINDS[L[i]], &k0 = KINDS[L[0]];
        if (gray_or_bgr && k.ch != 1 && k.ch != 3) return {VFSMS_ERR_BAD_ARG, fmt("check: tile %d has %d channels (1 or 3)", i, k.ch), {}};
        if (same_shape && (k.h != k0.h || k.w != k0.w || k.ch != k0.ch))
            return {VFSMS_ERR_BAD_ARG, fmt("check: %s %d is %d x %d x %d, %s 0 is %d x %d x %d", R.noun, i, k.h, k.w, k.ch, R.noun, k0.h, k0.w, k0.ch), {}};
        if (rewritten && !k.owned) return {VFSMS_ERR_BAD_ARG, fmt("check: tile %d comes from vfsms_tile_wrap", i), {}};
        if (pred && pred_refuses(k.ch)) return {VFSMS_ERR_BAD_ARG, fmt("the predicate refuses tile %d", i), {}};
    }
    for (int i = 0; rewritten && i < n; i++) for (int j = 0; j < i; j++) if (L[i] == L[j]) return {VFSMS_ERR_BAD_ARG, "check: a tile is named twice", {}};
    Verdict v{VFSMS_OK, "", {}};
    bool waited = false;
    for (int i = 0; i < n; i++) {
        if (KINDS[L[i]].fill == 2) { v.rc = VFSMS_ERR_BAD_ARG; v.say = "a reserved tile was never filled"; return v; }
        if (KINDS[L[i]].pending && !waited) { v.waits.push_back(L[i]); waited = true; }
    }
    return v;
}

struct Bed {
    vfsms_ctx *ctx; int64_t hd[sizeof(KINDS) / sizeof(KINDS[0])]; uint8_t wrapped[16 * 24];
    TileRec &rec(int k) { return ctx->tiles.at(hd[k]); }
    int make()
    {
        for (int k = 0; k < N_KINDS; k++) {
            const Kind &K = KINDS[k];
            if (!K.known) { hd[k] = 999999; continue; }
            uint8_t *p = wrapped;
            if (K.owned && hipMalloc((void **)&p, (size_t)K.h * K.w * K.ch) != hipSuccess) return 1;
            TileRec t = tile_rec(p, K.h, K.w, K.ch, K.w * K.ch, K.owned);
            t.fill = K.fill; t.pending = K.pending;
            if (K.pending && hipEventCreateWithFlags(&t.ready, hipEventDisableTiming) != hipSuccess) return 1;
            tile_register(ctx, t, &hd[k]);
        }
        return 0;
    }
    void drop()
    {
        for (auto &kv : ctx->tiles) { if (kv.second.owned) (void)hipFree(kv.second.ptr); if (kv.second.ready) (void)hipEventDestroy(kv.second.ready); }
        ctx->tiles.clear();
    }
};

static long g_lists = 0;
static int sweep_one(Bed &B, const Range &R, int flags, const int *L, int n)
{
    TileRule rule{R.lo, R.hi, R.got, R.noun, (flags & 1) != 0, (flags & 2) != 0, (flags & 4) != 0, nullptr};
    if (flags & 8) rule.pred = [](int i, const TileRec &t) { if (!pred_refuses(t.ch)) return VFSMS_OK; vfsms_set_error("the predicate refuses tile %d", i); return VFSMS_ERR_BAD_ARG; };
    int64_t handles[MAX_LEN + 1] = {0};
    for (int i = 0; i < n; i++) handles[i] = B.hd[L[i]];
    g_what = fmt("%d..%d, flags %d, list of %d: %d %d %d %d", R.lo, R.hi, flags, n, L[0], L[1], L[2], L[3]);
    B.rec(PENDING).pending = true; g_hip.log.clear(); g_err[0] = 0;
    const Verdict want = model(R, flags, L, n);
    std::vector<TileView> V;
    const int rc = tile_list(B.ctx, "check", rule, handles, n, V);
    CHECK(rc == want.rc);
    CHECK(rc == VFSMS_OK ? !g_err[0] : strstr(g_err, want.say.c_str()) != nullptr);
    // a refusal has enqueued nothing and handed nothing over; what a given-up tile stops is the hand-over itself, behind every check
    CHECK(g_hip.log.size() == want.waits.size() && B.rec(PENDING).pending == want.waits.empty());
    for (size_t k = 0; k < want.waits.size(); k++) CHECK(g_hip.log[k] == stub_name("stream_wait", B.rec(want.waits[k]).ready));
    if (rc == VFSMS_OK) {
        CHECK((int)V.size() == n);
        for (int i = 0; i < n; i++) {
            const TileRec &t = B.rec(L[i]);
            CHECK(V[i].ptr == t.ptr && V[i].stride == t.stride && V[i].h == t.h && V[i].w == t.w && V[i].ch == t.ch);
        }
    }
    return 0;
}
static int sweep(Bed &B)
{
    for (int n = 0; n <= MAX_LEN; n++) {
        int total = 1;
        for (int i = 0; i < n; i++) total *= N_KINDS;
        for (int code = 0; code < total; code++) {
            int L[MAX_LEN] = {0, 0, 0, 0};
            for (int i = 0, c = code; i < n; i++, c /= N_KINDS) L[i] = c % N_KINDS;
            g_lists++;
            for (const Range &R : RANGES) for (int flags = 0; flags < (1 << N_FLAGS); flags++) if (sweep_one(B, R, flags, L, n)) return 1;
        }
    }
    // the null pointer is refused as a count is
    std::vector<TileView> V;
    g_what = "null list"; g_hip.log.clear();
    CHECK(tile_list(B.ctx, "check", TileRule{1, 4096, false, "tile", false, false, false, nullptr}, nullptr, 2, V) == VFSMS_ERR_BAD_ARG && !strcmp(g_err, "check: 1..4096 tiles") && g_hip.log.empty());
    return 0;
}
// a reserved tile whose decoder thread hands it over while tile_list waits: the list comes back handed over, the copy's event waited for
static int handed_over_meanwhile(Bed &B)
{
    g_what = "a decoder thread fills a reserved tile";
    TileRec &t = B.rec(PENDING);
    t.pending = true; g_hip.log.clear(); g_err[0] = 0;
    { std::lock_guard<std::mutex> lk(B.ctx->tiles_mu); t.fill = 1; }
    std::thread decoder([&] {
        std::this_thread::sleep_for(std::chrono::milliseconds(20));      // (tile_list is most likely waiting by now; either order must work)
        std::lock_guard<std::mutex> lk(B.ctx->tiles_mu);
        t.fill = 0;
        B.ctx->tiles_cv.notify_all();
    });
    const int64_t handles[2] = {B.hd[0], B.hd[PENDING]};
    std::vector<TileView> V;
    const int rc = tile_list(B.ctx, "check", TileRule{1, 4096, false, "tile", true, true, true, nullptr}, handles, 2, V);
    decoder.join();
    CHECK(rc == VFSMS_OK && t.fill == 0 && !t.pending && V.size() == 2 && V[1].ptr == t.ptr);
    CHECK(g_hip.log.size() == 1 && g_hip.log[0] == stub_name("stream_wait", t.ready));
    // a refusal leaves a reserved tile alone and does not wait for it
    t.pending = true; t.fill = 1; g_hip.log.clear();
    const int64_t twice[3] = {B.hd[PENDING], B.hd[0], B.hd[0]};
    CHECK(tile_list(B.ctx, "check", TileRule{1, 4096, false, "tile", true, true, true, nullptr}, twice, 3, V) == VFSMS_ERR_BAD_ARG && strstr(g_err, "named twice"));
    CHECK(g_hip.log.empty() && t.fill == 1 && t.pending);
    t.fill = 0;
    return 0;
}

// ---- records, registration, lookup, the pool --------------------------------------------------------------------------------------------------
// every pooled buffer is one live allocation, no pointer twice, and the pool's byte count is the sum of its entries
static bool pool_holds_all_live(vfsms_ctx *ctx, long others = 0)
{
    std::vector<uint8_t *> p; size_t bytes = 0;
    for (auto &e : ctx->tile_pool) { p.push_back(e.ptr); bytes += e.bytes; }
    std::sort(p.begin(), p.end());
    return std::adjacent_find(p.begin(), p.end()) == p.end() && (long)p.size() + others == g_hip.live && bytes == ctx->tile_pool_bytes;
}
static int pool(vfsms_ctx *ctx)
{
    g_what = "records";
    const TileRec blank;
    CHECK(!blank.ptr && !blank.h && !blank.w && !blank.stride && !blank.owned && !blank.ready && !blank.pending && blank.ch == 1 && !blank.bytes && !blank.fill);
    uint8_t mem[8];
    const TileRec w = tile_rec(mem, 5, 7, 3, 32, false), o = tile_rec(mem, 5, 7, 3, 21, true);
    CHECK(w.ptr == mem && w.h == 5 && w.w == 7 && w.ch == 3 && w.stride == 32 && !w.owned && w.bytes == 0 && !w.ready && !w.pending && !w.fill);
    CHECK(o.owned && o.bytes == 105 && o.stride == 21);

    g_what = "register and find";
    int64_t ha = 0, hb = 0;
    const int64_t next = ctx->next_handle;
    tile_register(ctx, w, &ha); tile_register(ctx, o, &hb);
    CHECK(ha == next && hb == next + 1 && ctx->next_handle == next + 2 && ctx->tiles.size() == 2);
    TileRec *t = nullptr;
    CHECK(tile_find(ctx, "who", hb, &t) == VFSMS_OK && t == &ctx->tiles.at(hb) && t->bytes == 105);
    g_err[0] = 0; t = nullptr;
    CHECK(tile_find(ctx, "who", next + 2, &t) == VFSMS_ERR_BAD_ARG && !t && !strcmp(g_err, "who: unknown tile handle"));
    ctx->tiles.clear();

    // what vfsms_tile_free and the error paths of tile_reserve / focus_stack do with a buffer
    g_what = "pool return";
    uint8_t *b[4];
    for (auto &p : b) CHECK(hipMalloc((void **)&p, 64) == hipSuccess);
    g_hip.log.clear();
    CHECK(tile_pool_return(ctx, b[0], 64, false) == VFSMS_OK && g_hip.log.empty() && ctx->tile_pool.size() == 1 && !ctx->tile_pool[0].idle);
    CHECK(tile_pool_return(ctx, b[1], 64, true) == VFSMS_OK && g_hip.log.size() == 2 && count("event_create(") == 1);
    CHECK(ctx->tile_pool.size() == 2 && ctx->tile_pool[1].idle && g_hip.log[1] == stub_name("record", ctx->tile_pool[1].idle) && pool_holds_all_live(ctx, 2));
    g_hip.log.clear();
    fail_call("event_create", 1);                                // no event to be had: the buffer stays the caller's, the pool as it was
    CHECK(tile_pool_return(ctx, b[2], 64, true) == VFSMS_ERR_HIP && !g_hip.fail_kind && ctx->tile_pool.size() == 2 && ctx->tile_pool_bytes == 128 && pool_holds_all_live(ctx, 2));
    CHECK(count("record(") == 0 && count("free(") == 0);
    hipEvent_t spare;
    CHECK(hipEventCreateWithFlags(&spare, hipEventDisableTiming) == hipSuccess);
    ctx->event_pool.push_back(spare); g_hip.log.clear();
    CHECK(tile_pool_return(ctx, b[2], 64, true) == VFSMS_OK && ctx->event_pool.empty() && ctx->tile_pool[2].idle == spare);      // (an event of the pool first)
    CHECK(g_hip.log.size() == 1 && g_hip.log[0] == stub_name("record", spare) && pool_holds_all_live(ctx, 1));
    // the caps: a buffer that would take the pool over 8 GB, then one behind 256 entries, is freed behind a synchronisation
    g_what = "pool caps"; g_hip.log.clear();
    CHECK(tile_pool_return(ctx, b[3], ((size_t)8 << 30) - 191, true) == VFSMS_OK && ctx->tile_pool.size() == 3 && ctx->tile_pool_bytes == 192);
    CHECK(g_hip.log.size() == 2 && g_hip.log[0] == stub_name("sync", ctx->stream) && g_hip.log[1] == stub_name("free", b[3]) && pool_holds_all_live(ctx));
    while (ctx->tile_pool.size() < 256) {
        uint8_t *p;
        CHECK(hipMalloc((void **)&p, 16) == hipSuccess && tile_pool_return(ctx, p, 16, false) == VFSMS_OK);
    }
    uint8_t *over;
    CHECK(hipMalloc((void **)&over, 16) == hipSuccess);
    g_hip.log.clear();
    CHECK(tile_pool_return(ctx, over, 16, false) == VFSMS_OK && ctx->tile_pool.size() == 256 && ctx->tile_pool_bytes == 192 + 253 * 16);
    CHECK(g_hip.log.size() == 2 && g_hip.log[0] == stub_name("sync", ctx->stream) && g_hip.log[1] == stub_name("free", over) && pool_holds_all_live(ctx));
    for (auto &e : ctx->tile_pool) { (void)hipFree(e.ptr); if (e.idle) (void)hipEventDestroy(e.idle); }      // (tile_pools_free, api.hip)
    ctx->tile_pool.clear(); ctx->tile_pool_bytes = 0;
    return 0;
}

static int run()
{
    vfsms_ctx ctx;
    ctx.stream = (hipStream_t)0x1000; ctx.copy_stream = (hipStream_t)0x3000;
    if (pool(&ctx)) return 1;
    Bed B{&ctx, {}, {}};
    int bad = B.make();
    if (!bad) bad = sweep(B) || handed_over_meanwhile(B);
    B.drop();
    return bad;
}

int main()
{
    if (run()) return 1;
    if (g_hip.live != 0 || g_hip.events != 0) { fprintf(stderr, "%ld allocations and %ld events still live\n", g_hip.live, g_hip.events); return 1; }
    printf("tile_table_host_check: %d checks ok, %ld lists of up to %d of %d tiles x %d ranges x %d flags\n", g_checks, g_lists, MAX_LEN, N_KINDS,
           (int)(sizeof(RANGES) / sizeof(RANGES[0])), N_FLAGS);
    return 0;
}
