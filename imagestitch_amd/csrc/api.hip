// api.hip -- context management and the extern "C" entry points declared in include/vfsms.h.
#include "common.h"
#include "canvas_band.h"
#include "ingest_fill.h"
#include "tile_table.h"
#include "deep_bins.h"
#include "jpeg_huff_core.h"
#include "phase_resolve_math.h"
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <tuple>

int fuse_i64_device(vfsms_ctx *ctx, const long long *dA, const long long *dB, int r, int c, int ch, int dx, int dy,
                    uint8_t *d_out, int32_t *info, int method = 0, int levels = 4, int seam_blend = 0, int32_t *d_seam = nullptr);

// ---- errors -------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void vfsms_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" int vfsms_last_error(char *buf, int buflen)
{
    if (!buf || buflen <= 0) return VFSMS_ERR_BAD_ARG;
    snprintf(buf, (size_t)buflen, "%s", g_err);
    return VFSMS_OK;
}
extern "C" int vfsms_version(void) { return 100; }
extern "C" int vfsms_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// ---- arena ----------------------------------------------------------------------------------------------
int ctx_arena_reserve(vfsms_ctx *ctx, size_t bytes)
{
    bytes += 1 << 20;
    TRY(ctx->arena.reserve(bytes, ctx->stream, bytes / 4));
    ctx->arena_off = 0;
    return VFSMS_OK;
}
void *ctx_arena_alloc(vfsms_ctx *ctx, size_t bytes, size_t align)
{
    size_t off = (ctx->arena_off + align - 1) & ~(align - 1);
    if (off + bytes > ctx->arena.bytes()) return nullptr;
    ctx->arena_off = off + bytes;
    return ctx->arena.as<char>() + off;
}
// a record's layout function carves from a walk that starts where the arena stands (arena_walk.h) ...
ArenaWalk ctx_arena_walk(vfsms_ctx *ctx) { return ArenaWalk{ctx->arena.as<char>(), ctx->arena_off, ctx->arena.bytes()}; }
// ... and the arena moves on only when every take of the walk fitted; `what`: the error string of a walk that did not
int ctx_arena_commit(vfsms_ctx *ctx, const ArenaWalk &a, const char *what)
{
    if (!a.ok) { vfsms_set_error("%s", what); return VFSMS_ERR_CAPACITY; }
    ctx->arena_off = a.off;
    return VFSMS_OK;
}

// ---- per-stage profiling with HIP events on the context stream --------------------------------------------
int prof_begin(vfsms_ctx *ctx, const char *name)
{
    if (!ctx->prof_on) return -1;
    int id = -1;
    // stages enqueued on the second compute stream are booked under their own name ("bf_mfma@s2"): they run beside the first stream's stages,
    // so the per-stage times of a step no longer add up to its wall clock -- the reader sees which ones overlapped
    std::string key(name);
    if (ctx->stream2 && ctx->stream == ctx->stream2) key += "@s2";
    for (size_t k = 0; k < ctx->prof_names.size(); k++) if (ctx->prof_names[k] == key) { id = (int)k; break; }
    if (id < 0) { id = (int)ctx->prof_names.size(); ctx->prof_names.push_back(key); ctx->prof_ms.push_back(0.0); ctx->prof_calls.push_back(0); }
    ProfRec r; r.id = id;
    for (hipEvent_t *e : {&r.a, &r.b}) {
        if (!ctx->prof_pool.empty()) { *e = ctx->prof_pool.back(); ctx->prof_pool.pop_back(); }
        else if (hipEventCreate(e) != hipSuccess) return -1;
    }
    if (hipEventRecord(r.a, ctx->stream) != hipSuccess) return -1;
    ctx->prof_recs.push_back(r);
    return (int)ctx->prof_recs.size() - 1;
}
void prof_end(vfsms_ctx *ctx, int rec)
{
    if (rec < 0 || rec >= (int)ctx->prof_recs.size()) return;
    (void)hipEventRecord(ctx->prof_recs[rec].b, ctx->stream);
}
static int prof_collect(vfsms_ctx *ctx)
{
    if (ctx->prof_recs.empty()) return VFSMS_OK;
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (auto &r : ctx->prof_recs) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, r.a, r.b) == hipSuccess) { ctx->prof_ms[r.id] += ms; ctx->prof_calls[r.id] += 1; }
        ctx->prof_pool.push_back(r.a); ctx->prof_pool.push_back(r.b);
    }
    ctx->prof_recs.clear();
    return VFSMS_OK;
}
extern "C" int vfsms_profile_enable(vfsms_ctx *ctx, int on)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    TRY(prof_collect(ctx));
    ctx->prof_on = on != 0;
    return VFSMS_OK;
}
extern "C" int vfsms_profile_read(vfsms_ctx *ctx, char *names, int names_len, double *ms, int64_t *calls, int cap, int *n_out, int reset)
{
    if (!ctx || !n_out) return VFSMS_ERR_BAD_ARG;
    HIP_TRY(hipSetDevice(ctx->device));
    TRY(prof_collect(ctx));
    const int n = (int)ctx->prof_names.size();
    *n_out = n;
    std::string joined;
    for (int k = 0; k < n; k++) {
        if (k) joined += ",";
        joined += ctx->prof_names[k];
        if (k < cap) { if (ms) ms[k] = ctx->prof_ms[k]; if (calls) calls[k] = ctx->prof_calls[k]; }
    }
    if (names && names_len > 0) snprintf(names, (size_t)names_len, "%s", joined.c_str());
    if (reset) for (int k = 0; k < n; k++) { ctx->prof_ms[k] = 0; ctx->prof_calls[k] = 0; }
    return VFSMS_OK;
}

// ---- SURF tables (resizeHaarPattern for every layer; SURFInvoker constructor tables) -------------------
static void gaussian_kernel_f32(int n, double sigma, float *cf)   // cv::getGaussianKernel(n, sigma, CV_32F)
{
    const double scale2X = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) {
        const double x = i - (n - 1) * 0.5;
        cf[i] = (float)exp(scale2X * x * x);
        sum += cf[i];
    }
    sum = 1. / sum;
    for (int i = 0; i < n; i++) cf[i] = (float)(cf[i] * sum);
}

int ctx_prepare_surf(vfsms_ctx *ctx, const vfsms_surf_params *p)
{
    if (!p || p->n_octaves < 1 || p->n_octave_layers < 1 || (p->n_octave_layers + 2) * p->n_octaves > VFSMS_MAX_LAYERS ||
        p->hessian_threshold < 0 || p->n_octaves > 8) {
        vfsms_set_error("bad SURF parameters");
        return VFSMS_ERR_BAD_ARG;
    }
    // largest keypoint size = largest middle-layer size + its scale step -> descriptor window side
    {
        const int lpo = p->n_octave_layers + 2;
        const int top = (9 + 6 * (lpo - 1)) << (p->n_octaves - 1);
        const float s = (float)top * 1.2f / 9.0f;
        if ((int)(21 * s) > VFSMS_MAX_WIN) {
            vfsms_set_error("SURF parameters give descriptor windows > %d px (unsupported)", VFSMS_MAX_WIN);
            return VFSMS_ERR_UNSUPPORTED;
        }
    }
    if (ctx->tables_valid && memcmp(&ctx->cur_params, p, sizeof(*p)) == 0) return VFSMS_OK;
    static const int dx_s[3][5] = { {0, 2, 3, 7, 1}, {3, 2, 6, 7, -2}, {6, 2, 9, 7, 1} };
    static const int dy_s[3][5] = { {2, 0, 7, 3, 1}, {2, 3, 7, 6, -2}, {2, 6, 7, 9, 1} };
    static const int dxy_s[4][5] = { {1, 1, 4, 4, 1}, {5, 1, 8, 4, -1}, {1, 5, 4, 8, -1}, {5, 5, 8, 8, 1} };
    const int lpo = p->n_octave_layers + 2;
    const int nl = lpo * p->n_octaves;
    std::vector<LayerPat> L(nl);
    int step = 1, idx = 0;
    for (int o = 0; o < p->n_octaves; o++) {
        for (int l = 0; l < lpo; l++, idx++) {
            LayerPat &P = L[idx];
            P.size = (9 + 6 * l) << o; P.step = step; P.margin = (P.size / 2) / step; P.octave = o;
            const float ratio = (float)P.size / 9;
            for (int k = 0; k < 10; k++) {
                const int *src = k < 3 ? dx_s[k] : k < 6 ? dy_s[k - 3] : dxy_s[k - 6];
                const int x1 = (int)lrintf(ratio * src[0]), y1 = (int)lrintf(ratio * src[1]);
                const int x2 = (int)lrintf(ratio * src[2]), y2 = (int)lrintf(ratio * src[3]);
                P.box[k][0] = x1; P.box[k][1] = y1; P.box[k][2] = x2; P.box[k][3] = y2;
                for (int c = 0; c < 4; c++)
                    if (P.box[k][c] != vfsms_haar_corner(P.size, k, c)) {       // the LDS Hessian kernels bake these in
                        vfsms_set_error("internal: Haar pattern corner mismatch (size %d box %d)", P.size, k);
                        return VFSMS_ERR_UNSUPPORTED;
                    }
                P.w[k] = src[4] / ((float)(x2 - x1) * (y2 - y1));
            }
        }
        step *= 2;
    }
    SurfTables T;
    memset(&T, 0, sizeof(T));
    float G_ori[13], G_desc[20];
    gaussian_kernel_f32(13, 2.5f, G_ori);
    for (int i = -6; i <= 6; i++)
        for (int j = -6; j <= 6; j++)
            if (i * i + j * j <= 36) {
                T.aptx[T.nOriSamples] = i; T.apty[T.nOriSamples] = j;
                T.aptw[T.nOriSamples++] = G_ori[i + 6] * G_ori[j + 6];
            }
    for (int ang = 0; ang <= 360; ang++)
        for (int w = 0; w < 72; w++) {
            const int d = abs(ang - 5 * w);
            if (d < 30 || d > 330) T.oriMask[ang][w >> 5] |= 1u << (w & 31);
        }
    gaussian_kernel_f32(20, 3.3f, G_desc);
    for (int i = 0; i < 20; i++)
        for (int j = 0; j < 20; j++) T.DW[i * 20 + j] = G_desc[i] * G_desc[j];
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    TRY(ctx->d_layers.reserve(sizeof(LayerPat) * VFSMS_MAX_LAYERS, ctx->stream));
    TRY(ctx->d_tables.reserve(sizeof(SurfTables), ctx->stream));
    HIP_TRY(hipMemcpy(ctx->d_layers.as<void>(), L.data(), sizeof(LayerPat) * nl, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ctx->d_tables.as<void>(), &T, sizeof(T), hipMemcpyHostToDevice));
    ctx->n_layers = nl;
    ctx->cur_params = *p;
    ctx->tables_valid = true;
    return VFSMS_OK;
}

// ---- context ---------------------------------------------------------------------------------------------
extern "C" int vfsms_ctx_create(int device, vfsms_ctx **out)
{
    if (!out) return VFSMS_ERR_BAD_ARG;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { vfsms_set_error("no HIP device visible"); return VFSMS_ERR_NO_DEVICE; }
    if (device < 0 || device >= n) { vfsms_set_error("device %d out of range (%d visible)", device, n); return VFSMS_ERR_BAD_ARG; }
    HIP_TRY(hipSetDevice(device));
    vfsms_ctx *c = new vfsms_ctx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking);
    if (e != hipSuccess) { vfsms_set_error("hipStreamCreate: %s", hipGetErrorString(e)); delete c; return VFSMS_ERR_HIP; }
    *out = c;
    return VFSMS_OK;
}

// the pools whose entries stayed raw pointers (they move between a record and a pool, and carry events): each is freed here and nowhere else
// (the staging pools of the ingest: stage_pools_free, ingest_fill.h)
static void tile_pools_free(vfsms_ctx *ctx)
{
    for (auto &kv : ctx->tiles) { if (kv.second.owned) hipFree(kv.second.ptr); if (kv.second.ready) hipEventDestroy(kv.second.ready); }
    for (auto &pe : ctx->tile_pool) { hipFree(pe.ptr); if (pe.idle) hipEventDestroy(pe.idle); }
    ctx->tiles.clear(); ctx->tile_pool.clear(); ctx->tile_pool_bytes = 0;
}
// Only what has an order is written out: nothing may run when memory goes, the plans and the profile want live streams, and the members
// (device_buf.h) free themselves behind all of it
extern "C" int vfsms_ctx_destroy(vfsms_ctx *ctx)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    hipStreamSynchronize(ctx->copy_stream);
    if (ctx->stream2) hipStreamSynchronize(ctx->stream2);
    phase_destroy_plans(ctx);
    prof_collect(ctx);
    for (hipEvent_t e : ctx->prof_pool) hipEventDestroy(e);
    tile_pools_free(ctx);
    stage_pools_free(ctx);
    for (hipEvent_t ev : ctx->event_pool) hipEventDestroy(ev);
    if (ctx->ev_fork) hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) hipEventDestroy(ctx->ev_join);
    hipStreamDestroy(ctx->copy_stream);
    if (ctx->stream2) hipStreamDestroy(ctx->stream2);
    hipStreamDestroy(ctx->stream);
    delete ctx;
    return VFSMS_OK;
}
extern "C" int vfsms_ctx_sync(vfsms_ctx *ctx)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_ctx_sync_uploads(vfsms_ctx *ctx)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    return VFSMS_OK;
}
extern "C" void *vfsms_ctx_stream(vfsms_ctx *ctx) { return ctx ? (void *)ctx->stream : nullptr; }
extern "C" int vfsms_ctx_set_keypoint_capacity(vfsms_ctx *ctx, int cap)
{
    if (!ctx || cap < 0) return VFSMS_ERR_BAD_ARG;
    ctx->kp_cap_override = cap;
    return VFSMS_OK;
}
extern "C" int vfsms_ctx_set_offset_estimator(vfsms_ctx *ctx, int estimator, int tol_px)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    if ((estimator != VFSMS_OFFSET_MODE && estimator != VFSMS_OFFSET_CONSENSUS) || tol_px < 0 || tol_px > VFSMS_CONSENSUS_MAX_TOL) {
        vfsms_set_error("set_offset_estimator: estimator %d / tolerance %d (0 mode or 1 consensus; 0..%d px)", estimator, tol_px, VFSMS_CONSENSUS_MAX_TOL);
        return VFSMS_ERR_BAD_ARG;
    }
    ctx->offset_estimator = estimator; ctx->offset_tol = tol_px;
    return VFSMS_OK;
}
extern "C" int vfsms_ctx_set_offset_verifier(vfsms_ctx *ctx, int verifier, double threshold, int min_pixels)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    if ((verifier != VFSMS_VERIFY_NONE && verifier != VFSMS_VERIFY_NCC) || !(threshold >= -1.0 && threshold <= 1.0) || min_pixels < 0) {
        vfsms_set_error("set_offset_verifier: verifier %d / threshold %g / min_pixels %d (0 none or 1 ncc; -1..1; >= 0)", verifier, threshold, min_pixels);
        return VFSMS_ERR_BAD_ARG;
    }
    ctx->offset_verifier = verifier; ctx->verify_threshold = threshold; ctx->verify_min_pixels = min_pixels;
    return VFSMS_OK;
}
extern "C" int vfsms_ctx_set_phase_resolver(vfsms_ctx *ctx, int resolver, int peaks, double threshold, int min_pixels)
{
    if (!ctx) return VFSMS_ERR_BAD_ARG;
    if (!phase_resolver_ok(resolver) || !phase_resolve_params_ok(peaks, threshold, min_pixels)) {
        vfsms_set_error("set_phase_resolver: resolver %d / peaks %d / threshold %g / min_pixels %d (0 none or 1 ncc; 1..%d; -1..1; >= 0)", resolver, peaks,
                        threshold, min_pixels, VFSMS_PHASE_MAX_PEAKS);
        return VFSMS_ERR_BAD_ARG;
    }
    ctx->phase_resolver = resolver; ctx->phase_peaks = peaks; ctx->phase_threshold = threshold; ctx->phase_min_pixels = min_pixels;
    return VFSMS_OK;
}
static int kp_capacity(vfsms_ctx *ctx, int h, int w)
{
    if (ctx->kp_cap_override > 0) return ctx->kp_cap_override;
    return (int)((long long)h * w / 24) + 4096;
}
#define CTX_ENTER(ctx)                                                     \
    do {                                                                   \
        if (!(ctx)) { vfsms_set_error("null context"); return VFSMS_ERR_BAD_ARG; } \
        HIP_TRY(hipSetDevice((ctx)->device));                              \
    } while (0)

// ---- tiles -------------------------------------------------------------------------------------------------
// A pooled buffer may still be read by work enqueued on the compute stream when its tile was freed (vfsms_canvas_paste_tile and
// vfsms_canvas_fuse_tile_resident without an info readback only enqueue): the stream that writes the buffer next waits for the event
// recorded at vfsms_tile_free.
static int tile_buffer(vfsms_ctx *ctx, size_t bytes, uint8_t **p, hipStream_t writer)
{
    for (size_t k = 0; k < ctx->tile_pool.size(); k++)
        if (ctx->tile_pool[k].bytes == bytes) {
            PoolEnt e = ctx->tile_pool[k];
            ctx->tile_pool.erase(ctx->tile_pool.begin() + k);
            ctx->tile_pool_bytes -= e.bytes;
            if (e.idle) {
                if (writer != ctx->stream) HIP_TRY(hipStreamWaitEvent(writer, e.idle, 0));   // (same-stream reuse is ordered already)
                ctx->event_pool.push_back(e.idle);
            }
            *p = e.ptr;
            return VFSMS_OK;
        }
    HIP_TRY(hipMalloc((void **)p, bytes));
    return VFSMS_OK;
}
// ch > 1: an interleaved colour tile for the mosaic canvas (rows of w * ch bytes; `stride` in bytes); registration takes ch == 1 only
static int tile_upload_impl(vfsms_ctx *ctx, const uint8_t *img, int h, int w_px, int stride, int64_t *handle, bool async, int ch = 1)
{
    const int w = w_px * ch;                                 // bytes per row
    if (!img || !handle || h <= 0 || w_px <= 0 || ch < 1 || ch > 4 || stride < w) { vfsms_set_error("tile_upload: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TileRec t = tile_rec(nullptr, h, w_px, ch, w, true);
    TRY(tile_buffer(ctx, t.bytes, &t.ptr, async ? ctx->copy_stream : ctx->stream));
    if (async) {
        // the copy runs on the context's copy stream; the compute stream waits for it when a batch first names the tile
        if (!ctx->event_pool.empty()) { t.ready = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
        else HIP_TRY(hipEventCreateWithFlags(&t.ready, hipEventDisableTiming));
        HIP_TRY(hipMemcpy2DAsync(t.ptr, w, img, stride, w, h, hipMemcpyHostToDevice, ctx->copy_stream));
        HIP_TRY(hipEventRecord(t.ready, ctx->copy_stream));
        t.pending = true;
    } else {
        HIP_TRY(hipMemcpy2DAsync(t.ptr, w, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    tile_register(ctx, t, handle);
    return VFSMS_OK;
}
// the two resident tiles a job of `who` names, handed over (tile_ready); what else they must satisfy is the caller's to check
static int resident_pair(vfsms_ctx *ctx, const char *who, int k, const vfsms_ncc_job &j, TileRec **A, TileRec **B)
{
    if (tile_find(ctx, who, j.tile_a, A) != VFSMS_OK || tile_find(ctx, who, j.tile_b, B) != VFSMS_OK) {
        vfsms_set_error("%s: job %d names an unknown tile handle", who, k); return VFSMS_ERR_BAD_ARG;
    }
    TRY(tile_ready(ctx, **A)); TRY(tile_ready(ctx, **B));
    return VFSMS_OK;
}
// non-blocking: has the tile's image been handed over (or was it never a reserved tile)?  An unknown handle counts as ready: the
// evaluator reports it.  (csrc/grid.hip sizes speculative batches by this while decoder threads are still filling tiles.)
int tile_is_filled(vfsms_ctx *ctx, int64_t handle)
{
    std::lock_guard<std::mutex> lk(ctx->tiles_mu);
    auto it = ctx->tiles.find(handle);
    if (it == ctx->tiles.end()) return 1;
    if (it->second.fill == 1) return 0;
    // an asynchronous upload that has not landed yet (vfsms_tile_upload_async: ninety tiles queued on the copy stream in front of a path): the
    // speculative part of a batch takes what is there, like with tiles a decoder still owes -- the first batch does not wait for a whole
    // window of copies
    if (it->second.pending && it->second.ready) {
        const hipError_t e = hipEventQuery(it->second.ready);
        if (e == hipErrorNotReady) return 0;
        if (e != hipSuccess) { (void)hipGetLastError(); return 0; }      // (not left behind as the "last error" of an unrelated launch check)
    }
    return 1;
}
extern "C" int vfsms_tile_upload(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int64_t *handle)
{
    CTX_ENTER(ctx);
    return tile_upload_impl(ctx, img, h, w, stride, handle, false);
}
extern "C" int vfsms_tile_upload_async(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int64_t *handle)
{
    CTX_ENTER(ctx);
    return tile_upload_impl(ctx, img, h, w, stride, handle, true);
}
extern "C" int vfsms_tile_upload_ch(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride_bytes, int async, int64_t *handle)
{
    CTX_ENTER(ctx);
    return tile_upload_impl(ctx, img, h, w, stride_bytes, handle, async != 0, ch);
}
// ---- tiles whose pixels arrive later, from other threads: the ingest pipeline (Stitcher.py:68-69 decodes file after file BEFORE the
// first pair is registered; here the registration of tiles 0, 1, ... starts while tile k is still being decoded) -------------------------
// Every hand-over below is one TileFill (ingest_fill.h): it looks the tiles up, leases the staging and ends the tiles filled, given up or
// still reserved; the entries say what is staged and what is launched.
static int tile_reserve_impl(vfsms_ctx *ctx, int h, int w, int ch, int64_t *handle)
{
    if (!handle || h <= 0 || w <= 0 || ch < 1 || ch > 4) { vfsms_set_error("tile_reserve: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TileRec t = tile_rec(nullptr, h, w, ch, w * ch, true);
    t.fill = 1;
    TRY(tile_buffer(ctx, t.bytes, &t.ptr, ctx->copy_stream));
    if (!ctx->event_pool.empty()) { t.ready = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
    else {
        hipError_t e = hipEventCreateWithFlags(&t.ready, hipEventDisableTiming);
        if (e != hipSuccess) {                               // the buffer goes back to the pool instead of leaking
            (void)tile_pool_return(ctx, t.ptr, t.bytes, false);
            vfsms_set_error("tile_reserve: %s", hipGetErrorString(e)); return VFSMS_ERR_HIP;
        }
    }
    tile_register(ctx, t, handle);
    return VFSMS_OK;
}
extern "C" int vfsms_tile_reserve(vfsms_ctx *ctx, int h, int w, int64_t *handle)
{
    CTX_ENTER(ctx);
    return tile_reserve_impl(ctx, h, w, 1, handle);
}
extern "C" int vfsms_tile_reserve_ch(vfsms_ctx *ctx, int h, int w, int ch, int64_t *handle)
{
    CTX_ENTER(ctx);
    return tile_reserve_impl(ctx, h, w, ch, handle);
}
// May be called from ANY thread, concurrently with batch calls on the context's own thread: copies the pixels on the copy stream and returns
// when the copy has completed, so `img` (a decoder thread's staging buffer) can be reused at once.  img == NULL reports a failed decode:
// the batch call waiting for the tile returns an error instead of waiting forever.  `stride` in bytes; a row is w * ch bytes.
extern "C" int vfsms_tile_fill(vfsms_ctx *ctx, int64_t handle, const uint8_t *img, int stride)
{
    CTX_ENTER(ctx);
    TileFill f(ctx);
    TRY(f.begin_one(handle, "tile_fill", img == nullptr));
    if (!img) return VFSMS_OK;
    const size_t row = (size_t)f.w * f.ch;
    if (stride < f.w * f.ch) { vfsms_set_error("tile_fill: stride smaller than a row of the tile"); return f.refuse(VFSMS_ERR_BAD_ARG); }
    f.copy(f.dg, f.pack(img, stride, row, f.h), row * f.h);
    return f.finish();
}
// One decode, both planes (csrc/ingest_kernels.hip): `src` is what the decoder produced ONCE -- format 0: 8-bit gray, 1: Y Cb Cr interleaved,
// 2: Y Cb Cr X (4 bytes per pixel) -- and fills the reserved gray tile `gray` (the registration plane, cv2.imdecode(..., 0) of Stitcher.py:68-69)
// and / or the reserved 3-channel tile `color` (B G R, cv2.imdecode(..., IMREAD_COLOR) of Stitcher.py:382-403); either handle may be 0.
// The source rows go to a device staging buffer on the copy stream, the split / colour conversion runs there too, and the call returns when
// both tiles are complete.  Any thread.  src == NULL gives both tiles up.
#define VFSMS_SRC_YCC420_RAW 100      // internal: the raw planes of a 4:2:0 JPEG on the iMCU grid (jpeg_decode_raw420_host) -> k_ingest_420
// `host` (h * w pixels of `format`, densely packed) -> a device staging buffer -> the split kernel -> both tiles
static void fill_pair_upload(TileFill &f, const uint8_t *host, int format)
{
    const int h = f.h, w = f.w, pw = pad16(w), ph = pad16(h);
    const size_t need = format == VFSMS_SRC_YCC420_RAW ? (size_t)pw * ph * 3 / 2 : (size_t)h * w * ingest_source_pixel_bytes(format);
    if (format == VFSMS_SRC_GRAY8 && !f.dc) { f.copy(f.dg, host, need); return; }      // nothing to convert
    uint8_t *src = f.device(need);
    f.copy(src, host, need);
    f.run([&] { return format == VFSMS_SRC_YCC420_RAW ? launch_ingest_420(f.ctx->copy_stream, src, pw, ph, h, w, f.dg, f.dc)
                                                      : launch_ingest_split(f.ctx->copy_stream, src, f.dg, f.dc, (long long)h * w, format); });
}
extern "C" int vfsms_tile_fill_pair(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *src, int stride_bytes, int format)
{
    CTX_ENTER(ctx);
    TileFill f(ctx);
    const int spx = ingest_source_pixel_bytes(format);
    TRY(f.begin_pair(gray, color, "tile_fill_pair", src == nullptr));
    if (!src) return VFSMS_OK;
    if (!spx || stride_bytes < f.w * spx) { vfsms_set_error("tile_fill_pair: unknown format or stride smaller than a source row"); return f.refuse(VFSMS_ERR_BAD_ARG); }
    fill_pair_upload(f, f.pack(src, stride_bytes, (size_t)f.w * spx, f.h), format);
    return f.finish();
}

// A JPEG file's bytes -> the reserved gray tile and / or the reserved B G R tile, ONE decode (csrc/jpeg_host.cpp: the system's libjpeg-turbo,
// straight into a pinned staging buffer that is reused from call to call; Y only when no colour tile is asked for, the Y Cb Cr planes
// otherwise, colour conversion on the device).  Any thread; blocks until the tiles are complete.  When the decode cannot be done here
// (VFSMS_ERR_UNSUPPORTED: no libjpeg.so.8 on the host, not a 1- / 3-component JPEG; VFSMS_ERR_BAD_ARG: a damaged file, or a file whose size
// is not the tiles') BOTH TILES STAY RESERVED: the caller decodes some other way and fills them, or gives them up.
// what the three JPEG routes answer to a file of another size than the tiles' (CAPACITY: the decoder met it first); any other rc as it is
static int jpeg_size_check(const TileFill &f, int rc, int jh, int jw)
{
    if (rc != VFSMS_ERR_CAPACITY && (rc != VFSMS_OK || (jh == f.h && jw == f.w))) return rc;
    vfsms_set_error("%s: the file is %d x %d, the reserved tiles %d x %d", f.who, jh, jw, f.h, f.w);
    return VFSMS_ERR_BAD_ARG;
}
extern "C" int vfsms_tile_fill_jpeg(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!jpeg || !nbytes) { vfsms_set_error("tile_fill_jpeg: no data"); return VFSMS_ERR_BAD_ARG; }
    TileFill f(ctx);
    TRY(f.begin_pair(gray, color, "tile_fill_jpeg", false));
    // (the staging buffer is sized for either form: the interleaved planes are 3 bytes per pixel, the raw 4:2:0 planes 1.5 on the iMCU grid)
    const size_t cap = std::max((size_t)f.h * f.w * (f.dc ? 3 : 1), f.dc ? (size_t)pad16(f.w) * pad16(f.h) * 3 / 2 : (size_t)0);
    uint8_t *host = f.host(cap);
    int jh = 0, jw = 0, comp = 0;
    // Colour wanted and a 4:2:0 file: the host stops behind the IDCT, the device upsamples the chroma and converts (k_ingest_420).
    static const bool raw420 = !(getenv("VFSMS_JPEG_RAW420") && atoi(getenv("VFSMS_JPEG_RAW420")) == 0);
    int rc = VFSMS_ERR_UNSUPPORTED;
    if (f.dc && raw420) { rc = jpeg_decode_raw420_host(jpeg, nbytes, host, cap, &jh, &jw); comp = 420; }
    if (rc == VFSMS_ERR_UNSUPPORTED) rc = jpeg_decode_host(jpeg, nbytes, f.dc != nullptr, host, cap, &jh, &jw, &comp);
    rc = jpeg_size_check(f, rc, jh, jw);
    if (rc != VFSMS_OK) return f.refuse(rc);
    fill_pair_upload(f, host, comp == 420 ? VFSMS_SRC_YCC420_RAW : comp == 3 ? VFSMS_SRC_YCC24 : VFSMS_SRC_GRAY8);
    return f.finish();
}

// What both device decoders derive from a file's component count and block grid and the tiles that are wanted: the padded size, whether the
// three planes go through a scratch in the layout of jpeg_decode_raw420_host (`planes`) or a lone plane does (a colour tile alone from a gray
// file: the plane has no tile of its own), the scratch's size and the coefficients'
struct JpegTilePlan { int nc; const int *grid; int pw, ph; bool planes, via_scratch; size_t scratch_bytes, coef_bytes; };
static int jpeg_tile_plan(const TileFill &f, int nc, const int *grid, JpegTilePlan *P)
{
    const int pw = pad16(f.w), ph = pad16(f.h);
    const bool planes = nc == 3 && f.dc;
    *P = JpegTilePlan{nc, grid, pw, ph, planes, planes || (nc == 1 && !f.dg), planes ? (size_t)pw * ph * 3 / 2 : (size_t)f.h * f.w, 0};
    for (int k = 0; k < (f.dc ? nc : 1); k++) P->coef_bytes += (size_t)grid[2 * k] * grid[2 * k + 1] * 128;
    if (planes && (grid[0] * 8 != ph || grid[1] * 8 != pw || grid[2] * 16 != ph || grid[3] * 16 != pw || grid[4] != grid[2] || grid[5] != grid[3])) {
        vfsms_set_error("%s: the block grid is not the raw 4:2:0 layout's", f.who); return VFSMS_ERR_UNSUPPORTED;      // (cannot happen: both follow from h, w and 2x2, 1x1, 1x1)
    }
    return VFSMS_OK;
}
// the device end of both device decoders: the coefficients of a file lie on the device (`blocks`: per wanted component its grid of blocks,
// back to back; `quant`: a table per component) -> k_jpeg_idct -> the gray tile itself, or the three planes in `scratch` -> k_ingest_420, or
// the gray replication.  Stream-ordered on the copy stream
static int jpeg_coefficients_to_tiles(const TileFill &f, const JpegTilePlan &P, const uint16_t *quant, const int16_t *blocks, uint8_t *scratch)
{
    const int h = f.h, w = f.w;
    JpegIdctArgs A; memset(&A, 0, sizeof(A));
    A.ncomp = P.planes ? 3 : 1;
    for (int k = 0; k < A.ncomp; k++) {
        JpegIdctComp &C = A.c[k];
        C.coef = blocks + (size_t)A.total * 64; C.quant = quant + (size_t)k * (VFSMS_JPEG_COEF_TABLE_BYTES / 2);
        C.bcols = P.grid[2 * k + 1]; C.first = A.total;
        if (P.planes) {                                          // Y at pitch pw, then Cb, then Cr at pitch pw / 2: the whole grid, nothing cropped
            C.dst = k == 0 ? scratch : scratch + (size_t)P.pw * P.ph + (size_t)(k - 1) * (P.pw / 2) * (P.ph / 2);
            C.pitch = k == 0 ? P.pw : P.pw / 2; C.rows = P.grid[2 * k] * 8; C.cols = P.grid[2 * k + 1] * 8;
        } else { C.dst = f.dg ? f.dg : scratch; C.pitch = w; C.rows = h; C.cols = w; }
        A.total += (unsigned)P.grid[2 * k] * (unsigned)P.grid[2 * k + 1];
    }
    int rc = launch_jpeg_idct(f.ctx->copy_stream, A);
    if (rc == VFSMS_OK && P.planes) rc = launch_ingest_420(f.ctx->copy_stream, scratch, P.pw, P.ph, h, w, f.dg, f.dc);
    else if (rc == VFSMS_OK && f.dc) rc = launch_ingest_split(f.ctx->copy_stream, f.dg ? f.dg : scratch, nullptr, f.dc, (long long)h * w, VFSMS_SRC_GRAY8);
    return rc;
}

// Method.jpegDecoder = "device": the same contract as vfsms_tile_fill_jpeg, but the host stops behind the ENTROPY decode
// (jpeg_coefficients_host: jpeg_read_coefficients into pinned staging) and dequantisation, inverse DCT, level shift and range limit run on the
// device (k_jpeg_idct, csrc/jpeg_dec_kernels.hip), stream-ordered on the copy stream like everything else of the ingest.  Gray wanted alone:
// the luma blocks alone cross the link and the kernel writes the gray tile itself, cropped.  Colour wanted, a 4:2:0 file: the three planes go
// to a device scratch in the layout of jpeg_decode_raw420_host and k_ingest_420 runs on it unchanged.  Colour wanted, a one-component file:
// the plane is replicated as vfsms_tile_fill_pair replicates it.  A file this path does not take leaves BOTH TILES RESERVED.
extern "C" int vfsms_tile_fill_jpeg_dct(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!jpeg || !nbytes) { vfsms_set_error("tile_fill_jpeg_dct: no data"); return VFSMS_ERR_BAD_ARG; }
    TileFill f(ctx);
    TRY(f.begin_pair(gray, color, "tile_fill_jpeg_dct", false));
    // (the staging buffer is sized for any file of the tiles' size this path takes: three tables, the luma grid on whole 16 x 16 iMCUs at two
    // bytes a sample, and half as much again for the two chroma grids when a colour tile is wanted)
    const size_t cap = 3 * (size_t)VFSMS_JPEG_COEF_TABLE_BYTES + (size_t)pad16(f.w) * pad16(f.h) * (f.dc ? 3 : 2);
    uint8_t *host = f.host(cap);
    int jh = 0, jw = 0, nc = 0, grid[6] = {0, 0, 0, 0, 0, 0}; size_t need = 0; JpegTilePlan P;
    int rc = jpeg_size_check(f, jpeg_coefficients_host(jpeg, nbytes, f.dc == nullptr, host, cap, &jh, &jw, &nc, grid, &need), jh, jw);
    if (rc == VFSMS_OK) rc = jpeg_tile_plan(f, nc, grid, &P);
    if (rc != VFSMS_OK) return f.refuse(rc);
    // from here on the tiles end filled or given up
    uint8_t *coef = f.device(need), *scratch = P.via_scratch ? f.device(P.scratch_bytes) : nullptr;
    f.copy(coef, host, need);
    f.run([&] { return jpeg_coefficients_to_tiles(f, P, (const uint16_t *)coef, (const int16_t *)(coef + (size_t)nc * VFSMS_JPEG_COEF_TABLE_BYTES), scratch); });
    return f.finish();
}

// the bare operator behind it: block_rows x block_cols blocks of 64 int16 (natural order, block-row-major) and one uint16[64] table in, the
// plane of block_rows * 8 rows of block_cols * 8 samples out, `pitch` bytes apart.  Profile stage "jpeg_decode"
extern "C" int vfsms_jpeg_idct(vfsms_ctx *ctx, const int16_t *coef, const uint16_t *quant, int block_rows, int block_cols, uint8_t *out, int pitch)
{
    CTX_ENTER(ctx);
    if (!coef || !quant || !out || block_rows < 1 || block_cols < 1 || block_rows > 8192 || block_cols > 8192 || pitch < block_cols * 8) {
        vfsms_set_error("jpeg_idct: bad arguments (1..8192 blocks a side, pitch >= block_cols * 8)"); return VFSMS_ERR_BAD_ARG;
    }
    const size_t nblk = (size_t)block_rows * block_cols, cbytes = nblk * 128, pbytes = nblk * 64;
    TRY(ctx_arena_reserve(ctx, cbytes + pbytes + 128 + 4096));
    int16_t *d_coef = (int16_t *)ctx_arena_alloc(ctx, cbytes);
    uint16_t *d_q = (uint16_t *)ctx_arena_alloc(ctx, 128);
    uint8_t *d_out = (uint8_t *)ctx_arena_alloc(ctx, pbytes);
    if (!d_coef || !d_q || !d_out) { vfsms_set_error("arena exhausted (jpeg_idct)"); return VFSMS_ERR_CAPACITY; }
    HIP_TRY(hipMemcpyAsync(d_coef, coef, cbytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(hipMemcpyAsync(d_q, quant, 128, hipMemcpyHostToDevice, ctx->stream));
    JpegIdctArgs A; memset(&A, 0, sizeof(A));
    A.ncomp = 1; A.total = (unsigned)nblk;
    A.c[0].coef = d_coef; A.c[0].quant = d_q; A.c[0].dst = d_out; A.c[0].pitch = block_cols * 8; A.c[0].bcols = block_cols;
    A.c[0].rows = block_rows * 8; A.c[0].cols = block_cols * 8; A.c[0].first = 0;
    {
        ProfScope ps(ctx, "jpeg_decode");
        TRY(launch_jpeg_idct(ctx->stream, A));
    }
    HIP_TRY(hipMemcpy2DAsync(out, (size_t)pitch, d_out, (size_t)block_cols * 8, (size_t)block_cols * 8, (size_t)block_rows * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// the marker scan of a file (jpeg_scan_host: no libjpeg), once for the record's bound and once into the buffer that `buffer(bound)` yields
// for it: the record, its size and its header, or the scan's refusal with nothing written
template <typename Buffer>
static int jpeg_scan_record(const uint8_t *jpeg, size_t nbytes, Buffer buffer, uint8_t **rec, size_t *rec_bytes, JpegScanHeader *H)
{
    size_t bound = 0;
    const int rc = jpeg_scan_host(jpeg, nbytes, VFSMS_JPEG_HUFF_SUB_BITS, nullptr, 0, &bound);
    if (rc != VFSMS_ERR_CAPACITY) return rc;
    *rec = buffer(bound);
    TRY(jpeg_scan_host(jpeg, nbytes, VFSMS_JPEG_HUFF_SUB_BITS, *rec, bound, rec_bytes));
    memcpy(H, *rec, sizeof(*H));
    return VFSMS_OK;
}
// Method.jpegDecoder = "device-entropy": the contract of vfsms_tile_fill_jpeg_dct, but the host only scans the file for its markers and the
// entropy decode runs on the device too (csrc/jpeg_huff_kernels.hip), into a device buffer in the layout the inverse transform takes.  The
// compressed bytes alone cross the link.  The decode waits for the device between its stages (the round
// flags, the damage flags) on an event of its own; the tiles are written only after the damage flags came back clean.
extern "C" int vfsms_tile_fill_jpeg_huff(vfsms_ctx *ctx, int64_t gray, int64_t color, const uint8_t *jpeg, size_t nbytes)
{
    CTX_ENTER(ctx);
    if (!jpeg || !nbytes) { vfsms_set_error("tile_fill_jpeg_huff: no data"); return VFSMS_ERR_BAD_ARG; }
    TileFill f(ctx);
    TRY(f.begin_pair(gray, color, "tile_fill_jpeg_huff", false));
    size_t flags_at = 0, need = 0; uint8_t *host = nullptr;
    JpegScanHeader H; memset(&H, 0, sizeof(H)); JpegTilePlan P;
    // pinned staging with the decode's flag words behind the record
    auto staging = [&](size_t bound) { flags_at = (bound + 15) & ~(size_t)15; return f.host(flags_at + (VFSMS_JPEG_HUFF_MAX_ROUNDS + 2) * sizeof(uint32_t)); };
    int rc = jpeg_scan_record(jpeg, nbytes, staging, &host, &need, &H);
    rc = jpeg_size_check(f, rc, H.h, H.w);
    if (rc == VFSMS_OK) rc = jpeg_tile_plan(f, H.ncomp, H.grid6, &P);
    if (rc != VFSMS_OK) return f.refuse(rc);
    uint8_t *rec = f.device(need), *work = f.device(jpeg_huff_work_bytes(H, VFSMS_JPEG_HUFF_MAX_ROUNDS)), *coef = f.device(P.coef_bytes);
    uint8_t *scratch = P.via_scratch ? f.device(P.scratch_bytes) : nullptr;
    hipEvent_t sync = nullptr;
    if (f.ok()) f.e = hipEventCreateWithFlags(&sync, hipEventDisableTiming);
    f.copy(rec, host, need);
    bool refused = false;
    f.run([&] {
        int used = 0;
        int r = jpeg_huff_decode_device(ctx->copy_stream, sync, H, rec, work, (uint32_t *)(host + flags_at), VFSMS_JPEG_HUFF_MAX_ROUNDS, f.dc == nullptr,
                                        (int16_t *)coef, &used, nullptr);
        // a file handed back -- the decoders not in step, damage -- has touched no tile, and the decode has waited for all it launched
        refused = r == VFSMS_ERR_UNSUPPORTED || r == VFSMS_ERR_BAD_ARG;
        return r != VFSMS_OK ? r : jpeg_coefficients_to_tiles(f, P, (const uint16_t *)(rec + H.off_quant), (const int16_t *)coef, scratch);
    });
    rc = refused ? f.refuse(f.rc) : f.finish();                  // refused: both tiles stay reserved
    if (sync) hipEventDestroy(sync);
    return rc;
}

// the bare operator behind it: file bytes in, the layout of vfsms_jpeg_coefficients out, to a host array.  Profile stage "jpeg_entropy"
extern "C" int vfsms_jpeg_entropy_decode(vfsms_ctx *ctx, const uint8_t *jpeg, size_t nbytes, int max_rounds, uint8_t *out, size_t cap, int *h, int *w, int *ncomp,
                                         int *grid6, size_t *need, int *rounds_used)
{
    CTX_ENTER(ctx);
    if (!jpeg || !nbytes || !h || !w || !ncomp || !grid6 || !need) { vfsms_set_error("jpeg_entropy_decode: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    size_t rec_bytes = 0; std::vector<uint8_t> rec; uint8_t *rec_at = nullptr;
    JpegScanHeader H;
    int rc = jpeg_scan_record(jpeg, nbytes, [&](size_t bound) { rec.resize(bound); return rec.data(); }, &rec_at, &rec_bytes, &H);
    if (rc != VFSMS_OK) return rc;
    size_t coef_bytes = 0;
    for (int k = 0; k < H.ncomp; k++) { grid6[2 * k] = H.grid6[2 * k]; grid6[2 * k + 1] = H.grid6[2 * k + 1]; coef_bytes += (size_t)H.grid6[2 * k] * H.grid6[2 * k + 1] * 128; }
    const size_t tables = (size_t)H.ncomp * VFSMS_JPEG_COEF_TABLE_BYTES;
    *h = H.h; *w = H.w; *ncomp = H.ncomp; *need = tables + coef_bytes;
    if (!out || cap < *need) { vfsms_set_error("jpeg_entropy_decode: output buffer too small"); return VFSMS_ERR_CAPACITY; }
    const int rounds = max_rounds < 0 || max_rounds > H.nsub ? H.nsub : max_rounds;
    const size_t work = jpeg_huff_work_bytes(H, rounds);
    TRY(ctx_arena_reserve(ctx, rec_bytes + work + coef_bytes + 4096));
    uint8_t *d_rec = (uint8_t *)ctx_arena_alloc(ctx, rec_bytes), *d_work = (uint8_t *)ctx_arena_alloc(ctx, work);
    int16_t *d_coef = (int16_t *)ctx_arena_alloc(ctx, coef_bytes);
    if (!d_rec || !d_work || !d_coef) { vfsms_set_error("arena exhausted (jpeg_entropy_decode)"); return VFSMS_ERR_CAPACITY; }
    std::vector<uint32_t> flags((size_t)rounds + 2);
    hipEvent_t sync = nullptr;
    HIP_TRY(hipEventCreateWithFlags(&sync, hipEventDisableTiming));
    hipError_t e = hipMemcpyAsync(d_rec, rec.data(), rec_bytes, hipMemcpyHostToDevice, ctx->stream);
    int used = 0;
    if (e == hipSuccess) {
        ProfScope ps(ctx, "jpeg_entropy");
        rc = jpeg_huff_decode_device(ctx->stream, sync, H, d_rec, d_work, flags.data(), rounds, 0, d_coef, &used, ctx);
    }
    if (e == hipSuccess && rc == VFSMS_OK) e = hipMemcpyAsync(out + tables, d_coef, coef_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = hipStreamSynchronize(ctx->stream);
    hipEventDestroy(sync);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) { vfsms_set_error("jpeg_entropy_decode: %s", hipGetErrorString(e)); return VFSMS_ERR_HIP; }
    if (rc != VFSMS_OK) return rc;
    memcpy(out, rec.data() + H.off_quant, tables);
    if (rounds_used) *rounds_used = used;
    return VFSMS_OK;
}

extern "C" int vfsms_host_alloc(vfsms_ctx *ctx, size_t bytes, void **ptr)
{
    CTX_ENTER(ctx);
    if (!ptr || !bytes) { vfsms_set_error("host_alloc: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
    return VFSMS_OK;
}
extern "C" int vfsms_host_free(vfsms_ctx *ctx, void *ptr)
{
    CTX_ENTER(ctx);
    if (!ptr) return VFSMS_OK;
    HIP_TRY(hipStreamSynchronize(ctx->copy_stream));
    HIP_TRY(hipHostFree(ptr));
    return VFSMS_OK;
}
extern "C" int vfsms_tile_wrap(vfsms_ctx *ctx, const void *device_ptr, int h, int w, int stride, int64_t *handle)
{
    CTX_ENTER(ctx);
    if (!device_ptr || !handle || h <= 0 || w <= 0 || stride < w) { vfsms_set_error("tile_wrap: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    tile_register(ctx, tile_rec((uint8_t *)device_ptr, h, w, 1, stride, false), handle);
    return VFSMS_OK;
}
extern "C" int vfsms_tile_free(vfsms_ctx *ctx, int64_t handle)
{
    CTX_ENTER(ctx);
    TileRec *t;
    if (tile_find(ctx, "tile_free", handle, &t) != VFSMS_OK) { vfsms_set_error("tile_free: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    {
        std::lock_guard<std::mutex> lk(ctx->tiles_mu);       // (fill is written by decoder threads)
        if (t->fill == 1) { vfsms_set_error("tile_free: the tile is reserved and its decoder has not filled it yet"); return VFSMS_ERR_BAD_ARG; }
    }
    // an upload may still be in flight; compute work on the tile may only be ENQUEUED (canvas paste / resident fuse return early)
    if (t->pending) HIP_TRY(hipEventSynchronize(t->ready));
    if (t->ready) ctx->event_pool.push_back(t->ready);
    if (t->owned) TRY(tile_pool_return(ctx, t->ptr, t->bytes, true));
    { std::lock_guard<std::mutex> lk(ctx->tiles_mu); ctx->tiles.erase(handle); }
    return VFSMS_OK;
}

// ---- helpers ---------------------------------------------------------------------------------------------------
static int upload_image(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, uint8_t **d)
{
    *d = (uint8_t *)ctx_arena_alloc(ctx, (size_t)h * w);
    if (!*d) { vfsms_set_error("arena exhausted (image upload)"); return VFSMS_ERR_CAPACITY; }
    HIP_TRY(hipMemcpy2DAsync(*d, w, img, stride, w, h, hipMemcpyHostToDevice, ctx->stream));
    return VFSMS_OK;
}
template <typename T>
static int upload_array(vfsms_ctx *ctx, const T *src, size_t n, T **d)
{
    *d = (T *)ctx_arena_alloc(ctx, sizeof(T) * (n ? n : 1));
    if (!*d) { vfsms_set_error("arena exhausted (array upload)"); return VFSMS_ERR_CAPACITY; }
    if (n) HIP_TRY(hipMemcpyAsync(*d, src, sizeof(T) * n, hipMemcpyHostToDevice, ctx->stream));
    return VFSMS_OK;
}

// small host->device uploads of launch records through one pinned staging buffer (a pageable hipMemcpyAsync is staged by
// the runtime and costs a synchronisation each); safe to reuse because every entry point is synchronous at return
int ctx_upload_small(vfsms_ctx *ctx, const void *src, size_t bytes, void **d)
{
    *d = ctx_arena_alloc(ctx, bytes ? bytes : 1);
    if (!*d) { vfsms_set_error("arena exhausted (record upload)"); return VFSMS_ERR_CAPACITY; }
    return ctx_copy_small(ctx, src, bytes, *d);
}
// the same to an array the caller's layout walk took
int ctx_copy_small(vfsms_ctx *ctx, const void *src, size_t bytes, void *d)
{
    const size_t need = ctx->pinned_off + bytes;
    if (need > ctx->pinned.bytes()) {                               // (the synchronisation of the growth: earlier copies out of the old buffer have landed)
        TRY(ctx->pinned.reserve(need, ctx->stream, std::max<size_t>(4 * need, (size_t)1 << 20) - need));
        ctx->pinned_off = 0;
    }
    char *stage = ctx->pinned.as<char>() + ctx->pinned_off;
    memcpy(stage, src, bytes);
    HIP_TRY(hipMemcpyAsync(d, stage, bytes, hipMemcpyHostToDevice, ctx->stream));
    ctx->pinned_off += (bytes + 255) & ~(size_t)255;
    return VFSMS_OK;
}

// ---- integral ----------------------------------------------------------------------------------------------------
extern "C" int vfsms_integral_u8_i32(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int32_t *sum_out)
{
    CTX_ENTER(ctx);
    if (!img || !sum_out || h <= 0 || w <= 0 || stride < w) { vfsms_set_error("integral: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    const size_t sbytes = sizeof(int32_t) * (size_t)(h + 1) * (w + 1);
    TRY(ctx_arena_reserve(ctx, (size_t)h * w + sbytes + integral_carry_bytes(h, w) + 8192));
    RoiDev R; memset(&R, 0, sizeof(R));
    uint8_t *d_img;
    TRY(upload_image(ctx, img, h, w, stride, &d_img));
    R.img = d_img; R.stride = w; R.h = h; R.w = w;
    R.sum = (int32_t *)ctx_arena_alloc(ctx, sbytes);
    R.ipitch = (w + 3) & ~3;
    R.icarry = (int32_t *)ctx_arena_alloc(ctx, integral_carry_bytes(h, w));
    if (!R.sum || !R.icarry) { vfsms_set_error("arena exhausted (integral)"); return VFSMS_ERR_CAPACITY; }
    RoiDev *d_R;
    TRY(upload_array(ctx, &R, 1, &d_R));
    TRY(launch_integral(ctx, d_R, 1, h, w));
    HIP_TRY(hipMemcpyAsync(sum_out, R.sum, sbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// ---- one SURF run: n sources detected (and described) in fused launches ------------------------------------------------------------
// Every entry point that runs SURF goes through these phases, in this order: surf_run_bytes into the caller's ONE ctx_arena_reserve (it
// resets the arena), surf_run_carve, surf_run_prepare, surf_run_launch over one or more ranges of the sources, surf_run_readback, the caller's own
// hipStreamSynchronize (it may enqueue copies of its own first), surf_run_check.
// The one place that knows a run's arena block: the counters, per source its enhancement job and its ROI, the uploaded records
void surf_run_layout(ArenaWalk &a, SurfRun *run, const SurfSrc *S, int n, const vfsms_surf_params *p, const SurfEnh &enh)
{
    run->R.resize(n); run->E.resize(enh.mode ? n : 0);
    run->cblock = a.take<int>(16 * (size_t)n);
    for (int i = 0; i < n; i++) {
        const uint8_t *px = S[i].p; int stride = S[i].stride;
        if (enh.mode) {            // Stitcher.py:327-334: the ROI strips are equalised / CLAHE'd before detectAndDescribe
            enhance_layout(a, &run->E[i], px, stride, S[i].h, S[i].w, enh.mode, enh.tile_grid);
            px = run->E[i].dst; stride = S[i].w;
        }
        surf_roi_layout(a, &run->R[i], px, stride, S[i].h, S[i].w, S[i].cap, p);
        run->R[i].counters = run->cblock ? run->cblock + 16 * i : nullptr;
    }
    run->dR = a.take<RoiDev>(n);
    run->dE = enh.mode ? a.take<EnhJob>(n) : nullptr;
}
// with the work lists of the describe launches over the sources [0, split) and [split, n) (launch_surf_describe carves them when it runs)
static size_t surf_run_bytes(const SurfSrc *S, int n, const vfsms_surf_params *p, const SurfEnh &enh, int split = 0)
{
    ArenaWalk a; SurfRun run; DescWork W;
    surf_run_layout(a, &run, S, n, p, enh);
    size_t cap0 = 0, cap1 = 0;
    for (int i = 0; i < n; i++) (i < split ? cap0 : cap1) += (size_t)S[i].cap;
    if (split > 0) surf_describe_layout(a, &W, cap0);
    if (split < n) surf_describe_layout(a, &W, cap1);
    return a.off;
}
static int surf_run_carve(vfsms_ctx *ctx, SurfRun *run, const SurfSrc *S, int n, const vfsms_surf_params *p, const SurfEnh &enh)
{
    ArenaWalk a = ctx_arena_walk(ctx);
    surf_run_layout(a, run, S, n, p, enh);
    TRY(ctx_arena_commit(ctx, a, "arena exhausted while carving a SURF run"));
    return ctx_copy_small(ctx, run->R.data(), sizeof(RoiDev) * n, run->dR);
}
// the enhancement and the zeroed counters, enqueued behind every record upload of the call (a fused batch uploads its match records
// in between: copies next to copies, then the device work)
static int surf_run_prepare(vfsms_ctx *ctx, SurfRun *run, const SurfEnh &enh)
{
    const int n = (int)run->R.size();
    if (enh.mode) {
        TRY(ctx_copy_small(ctx, run->E.data(), sizeof(EnhJob) * n, run->dE));
        TRY(launch_enhance(ctx, run->dE, run->E.data(), n, enh.mode, enh.clip_limit, enh.tile_grid));
    }
    HIP_TRY(hipMemsetAsync(run->cblock, 0, sizeof(int) * 16 * n, ctx->stream));
    return VFSMS_OK;
}
static int surf_run_launch(vfsms_ctx *ctx, const SurfRun &run, int first, int count, bool describe, const vfsms_surf_params *p)
{
    TRY(launch_surf_detect(ctx, run.dR + first, run.R.data() + first, count, p));
    if (describe) TRY(launch_surf_describe(ctx, run.dR + first, run.R.data() + first, count, p));
    return VFSMS_OK;
}
static int surf_run_readback(vfsms_ctx *ctx, SurfRun *run)
{
    run->counters.resize(16 * run->R.size());
    HIP_TRY(hipMemcpyAsync(run->counters.data(), run->cblock, sizeof(int) * run->counters.size(), hipMemcpyDeviceToHost, ctx->stream));
    return VFSMS_OK;
}
// after the caller's synchronisation; source i is reported as `unit` index0 + i of `total`
static int surf_run_check(const SurfRun &run, const char *who, const char *unit, int index0, int total)
{
    for (size_t i = 0; i < run.R.size(); i++)
        if (run.counters[16 * i + 2] || run.counters[16 * i] > run.R[i].cap) {
            vfsms_set_error("%s: %s %d of %d (%d x %d) exceeded %d keypoint candidates (raise with vfsms_ctx_set_keypoint_capacity)",
                            who, unit, index0 + (int)i, total, run.R[i].h, run.R[i].w, run.R[i].cap);
            return VFSMS_ERR_CAPACITY;
        }
    return VFSMS_OK;
}
// kept keypoints of described source i
static int surf_run_count(const SurfRun &run, int i) { return run.counters[16 * (size_t)i + 1]; }

// ---- SURF (host buffers) ------------------------------------------------------------------------------------------
static int surf_host(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, const vfsms_surf_params *params,
                     float *kps_xy, float *desc, vfsms_keypoint *kps_full, int cap, int *n_out, bool describe)
{
    CTX_ENTER(ctx);
    if (!img || !params || !n_out || h <= 0 || w <= 0 || stride < w || cap < 0) { vfsms_set_error("surf: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_prepare_surf(ctx, params));
    const int dim = params->extended ? 128 : 64;
    const SurfEnh plain{0, 0.0, 0};
    SurfSrc src{nullptr, w, h, w, kp_capacity(ctx, h, w)};
    TRY(ctx_arena_reserve(ctx, (size_t)h * w + surf_run_bytes(&src, 1, params, plain) + 65536));
    ctx->pinned_off = 0;                                    // entry points are synchronous: the staging buffer is free again
    uint8_t *d_img;
    TRY(upload_image(ctx, img, h, w, stride, &d_img));
    src.p = d_img;
    SurfRun run;
    TRY(surf_run_carve(ctx, &run, &src, 1, params, plain));
    TRY(surf_run_prepare(ctx, &run, plain));
    TRY(surf_run_launch(ctx, run, 0, 1, describe, params));
    TRY(surf_run_readback(ctx, &run));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    TRY(surf_run_check(run, "surf", "image", 0, 1));
    const RoiDev &R = run.R[0];
    const int n = describe ? surf_run_count(run, 0) : run.counters[0];      // undescribed: the candidates
    *n_out = n;
    if (n > cap) { vfsms_set_error("surf: %d keypoints exceed the caller's capacity %d", n, cap); return VFSMS_ERR_CAPACITY; }
    if (n > 0) {
        if (describe) {
            if (kps_xy) HIP_TRY(hipMemcpyAsync(kps_xy, R.kps_xy, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
            if (desc) HIP_TRY(hipMemcpyAsync(desc, R.desc, sizeof(float) * (size_t)n * dim, hipMemcpyDeviceToHost, ctx->stream));
            if (kps_full) HIP_TRY(hipMemcpyAsync(kps_full, R.kps_out, sizeof(vfsms_keypoint) * n, hipMemcpyDeviceToHost, ctx->stream));
        } else if (kps_full) {
            HIP_TRY(hipMemcpyAsync(kps_full, R.kps, sizeof(vfsms_keypoint) * n, hipMemcpyDeviceToHost, ctx->stream));
        }
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return VFSMS_OK;
}
extern "C" int vfsms_surf_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                                          const vfsms_surf_params *params, float *kps_xy, float *desc,
                                          vfsms_keypoint *kps_full, int cap, int *n_out)
{
    return surf_host(ctx, img, h, w, stride, params, kps_xy, desc, kps_full, cap, n_out, true);
}
extern "C" int vfsms_surf_detect(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                                 const vfsms_surf_params *params, vfsms_keypoint *kps_full, int cap, int *n_out)
{
    return surf_host(ctx, img, h, w, stride, params, nullptr, nullptr, kps_full, cap, n_out, false);
}

// ---- matching (host buffers) -----------------------------------------------------------------------------------------
static int pick_nsplit(int nq, int nt, int njobs, int dim)
{
    const int qpw = dim == 64 ? 128 : 64;                 // queries per wave
    const long long waves = (long long)((nq + qpw - 1) / qpw) * njobs;
    // aim at >= 16 waves per SIMD (1024 SIMDs) so the last, partially filled round of workgroups is a small tail
    int ns = (int)((16384 + waves - 1) / (waves > 0 ? waves : 1));
    ns = std::max(1, std::min(ns, 64));
    ns = std::min(ns, std::max(1, nt / 64));
    return ns;
}

// train splits of the MFMA filter: a wave holds 64 queries and two waves share a SIMD, so aim at >= 4 rounds of the
// 2048 wave slots; more splits mean more candidate lists to verify, hence the cap
// Round 6: and at least one split per BFM_SPLIT_TRAINS trains.  The candidate lists hold BFM_CAPL = 32 entries per (list, query); what a
// list admits grows with the trains it covers (the threshold window of the bounds pass is an absolute 5e-3 in squared distance; 1.7e-2 when these figures were taken), and a
// query whose list overflows is verified by an exhaustive scan of ALL trains.  configs[4]'s strips (37 k keypoints, large batches: the
// wave count alone asked for ONE split) spent 11 ms per launch in k_bf_verify_d64 against 0.24 ms at the headline's 8.7 k; with the
// train rule 4.1 ms (one split per 10240 trains; 5120: another 3 % off the search, profiles/r06_ab_bf_split_4096.txt).
#ifndef BFM_SPLIT_TRAINS
#define BFM_SPLIT_TRAINS 5120
#endif
static int pick_filter_nsplit(int nq, int njobs, int nt = 0)
{
    const long long waves = (long long)((nq + 63) / 64) * njobs;
    int ns = (int)((8192 + waves - 1) / (waves > 0 ? waves : 1));
    ns = std::max(ns, (nt + BFM_SPLIT_TRAINS - 1) / BFM_SPLIT_TRAINS);
    return std::max(1, std::min(ns, 8));
}

// Hamming search: a wave owns 64 queries and walks its share of the trains: split the trains so that a batch fills the chip a few times over
static int pick_hamming_nsplit(int capq, int njobs)
{
    const long long waves = (long long)((capq + 63) / 64) * njobs;
    return (int)std::max<long long>(1, std::min<long long>(8, (8192 + waves - 1) / waves));
}

// integer 128-d search (k_bf_i8_d128): a wave owns 64 queries; `waves` over all the jobs of the launch, maxt the largest train set.  Splits
// are whole 16-train tiles, at least 256 trains each while the chip is short of waves
static int pick_i8_nsplit(long long waves, int maxt)
{
    waves = std::max<long long>(waves, 1);
    return (int)std::max<long long>(1, std::min<long long>({8, (4096 + waves - 1) / waves, (long long)(maxt + 255) / 256}));
}

static bool bf_force_exact()
{
    static const bool v = getenv("VFSMS_BF_EXACT") && atoi(getenv("VFSMS_BF_EXACT")) != 0;
    return v;
}

// ---- one 2-NN search + vote run: n (query set, train set) jobs in fused launches ------------------------------------------------------
// The phases mirror a SURF run's: match_run_bytes into the caller's ONE ctx_arena_reserve, match_run_carve (wires and uploads the
// records), match_run_launch over one or more ranges of the jobs, match_run_readback in front of the caller's synchronisation.
// k_bf_l2* on the float descriptors (filtered or not: the plan) / k_bf_i8_d128 on the int8 rows / k_bf_hamming_jobs on 32-byte rows behind q, t
// SEARCH_NONE: the caller has filled the jobs' pairs (MatchJob::pairs_given), and the tail starts from them
enum MatchSearch { SEARCH_NONE, SEARCH_FLOAT, SEARCH_I8_D128, SEARCH_HAMMING };
// 64-d descriptors leave the descriptor kernel with norm <= 1: their 2-NN search runs as an MFMA candidate filter plus exact verification
// (match_kernels.hip); other widths, or VFSMS_BF_EXACT=1, take the exhaustive VALU kernel.  The split counts follow the set sizes the
// CALLER expects, (fq, ft) for the filter and (eq, et) for the exhaustive kernel: the true counts of feature sets, the typical occupancy
// of the capacity in a fused batch.
static MatchPlan match_plan_float(int dim, int njobs, int fq, int ft, int eq, int et)
{
    MatchPlan P;
    P.filtered = dim == 64 && !bf_force_exact();
    P.cns = pick_filter_nsplit(fq, njobs, ft);
    P.ns = P.filtered ? 1 : pick_nsplit(eq, et, njobs, dim);
    return P;
}
// the raw pixels of a job's two strips, for the overlap check behind the vote (verify_kernels.hip)
static void match_set_strips(MatchDev *m, const StripTable::Strip &A, const StripTable::Strip &B)
{
    m->va = A.p; m->vsa = A.stride; m->vb = B.p; m->vsb = B.stride; m->vh = A.h; m->vw = A.w;
}
// The one place that knows a run's arena block: the result rows (one block: one copy back), per job its arrays, the uploaded records
void match_run_layout(ArenaWalk &a, MatchRun *run, const MatchJob *J, int n, int dim, const MatchPlan &P)
{
    run->P = P; run->dim = dim; run->M.assign(n, MatchDev{});
    run->rblock = a.take<int32_t>(VFSMS_ATTEMPT_INTS * (size_t)n);
    for (int k = 0; k < n; k++) {
        MatchDev &m = run->M[k];
        match_layout(a, &m, J[k].capq, dim, P.ns);
        if (P.filtered) match_filter_layout(a, &m, J[k].capq, J[k].capt, P.cns);
        m.result = run->rblock ? run->rblock + VFSMS_ATTEMPT_INTS * J[k].row : nullptr;
        m.q = J[k].q; m.t = J[k].t; m.kq = J[k].kq; m.kt = J[k].kt; m.nq_ptr = J[k].nq_ptr; m.nt_ptr = J[k].nt_ptr;
        m.q8 = J[k].q8; m.t8 = J[k].t8; m.qn2 = J[k].qn2; m.tn2 = J[k].tn2; m.pairs_given = J[k].pairs_given;
        if (J[k].sa) match_set_strips(&m, *J[k].sa, *J[k].sb);
    }
    run->dM = a.take<MatchDev>(n);
}
static size_t match_run_bytes(const MatchJob *J, int n, const MatchPlan &P) { ArenaWalk a; MatchRun run; match_run_layout(a, &run, J, n, 0, P); return a.off; }
static int match_run_carve(vfsms_ctx *ctx, MatchRun *run, const MatchJob *J, int n, int dim, const MatchPlan &P)
{
    ArenaWalk a = ctx_arena_walk(ctx);
    match_run_layout(a, run, J, n, dim, P);
    TRY(ctx_arena_commit(ctx, a, "arena exhausted while carving a match run"));
    return ctx_copy_small(ctx, run->M.data(), sizeof(MatchDev) * n, run->dM);
}
// the search of `search`, then the tail (common.h: MatchTailKind), of jobs [first, first + count); maxq / maxt: the largest query / train set to cover
static int match_run_launch(vfsms_ctx *ctx, const MatchRun &run, int first, int count, int maxq, int maxt, MatchSearch search, const MatchTail &tail)
{
    const MatchDev *dM = run.dM + first;
    if (search == SEARCH_HAMMING) { TRY(launch_bf_hamming(ctx, dM, count, maxq, run.P.ns, tail.max_dist)); }
    else if (search == SEARCH_I8_D128) { TRY(launch_bf_i8_d128(ctx, dM, count, maxq, run.P.ns)); }
    else if (search == SEARCH_FLOAT && run.P.filtered) { TRY(launch_bf_l2_filtered(ctx, dM, count, maxq, maxt, run.P.cns)); }
    else if (search == SEARCH_FLOAT) { TRY(launch_bf_l2(ctx, dM, count, maxq, run.P.ns, run.dim)); }
    return launch_match_tail(ctx, dM, count, maxq, tail);
}
static int match_run_readback(vfsms_ctx *ctx, const MatchRun &run, int32_t *rows)
{
    HIP_TRY(hipMemcpyAsync(rows, run.rblock, sizeof(int32_t) * VFSMS_ATTEMPT_INTS * run.M.size(), hipMemcpyDeviceToHost, ctx->stream));
    return VFSMS_OK;
}

// the (nq, nt) of n jobs, on the device behind J[k].nq_ptr / nt_ptr.  Through the pinned staging buffer (free again: entry points are
// synchronous), which takes its copy NOW: cnt may leave scope before the stream runs
static int match_upload_counts(vfsms_ctx *ctx, MatchJob *J, int n, const int *cnt)
{
    int *d;
    ctx->pinned_off = 0;
    TRY(ctx_upload_small(ctx, cnt, sizeof(int) * 2 * n, (void **)&d));
    for (int k = 0; k < n; k++) { J[k].nq_ptr = d + 2 * k; J[k].nt_ptr = d + 2 * k + 1; }
    return VFSMS_OK;
}

// ---- the matcher operators: one job each, on a match run ----------------------------------------------------------------------------
// vfsms_bf_l2_knn2 / _ratio: one job of host descriptors.  Rows of norm <= 1 (SURF's are L2-normalised) take the MFMA-filtered plan,
// anything else the exhaustive one: a probe in front of the run decides, and ONE reservation covers the larger of the two
static int bf_l2_host(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim, MatchRun *run, const MatchTail &tail)
{
    MatchJob J{};
    J.capq = std::max(nq, 1); J.capt = std::max(nt, 1);
    const MatchPlan exhaustive{false, pick_nsplit(nq, nt, 1, dim), 0}, filter{true, 1, pick_filter_nsplit(nq, 1, nt)};
    const bool try_filter = dim == 64 && nq > 0 && nt > 0 && !bf_force_exact();
    TRY(ctx_arena_reserve(ctx, sizeof(float) * ((size_t)nq + nt) * dim +
                               std::max(match_run_bytes(&J, 1, exhaustive), try_filter ? match_run_bytes(&J, 1, filter) : 0) + 65536));
    float *dq, *dt;
    TRY(upload_array(ctx, q, (size_t)nq * dim, &dq));
    TRY(upload_array(ctx, t, (size_t)nt * dim, &dt));
    J.q = dq; J.t = dt;
    const int cnt[2] = {nq, nt};
    TRY(match_upload_counts(ctx, &J, 1, cnt));
    bool filtered = false;
    if (try_filter) {
        unsigned *d_max = (unsigned *)ctx_arena_alloc(ctx, sizeof(unsigned));
        HIP_TRY(hipMemsetAsync(d_max, 0, sizeof(unsigned), ctx->stream));
        TRY(launch_max_norm2_d64(ctx, dq, nq, d_max));
        TRY(launch_max_norm2_d64(ctx, dt, nt, d_max));
        unsigned bits = 0;
        HIP_TRY(hipMemcpyAsync(&bits, d_max, sizeof(bits), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        float m; memcpy(&m, &bits, sizeof(m));
        filtered = m <= 1.0001f;
    }
    TRY(match_run_carve(ctx, run, &J, 1, dim, filtered ? filter : exhaustive));
    return match_run_launch(ctx, *run, 0, 1, J.capq, J.capt, SEARCH_FLOAT, tail);
}

extern "C" int vfsms_bf_l2_knn2_ratio(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim,
                                      double ratio, int32_t *pairs, int cap, int *m_out)
{
    CTX_ENTER(ctx);
    if (!m_out || nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) { vfsms_set_error("bf_l2: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    *m_out = 0;
    if (nq == 0 || nt == 0) return VFSMS_OK;
    MatchRun run;
    TRY(bf_l2_host(ctx, q, nq, t, nt, dim, &run, MatchTail{TAIL_PAIRS, ratio, -1, 0}));
    const MatchDev &M = run.M[0];
    int mc[4];
    HIP_TRY(hipMemcpyAsync(mc, M.mcount, sizeof(mc), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    *m_out = mc[0];
    if (mc[0] > cap) { vfsms_set_error("bf_l2: %d matches exceed capacity %d", mc[0], cap); return VFSMS_ERR_CAPACITY; }
    if (mc[0] > 0 && pairs) {
        HIP_TRY(hipMemcpyAsync(pairs, M.pairs, sizeof(int32_t) * 2 * mc[0], hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return VFSMS_OK;
}

extern "C" int vfsms_bf_l2_knn2(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int dim,
                                int32_t *idx1, float *d1, float *d2)
{
    CTX_ENTER(ctx);
    if (nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) { vfsms_set_error("bf_l2_knn2: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (nq == 0) return VFSMS_OK;
    if (nt == 0) {
        for (int i = 0; i < nq; i++) { if (idx1) idx1[i] = -1; if (d1) d1[i] = INFINITY; if (d2) d2[i] = INFINITY; }
        return VFSMS_OK;
    }
    MatchRun run;
    TRY(bf_l2_host(ctx, q, nq, t, nt, dim, &run, MatchTail{TAIL_KNN, 0.0, -1, 0}));
    const MatchDev &M = run.M[0];
    if (idx1) HIP_TRY(hipMemcpyAsync(idx1, M.i1, sizeof(int) * nq, hipMemcpyDeviceToHost, ctx->stream));
    if (d1) HIP_TRY(hipMemcpyAsync(d1, M.d1, sizeof(float) * nq, hipMemcpyDeviceToHost, ctx->stream));
    if (d2) HIP_TRY(hipMemcpyAsync(d2, M.d2, sizeof(float) * nq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// vfsms_bf_l2_knn2_u8d128: one job of host descriptors through the integer search of the fused SIFT batch (k_pack_i8_d128 +
// k_bf_i8_d128), the way the batch drives it: rows packed to sift_pad_rows, device counts, whole-tile splits.  A test and diagnostic
// operator: VFSMS_BF_EXACT does not apply
static bool u8_elements(const float *a, size_t n)
{
    for (size_t k = 0; k < n; k++) {
        const float v = a[k];
        if (!(v >= 0.f && v <= 255.f) || v != (float)(int)v) return false;       // a NaN fails the first compare
    }
    return true;
}
extern "C" int vfsms_bf_l2_knn2_u8d128(vfsms_ctx *ctx, const float *q, int nq, const float *t, int nt, int nsplit,
                                       int32_t *idx1, float *d1, float *d2)
{
    CTX_ENTER(ctx);
    if (nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) { vfsms_set_error("bf_l2_knn2_u8d128: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (nsplit < 0 || nsplit > 8) { vfsms_set_error("bf_l2_knn2_u8d128: nsplit %d outside 0..8", nsplit); return VFSMS_ERR_BAD_ARG; }
    if (!u8_elements(q, (size_t)nq * 128) || !u8_elements(t, (size_t)nt * 128)) {
        vfsms_set_error("bf_l2_knn2_u8d128: every element must be an integer in 0..255");
        return VFSMS_ERR_BAD_ARG;
    }
    if (nq == 0) return VFSMS_OK;
    if (nt == 0) {
        for (int i = 0; i < nq; i++) { if (idx1) idx1[i] = -1; if (d1) d1[i] = INFINITY; if (d2) d2[i] = INFINITY; }
        return VFSMS_OK;
    }
    MatchJob J{};
    J.capq = nq; J.capt = nt;
    const MatchPlan P{false, nsplit ? nsplit : pick_i8_nsplit((nq + 63) / 64, nt), 0};
    const size_t pq = sift_pad_rows(nq), pt = sift_pad_rows(nt);
    TRY(ctx_arena_reserve(ctx, sizeof(float) * ((size_t)nq + nt) * 128 + (128 + sizeof(int)) * (pq + pt) + match_run_bytes(&J, 1, P) + 65536));
    float *dq, *dt;
    TRY(upload_array(ctx, q, (size_t)nq * 128, &dq));
    TRY(upload_array(ctx, t, (size_t)nt * 128, &dt));
    int8_t *q8 = (int8_t *)ctx_arena_alloc(ctx, 128 * pq), *t8 = (int8_t *)ctx_arena_alloc(ctx, 128 * pt);
    int *qn = (int *)ctx_arena_alloc(ctx, sizeof(int) * pq), *tn = (int *)ctx_arena_alloc(ctx, sizeof(int) * pt);
    if (!q8 || !t8 || !qn || !tn) { vfsms_set_error("bf_l2_knn2_u8d128: arena exhausted (packed rows)"); return VFSMS_ERR_CAPACITY; }
    J.q = dq; J.t = dt; J.q8 = q8; J.t8 = t8; J.qn2 = qn; J.tn2 = tn;
    const int cnt[2] = {nq, nt};
    TRY(match_upload_counts(ctx, &J, 1, cnt));
    const PackJob pj[2] = {{dq, J.nq_ptr, q8, qn}, {dt, J.nt_ptr, t8, tn}};
    PackJob *dP;
    TRY(ctx_upload_small(ctx, pj, sizeof(pj), (void **)&dP));
    TRY(launch_pack_i8_d128(ctx, dP, 2, std::max(nq, nt)));
    MatchRun run;
    TRY(match_run_carve(ctx, &run, &J, 1, 128, P));
    TRY(match_run_launch(ctx, run, 0, 1, nq, nt, SEARCH_I8_D128, MatchTail{TAIL_KNN, 0.0, -1, 0}));
    const MatchDev &M = run.M[0];
    if (idx1) HIP_TRY(hipMemcpyAsync(idx1, M.i1, sizeof(int) * nq, hipMemcpyDeviceToHost, ctx->stream));
    if (d1) HIP_TRY(hipMemcpyAsync(d1, M.d1, sizeof(float) * nq, hipMemcpyDeviceToHost, ctx->stream));
    if (d2) HIP_TRY(hipMemcpyAsync(d2, M.d2, sizeof(float) * nq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

extern "C" int vfsms_bf_hamming_nn(vfsms_ctx *ctx, const uint8_t *q, int nq, const uint8_t *t, int nt, int nbytes,
                                   int max_dist, int32_t *pairs, int cap, int *m_out)
{
    CTX_ENTER(ctx);
    if (!m_out || nq < 0 || nt < 0 || (nq && !q) || (nt && !t)) { vfsms_set_error("bf_hamming: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    *m_out = 0;
    if (nq == 0 || nt == 0) return VFSMS_OK;
    if (nbytes != 32) { vfsms_set_error("bf_hamming: only 32-byte descriptors supported"); return VFSMS_ERR_UNSUPPORTED; }
    // one job of the batched matcher without keypoints, hence without votes: the merged 1-NN comes back and the pair list is built here
    MatchJob J{};
    J.capq = nq; J.capt = nt;
    const MatchPlan P{false, pick_hamming_nsplit(nq, 1), 0};
    TRY(ctx_arena_reserve(ctx, ((size_t)nq + nt) * 32 + match_run_bytes(&J, 1, P) + 65536));
    uint8_t *dq, *dt;
    TRY(upload_array(ctx, q, (size_t)nq * 32, &dq));
    TRY(upload_array(ctx, t, (size_t)nt * 32, &dt));
    J.q = (const float *)dq; J.t = (const float *)dt;
    const int cnt[2] = {nq, nt};
    TRY(match_upload_counts(ctx, &J, 1, cnt));
    MatchRun run;
    TRY(match_run_carve(ctx, &run, &J, 1, 32, P));
    TRY(match_run_launch(ctx, run, 0, 1, nq, nt, SEARCH_HAMMING, MatchTail{TAIL_KNN, 0.0, max_dist, 0, true}));
    std::vector<int> hi(nq); std::vector<float> hd(nq);
    HIP_TRY(hipMemcpyAsync(hi.data(), run.M[0].i1, sizeof(int) * nq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipMemcpyAsync(hd.data(), run.M[0].d1, sizeof(float) * nq, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    int m = 0;
    for (int i = 0; i < nq; i++) {
        if (hi[i] < 0) continue;
        if (max_dist >= 0 && !(hd[i] < max_dist)) continue;
        if (m < cap && pairs) { pairs[2 * m] = hi[i]; pairs[2 * m + 1] = i; }
        m++;
    }
    *m_out = m;
    if (m > cap) { vfsms_set_error("bf_hamming: %d matches exceed capacity %d", m, cap); return VFSMS_ERR_CAPACITY; }
    return VFSMS_OK;
}

// vfsms_mode_offset / vfsms_consensus_offset: one job of the caller's matches, no search, through the tail of the named estimator
static int offset_from_pairs(vfsms_ctx *ctx, const char *what, const float *kpsA, int nA, const float *kpsB, int nB,
                             const int32_t *pairs, int m, int estimator, int tol, int offset_evaluate, int32_t *out4)
{
    CTX_ENTER(ctx);
    if (!out4 || m < 0 || nA < 0 || nB < 0) { vfsms_set_error("%s: bad arguments", what); return VFSMS_ERR_BAD_ARG; }
    out4[0] = out4[1] = out4[2] = out4[3] = 0;
    if (m == 0) return VFSMS_OK;
    for (int k = 0; k < m; k++)
        if (pairs[2 * k] < 0 || pairs[2 * k] >= nB || pairs[2 * k + 1] < 0 || pairs[2 * k + 1] >= nA) {
            vfsms_set_error("%s: match index out of range", what); return VFSMS_ERR_BAD_ARG;
        }
    MatchJob J{};
    J.capq = J.capt = m; J.pairs_given = 1;
    const MatchPlan P{false, 1, 0};
    TRY(ctx_arena_reserve(ctx, sizeof(float) * 2 * ((size_t)nA + nB) + match_run_bytes(&J, 1, P) + 65536));
    float *dA, *dB;
    TRY(upload_array(ctx, kpsA, (size_t)2 * nA, &dA));
    TRY(upload_array(ctx, kpsB, (size_t)2 * nB, &dB));
    J.kq = dA; J.kt = dB;
    const int cnt[2] = {m, m};
    TRY(match_upload_counts(ctx, &J, 1, cnt));
    MatchRun run;
    TRY(match_run_carve(ctx, &run, &J, 1, 64, P));
    HIP_TRY(hipMemcpyAsync(run.M[0].pairs, pairs, sizeof(int32_t) * 2 * m, hipMemcpyHostToDevice, ctx->stream));
    TRY(match_run_launch(ctx, run, 0, 1, m, m, SEARCH_NONE, MatchTail{TAIL_GIVEN_PAIRS, 0.0, -1, offset_evaluate, false, estimator, tol}));
    int32_t res[VFSMS_ATTEMPT_INTS];
    TRY(match_run_readback(ctx, run, res));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < 4; k++) out4[k] = res[k];
    return VFSMS_OK;
}

extern "C" int vfsms_mode_offset(vfsms_ctx *ctx, const float *kpsA, int nA, const float *kpsB, int nB,
                                 const int32_t *pairs, int m, int offset_evaluate, int32_t *out4)
{
    return offset_from_pairs(ctx, "mode_offset", kpsA, nA, kpsB, nB, pairs, m, VFSMS_OFFSET_MODE, 0, offset_evaluate, out4);
}

extern "C" int vfsms_consensus_offset(vfsms_ctx *ctx, const float *kpsA, int nA, const float *kpsB, int nB,
                                      const int32_t *pairs, int m, int tol_px, int offset_evaluate, int32_t *out4)
{
    if (tol_px < 0 || tol_px > VFSMS_CONSENSUS_MAX_TOL) { vfsms_set_error("consensus_offset: tolerance %d outside 0..%d", tol_px, VFSMS_CONSENSUS_MAX_TOL); return VFSMS_ERR_BAD_ARG; }
    return offset_from_pairs(ctx, "consensus_offset", kpsA, nA, kpsB, nB, pairs, m, VFSMS_OFFSET_CONSENSUS, tol_px, offset_evaluate, out4);
}

// vfsms_verify_ncc: the verifier's three kernels on one job whose result row names the vote as accepted; the decision is the caller's
extern "C" int vfsms_verify_ncc(vfsms_ctx *ctx, const uint8_t *a, int a_stride, const uint8_t *b, int b_stride, int h, int w,
                                int dx, int dy, int min_pixels, int64_t *out8)
{
    CTX_ENTER(ctx);
    if (!a || !b || !out8 || h <= 0 || w <= 0 || a_stride < w || b_stride < w || min_pixels < 0) { vfsms_set_error("verify_ncc: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_arena_reserve(ctx, 2 * (size_t)h * w + 65536));
    ctx->pinned_off = 0;
    uint8_t *da, *db;
    TRY(upload_image(ctx, a, h, w, a_stride, &da));
    TRY(upload_image(ctx, b, h, w, b_stride, &db));
    MatchDev M; memset(&M, 0, sizeof(M));
    int32_t row[VFSMS_ATTEMPT_INTS] = {1, dx, dy, 0, 0, 0, 0, 0};
    TRY(upload_array(ctx, row, VFSMS_ATTEMPT_INTS, &M.result));
    M.vsum = (unsigned long long *)ctx_arena_alloc(ctx, 64);
    if (!M.vsum) { vfsms_set_error("verify_ncc: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    M.va = da; M.vb = db; M.vsa = w; M.vsb = w; M.vh = h; M.vw = w;
    MatchDev *dM;
    TRY(upload_array(ctx, &M, 1, &dM));
    TRY(launch_verify(ctx, dM, 1, -1.0, min_pixels));
    HIP_TRY(hipMemcpyAsync(out8, M.vsum, 64, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// vfsms_ncc_search_batch: the window search of adjust_kernels.hip over pairs of resident tiles; every launch of the batch is enqueued
// before the one synchronisation that brings the results back
extern "C" int vfsms_ncc_search_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int radius, int min_pixels, int32_t *best4, int32_t *surface)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n > 0 && (!jobs || !best4)) || min_pixels < 0) { vfsms_set_error("ncc_search: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (radius < 1 || radius > VFSMS_ADJUST_MAX_RADIUS) { vfsms_set_error("ncc_search: radius %d outside 1..%d", radius, VFSMS_ADJUST_MAX_RADIUS); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    std::vector<AdjJob> H(n);
    for (int k = 0; k < n; k++) {
        TileRec *pA, *pB;
        TRY(resident_pair(ctx, "ncc_search", k, jobs[k], &pA, &pB));
        const TileRec &A = *pA, &B = *pB;
        if (A.ch != 1 || B.ch != 1) { vfsms_set_error("ncc_search: job %d names a colour tile; the search takes single-channel tiles", k); return VFSMS_ERR_BAD_ARG; }
        if (A.h != B.h || A.w != B.w) { vfsms_set_error("ncc_search: the tiles of job %d are %d x %d and %d x %d", k, A.h, A.w, B.h, B.w); return VFSMS_ERR_BAD_ARG; }
        H[k].a = A.ptr; H[k].b = B.ptr; H[k].sa = A.stride; H[k].sb = B.stride; H[k].h = A.h; H[k].w = A.w; H[k].dx = jobs[k].dx; H[k].dy = jobs[k].dy;
    }
    const size_t CC = (size_t)(2 * radius + 1) * (2 * radius + 1);
    const int part = 32768;                                  // jobs per launch (a grid dimension holds 65535)
    const size_t sums_bytes = adjust_sums_bytes(std::min(n, part), radius);
    TRY(ctx_arena_reserve(ctx, sizeof(AdjJob) * (size_t)n + sums_bytes + sizeof(int32_t) * (size_t)n * (4 + (surface ? CC : 0)) + 65536));
    ctx->pinned_off = 0;
    AdjJob *dJ;
    TRY(ctx_upload_small(ctx, H.data(), sizeof(AdjJob) * (size_t)n, (void **)&dJ));
    unsigned long long *d_sums = (unsigned long long *)ctx_arena_alloc(ctx, sums_bytes);
    int32_t *d_best = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 4 * (size_t)n);
    int32_t *d_surf = surface ? (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * CC * (size_t)n) : nullptr;
    if (!d_sums || !d_best || (surface && !d_surf)) { vfsms_set_error("ncc_search: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    for (int k0 = 0; k0 < n; k0 += part)                     // (stream order: a part's sums are cleared after the part before it was scored)
        TRY(launch_adjust_search(ctx, dJ + k0, H.data() + k0, std::min(part, n - k0), radius, min_pixels, d_sums, d_best + 4 * (size_t)k0,
                                 d_surf ? d_surf + CC * (size_t)k0 : nullptr));
    HIP_TRY(hipMemcpyAsync(best4, d_best, sizeof(int32_t) * 4 * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    if (surface) HIP_TRY(hipMemcpyAsync(surface, d_surf, sizeof(int32_t) * CC * (size_t)n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// the resident single-channel pair of one shape that job k of `who` names -> an AdjJob
static int adj_job_of(vfsms_ctx *ctx, const char *who, int k, const vfsms_ncc_job &j, AdjJob *out)
{
    TileRec *pA, *pB;
    TRY(resident_pair(ctx, who, k, j, &pA, &pB));
    const TileRec &A = *pA, &B = *pB;
    if (A.ch != 1 || B.ch != 1) { vfsms_set_error("%s: job %d names a colour tile; the search takes single-channel tiles", who, k); return VFSMS_ERR_BAD_ARG; }
    if (A.h != B.h || A.w != B.w) { vfsms_set_error("%s: the tiles of job %d are %d x %d and %d x %d", who, k, A.h, A.w, B.h, B.w); return VFSMS_ERR_BAD_ARG; }
    *out = AdjJob{A.ptr, B.ptr, A.stride, B.stride, A.h, A.w, j.dx, j.dy};
    return VFSMS_OK;
}

// vfsms_ncc_wide_batch: wide_kernels.hip around the search of adjust_kernels.hip; every launch of the batch is enqueued before the one
// synchronisation that brings the results back
extern "C" int vfsms_ncc_wide_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int radius, int factor, int peaks, int min_pixels,
                                    int32_t *out8, int32_t *seeds, uint8_t *reduced)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n > 0 && (!jobs || !out8)) || min_pixels < 0 || (reduced && n != 1)) { vfsms_set_error("ncc_wide: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (radius < 1 || radius > VFSMS_WIDE_MAX_RADIUS) { vfsms_set_error("ncc_wide: radius %d outside 1..%d", radius, VFSMS_WIDE_MAX_RADIUS); return VFSMS_ERR_BAD_ARG; }
    if (factor != 2 && factor != 4 && factor != 8) { vfsms_set_error("ncc_wide: factor %d (2, 4 or 8)", factor); return VFSMS_ERR_BAD_ARG; }
    if (peaks < 1 || peaks > VFSMS_WIDE_MAX_PEAKS) { vfsms_set_error("ncc_wide: %d peaks outside 1..%d", peaks, VFSMS_WIDE_MAX_PEAKS); return VFSMS_ERR_BAD_ARG; }
    const int F = factor, K = peaks, Rc = (radius + F - 1) / F, rf = std::min(F, radius);
    if (Rc > VFSMS_ADJUST_MAX_RADIUS) { vfsms_set_error("ncc_wide: radius %d at factor %d leaves a coarse radius of %d (at most %d)", radius, F, Rc, VFSMS_ADJUST_MAX_RADIUS); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    std::vector<WideJob> W(n);
    std::vector<AdjJob> HC(n), HF((size_t)n * K);
    size_t plane_bytes = 0;
    for (int k = 0; k < n; k++) {
        WideJob &J = W[k];
        TRY(adj_job_of(ctx, "ncc_wide", k, jobs[k], &J.src));
        J.ox = ((J.src.dx % F) + F) % F; J.oy = ((J.src.dy % F) + F) % F;
        J.hc = (J.src.h - J.ox) / F; J.wc = (J.src.w - J.oy) / F;
        if (J.hc < 1 || J.wc < 1) { vfsms_set_error("ncc_wide: the %d x %d tiles of job %d leave no block of %d x %d", J.src.h, J.src.w, k, F, F); return VFSMS_ERR_BAD_ARG; }
        J.sc = (J.wc + 15) & ~15;
        plane_bytes += 2 * ((((size_t)J.hc * J.sc + 64) + 255) & ~(size_t)255);
        // The grid of a fine search is sized from a host job, and the centres of the fine jobs exist only on the device.  A seed's centre is
        // (dx + cx, dy + cy) with |cx|, |cy| <= radius - rf, so its overlap has at most h - |dx + cx| + rf <= h - (|dx| - (radius - rf)) + rf
        // rows under any candidate; the host job below has exactly that bound under the search's own formula (h - |dx'| + rf), columns alike.
        AdjJob B = J.src;
        B.dx = (J.src.dx < 0 ? -1 : 1) * std::max(0, std::abs(J.src.dx) - (radius - rf));
        B.dy = (J.src.dy < 0 ? -1 : 1) * std::max(0, std::abs(J.src.dy) - (radius - rf));
        for (int q = 0; q < K; q++) HF[(size_t)k * K + q] = B;
    }
    const int Cc = 2 * Rc + 1, CCc = Cc * Cc;
    const int part = 32768 / VFSMS_WIDE_MAX_PEAKS;             // jobs per launch sequence: its part * K fine jobs fit a grid dimension's 32768
    const int np_max = std::min(n, part);
    const size_t sums_bytes = std::max(adjust_sums_bytes(np_max, Rc), adjust_sums_bytes(np_max * K, rf));
    const size_t ints = (size_t)n * (8 + VFSMS_WIDE_MAX_PEAKS * 6) + (size_t)np_max * (4 + CCc + 4 * K);
    TRY(ctx_arena_reserve(ctx, plane_bytes + sizeof(WideJob) * (size_t)n + sizeof(AdjJob) * ((size_t)n + (size_t)np_max * K) + sums_bytes + sizeof(int32_t) * ints + 65536));
    ctx->pinned_off = 0;
    for (int k = 0; k < n; k++) {
        WideJob &J = W[k];
        const size_t pb = (size_t)J.hc * J.sc + 64;             // 64 bytes behind the last row: the search loads aligned dwords
        J.ac = (uint8_t *)ctx_arena_alloc(ctx, pb); J.bc = (uint8_t *)ctx_arena_alloc(ctx, pb);
        if (!J.ac || !J.bc) { vfsms_set_error("ncc_wide: arena exhausted"); return VFSMS_ERR_CAPACITY; }
        HC[k] = AdjJob{J.ac, J.bc, J.sc, J.sc, J.hc, J.wc, (J.src.dx - J.ox) / F, (J.src.dy - J.oy) / F};
    }
    WideJob *dW; AdjJob *dC;
    TRY(ctx_upload_small(ctx, W.data(), sizeof(WideJob) * (size_t)n, (void **)&dW));
    TRY(ctx_upload_small(ctx, HC.data(), sizeof(AdjJob) * (size_t)n, (void **)&dC));
    AdjJob *d_fine = (AdjJob *)ctx_arena_alloc(ctx, sizeof(AdjJob) * (size_t)np_max * K);
    unsigned long long *d_sums = (unsigned long long *)ctx_arena_alloc(ctx, sums_bytes);
    int32_t *d_out8 = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 8 * (size_t)n);
    int32_t *d_seeds = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * VFSMS_WIDE_MAX_PEAKS * 6 * (size_t)n);
    int32_t *d_cbest = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 4 * (size_t)np_max);
    int32_t *d_surf = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * (size_t)CCc * np_max);
    int32_t *d_fbest = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 4 * (size_t)np_max * K);
    if (!d_fine || !d_sums || !d_out8 || !d_seeds || !d_cbest || !d_surf || !d_fbest) { vfsms_set_error("ncc_wide: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    {
        ProfScope ps(ctx, "repair");
        for (int k0 = 0; k0 < n; k0 += part) {                // (stream order: a part's scratch is reused after the part before it was picked)
            const int np = std::min(part, n - k0);
            TRY(launch_wide_reduce(ctx, dW + k0, W.data() + k0, np, F));
            TRY(launch_adjust_search(ctx, dC + k0, HC.data() + k0, np, Rc, std::max(1, min_pixels / (F * F)), d_sums, d_cbest, d_surf));
            TRY(launch_wide_seeds(ctx, dW + k0, np, radius, F, K, d_surf, d_fine, d_seeds + VFSMS_WIDE_MAX_PEAKS * 6 * (size_t)k0, d_out8 + 8 * (size_t)k0));
            TRY(launch_adjust_search(ctx, d_fine, HF.data() + (size_t)k0 * K, np * K, rf, min_pixels, d_sums, d_fbest, nullptr));
            TRY(launch_wide_pick(ctx, np, K, d_fbest, d_seeds + VFSMS_WIDE_MAX_PEAKS * 6 * (size_t)k0, d_out8 + 8 * (size_t)k0));
        }
    }
    // results land in staging first: a failure below leaves the caller's arrays untouched
    std::vector<int32_t> h_out((size_t)n * 8), h_seeds(seeds ? (size_t)n * VFSMS_WIDE_MAX_PEAKS * 6 : 0);
    std::vector<uint8_t> h_red(reduced ? ((size_t)W[0].hc * W[0].sc) * 2 : 0);
    HIP_TRY(hipMemcpyAsync(h_out.data(), d_out8, sizeof(int32_t) * h_out.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (seeds) HIP_TRY(hipMemcpyAsync(h_seeds.data(), d_seeds, sizeof(int32_t) * h_seeds.size(), hipMemcpyDeviceToHost, ctx->stream));
    if (reduced) {
        const size_t pb = (size_t)W[0].hc * W[0].sc;
        HIP_TRY(hipMemcpyAsync(h_red.data(), W[0].ac, pb, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipMemcpyAsync(h_red.data() + pb, W[0].bc, pb, hipMemcpyDeviceToHost, ctx->stream));
    }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    memcpy(out8, h_out.data(), sizeof(int32_t) * h_out.size());
    if (seeds) memcpy(seeds, h_seeds.data(), sizeof(int32_t) * h_seeds.size());
    if (reduced) {
        const WideJob &J = W[0];
        for (int p = 0; p < 2; p++)
            for (int u = 0; u < J.hc; u++) memcpy(reduced + ((size_t)p * J.hc + u) * J.wc, h_red.data() + ((size_t)p * J.hc + u) * J.sc, J.wc);
    }
    return VFSMS_OK;
}

// vfsms_overlap_sums_batch: overlap_rows_sums of overlap_sums.h over whole resident tiles (wide_kernels.hip: k_wide_sums)
extern "C" int vfsms_overlap_sums_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int64_t *out6)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n > 0 && (!jobs || !out6))) { vfsms_set_error("overlap_sums: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    std::vector<AdjJob> H(n);
    for (int k = 0; k < n; k++) TRY(adj_job_of(ctx, "overlap_sums", k, jobs[k], &H[k]));
    const size_t out_bytes = sizeof(unsigned long long) * 6 * (size_t)n;
    TRY(ctx_arena_reserve(ctx, sizeof(AdjJob) * (size_t)n + out_bytes + 65536));
    ctx->pinned_off = 0;
    AdjJob *dJ;
    TRY(ctx_upload_small(ctx, H.data(), sizeof(AdjJob) * (size_t)n, (void **)&dJ));
    unsigned long long *d_out = (unsigned long long *)ctx_arena_alloc(ctx, out_bytes);
    if (!d_out) { vfsms_set_error("overlap_sums: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    const int part = 32768;
    for (int k0 = 0; k0 < n; k0 += part) TRY(launch_overlap_sums(ctx, dJ + k0, H.data() + k0, std::min(part, n - k0), d_out + 6 * (size_t)k0));
    HIP_TRY(hipMemcpyAsync(out6, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// ---- phase correlation ---------------------------------------------------------------------------------------------------
extern "C" int vfsms_phase_correlate_u8(vfsms_ctx *ctx, const uint8_t *a, const uint8_t *b, int h, int w,
                                        int stride_a, int stride_b, double *out3)
{
    CTX_ENTER(ctx);
    if (!a || !b || !out3 || h <= 0 || w <= 0 || stride_a < w || stride_b < w) { vfsms_set_error("phase: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    size_t pb = 0;
    TRY(phase_bytes(ctx, h, w, 1, &pb));
    TRY(ctx_arena_reserve(ctx, 2 * (size_t)h * w + pb + 65536));
    ctx->pinned_off = 0;
    uint8_t *da, *db;
    TRY(upload_image(ctx, a, h, w, stride_a, &da));
    TRY(upload_image(ctx, b, h, w, stride_b, &db));
    double *d_out = (double *)ctx_arena_alloc(ctx, 3 * sizeof(double));
    TRY(phase_correlate_device(ctx, da, w, db, w, h, w, d_out));
    HIP_TRY(hipMemcpyAsync(out3, d_out, 3 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// ---- phase correlation resolved by overlap correlation (phase_resolve_kernels.hip) -----------------------------------------------------
// The one place that knows what nb jobs of one strip shape take from the arena beyond the results and ahead of the correlation's own
// scratch (phase_layout): the correlation's output, the peaks, the candidates' sums, the uploaded strips
void phase_resolve_layout(ArenaWalk &a, PhaseResolveDev *d, int nb, int K)
{
    d->out3 = a.take<double>(3 * (size_t)nb);
    d->peaks = a.take<PhasePeak>((size_t)nb * K);
    d->sums = a.take<unsigned long long>(phase_resolve_sums_bytes(nb, K) / sizeof(unsigned long long));
    d->jobs = a.take<PhaseJobHost>(nb);
}
static int phase_resolve_bytes(vfsms_ctx *ctx, int h, int w, int nb, int K, size_t *bytes)
{
    ArenaWalk a; PhaseResolveDev d; PhaseScratch sc;
    phase_resolve_layout(a, &d, nb, K);
    TRY(phase_layout(ctx, a, &sc, h, w, nb, K));
    *bytes = a.off;
    return VFSMS_OK;
}
// nb jobs of one strip shape: correlation with the peak sink, then the candidates; results at d_rows / d_cands / d_pk (device, nb records each)
static int phase_resolve_group(vfsms_ctx *ctx, const PhaseJobHost *pj, int nb, int h, int w, int K, double threshold, int min_pixels,
                               int32_t *d_rows, int32_t *d_cands, int32_t *d_pk)
{
    ArenaWalk a = ctx_arena_walk(ctx);
    PhaseResolveDev d;
    phase_resolve_layout(a, &d, nb, K);
    TRY(ctx_arena_commit(ctx, a, "phase_resolve: arena exhausted"));
    TRY(ctx_copy_small(ctx, pj, sizeof(PhaseJobHost) * (size_t)nb, d.jobs));
    const PhasePeakSink sink = {K, d.peaks};
    TRY(phase_correlate_batch_device(ctx, pj, nb, h, w, d.out3, &sink));
    int oM, oN;
    phase_surface_size(h, w, &oM, &oN);
    return launch_phase_resolve(ctx, d.jobs, d.peaks, nb, K, oM, oN, h, w, threshold, min_pixels, d.sums, d_rows, d_cands, d_pk);
}

extern "C" int vfsms_phase_resolve_u8(vfsms_ctx *ctx, const uint8_t *a, const uint8_t *b, int h, int w, int stride_a, int stride_b,
                                      int peaks, double threshold, int min_pixels, int32_t *row8, int32_t *cands, int32_t *peaks_out)
{
    CTX_ENTER(ctx);
    if (!a || !b || !row8 || h <= 0 || w <= 0 || stride_a < w || stride_b < w || !phase_resolve_params_ok(peaks, threshold, min_pixels)) {
        vfsms_set_error("phase_resolve: bad arguments"); return VFSMS_ERR_BAD_ARG;
    }
    size_t need = 0;
    TRY(phase_resolve_bytes(ctx, h, w, 1, peaks, &need));
    const size_t res = sizeof(int32_t) * (VFSMS_ATTEMPT_INTS + 16 * (size_t)peaks + 2 * (size_t)peaks);
    TRY(ctx_arena_reserve(ctx, 2 * (size_t)h * w + need + res + 65536));
    ctx->pinned_off = 0;
    uint8_t *da, *db;
    TRY(upload_image(ctx, a, h, w, stride_a, &da));
    TRY(upload_image(ctx, b, h, w, stride_b, &db));
    int32_t *d_rows = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * VFSMS_ATTEMPT_INTS);
    int32_t *d_cands = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 16 * (size_t)peaks);
    int32_t *d_pk = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 2 * (size_t)peaks);
    if (!d_rows || !d_cands || !d_pk) { vfsms_set_error("phase_resolve: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    PhaseJobHost j; j.a = da; j.b = db; j.sa = w; j.sb = w;
    TRY(phase_resolve_group(ctx, &j, 1, h, w, peaks, threshold, min_pixels, d_rows, d_cands, d_pk));
    HIP_TRY(hipMemcpyAsync(row8, d_rows, sizeof(int32_t) * VFSMS_ATTEMPT_INTS, hipMemcpyDeviceToHost, ctx->stream));
    if (cands) HIP_TRY(hipMemcpyAsync(cands, d_cands, sizeof(int32_t) * 16 * (size_t)peaks, hipMemcpyDeviceToHost, ctx->stream));
    if (peaks_out) HIP_TRY(hipMemcpyAsync(peaks_out, d_pk, sizeof(int32_t) * 2 * (size_t)peaks, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

static int resolve_job(vfsms_ctx *ctx, const vfsms_roi_pair &j, const uint8_t **pa, int *sa, const uint8_t **pb, int *sb)
{
    TileRec *pA, *pB;
    TRY(tile_find(ctx, "attempt", j.tile_a, &pA)); TRY(tile_find(ctx, "attempt", j.tile_b, &pB));
    TileRec &A = *pA, &B = *pB;
    if (A.ch != 1 || B.ch != 1) { vfsms_set_error("attempt: registration takes single-channel tiles"); return VFSMS_ERR_BAD_ARG; }
    TRY(tile_ready(ctx, A)); TRY(tile_ready(ctx, B));
    if (j.h <= 0 || j.w <= 0 || j.ay0 < 0 || j.ax0 < 0 || j.by0 < 0 || j.bx0 < 0 || j.ay0 + j.h > A.h || j.ax0 + j.w > A.w ||
        j.by0 + j.h > B.h || j.bx0 + j.w > B.w) { vfsms_set_error("attempt: ROI outside its tile"); return VFSMS_ERR_BAD_ARG; }
    *pa = A.ptr + (size_t)j.ay0 * A.stride + j.ax0; *sa = A.stride;
    *pb = B.ptr + (size_t)j.by0 * B.stride + j.bx0; *sb = B.stride;
    return VFSMS_OK;
}

// ---- strip table of a fused batch -----------------------------------------------------------------------------------------------
// The 2n ROI slots of a batch (job ord[s]'s A strip, its B strip) name fewer distinct strips: at a turn of the serpentine path the
// failed direction-1 attempt's B strip is the next pair's direction-3 A strip, and both are in the batch (28 of the bench grid's 242
// strips).  Detecting and describing a strip depends on its pixels alone, so each distinct strip is carved and run once and the match
// blocks of every job that uses it read it.  The key is the strip's first pixel (after the tile's stride), its stride and its shape, not
// the tile handle: vfsms_tile_wrap can give one buffer two handles.  Scope: one call; nothing is kept across calls.
// A strip's part is that of the first slot that uses it (slots < n0: part 0), so part 1's jobs may read part-0 strips -- described
// before part 0's search, in stream order -- and never the other way round.  Slots run in (shape) order and a strip has its job's shape,
// so the order of first use is already the (part, shape) order the shape-run launchers need.
// VFSMS_STRIP_DEDUP=0 carves every slot a strip of its own (2s, 2s + 1: the layout before the table) for A/B runs.
static int build_strip_table(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, const int *ord, int n, int n0, StripTable *T)
{
    static const bool dedup = !(getenv("VFSMS_STRIP_DEDUP") && atoi(getenv("VFSMS_STRIP_DEDUP")) == 0);
    std::map<std::tuple<const uint8_t *, int, int, int>, int> seen;
    T->strips.clear(); T->a.assign(n, 0); T->b.assign(n, 0); T->u0 = 0;
    auto strip_of = [&](const uint8_t *p, int stride, int h, int w) {
        if (dedup) {
            auto it = seen.emplace(std::make_tuple(p, stride, h, w), (int)T->strips.size());
            if (!it.second) return it.first->second;
        }
        T->strips.push_back(StripTable::Strip{p, stride, h, w});
        return (int)T->strips.size() - 1;
    };
    for (int s = 0; s < n; s++) {
        const vfsms_roi_pair &j = jobs[ord[s]];
        const uint8_t *pa, *pb; int sa, sb;
        TRY(resolve_job(ctx, j, &pa, &sa, &pb, &sb));
        T->a[s] = strip_of(pa, sa, j.h, j.w);
        T->b[s] = strip_of(pb, sb, j.h, j.w);
        if (s == n0 - 1) T->u0 = (int)T->strips.size();
    }
    return VFSMS_OK;
}

// ---- jobs of one ROI shape next to each other ------------------------------------------------------------------------------------
// The kernels whose grid follows the image size are launched per run of equal shapes (common.h: shape_runs), and a batched
// transform takes one shape: every batch puts its jobs in the stable (h, w) order.  Slot s holds job ord[s]; results go to the job's row.
static std::vector<int> shape_order(const vfsms_roi_pair *jobs, int n)
{
    std::vector<int> ord(n);
    for (int k = 0; k < n; k++) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](int x, int y) {
        return jobs[x].h != jobs[y].h ? jobs[x].h < jobs[y].h : jobs[x].w < jobs[y].w; });
    return ord;
}
// the run of equal shapes that starts at position g0 of n ends before the position returned; shape_at(k) -> (h, w) of position k
template <typename ShapeAt>
static int shape_run_end(int g0, int n, ShapeAt shape_at)
{
    int g1 = g0 + 1;
    while (g1 < n && shape_at(g1) == shape_at(g0)) g1++;
    return g1;
}

// ---- the phase batches: one driver over the runs of equal shapes ------------------------------------------------------------------------
// Attempts of one ROI size (all of them, in practice) run as ONE batched transform; other sizes follow group by group.  ONE
// ctx_arena_reserve: the results of all n jobs (result_bytes, *d_results, set before the first group runs) and behind them the scratch of
// the largest group (bytes_of(h, w, nb, &bytes)), rewound for every group -- stream order makes the reuse safe.  run_group(pj, nb, h, w, g0)
// enqueues the nb jobs of a group whose strips are pj; its results go to slots g0.. of the result block, which is in GROUP order: slot k
// holds job order[k], and the caller un-permutes on the host behind its one synchronisation.
template <typename BytesOf, typename RunGroup>
static int phase_shape_groups(vfsms_ctx *ctx, const char *who, const vfsms_roi_pair *jobs, int n, size_t result_bytes, BytesOf bytes_of, RunGroup run_group,
                              std::vector<int> *order, void **d_results)
{
    *order = shape_order(jobs, n);
    const std::vector<int> &ord = *order;
    auto shape_at = [&](int k) { return std::make_pair(jobs[ord[k]].h, jobs[ord[k]].w); };
    size_t need = 0;
    for (int g0 = 0, g1; g0 < n; g0 = g1) {
        g1 = shape_run_end(g0, n, shape_at);
        size_t gb = 0;
        TRY(bytes_of(jobs[ord[g0]].h, jobs[ord[g0]].w, g1 - g0, &gb));
        need = std::max(need, gb);
    }
    TRY(ctx_arena_reserve(ctx, need + result_bytes + 65536));
    ctx->pinned_off = 0;
    *d_results = ctx_arena_alloc(ctx, result_bytes);
    if (!*d_results) { vfsms_set_error("%s: arena exhausted", who); return VFSMS_ERR_CAPACITY; }
    const size_t mark = ctx->arena_off;
    std::vector<PhaseJobHost> pj(n);
    for (int g0 = 0, g1; g0 < n; g0 = g1) {
        g1 = shape_run_end(g0, n, shape_at);
        for (int k = g0; k < g1; k++) {
            const uint8_t *pa, *pb; int sa, sb;
            TRY(resolve_job(ctx, jobs[ord[k]], &pa, &sa, &pb, &sb));
            pj[k].a = pa; pj[k].b = pb; pj[k].sa = sa; pj[k].sb = sb;
        }
        ctx->arena_off = mark;
        TRY(run_group(pj.data() + g0, g1 - g0, jobs[ord[g0]].h, jobs[ord[g0]].w, g0));
    }
    return VFSMS_OK;
}

extern "C" int vfsms_attempt_phase_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, double *out)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!jobs || !out))) { vfsms_set_error("attempt_phase: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    std::vector<int> order;
    double *d_out = nullptr;
    TRY(phase_shape_groups(ctx, "attempt_phase", jobs, n, sizeof(double) * 3 * n,
                           [&](int h, int w, int nb, size_t *bytes) { return phase_bytes(ctx, h, w, nb, bytes); },
                           [&](const PhaseJobHost *pj, int nb, int h, int w, int g0) { return phase_correlate_batch_device(ctx, pj, nb, h, w, d_out + 3 * g0); },
                           &order, (void **)&d_out));
    std::vector<double> tmp((size_t)3 * n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), d_out, sizeof(double) * 3 * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) for (int c = 0; c < 3; c++) out[3 * order[k] + c] = tmp[3 * k + c];
    return VFSMS_OK;
}

extern "C" int vfsms_attempt_phase_resolve_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, int peaks, double threshold, int min_pixels,
                                                 int32_t *rows, int32_t *cands, int32_t *peaks_out)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!jobs || !rows)) || !phase_resolve_params_ok(peaks, threshold, min_pixels)) {
        vfsms_set_error("attempt_phase_resolve: bad arguments (peaks 1..%d, threshold -1..1, min_pixels >= 0)", VFSMS_PHASE_MAX_PEAKS); return VFSMS_ERR_BAD_ARG;
    }
    if (n == 0) return VFSMS_OK;
    const int K = peaks;
    const size_t RI = VFSMS_ATTEMPT_INTS, CI = 16 * (size_t)K, PI = 2 * (size_t)K;
    // the result block on the device and its copy on the host: [n] rows, [n] candidate tables, [n] peak positions
    std::vector<int> order;
    int32_t *d_rows = nullptr;
    TRY(phase_shape_groups(ctx, "attempt_phase_resolve", jobs, n, sizeof(int32_t) * (RI + CI + PI) * (size_t)n,
                           [&](int h, int w, int nb, size_t *bytes) { return phase_resolve_bytes(ctx, h, w, nb, K, bytes); },
                           [&](const PhaseJobHost *pj, int nb, int h, int w, int g0) {
                               return phase_resolve_group(ctx, pj, nb, h, w, K, threshold, min_pixels, d_rows + RI * g0, d_rows + RI * n + CI * g0,
                                                          d_rows + (RI + CI) * n + PI * g0); },
                           &order, (void **)&d_rows));
    const int32_t *d_cands = d_rows + RI * n, *d_pk = d_cands + CI * n;
    std::vector<int32_t> tmp((RI + CI + PI) * (size_t)n);
    int32_t *t_rows = tmp.data(), *t_cands = t_rows + RI * n, *t_pk = t_cands + CI * n;
    HIP_TRY(hipMemcpyAsync(t_rows, d_rows, sizeof(int32_t) * RI * n, hipMemcpyDeviceToHost, ctx->stream));
    if (cands) HIP_TRY(hipMemcpyAsync(t_cands, d_cands, sizeof(int32_t) * CI * n, hipMemcpyDeviceToHost, ctx->stream));
    if (peaks_out) HIP_TRY(hipMemcpyAsync(t_pk, d_pk, sizeof(int32_t) * PI * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int k = 0; k < n; k++) {
        memcpy(rows + RI * order[k], t_rows + RI * k, sizeof(int32_t) * RI);
        if (cands) memcpy(cands + CI * order[k], t_cands + CI * k, sizeof(int32_t) * CI);
        if (peaks_out) memcpy(peaks_out + PI * order[k], t_pk + PI * k, sizeof(int32_t) * PI);
    }
    return VFSMS_OK;
}

// ---- fused SURF + BF + ratio + mode attempts --------------------------------------------------------------------------------
// the second compute stream and its fork / join events (created on first use)
static int ctx_second_stream(vfsms_ctx *ctx)
{
    if (ctx->stream2) return VFSMS_OK;
    HIP_TRY(hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming));
    return VFSMS_OK;
}
// ctx->stream is what every launcher enqueues on: swapped for a scope, restored on every way out of it
struct StreamSwap {
    vfsms_ctx *c; hipStream_t saved;
    StreamSwap(vfsms_ctx *ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { ctx->stream = s; }
    ~StreamSwap() { c->stream = saved; }
};
// Joins the second stream on EVERY way out of the forked region of attempt_surf_impl: an error return behind the fork (e.g. a capacity
// overflow of part 1's describe) would otherwise let the caller's retry reset and reuse the arena while part 0's search still runs on it.
struct SecondStreamJoin {
    vfsms_ctx *c; bool armed = false;
    explicit SecondStreamJoin(vfsms_ctx *ctx) : c(ctx) {}
    ~SecondStreamJoin() { if (armed && c->stream2) (void)hipStreamSynchronize(c->stream2); }
};

static int attempt_surf_impl(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, const vfsms_surf_params *params, double ratio,
                             int offset_evaluate, int enh_mode, double clip_limit, int tile_grid, int32_t *out)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!jobs || !out)) || !params) { vfsms_set_error("attempt_surf: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    TRY(ctx_prepare_surf(ctx, params));
    const int dim = params->extended ? 128 : 64;
    int maxcap = 0;
    for (int k = 0; k < n; k++) maxcap = std::max(maxcap, kp_capacity(ctx, jobs[k].h, jobs[k].w));
    // (the registrar sizes the capacity at 1.5x the largest ROI seen: the filter is split for 2/3 of it, the exhaustive kernel for its typical occupancy)
    const MatchPlan P = match_plan_float(dim, n, maxcap * 2 / 3, maxcap * 2 / 3, maxcap / 3, maxcap / 3);
    // Two pipes at once -- built, measured, OFF by default.  The 2-NN search lives on the matrix cores (k_bf_mfma16_d64: MFMA pipe 55-65 %
    // busy, VALU idle), detection on the VALU and the texture-address path.  With VFSMS_OVERLAP=1 a large batch is cut in two parts of
    // slots: part 0 (VFSMS_OVERLAP_PCT, default 70 %) is detected and described, then its search + ratio + vote run on the second stream
    // BESIDE the detect stage of part 1 (the persistent descriptor kernel takes every CU's LDS, so what can overlap is integral / Hessian /
    // NMS / sort / orientation of part 1).  Same kernels, same results (the GPU suite passes either way).  On the bench (A B A B, one call,
    // profiles/r05_ab_overlap.txt): 52.03 ms per step on one stream, 52.85 with the overlap -- the second stream's 5.5 ms of stages do run
    // concurrently (stage sum 57.4 ms against 52.8 ms of wall clock), but Hessian and integral slow down by what the search takes from
    // them (8.95 vs 6.85 ms, 1.25 vs 0.38 ms) and the halved launches add their tails: these kernels fill the chip on their own, a second
    // queue only re-divides it.  (Rounds 2-3 found the same for two half batches of the same mix.)  Round 6: the search beside DESCRIBE
    // instead cannot happen at all -- k_describe holds 6 x 80 of a SIMD's 512 VGPRs, a k_bf_mfma16_d64<1> wave needs 168.
    static const bool overlap_on = getenv("VFSMS_OVERLAP") && atoi(getenv("VFSMS_OVERLAP")) != 0;
    static const int overlap_pct = getenv("VFSMS_OVERLAP_PCT") ? atoi(getenv("VFSMS_OVERLAP_PCT")) : 70;
    const int n0 = (overlap_on && P.filtered && n >= 12) ? std::min(n - 2, std::max(2, n * overlap_pct / 100)) : n;
    const std::vector<int> ord = shape_order(jobs, n);       // the column strips, then the strips of the turn candidates
    StripTable T;
    TRY(build_strip_table(ctx, jobs, ord.data(), n, n0, &T));
    const int u = (int)T.strips.size(), u0 = T.u0;
    std::vector<SurfSrc> S(u);
    for (int i = 0; i < u; i++) {
        const StripTable::Strip &s = T.strips[i];
        S[i] = SurfSrc{s.p, s.stride, s.h, s.w, kp_capacity(ctx, s.h, s.w)};
    }
    std::vector<MatchJob> J(n, MatchJob{});
    for (int s_ = 0; s_ < n; s_++) {
        J[s_].capq = J[s_].capt = kp_capacity(ctx, jobs[ord[s_]].h, jobs[ord[s_]].w);
        J[s_].row = ord[s_];
        J[s_].sa = &T.strips[T.a[s_]]; J[s_].sb = &T.strips[T.b[s_]];       // the tile's pixels, not the enhanced copy
    }
    const SurfEnh enh{enh_mode, clip_limit, tile_grid};
    const MatchTail tail{TAIL_VOTE, ratio, -1, offset_evaluate};
    TRY(ctx_arena_reserve(ctx, surf_run_bytes(S.data(), u, params, enh, u0) + match_run_bytes(J.data(), n, P) + 65536));
    ctx->pinned_off = 0;
    SurfRun surf; MatchRun match;
    TRY(surf_run_carve(ctx, &surf, S.data(), u, params, enh));
    for (int s_ = 0; s_ < n; s_++) {
        const RoiDev &A = surf.R[T.a[s_]], &B = surf.R[T.b[s_]];
        J[s_].q = A.desc; J[s_].t = B.desc; J[s_].kq = A.kps_xy; J[s_].kt = B.kps_xy;
        J[s_].nq_ptr = A.counters + 1; J[s_].nt_ptr = B.counters + 1;
    }
    TRY(match_run_carve(ctx, &match, J.data(), n, dim, P));
    TRY(surf_run_prepare(ctx, &surf, enh));
    if (n0 < n) TRY(ctx_second_stream(ctx));
    TRY(surf_run_launch(ctx, surf, 0, u0, true, params));
    SecondStreamJoin join_guard(ctx);
    if (n0 < n) {
        HIP_TRY(hipEventRecord(ctx->ev_fork, ctx->stream));
        HIP_TRY(hipStreamWaitEvent(ctx->stream2, ctx->ev_fork, 0));
        join_guard.armed = true;
        {
            StreamSwap on_second(ctx, ctx->stream2);              // the launchers enqueue on ctx->stream (their profiling events too)
            TRY(match_run_launch(ctx, match, 0, n0, maxcap, maxcap, SEARCH_FLOAT, tail));
            HIP_TRY(hipEventRecord(ctx->ev_join, ctx->stream2));
        }
        TRY(surf_run_launch(ctx, surf, u0, u - u0, true, params));
        TRY(match_run_launch(ctx, match, n0, n - n0, maxcap, maxcap, SEARCH_FLOAT, tail));
        HIP_TRY(hipStreamWaitEvent(ctx->stream, ctx->ev_join, 0));
        join_guard.armed = false;                        // joined in stream order: the synchronisation below covers both streams
    } else {
        TRY(match_run_launch(ctx, match, 0, n, maxcap, maxcap, SEARCH_FLOAT, tail));
    }
    // counters of all strips and results of all jobs live in two contiguous blocks: one memset, two D2H copies, one synchronisation per batch
    TRY(surf_run_readback(ctx, &surf));
    TRY(match_run_readback(ctx, match, out));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return surf_run_check(surf, "attempt_surf", "strip", 0, u);
}

extern "C" int vfsms_attempt_surf_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                                        const vfsms_surf_params *params, double ratio, int offset_evaluate, int32_t *out)
{
    return attempt_surf_impl(ctx, jobs, n, params, ratio, offset_evaluate, 0, 0.0, 0, out);
}
extern "C" int vfsms_attempt_surf_batch_enhanced(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n, const vfsms_surf_params *params,
                                                 double ratio, int offset_evaluate, int enhance_mode, double clip_limit, int tile_grid,
                                                 int32_t *out)
{
    TRY(enhance_check_args("attempt_surf", enhance_mode, tile_grid));
    return attempt_surf_impl(ctx, jobs, n, params, ratio, offset_evaluate, enhance_mode, clip_limit, tile_grid, out);
}

// ---- enhancement (host buffers) ---------------------------------------------------------------------------------------------------
extern "C" int vfsms_enhance_u8(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, int mode, double clip_limit, int tile_grid,
                                uint8_t *out)
{
    CTX_ENTER(ctx);
    if (!img || !out || h <= 0 || w <= 0 || stride < w || mode < 1 || mode > 2) { vfsms_set_error("enhance: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(enhance_check_args("enhance", mode, tile_grid));
    TRY(ctx_arena_reserve(ctx, (size_t)h * w + enhance_scratch_bytes(h, w, mode, tile_grid) + 65536));
    ctx->pinned_off = 0;
    uint8_t *d_img;
    TRY(upload_image(ctx, img, h, w, stride, &d_img));
    EnhJob J, *dJ;
    TRY(enhance_carve(ctx, &J, d_img, w, h, w, mode, tile_grid));
    TRY(ctx_upload_small(ctx, &J, sizeof(J), (void **)&dJ));
    TRY(launch_enhance(ctx, dJ, &J, 1, mode, clip_limit, tile_grid));
    HIP_TRY(hipMemcpyAsync(out, J.dst, (size_t)h * w, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// ---- device-resident feature sets: the payload of Stitcher.tempImageFeature (Stitcher.py:14-18, 278-290) -----------------------------
// The described sources of a run leave the arena as feature sets in ONE allocation shared by the sets (a hipMalloc / hipFree pair per set
// costs more than describing it), released with the last of them (vfsms_features_free).  A set without keypoints owns nothing: block 0,
// null pointers.  The copies are only enqueued: the caller synchronises before the arena is reused.
static int feats_from_run(vfsms_ctx *ctx, const SurfRun &run, int dim, int64_t *feats, int *counts)
{
    const int m = (int)run.R.size();
    auto set_bytes = [&](int k) { return (((size_t)surf_run_count(run, k) * (2 + dim) * sizeof(float)) + 255) & ~(size_t)255; };
    size_t total = 0;
    for (int k = 0; k < m; k++) total += set_bytes(k);
    char *base = nullptr; int64_t blk = 0;
    if (total) {
        DevBuf mem;
        TRY(mem.reserve(total, ctx->stream));
        base = mem.as<char>();
        blk = ctx->next_handle++;
        ctx->feat_blocks.emplace(blk, FeatBlock{std::move(mem), 0});
    }
    size_t off = 0;
    for (int k = 0; k < m; k++) {
        FeatRec F; F.n = surf_run_count(run, k); F.dim = dim; F.kps_xy = nullptr; F.desc = nullptr;
        if (F.n > 0) {
            F.block = blk; ctx->feat_blocks.at(blk).refs++;
            F.kps_xy = (float *)(base + off); F.desc = base + off + sizeof(float) * 2 * F.n;
            off += set_bytes(k);
            HIP_TRY(hipMemcpyAsync(F.kps_xy, run.R[k].kps_xy, sizeof(float) * 2 * F.n, hipMemcpyDeviceToDevice, ctx->stream));
            HIP_TRY(hipMemcpyAsync(F.desc, run.R[k].desc, sizeof(float) * (size_t)F.n * dim, hipMemcpyDeviceToDevice, ctx->stream));
        }
        feats[k] = ctx->next_handle++;
        ctx->feats[feats[k]] = F;
        counts[k] = F.n;
    }
    return VFSMS_OK;
}

extern "C" int vfsms_features_surf(vfsms_ctx *ctx, int64_t tile, int y0, int x0, int h, int w, const vfsms_surf_params *params,
                                   int enhance_mode, double clip_limit, int tile_grid, int64_t *feat, int *n_out)
{
    CTX_ENTER(ctx);
    TileRec *pT;
    if (tile_find(ctx, "features_surf", tile, &pT) != VFSMS_OK || !params || !feat || !n_out) { vfsms_set_error("features_surf: bad arguments / unknown tile"); return VFSMS_ERR_BAD_ARG; }
    TileRec &T = *pT;
    if (T.ch != 1) { vfsms_set_error("features_surf: registration takes single-channel tiles"); return VFSMS_ERR_BAD_ARG; }
    TRY(tile_ready(ctx, T));
    if (h <= 0 || w <= 0 || y0 < 0 || x0 < 0 || y0 + h > T.h || x0 + w > T.w) { vfsms_set_error("features_surf: ROI outside the tile"); return VFSMS_ERR_BAD_ARG; }
    TRY(enhance_check_args("features_surf", enhance_mode, tile_grid));
    TRY(ctx_prepare_surf(ctx, params));
    const SurfSrc src{T.ptr + (size_t)y0 * T.stride + x0, T.stride, h, w, kp_capacity(ctx, h, w)};
    const SurfEnh enh{enhance_mode, clip_limit, tile_grid};
    TRY(ctx_arena_reserve(ctx, surf_run_bytes(&src, 1, params, enh) + 65536));
    ctx->pinned_off = 0;
    SurfRun run;
    TRY(surf_run_carve(ctx, &run, &src, 1, params, enh));
    TRY(surf_run_prepare(ctx, &run, enh));
    TRY(surf_run_launch(ctx, run, 0, 1, true, params));
    TRY(surf_run_readback(ctx, &run));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    TRY(surf_run_check(run, "features_surf", "rectangle", 0, 1));
    TRY(feats_from_run(ctx, run, params->extended ? 128 : 64, feat, n_out));
    if (*n_out > 0) HIP_TRY(hipStreamSynchronize(ctx->stream));      // the copies out of the arena have landed before the next call reuses it
    return VFSMS_OK;
}

// Whole-tile feature sets of MANY tiles in fused launches: the line scans of Main.py:29-51 (4 of the 6 demo datasets) call
// calculateOffsetForFeatureSearch pair after pair (Stitcher.py:260-304); with all tiles of a scan in HBM every tile is described once, up to
// 16 per launch sequence, and the N - 1 matches + mode votes run as one batch (vfsms_features_match_offset_batch) -- one host synchronisation
// per 16 tiles instead of two per tile.
static int features_surf_batch_impl(vfsms_ctx *ctx, const int64_t *tiles, int n, const vfsms_surf_params *params,
                                    int enhance_mode, double clip_limit, int tile_grid, int64_t *feats, int *counts);
extern "C" int vfsms_features_surf_batch(vfsms_ctx *ctx, const int64_t *tiles, int n, const vfsms_surf_params *params,
                                         int enhance_mode, double clip_limit, int tile_grid, int64_t *feats, int *counts)
{
    // the output array is cleared BEFORE anything can fail: the clean-up below frees every live handle it finds in it, and a caller's array
    // may still hold handles of an earlier call (they are the caller's; an early error -- bad arguments, unsupported parameters -- must not
    // release them)
    if (feats && n > 0) for (int k = 0; k < n; k++) feats[k] = 0;
    const int rc = features_surf_batch_impl(ctx, tiles, n, params, enhance_mode, clip_limit, tile_grid, feats, counts);
    if (rc != VFSMS_OK && ctx && feats && n > 0) {
        // an error in chunk 2 or later (e.g. VFSMS_ERR_CAPACITY): the sets of the earlier chunks never reach the caller -- release them
        // (and their shared block) here; the error text of the failure is kept
        char msg[512]; vfsms_last_error(msg, sizeof(msg));
        for (int k = 0; k < n; k++)
            if (feats[k] && ctx->feats.count(feats[k])) { vfsms_features_free(ctx, feats[k]); feats[k] = 0; }
        vfsms_set_error("%s", msg);
    }
    return rc;
}
static int features_surf_batch_impl(vfsms_ctx *ctx, const int64_t *tiles, int n, const vfsms_surf_params *params,
                                    int enhance_mode, double clip_limit, int tile_grid, int64_t *feats, int *counts)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!tiles || !feats || !counts)) || !params) { vfsms_set_error("features_surf_batch: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(enhance_check_args("features_surf_batch", enhance_mode, tile_grid));
    TRY(ctx_prepare_surf(ctx, params));
    const SurfEnh enh{enhance_mode, clip_limit, tile_grid};
    for (int k = 0; k < n; k++) feats[k] = 0;
    for (int c0 = 0; c0 < n;) {
        // a chunk: at most 16 tiles and ~6 GB of scratch
        int c1 = c0; size_t need = 0;
        std::vector<TileRec *> T; std::vector<SurfSrc> S;
        while (c1 < n && c1 - c0 < 16) {
            TileRec *pt;
            TRY(tile_find(ctx, "features_surf_batch", tiles[c1], &pt));
            TileRec &t = *pt;
            if (t.ch != 1) { vfsms_set_error("features_surf_batch: registration takes single-channel tiles"); return VFSMS_ERR_BAD_ARG; }
            const SurfSrc src{t.ptr, t.stride, t.h, t.w, kp_capacity(ctx, t.h, t.w)};
            const size_t b = surf_run_bytes(&src, 1, params, enh);
            if (c1 > c0 && need + b > ((size_t)6 << 30)) break;
            need += b; T.push_back(&t); S.push_back(src); c1++;
        }
        const int m = c1 - c0;
        TRY(ctx_arena_reserve(ctx, need + 65536));
        ctx->pinned_off = 0;
        for (int k = 0; k < m; k++) TRY(tile_ready(ctx, *T[k]));
        SurfRun run;
        TRY(surf_run_carve(ctx, &run, S.data(), m, params, enh));
        TRY(surf_run_prepare(ctx, &run, enh));
        TRY(surf_run_launch(ctx, run, 0, m, true, params));
        TRY(surf_run_readback(ctx, &run));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        TRY(surf_run_check(run, "features_surf_batch", "tile", c0, n));
        TRY(feats_from_run(ctx, run, params->extended ? 128 : 64, feats + c0, counts + c0));
        HIP_TRY(hipStreamSynchronize(ctx->stream));          // the copies out of the arena have landed before the next chunk reuses it
        c0 = c1;
    }
    return VFSMS_OK;
}

// a feature set does not own its tile's pixels, so its vote cannot be verified on the device: refuse rather than skip the check
static int features_refuse_verifier(vfsms_ctx *ctx, const char *what)
{
    if (ctx->offset_verifier == VFSMS_VERIFY_NONE) return VFSMS_OK;
    vfsms_set_error("%s: feature sets carry no pixels, so the offset verifier cannot judge their vote -- set VFSMS_VERIFY_NONE around this "
                    "call and check the offset with vfsms_verify_ncc on the two tiles", what);
    return VFSMS_ERR_UNSUPPORTED;
}

// matchDescriptors + getOffsetByMode of n (query set A_k, train set B_k) jobs as ONE batch; `who` prefixes the errors
static int features_match_impl(vfsms_ctx *ctx, const char *who, const int64_t *feat_a, const int64_t *feat_b, int n, double ratio,
                               int offset_evaluate, int32_t *out)
{
    if (n < 0 || (n && (!feat_a || !feat_b || !out))) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    TRY(features_refuse_verifier(ctx, who));
    std::vector<MatchJob> J;
    std::vector<int> live, cnt;
    int maxq = 0, maxt = 0, dim = 0;
    for (int k = 0; k < n; k++) {
        auto ia = ctx->feats.find(feat_a[k]), ib = ctx->feats.find(feat_b[k]);
        if (ia == ctx->feats.end() || ib == ctx->feats.end()) { vfsms_set_error("%s: unknown handle", who); return VFSMS_ERR_BAD_ARG; }
        const FeatRec &a = ia->second, &b = ib->second;
        if (a.dim != b.dim || (dim && a.dim != dim)) { vfsms_set_error("%s: descriptor kinds differ", who); return VFSMS_ERR_BAD_ARG; }
        dim = a.dim;
        for (int c = 0; c < VFSMS_ATTEMPT_INTS; c++) out[VFSMS_ATTEMPT_INTS * k + c] = 0;
        out[VFSMS_ATTEMPT_INTS * k + 4] = a.n; out[VFSMS_ATTEMPT_INTS * k + 5] = b.n;
        if (a.n == 0 || b.n == 0) continue;
        MatchJob j{};
        j.q = (const float *)a.desc; j.t = (const float *)b.desc; j.kq = a.kps_xy; j.kt = b.kps_xy;
        j.capq = a.n; j.capt = b.n; j.row = (int)live.size();
        J.push_back(j); live.push_back(k); cnt.push_back(a.n); cnt.push_back(b.n);
        maxq = std::max(maxq, a.n); maxt = std::max(maxt, b.n);
    }
    const int m = (int)live.size();
    if (m == 0) return VFSMS_OK;
    const MatchPlan P = match_plan_float(dim, m, maxq, maxt, maxq, maxt);       // SURF descriptors are L2-normalised by construction
    TRY(ctx_arena_reserve(ctx, match_run_bytes(J.data(), m, P) + 65536));
    TRY(match_upload_counts(ctx, J.data(), m, cnt.data()));
    MatchRun run;
    TRY(match_run_carve(ctx, &run, J.data(), m, dim, P));
    TRY(match_run_launch(ctx, run, 0, m, maxq, maxt, SEARCH_FLOAT, MatchTail{TAIL_VOTE, ratio, -1, offset_evaluate}));
    std::vector<int32_t> res((size_t)VFSMS_ATTEMPT_INTS * m);
    TRY(match_run_readback(ctx, run, res.data()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int j = 0; j < m; j++)
        for (int c = 0; c < VFSMS_ATTEMPT_INTS; c++) out[VFSMS_ATTEMPT_INTS * live[j] + c] = res[(size_t)VFSMS_ATTEMPT_INTS * j + c];
    return VFSMS_OK;
}
// out[8 * k ..] as vfsms_features_match_offset
extern "C" int vfsms_features_match_offset_batch(vfsms_ctx *ctx, const int64_t *feat_a, const int64_t *feat_b, int n, double ratio,
                                                 int offset_evaluate, int32_t *out)
{
    CTX_ENTER(ctx);
    return features_match_impl(ctx, "features_match_batch", feat_a, feat_b, n, ratio, offset_evaluate, out);
}
// matchDescriptors + getOffsetByMode on two resident sets (query = A, train = B): out[8] as in vfsms_attempt_surf_batch
extern "C" int vfsms_features_match_offset(vfsms_ctx *ctx, int64_t feat_a, int64_t feat_b, double ratio, int offset_evaluate, int32_t *out)
{
    CTX_ENTER(ctx);
    if (!ctx->feats.count(feat_a) || !ctx->feats.count(feat_b) || !out) { vfsms_set_error("features_match: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    return features_match_impl(ctx, "features_match", &feat_a, &feat_b, 1, ratio, offset_evaluate, out);
}

extern "C" int vfsms_features_free(vfsms_ctx *ctx, int64_t feat)
{
    CTX_ENTER(ctx);
    auto it = ctx->feats.find(feat);
    if (it == ctx->feats.end()) { vfsms_set_error("features_free: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    auto bt = ctx->feat_blocks.find(it->second.block);       // (a set without keypoints has no block)
    if (bt != ctx->feat_blocks.end() && --bt->second.refs == 0) {
        TRY(bt->second.base.release(ctx->stream));
        ctx->feat_blocks.erase(bt);
    }
    ctx->feats.erase(it);
    return VFSMS_OK;
}

extern "C" int vfsms_features_download(vfsms_ctx *ctx, int64_t feat, float *kps_xy, float *desc, int cap, int *n_out, int *dim_out)
{
    CTX_ENTER(ctx);
    auto it = ctx->feats.find(feat);
    if (it == ctx->feats.end() || !n_out) { vfsms_set_error("features_download: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    const FeatRec &F = it->second;
    *n_out = F.n;
    if (dim_out) *dim_out = F.dim;
    if (F.n > cap) { vfsms_set_error("features_download: %d keypoints exceed the caller's capacity %d", F.n, cap); return VFSMS_ERR_CAPACITY; }
    if (F.n > 0) {
        if (kps_xy) HIP_TRY(hipMemcpyAsync(kps_xy, F.kps_xy, sizeof(float) * 2 * F.n, hipMemcpyDeviceToHost, ctx->stream));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, F.desc, sizeof(float) * (size_t)F.n * F.dim, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return VFSMS_OK;
}

// ---- fuse ----------------------------------------------------------------------------------------------------------------------
// The four int64 operators share everything behind their own argument checks: both regions up, the fade's geometry decisions + the blend of
// `method` (fuse_i64_device: 0 fadeInAndFadeOut, 1 trigonometric, 2 multiBandBlending, 3 optimalSeamLine), the bytes (and the seam) down.
static int fuse_i64_host(vfsms_ctx *ctx, const char *what, const int64_t *A, const int64_t *B, int r, int c, int ch, int dx, int dy,
                         uint8_t *out, int32_t *info, int method, int levels, int blend, int32_t *seam_out)
{
    const size_t nel = (size_t)r * c * ch, nseam = sizeof(int32_t) * ((size_t)r + c);
    TRY(ctx_arena_reserve(ctx, nel * 17 + sizeof(float) * 4 * ((size_t)r + c) + sizeof(int) * 4 * ((size_t)r + c) + (seam_out ? nseam : 0) + 65536));
    long long *dA, *dB;
    TRY(upload_array(ctx, (const long long *)A, nel, &dA));
    TRY(upload_array(ctx, (const long long *)B, nel, &dB));
    uint8_t *d_out = (uint8_t *)ctx_arena_alloc(ctx, nel);
    int32_t *d_seam = seam_out ? (int32_t *)ctx_arena_alloc(ctx, nseam) : nullptr;
    if (!d_out || (seam_out && !d_seam)) { vfsms_set_error("%s: arena exhausted", what); return VFSMS_ERR_CAPACITY; }
    TRY(fuse_i64_device(ctx, dA, dB, r, c, ch, dx, dy, d_out, info, method, levels, blend, d_seam));
    HIP_TRY(hipMemcpyAsync(out, d_out, nel, hipMemcpyDeviceToHost, ctx->stream));
    if (seam_out) HIP_TRY(hipMemcpyAsync(seam_out, d_seam, nseam, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

extern "C" int vfsms_fuse_fade_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                                   int dx, int dy, uint8_t *out, int32_t *info)
{
    CTX_ENTER(ctx);
    if (!A || !B || !out || r <= 0 || c <= 0 || ch < 1 || ch > 4) { vfsms_set_error("fuse_i64: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    return fuse_i64_host(ctx, "fuse_i64", A, B, r, c, ch, dx, dy, out, info, 0, 4, 0, nullptr);
}

// ImageFusion.fuseByTrigonometric (ImageFusion.py:246-293) on the reference's own array representation
extern "C" int vfsms_fuse_trig_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                                   int dx, int dy, uint8_t *out, int32_t *info)
{
    CTX_ENTER(ctx);
    if (!A || !B || !out || r <= 0 || c <= 0 || ch < 1 || ch > 4) { vfsms_set_error("fuse_trig_i64: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    return fuse_i64_host(ctx, "fuse_trig_i64", A, B, r, c, ch, dx, dy, out, info, 1, 4, 0, nullptr);
}

// multiBandBlending on the reference's own array representation: the seam from the fade's geometry (degenerate corner geometries
// fail as the fade's do), then the Laplacian-pyramid blend of multiband_kernels.hip with `levels` levels
extern "C" int vfsms_fuse_multiband_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                                        int dx, int dy, int levels, uint8_t *out, int32_t *info)
{
    CTX_ENTER(ctx);
    if (!A || !B || !out || r <= 0 || c <= 0 || ch < 1 || ch > 4) { vfsms_set_error("fuse_multiband_i64: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (levels < 1 || levels > VFSMS_MB_MAX_LEVELS) { vfsms_set_error("fuse_multiband_i64: levels must be 1..%d", VFSMS_MB_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    return fuse_i64_host(ctx, "fuse_multiband_i64", A, B, r, c, ch, dx, dy, out, info, 2, levels, 0, nullptr);
}

// optimalSeamLine on the reference's own array representation: the fade's geometry decisions (degenerate corner geometries fail as the
// fade's do), then energy, seam and label of seam_kernels.hip; blend 0: every pixel from one input, 1: the label plane as the mask of the
// pyramid blend with `levels`.  seam_out (optional): r + c ints
extern "C" int vfsms_fuse_seam_i64(vfsms_ctx *ctx, const int64_t *A, const int64_t *B, int r, int c, int ch,
                                   int dx, int dy, int blend, int levels, uint8_t *out, int32_t *info, int32_t *seam_out)
{
    CTX_ENTER(ctx);
    if (!A || !B || !out || r <= 0 || c <= 0 || ch < 1 || ch > 4) { vfsms_set_error("fuse_seam_i64: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (blend < 0 || blend > 1) { vfsms_set_error("fuse_seam_i64: blend must be 0 (none) or 1 (multiBandBlending)"); return VFSMS_ERR_BAD_ARG; }
    if (blend == 1 && (levels < 1 || levels > VFSMS_MB_MAX_LEVELS)) { vfsms_set_error("fuse_seam_i64: levels must be 1..%d", VFSMS_MB_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    const int rc = fuse_i64_host(ctx, "fuse_seam_i64", A, B, r, c, ch, dx, dy, out, info, 3, levels, blend, seam_out);
    if (rc != VFSMS_OK) {                                      // a refused geometry (or a failed run): info[0] = -1, output zero, no seam
        if (info) info[0] = -1;
        memset(out, 0, (size_t)r * c * ch);
        if (seam_out) for (size_t k = 0; k < (size_t)r + c; k++) seam_out[k] = -1;
    }
    return rc;
}

int fuse_i64_ramps(vfsms_ctx *ctx, const long long *dA, int r, int c, int ch, int dx, int dy, int force_corner,
                   float *h_ramps, int32_t *info);

extern "C" int vfsms_fuse_ramps_i64(vfsms_ctx *ctx, const int64_t *A, int r, int c, int ch, int dx, int dy,
                                    int force_corner, float *ramps, int32_t *info)
{
    CTX_ENTER(ctx);
    if (!A || !ramps || r <= 0 || c <= 0 || ch < 1 || ch > 4) { vfsms_set_error("fuse_ramps: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    const size_t nel = (size_t)r * c * ch;
    TRY(ctx_arena_reserve(ctx, nel * 8 + sizeof(float) * 8 * ((size_t)r + c) + 65536));
    long long *dA;
    TRY(upload_array(ctx, (const long long *)A, nel, &dA));
    TRY(fuse_i64_ramps(ctx, dA, r, c, ch, dx, dy, force_corner, ramps, info));
    return VFSMS_OK;
}

// a canvas that enqueued work may still read, back to the device: one synchronisation, then the record's own destructor
static int canvas_release(vfsms_ctx *ctx, CanvasRec &cv)
{
    if (cv.pix) HIP_TRY(hipStreamSynchronize(ctx->stream));
    cv = CanvasRec();
    return VFSMS_OK;
}
// the buffers of a rows x cols x ch canvas (the spare's, when it is of that size) in their initial state.  Enqueue only
static int canvas_build(vfsms_ctx *ctx, CanvasRec &cv, int rows, int cols, int ch)
{
    if (ctx->spare_canvas.rows == rows && ctx->spare_canvas.cols == cols && ctx->spare_canvas.ch == ch) {
        cv = std::move(ctx->spare_canvas); ctx->spare_canvas = CanvasRec();
        cv.placed.clear(); cv.mb_levels = 4; cv.seam_blend = 0; cv.pend.levels = -1;     // same size as the canvas freed last: its buffers, re-initialised below in stream order
    } else {
        TRY(canvas_release(ctx, ctx->spare_canvas));             // a spare of another size goes first: the two never stand side by side
        cv.rows = rows; cv.cols = cols; cv.ch = ch;
        TRY(cv.pix.reserve((size_t)rows * cols * ch, ctx->stream));
        TRY(cv.mask.reserve((size_t)rows * cols, ctx->stream));
        TRY(cv.d_err.reserve(sizeof(int), ctx->stream));
        TRY(cv.scratch.reserve(canvas_scratch_bytes(rows, cols), ctx->stream));
    }
    TRY(canvas_scratch_init(ctx, &cv));
    HIP_TRY(hipMemsetAsync(cv.d_err.as<void>(), 0, sizeof(int), ctx->stream));
    HIP_TRY(hipMemsetAsync(cv.pix.as<void>(), 0, (size_t)rows * cols * ch, ctx->stream));
    HIP_TRY(hipMemsetAsync(cv.mask.as<void>(), 0, (size_t)rows * cols, ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_canvas_create(vfsms_ctx *ctx, int rows, int cols, int ch, int64_t *handle)
{
    CTX_ENTER(ctx);
    if (!handle || rows <= 0 || cols <= 0 || ch < 1 || ch > 4) { vfsms_set_error("canvas_create: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    CanvasRec cv;
    const int rc = canvas_build(ctx, cv, rows, cols, ch);
    if (rc != VFSMS_OK) {                                      // a half-built canvas goes back whole; its initialisation may be enqueued already
        hipStreamSynchronize(ctx->stream);
        return rc;
    }
    *handle = ctx->next_handle++;
    ctx->canvases.emplace(*handle, std::move(cv));
    return VFSMS_OK;
}
// the canvas behind a handle; `who`: the entry point, for the message
static int canvas_find(vfsms_ctx *ctx, const char *who, int64_t canvas, CanvasRec **cv)
{
    auto it = ctx->canvases.find(canvas);
    if (it == ctx->canvases.end()) { vfsms_set_error("%s: unknown canvas handle", who); return VFSMS_ERR_BAD_ARG; }
    *cv = &it->second;
    return VFSMS_OK;
}
extern "C" int vfsms_canvas_free(vfsms_ctx *ctx, int64_t handle)
{
    CTX_ENTER(ctx);
    CanvasRec *cv;
    TRY(canvas_find(ctx, "canvas_free", handle, &cv));
    TRY(canvas_release(ctx, ctx->spare_canvas));               // one spare at a time: the older one goes back to the device
    ctx->spare_canvas = std::move(*cv);                        // kept for a canvas of the same size (stream order makes the reuse safe)
    ctx->canvases.erase(handle);
    return VFSMS_OK;
}

// ---- one tile onto the canvas: every entry point below is translate -> check -> place (Placement: common.h) ---------------------------------
// the `method` of vfsms_canvas_fuse_tile*_m and the `mode` of vfsms_canvas_blend_tile* as the one mode code (vfsms_canvas_mode)
static int canvas_mode_of_method(int method, int *mode)
{
    static const int modes[4] = {VFSMS_CANVAS_FADE, VFSMS_CANVAS_TRIG, VFSMS_CANVAS_MULTIBAND, VFSMS_CANVAS_SEAMLINE};
    if (method < 0 || method > 3) { vfsms_set_error("canvas_fuse_tile: method must be 0 (fadeInAndFadeOut), 1 (trigonometric), 2 (multiBandBlending) or 3 (optimalSeamLine)"); return VFSMS_ERR_BAD_ARG; }
    *mode = modes[method];
    return VFSMS_OK;
}
static int canvas_mode_of_blend(int blend, int *mode)
{
    static const int modes[3] = {VFSMS_CANVAS_AVERAGE, VFSMS_CANVAS_MAXIMUM, VFSMS_CANVAS_MINIMUM};
    if (blend < 0 || blend > 2) { vfsms_set_error("canvas_blend_tile: mode must be 0 (average), 1 (maximum) or 2 (minimum)"); return VFSMS_ERR_BAD_ARG; }
    *mode = modes[blend];
    return VFSMS_OK;
}
static bool canvas_mode_fuses(int mode)        // the fade family: statistics + operator (canvas_fuse_device), with ramps in the arena's budget
{
    return mode == VFSMS_CANVAS_FADE || mode == VFSMS_CANVAS_TRIG || mode == VFSMS_CANVAS_MULTIBAND || mode == VFSMS_CANVAS_SEAMLINE;
}
// the only place a placement is judged: mode, tile rectangle inside the canvas, ROI inside the tile rectangle
static int canvas_check(const char *who, const CanvasRec *cv, const Placement &p)
{
    if (p.mode != VFSMS_CANVAS_PASTE && !canvas_mode_fuses(p.mode) &&
        p.mode != VFSMS_CANVAS_AVERAGE && p.mode != VFSMS_CANVAS_MAXIMUM && p.mode != VFSMS_CANVAS_MINIMUM) {
        vfsms_set_error("%s: mode must be -1 (paste), 0 (fadeInAndFadeOut), 1 (trigonometric), 2 / 3 / 4 (average / maximum / minimum), 6 (multiBandBlending), 7 (optimalSeamLine)", who);
        return VFSMS_ERR_BAD_ARG;
    }
    if (p.h <= 0 || p.w <= 0 || p.y0 < 0 || p.x0 < 0 || p.y0 + p.h > cv->rows || p.x0 + p.w > cv->cols) {
        vfsms_set_error("%s: tile rectangle outside the canvas", who); return VFSMS_ERR_BAD_ARG;
    }
    if (p.mode != VFSMS_CANVAS_PASTE && p.ry1 > p.ry0 && p.rx1 > p.rx0 &&
        (p.ry0 < p.y0 || p.rx0 < p.x0 || p.ry1 > p.y0 + p.h || p.rx1 > p.x0 + p.w)) {
        vfsms_set_error("%s: fuse ROI must lie inside the tile rectangle", who); return VFSMS_ERR_BAD_ARG;
    }
    return VFSMS_OK;
}
// the ramps a fuse may put into the arena, ahead of its launches (and behind a host tile's upload)
static size_t canvas_arena_bytes(const Placement &p)
{
    return (canvas_mode_fuses(p.mode) ? sizeof(float) * 8 * ((size_t)p.r() + p.c()) : 0) + 65536;
}
// a checked placement -> its launcher.  Enqueue only, unless a fuse is asked for `info`
static int canvas_place(vfsms_ctx *ctx, CanvasRec *cv, const uint8_t *d_tile, const Placement &p, int32_t *info)
{
    if (p.mode == VFSMS_CANVAS_PASTE) return canvas_paste_device(ctx, cv, d_tile, p);
    if (canvas_mode_fuses(p.mode)) return canvas_fuse_device(ctx, cv, d_tile, p, info);
    return canvas_blend_device(ctx, cv, d_tile, p);
}
// a tile from host memory: uploaded into the arena, placed, and the call returns when the canvas holds it
static int canvas_place_host(vfsms_ctx *ctx, const char *who, int64_t canvas, const uint8_t *tile, const Placement &p, int32_t *info)
{
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    if (!tile) { vfsms_set_error("%s: null tile", who); return VFSMS_ERR_BAD_ARG; }
    TRY(canvas_check(who, cv, p));
    const size_t nb = (size_t)p.h * p.w * cv->ch;
    TRY(ctx_arena_reserve(ctx, nb + canvas_arena_bytes(p)));
    uint8_t *d_tile;
    TRY(upload_array(ctx, tile, nb, &d_tile));
    TRY(canvas_place(ctx, cv, d_tile, p, info));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
// a resident tile of the canvas's channel count: known, handed over (tile_ready) and densely packed; its shape completes the placement
static int canvas_resident_tile(vfsms_ctx *ctx, const char *who, const CanvasRec *cv, int64_t tile, Placement *p, const uint8_t **d_tile)
{
    TileRec *pt;
    TRY(tile_find(ctx, who, tile, &pt));
    TileRec &tr = *pt;
    TRY(tile_ready(ctx, tr));
    if (cv->ch != tr.ch || tr.stride != tr.w * tr.ch) {
        vfsms_set_error("%s: a resident tile must have the canvas's channel count and be densely packed (stride == w * ch)", who); return VFSMS_ERR_BAD_ARG;
    }
    p->h = tr.h; p->w = tr.w; *d_tile = tr.ptr;
    return VFSMS_OK;
}
// enqueued only (resident tiles need no host synchronisation; stream order keeps the canvas consistent), unless `info` is read back
static int canvas_place_resident(vfsms_ctx *ctx, const char *who, int64_t canvas, int64_t tile, Placement p, int32_t *info)
{
    CanvasRec *cv; const uint8_t *d_tile;
    TRY(canvas_find(ctx, who, canvas, &cv));
    TRY(canvas_resident_tile(ctx, who, cv, tile, &p, &d_tile));
    TRY(canvas_check(who, cv, p));
    if (canvas_mode_fuses(p.mode)) TRY(ctx_arena_reserve(ctx, canvas_arena_bytes(p)));
    TRY(canvas_place(ctx, cv, d_tile, p, info));
    if (info) HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

extern "C" int vfsms_canvas_paste(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w, int y0, int x0)
{
    CTX_ENTER(ctx);
    return canvas_place_host(ctx, "canvas_paste", canvas, tile, Placement{h, w, y0, x0, 0, 0, 0, 0, 0, 0, VFSMS_CANVAS_PASTE}, nullptr);
}
extern "C" int vfsms_canvas_fuse_tile_m(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                                        int y0, int x0, int ry0, int rx0, int ry1, int rx1, int dx, int dy, int method, int32_t *info)
{
    CTX_ENTER(ctx);
    int mode;
    TRY(canvas_mode_of_method(method, &mode));
    return canvas_place_host(ctx, "canvas_fuse_tile", canvas, tile, Placement{h, w, y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode}, info);
}
extern "C" int vfsms_canvas_fuse_tile(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                                      int y0, int x0, int ry0, int rx0, int ry1, int rx1, int dx, int dy, int32_t *info)
{
    return vfsms_canvas_fuse_tile_m(ctx, canvas, tile, h, w, y0, x0, ry0, rx0, ry1, rx1, dx, dy, 0, info);
}
extern "C" int vfsms_canvas_blend_tile(vfsms_ctx *ctx, int64_t canvas, const uint8_t *tile, int h, int w,
                                       int y0, int x0, int ry0, int rx0, int ry1, int rx1, int mode)
{
    CTX_ENTER(ctx);
    TRY(canvas_mode_of_blend(mode, &mode));
    return canvas_place_host(ctx, "canvas_blend_tile", canvas, tile, Placement{h, w, y0, x0, ry0, rx0, ry1, rx1, 0, 0, mode}, nullptr);
}
extern "C" int vfsms_canvas_paste_tile(vfsms_ctx *ctx, int64_t canvas, int64_t tile, int y0, int x0)
{
    CTX_ENTER(ctx);
    return canvas_place_resident(ctx, "canvas_paste_tile", canvas, tile, Placement{0, 0, y0, x0, 0, 0, 0, 0, 0, 0, VFSMS_CANVAS_PASTE}, nullptr);
}
extern "C" int vfsms_canvas_fuse_tile_resident_m(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                                 int y0, int x0, int ry0, int rx0, int ry1, int rx1, int dx, int dy, int method, int32_t *info)
{
    CTX_ENTER(ctx);
    int mode;
    TRY(canvas_mode_of_method(method, &mode));
    return canvas_place_resident(ctx, "canvas_fuse_tile", canvas, tile, Placement{0, 0, y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode}, info);
}
// fuseMethod "average" / "maximum" / "minimum" (mode 0 / 1 / 2) with a resident tile
extern "C" int vfsms_canvas_blend_tile_resident(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                                int y0, int x0, int ry0, int rx0, int ry1, int rx1, int mode)
{
    CTX_ENTER(ctx);
    TRY(canvas_mode_of_blend(mode, &mode));
    return canvas_place_resident(ctx, "canvas_blend_tile", canvas, tile, Placement{0, 0, y0, x0, ry0, rx0, ry1, rx1, 0, 0, mode}, nullptr);
}
extern "C" int vfsms_canvas_fuse_tile_resident(vfsms_ctx *ctx, int64_t canvas, int64_t tile,
                                               int y0, int x0, int ry0, int rx0, int ry1, int rx1, int dx, int dy, int32_t *info)
{
    return vfsms_canvas_fuse_tile_resident_m(ctx, canvas, tile, y0, x0, ry0, rx0, ry1, rx1, dx, dy, 0, info);
}
// The whole mosaic walk of Stitcher.getStitchByOffset (Stitcher.py:434-483) over resident tiles as ONE call: per tile the nine ints
// [y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode] of a Placement, mode a vfsms_canvas_mode.
// Enqueue only (one library call per mosaic instead of one per tile; the device chain stays two launches per tile); geometry errors are latched
// in the canvas and reported by the download, as with vfsms_canvas_fuse_tile_resident(info = NULL).
extern "C" int vfsms_canvas_assemble_resident(vfsms_ctx *ctx, int64_t canvas, int n, const int64_t *tiles, const int32_t *geom)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_assemble_resident";
    if (n < 0 || (n > 0 && (!tiles || !geom))) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    struct Row { Placement p; const uint8_t *d_tile; };
    std::vector<Row> rows(n);
    for (int i = 0; i < n; i++) {                       // everything is checked before anything is enqueued
        const int32_t *g = geom + 9 * (size_t)i;
        rows[i].p = Placement{0, 0, g[0], g[1], g[2], g[3], g[4], g[5], g[6], g[7], g[8]};
        TRY(canvas_resident_tile(ctx, who, cv, tiles[i], &rows[i].p, &rows[i].d_tile));
        TRY(canvas_check(who, cv, rows[i].p));
    }
    for (const Row &row : rows) {
        if (canvas_mode_fuses(row.p.mode)) TRY(ctx_arena_reserve(ctx, canvas_arena_bytes(row.p)));
        TRY(canvas_place(ctx, cv, row.d_tile, row.p, nullptr));
    }
    return VFSMS_OK;
}
// the level count of the canvas's multiBandBlending fuses; a new canvas starts at 4
extern "C" int vfsms_canvas_set_multiband_levels(vfsms_ctx *ctx, int64_t canvas, int levels)
{
    CTX_ENTER(ctx);
    CanvasRec *cv;
    TRY(canvas_find(ctx, "canvas_set_multiband_levels", canvas, &cv));
    if (levels < 1 || levels > VFSMS_MB_MAX_LEVELS) { vfsms_set_error("canvas_set_multiband_levels: levels must be 1..%d", VFSMS_MB_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    cv->mb_levels = levels;
    return VFSMS_OK;
}
// how the canvas's optimalSeamLine fuses merge the two sides of the seam: 0 none (every pixel from one input),
// 1 multiBandBlending with the canvas's level count; a new canvas starts at 0
extern "C" int vfsms_canvas_set_seam_blend(vfsms_ctx *ctx, int64_t canvas, int blend)
{
    CTX_ENTER(ctx);
    CanvasRec *cv;
    TRY(canvas_find(ctx, "canvas_set_seam_blend", canvas, &cv));
    if (blend < 0 || blend > 1) { vfsms_set_error("canvas_set_seam_blend: blend must be 0 (none) or 1 (multiBandBlending)"); return VFSMS_ERR_BAD_ARG; }
    cv->seam_blend = blend;
    return VFSMS_OK;
}
// rows [row0, row0 + nrows) of the canvas to the host, with the sticky error flag of the fuses that ran without a readback.  Never-written
// pixels are still 0 (the canvas is zero-initialised), exactly Stitcher.py:485
static int canvas_read_rows(vfsms_ctx *ctx, const CanvasRec *cv, int row0, int nrows, uint8_t *out)
{
    const size_t pitch = (size_t)cv->cols * cv->ch;
    int flag = 0;
    TRY(canvas_flag_read(ctx, cv, &flag));
    if (nrows > 0) HIP_TRY(hipMemcpyAsync(out, cv->pix.as<uint8_t>() + (size_t)row0 * pitch, (size_t)nrows * pitch, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return canvas_flag_verdict(flag);
}
extern "C" int vfsms_canvas_download(vfsms_ctx *ctx, int64_t canvas, uint8_t *out)
{
    CTX_ENTER(ctx);
    CanvasRec *cv;
    TRY(canvas_find(ctx, "canvas_download", canvas, &cv));
    if (!out) { vfsms_set_error("canvas_download: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    return canvas_read_rows(ctx, cv, 0, cv->rows, out);
}

// rows [row0, row0 + nrows) of the canvas: a multi-GB mosaic leaves the device band by band (streamed write-out, Stitcher.py:174-179)
extern "C" int vfsms_canvas_download_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, uint8_t *out)
{
    CTX_ENTER(ctx);
    CanvasRec *cv;
    TRY(canvas_find(ctx, "canvas_download_rows", canvas, &cv));
    TRY(canvas_band_check("canvas_download_rows", out != nullptr, cv->rows, row0, nrows, {}));
    return canvas_read_rows(ctx, cv, row0, nrows, out);
}

// the same rows (out0 may be NULL) and levels 1 .. `levels` of them (pyramid_kernels.hip, specified by tests/pyramid_ref.py) back to back in
// out_levels: what a pyramidal writer needs of a band, with the canvas bytes read from HBM once and one synchronisation at the end.  The
// band must produce complete level rows that depend on no other band: it starts at a multiple of 2^levels and is a multiple of 2^levels
// rows long unless it ends at the last row
extern "C" int vfsms_canvas_download_rows_pyramid(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels,
                                                  uint8_t *out0, uint8_t *out_levels, size_t cap_levels)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_download_rows_pyramid";
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    if (levels < 1 || levels > VFSMS_PYRAMID_MAX_LEVELS) { vfsms_set_error("%s: levels must be 1..%d", who, VFSMS_PYRAMID_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    TRY(canvas_band_check(who, out_levels != nullptr, cv->rows, row0, nrows, {{1 << levels, "2^levels"}}));
    const size_t need = pyramid_band_bytes(cv->rows, cv->cols, cv->ch, row0, nrows, levels);
    if (cap_levels < need) { vfsms_set_error("%s: the levels take %zu bytes, out_levels holds %zu", who, need, cap_levels); return VFSMS_ERR_BAD_ARG; }
    TRY(cv->pyr.reserve(need, ctx->stream));                    // first use, or a larger band than before
    TRY(pyramid_band_device(ctx, cv, row0, nrows, levels, cv->pyr.as<uint8_t>()));
    HIP_TRY(hipMemcpyAsync(out_levels, cv->pyr.as<uint8_t>(), need, hipMemcpyDeviceToHost, ctx->stream));
    if (out0) return canvas_read_rows(ctx, cv, row0, nrows, out0);
    return canvas_read_rows(ctx, cv, 0, 0, nullptr);             // (the sticky flag and the synchronisation alone)
}

// ---- the JPEG encoder on the device (Method.jpegEncoder = "device"; jpeg_enc_kernels.hip, specified by tests/jpeg_enc_ref.py) ------------
// The entropy-coded bytes of rows [row0, row0 + nrows) of the canvas -- never-written pixels are 0, as canvas_read_rows defines the image --
// with an RSTn behind every restart interval but the image's last.  The band contract: row0 is a multiple of the MCU height (16 colour, 8
// gray); the MCUs in front of the band are a multiple of the interval, and so are the band's own unless it ends at the last row.  Then the
// bytes of all bands behind vfsms_jpeg_header and in front of FF D9 are the file.  *nbytes = the size, also on VFSMS_ERR_CAPACITY
extern "C" int vfsms_canvas_encode_jpeg_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int quality, int restart_mcus,
                                             uint8_t *out, size_t cap, size_t *nbytes)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_encode_jpeg_rows";
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    TRY(canvas_band_check(who, nbytes != nullptr, cv->rows, row0, nrows, {}));     // (MCU rows and restart intervals have texts of their own, below)
    int interval = 0;
    TRY(jpeg_check_geometry(who, cv->rows, cv->cols, cv->ch, quality, restart_mcus, &interval));
    const int mcu = cv->ch == 3 ? 16 : 8, mw = (cv->cols + mcu - 1) / mcu;
    const bool last = row0 + nrows == cv->rows;
    if (row0 % mcu || (!last && nrows % mcu)) { vfsms_set_error("%s: rows [%d, %d) do not start and end on MCU rows of %d", who, row0, row0 + nrows, mcu); return VFSMS_ERR_BAD_ARG; }
    if (((long long)(row0 / mcu) * mw) % interval || (!last && ((long long)(nrows / mcu) * mw) % interval)) {
        vfsms_set_error("%s: rows [%d, %d) of %d MCUs each are not whole restart intervals of %d MCUs", who, row0, row0 + nrows, mw, interval);
        return VFSMS_ERR_BAD_ARG;
    }
    int flag = 0;                                                  // the sticky geometry flag, as vfsms_canvas_download_rows reads it
    TRY(canvas_flag_read(ctx, cv, &flag));
    TRY(jpeg_encode_band_device(ctx, &cv->jpeg, cv->pix.as<uint8_t>(), cv->rows, cv->cols, cv->ch, (size_t)cv->cols * cv->ch, 1, row0, nrows, quality, interval, out, cap, nbytes));
    return canvas_flag_verdict(flag);
}

// the caller's h x w x ch image (rows `stride` bytes apart), densely packed in the context's staging buffer (ctx->jpeg_scratch.img, whichever
// coder reads it): enqueued; *pitch = a row's bytes
static int stage_host_image(vfsms_ctx *ctx, const char *who, const uint8_t *img, int h, int w, int ch, int stride, size_t *pitch)
{
    if ((long long)stride < (long long)w * ch) { vfsms_set_error("%s: stride %d is less than a row's %lld bytes", who, stride, (long long)w * ch); return VFSMS_ERR_BAD_ARG; }
    *pitch = (size_t)w * ch;
    TRY(ctx->jpeg_scratch.img.reserve(*pitch * h, ctx->stream));
    HIP_TRY(hipMemcpy2DAsync(ctx->jpeg_scratch.img.as<void>(), *pitch, img, (size_t)stride, *pitch, (size_t)h, hipMemcpyHostToDevice, ctx->stream));
    return VFSMS_OK;
}

// A whole image on the host (1 channel, or 3: B G R with bgr != 0, else R G B; rows `stride` bytes apart) -> a complete file, the bytes of
// tests/jpeg_enc_ref.py's encode().  *nbytes = the size, also on VFSMS_ERR_CAPACITY
extern "C" int vfsms_jpeg_encode_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int quality, int restart_mcus,
                                        uint8_t *out, size_t cap, size_t *nbytes)
{
    CTX_ENTER(ctx);
    const char *who = "jpeg_encode_device";
    if (!img || !nbytes) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    int interval = 0;
    TRY(jpeg_check_geometry(who, h, w, ch, quality, restart_mcus, &interval));
    JpegScratch *s = &ctx->jpeg_scratch;
    size_t pitch = 0, hn = 0, bn = 0;
    TRY(stage_host_image(ctx, who, img, h, w, ch, stride, &pitch));
    TRY(vfsms_jpeg_header(h, w, ch, quality, restart_mcus, out, out ? cap : 0, &hn) == VFSMS_ERR_BAD_ARG ? VFSMS_ERR_BAD_ARG : VFSMS_OK);
    const bool room = out && cap > hn + 2;
    const int rc = jpeg_encode_band_device(ctx, s, s->img.as<uint8_t>(), h, w, ch, pitch, bgr != 0, 0, h, quality, interval, room ? out + hn : nullptr, room ? cap - hn - 2 : 0, &bn);
    *nbytes = hn + bn + 2;
    if (rc != VFSMS_OK) return rc;
    out[hn + bn] = 0xFF; out[hn + bn + 1] = 0xD9;
    return VFSMS_OK;
}

// ---- the two tile coders of pyramidal TIFF: the Coder of canvas_tile_band (canvas_band.h) and of the image-order operator below, over one
// scratch; limit: what one call takes of an image
struct JpegTileCoder {
    static constexpr int codec = VFSMS_PYR_CODEC_JPEG;
    vfsms_ctx *ctx; JpegScratch *s; int ch, bgr, tile, quality, restart_mcus, interval; JpegTilesRun run;
    int limit(const char *who, int h, long long tr, long long) const { if (tr * (tile / 8) > 65535) { vfsms_set_error("%s: %d rows are more tile rows than one call takes", who, h); return VFSMS_ERR_BAD_ARG; } return VFSMS_OK; }
    int count(const JpegTileJob *jobs, int n_jobs, const int *d_flag, int *flag) { return jpeg_tiles_count_device(ctx, s, jobs, n_jobs, ch, bgr, tile, quality, restart_mcus, interval, d_flag, flag, &run); }
    int write(uint8_t *out) { return jpeg_tiles_write_device(ctx, s, &run, out); }
};
struct DeflateTileCoder {
    static constexpr int codec = VFSMS_PYR_CODEC_DEFLATE;
    vfsms_ctx *ctx; DeflateScratch *s; int ch, bgr, tile; DeflateTilesRun run;
    int limit(const char *who, int, long long, long long n_tiles) const { if (n_tiles > 0x7fffffff) { vfsms_set_error("%s: %lld tiles are more than one call takes", who, n_tiles); return VFSMS_ERR_BAD_ARG; } return VFSMS_OK; }
    int count(const JpegTileJob *jobs, int n_jobs, const int *d_flag, int *flag) { return deflate_tiles_count_device(ctx, s, jobs, n_jobs, ch, bgr, tile, d_flag, flag, &run); }
    int write(uint8_t *out) { return deflate_tiles_write_device(ctx, s, &run, out); }
};
// the image-order operator behind vfsms_jpeg_encode_tiles_device and vfsms_deflate_encode_tiles_device, which have checked their pointers and
// the coder's geometry: the image staged, one job, count, capacity (nothing is written then), write, the offsets
template <class Coder>
static int encode_tiles_image(vfsms_ctx *ctx, const char *who, Coder &coder, const uint8_t *img, int h, int w, int stride,
                              uint8_t *out, size_t cap, size_t *nbytes, uint64_t *offsets, int offsets_cap)
{
    const long long tr = (h + coder.tile - 1) / coder.tile, n_tiles = tr * ((w + coder.tile - 1) / coder.tile);
    TRY(coder.limit(who, h, tr, n_tiles));
    if (offsets_cap < n_tiles + 1) { vfsms_set_error("%s: %lld tiles need %lld offsets, `offsets` holds %d", who, n_tiles, n_tiles + 1, offsets_cap); return VFSMS_ERR_BAD_ARG; }
    size_t pitch = 0;
    TRY(stage_host_image(ctx, who, img, h, w, coder.ch, stride, &pitch));
    const JpegTileJob job = {ctx->jpeg_scratch.img.as<uint8_t>(), pitch * h, pitch, 0, h, w, 0, (int)tr};
    TRY(coder.count(&job, 1, nullptr, nullptr));
    const unsigned long long total = coder.run.tile_offs[(size_t)n_tiles];
    *nbytes = (size_t)total;
    if (!out || cap < total) { vfsms_set_error("%s: the tiles take %llu bytes, the buffer holds %zu", who, total, out ? cap : (size_t)0); return VFSMS_ERR_CAPACITY; }
    TRY(coder.write(out));
    for (long long t = 0; t <= n_tiles; t++) offsets[t] = coder.run.tile_offs[(size_t)t];
    return VFSMS_OK;
}

// ---- JPEG tiles for pyramidal TIFF (Method.pyramidCompression = "jpeg"; jpeg_enc_kernels.hip in tile order, specified by tests/tiff_jpeg_ref.py) --
// A whole image on the host -> the abbreviated streams of its tile x tile tiles (SOI, SOF0, DRI, SOS, scan, EOI; the tables are
// vfsms_tiff_jpeg_tables'), row-major and back to back in `out`; offsets[0 .. n_tiles]: where every stream starts, the last being the total.
// Samples beyond the last row or column repeat it.  *nbytes = the size needed, also on VFSMS_ERR_CAPACITY (nothing is written then)
extern "C" int vfsms_jpeg_encode_tiles_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int tile, int quality,
                                              int restart_mcus, uint8_t *out, size_t cap, size_t *nbytes, uint64_t *offsets, int offsets_cap)
{
    CTX_ENTER(ctx);
    const char *who = "jpeg_encode_tiles_device";
    if (!img || !nbytes || !offsets || h < 1 || w < 1) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    int interval = 0;
    TRY(jpeg_check_tile_geometry(who, tile, ch, quality, restart_mcus, &interval));
    JpegTileCoder coder{ctx, &ctx->jpeg_scratch, ch, bgr != 0, tile, quality, restart_mcus, interval, {}};
    return encode_tiles_image(ctx, who, coder, img, h, w, stride, out, cap, nbytes, offsets, offsets_cap);
}

// Every tile row of level 0 and of levels 1 .. levels that the band [row0, row0 + nrows) of the canvas COMPLETES, as finished tile streams
// back to back in `out`, with int64 records {level, tile number in the level (row-major), offset in `out`, bytes} in `index` in that order:
// level after level, a level's tiles row-major.  The band contract: vfsms_canvas_download_rows_pyramid's (levels may be 0 here), row0 a
// multiple of the tile, nrows a multiple of the tile unless the band ends at the last row, bands in order from row 0 with one tile and level
// count.  The rows of a reduced level that do not fill a tile row yet wait in the canvas record on the device (PyrPending) for the
// bands that complete it; the last band flushes them.  Nothing of the reduced levels crosses the link as pixels.  One counting pass, one
// scan, one writing pass and one copy over all levels together; the sizes come back in one synchronisation, the payload in the one that
// ends the call.  *nbytes, *n_index = the sizes needed, also on VFSMS_ERR_CAPACITY (nothing is written and no row is consumed then: the
// call may be repeated).  The sticky geometry flag as vfsms_canvas_download_rows
extern "C" int vfsms_canvas_encode_pyramid_tiles(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels, int tile, int quality, int restart_mcus,
                                                 uint8_t *out, size_t cap, size_t *nbytes, int64_t *index, int index_cap, int *n_index)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_encode_pyramid_tiles";
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    if (levels < 0 || levels > VFSMS_PYRAMID_MAX_LEVELS) { vfsms_set_error("%s: levels must be 0..%d", who, VFSMS_PYRAMID_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    int interval = 0;
    TRY(jpeg_check_tile_geometry(who, tile, cv->ch, quality, restart_mcus, &interval));
    TRY(canvas_band_check(who, nbytes && n_index, cv->rows, row0, nrows, {{1 << levels, "2^levels"}, {tile, "the tile"}}));
    JpegTileCoder coder{ctx, &cv->jpeg, cv->ch, 1, tile, quality, restart_mcus, interval, {}};
    const auto reduce = [&](uint8_t *const *lvl) { return pyramid_band_device_at(ctx, cv, row0, nrows, levels, lvl, "pyramid_jpeg.levels"); };
    return canvas_tile_band(ctx, cv, who, row0, nrows, levels, tile, coder, reduce, out, cap, nbytes, index, index_cap, n_index);
}

// ---- lossless tiles for pyramidal TIFF (Method.pyramidCompression = "deflate-device"; deflate_kernels.hip, specified by tests/deflate_ref.py) ------
// A whole image on the host -> the zlib streams of its tile x tile tiles (TIFF predictor 2, then deflate restricted to runs at distance 1 and
// one dynamic block a tile), row-major and back to back in `out`; offsets[0 .. n_tiles]: where every stream starts, the last being the total.
// Colour is stored R G B (bgr != 0: the rows are B G R).  Samples beyond the last row or column are 0.  *nbytes = the size needed, also on
// VFSMS_ERR_CAPACITY (nothing is written then)
extern "C" int vfsms_deflate_encode_tiles_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int tile,
                                                 uint8_t *out, size_t cap, size_t *nbytes, uint64_t *offsets, int offsets_cap)
{
    CTX_ENTER(ctx);
    const char *who = "deflate_encode_tiles_device";
    if (!img || !nbytes || !offsets || h < 1 || w < 1) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    TRY(deflate_check_tile_geometry(who, tile, ch));
    DeflateTileCoder coder{ctx, &ctx->deflate_scratch, ch, bgr != 0, tile, {}};
    return encode_tiles_image(ctx, who, coder, img, h, w, stride, out, cap, nbytes, offsets, offsets_cap);
}

// vfsms_canvas_encode_pyramid_tiles with the lossless coder: the same band contract, index records and capacity behaviour (on
// VFSMS_ERR_CAPACITY nothing is consumed and the band may be repeated), over the same walk of the canvas's pending rows.  A walk belongs to
// the coder that started it at row0 = 0: a band of this entry that continues a walk of the JPEG entry -- or the reverse -- is refused with
// VFSMS_ERR_BAD_ARG and the walk stays as it was.  The canvas is B G R; the tiles are stored R G B, zero beyond a level's last row and column
extern "C" int vfsms_canvas_encode_pyramid_tiles_deflate(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int levels, int tile,
                                                         uint8_t *out, size_t cap, size_t *nbytes, int64_t *index, int index_cap, int *n_index)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_encode_pyramid_tiles_deflate";
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    if (levels < 0 || levels > VFSMS_PYRAMID_MAX_LEVELS) { vfsms_set_error("%s: levels must be 0..%d", who, VFSMS_PYRAMID_MAX_LEVELS); return VFSMS_ERR_BAD_ARG; }
    TRY(deflate_check_tile_geometry(who, tile, cv->ch));
    TRY(canvas_band_check(who, nbytes && n_index, cv->rows, row0, nrows, {{1 << levels, "2^levels"}, {tile, "the tile"}}));
    DeflateTileCoder coder{ctx, &cv->deflate, cv->ch, 1, tile, {}};
    const auto reduce = [&](uint8_t *const *lvl) { return pyramid_band_device_at(ctx, cv, row0, nrows, levels, lvl, "pyramid_deflate.levels"); };
    return canvas_tile_band(ctx, cv, who, row0, nrows, levels, tile, coder, reduce, out, cap, nbytes, index, index_cap, n_index);
}

// ---- PNG coded on the device (Method.pngEncoder = "device"; deflate_kernels.hip over deflate_kernels.hip's passes, specified by tests/png_ref.py) ------
// A whole image on the host (B G R with bgr != 0, else R G B; rows `stride` bytes apart) -> the IDAT chunks of its segments of `segment_rows`
// rows, back to back, CRC-32 included, and the Adler-32 of its filtered bytes: behind the signature, IHDR and IDAT(78 01) and in front of the
// closing IDAT and IEND they are the file.  *nbytes = the size needed, also on VFSMS_ERR_CAPACITY (nothing is written then)
extern "C" int vfsms_png_encode_device(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int ch, int stride, int bgr, int segment_rows,
                                       uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler)
{
    CTX_ENTER(ctx);
    const char *who = "png_encode_device";
    if (!img || !nbytes || !adler) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    TRY(png_check_geometry(who, segment_rows, h, w, ch));
    size_t pitch = 0;
    TRY(stage_host_image(ctx, who, img, h, w, ch, stride, &pitch));
    return png_encode_band_device(ctx, &ctx->deflate_scratch, ctx->jpeg_scratch.img.as<uint8_t>(), h, w, ch, pitch, bgr != 0, 0, h, segment_rows, out, cap, nbytes, adler, nullptr, nullptr);
}

// Rows [row0, row0 + nrows) of the canvas -- never-written pixels are 0, as canvas_read_rows defines the image -- coded the same way; *adler is
// the band's own Adler-32.  The band contract: row0 a multiple of segment_rows, nrows too unless the band ends at the last row.  The entry keeps
// no state between bands: the row above row0 is read from the canvas, so any band may be asked for, again and in any order, and no pyramid
// walk in progress is disturbed.  The sticky geometry flag as vfsms_canvas_download_rows
extern "C" int vfsms_canvas_encode_png_rows(vfsms_ctx *ctx, int64_t canvas, int row0, int nrows, int segment_rows,
                                            uint8_t *out, size_t cap, size_t *nbytes, uint32_t *adler)
{
    CTX_ENTER(ctx);
    const char *who = "canvas_encode_png_rows";
    CanvasRec *cv;
    TRY(canvas_find(ctx, who, canvas, &cv));
    TRY(png_check_geometry(who, segment_rows, cv->rows, cv->cols, cv->ch));
    TRY(canvas_band_check(who, nbytes && adler, cv->rows, row0, nrows, {{segment_rows, "segment_rows"}}));
    int flag = 0;                                                  // the sticky geometry flag comes back with the sizes
    const int rc = png_encode_band_device(ctx, &cv->deflate, cv->pix.as<uint8_t>(), cv->rows, cv->cols, cv->ch, (size_t)cv->cols * cv->ch, 1, row0, nrows, segment_rows,
                                          out, cap, nbytes, adler, cv->d_err.as<int>(), &flag);
    if (rc != VFSMS_OK && rc != VFSMS_ERR_CAPACITY) return rc;
    TRY(canvas_flag_verdict(flag));
    return rc;
}

// ---- shading correction (Method.shadingCorrection; shading_kernels.hip, specified by tests/shading_ref.py) ----------------------------
// what the calls that take a list of tiles ask of it (TileRule, tile_table.h: count, noun, gray or B G R, one shape, rewritten)
static const TileRule SHADE_READ{1, VFSMS_SHADE_MAX_TILES, false, "tile", false, true, false, nullptr};
static const TileRule SHADE_REWRITE{1, VFSMS_SHADE_MAX_TILES, false, "tile", false, true, true, nullptr};
static const TileRule ANY_REWRITE{1, VFSMS_SHADE_MAX_TILES, false, "tile", false, false, true, nullptr};
static const TileRule FOCUS_STACK{VFSMS_FOCUS_MIN_PLANES, VFSMS_FOCUS_MAX_PLANES, true, "plane", true, true, false, nullptr};
static const TileRule FOCUS_SCORES{1, VFSMS_FOCUS_MAX_TILES, true, "tile", true, false, false, nullptr};
static int shade_field_new(vfsms_ctx *ctx, int h, int w, int ch, bool estimated, ShadeRec *F)
{
    const size_t P = (size_t)h * w * ch, Pa = (P + 127) & ~(size_t)127;      // the three planes stay 256-byte aligned
    F->h = h; F->w = w; F->ch = ch; F->estimated = estimated; F->q8 = nullptr; F->prof = nullptr;
    TRY(F->gain.reserve(estimated ? Pa * 5 : Pa * 2, ctx->stream));
    if (estimated) { F->q8 = F->gain.as<uint16_t>() + Pa; F->prof = (uint8_t *)(F->q8 + Pa); }
    return VFSMS_OK;
}
extern "C" int vfsms_shading_estimate(vfsms_ctx *ctx, int n, const int64_t *tiles, int percentile, int radius, int64_t *field)
{
    CTX_ENTER(ctx);
    if (!field || percentile < 0 || percentile > 100 || radius < 1 || radius > VFSMS_SHADE_MAX_RADIUS) {
        vfsms_set_error("shading_estimate: percentile %d / radius %d (0..100; 1..%d)", percentile, radius, VFSMS_SHADE_MAX_RADIUS);
        return VFSMS_ERR_BAD_ARG;
    }
    std::vector<TileView> H;
    TRY(tile_list(ctx, "shading_estimate", SHADE_READ, tiles, n, H));
    TRY(ctx_arena_reserve(ctx, sizeof(TileView) * 2 * (size_t)n + 65536));
    ctx->pinned_off = 0;
    ShadeRec F;
    TRY(shade_field_new(ctx, H[0].h, H[0].w, H[0].ch, true, &F));
    int rc = shade_estimate_device(ctx, H.data(), n, F.h, F.w, F.ch, percentile, radius, F.gain.as<uint16_t>(), F.q8, F.prof);
    if (rc == VFSMS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { vfsms_set_error("shading_estimate: the kernels failed"); rc = VFSMS_ERR_HIP; }
    if (rc != VFSMS_OK) { hipStreamSynchronize(ctx->stream); return rc; }      // (the field goes with F; nothing enqueued may still write it)
    *field = ctx->next_handle++;
    ctx->shade_fields.emplace(*field, std::move(F));
    return VFSMS_OK;
}
extern "C" int vfsms_shading_from_gain(vfsms_ctx *ctx, const uint16_t *gain, int h, int w, int ch, int64_t *field)
{
    CTX_ENTER(ctx);
    if (!gain || !field || h <= 0 || w <= 0 || ch < 1 || ch > 4) { vfsms_set_error("shading_from_gain: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    ShadeRec F;
    TRY(shade_field_new(ctx, h, w, ch, false, &F));
    if (hipMemcpy(F.gain.as<void>(), gain, sizeof(uint16_t) * (size_t)h * w * ch, hipMemcpyHostToDevice) != hipSuccess) {
        vfsms_set_error("shading_from_gain: the upload failed"); return VFSMS_ERR_HIP;
    }
    *field = ctx->next_handle++;
    ctx->shade_fields.emplace(*field, std::move(F));
    return VFSMS_OK;
}
extern "C" int vfsms_shading_download(vfsms_ctx *ctx, int64_t field, uint16_t *gain, uint16_t *smooth_q8, uint8_t *profile)
{
    CTX_ENTER(ctx);
    auto it = ctx->shade_fields.find(field);
    if (it == ctx->shade_fields.end()) { vfsms_set_error("shading_download: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    if (!gain) { vfsms_set_error("shading_download: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    const ShadeRec &F = it->second;
    const size_t P = (size_t)F.h * F.w * F.ch;
    HIP_TRY(hipMemcpyAsync(gain, F.gain.as<uint16_t>(), sizeof(uint16_t) * P, hipMemcpyDeviceToHost, ctx->stream));
    if (smooth_q8) { if (F.estimated) HIP_TRY(hipMemcpyAsync(smooth_q8, F.q8, sizeof(uint16_t) * P, hipMemcpyDeviceToHost, ctx->stream)); else memset(smooth_q8, 0, sizeof(uint16_t) * P); }
    if (profile) { if (F.estimated) HIP_TRY(hipMemcpyAsync(profile, F.prof, P, hipMemcpyDeviceToHost, ctx->stream)); else memset(profile, 0, P); }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_shading_apply(vfsms_ctx *ctx, int64_t field, int n, const int64_t *tiles)
{
    CTX_ENTER(ctx);
    auto it = ctx->shade_fields.find(field);
    if (it == ctx->shade_fields.end()) { vfsms_set_error("shading_apply: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    const ShadeRec &F = it->second;
    TileRule rule = SHADE_REWRITE;
    rule.pred = [&F](int, const TileRec &t) {                // (the tiles are of one shape: tile 0 answers for all)
        if (t.h == F.h && t.w == F.w && t.ch == F.ch) return VFSMS_OK;
        vfsms_set_error("shading_apply: the tiles are %d x %d x %d, the field is %d x %d x %d", t.h, t.w, t.ch, F.h, F.w, F.ch);
        return VFSMS_ERR_BAD_ARG;
    };
    std::vector<TileView> H;
    TRY(tile_list(ctx, "shading_apply", rule, tiles, n, H));
    TRY(ctx_arena_reserve(ctx, sizeof(TileView) * 2 * (size_t)n + 65536));
    ctx->pinned_off = 0;
    TRY(shade_apply_device(ctx, H.data(), n, F.h, F.w, F.ch, F.gain.as<uint16_t>()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // the tile table went through the pinned staging buffer: synchronous like every call that uses it
    return VFSMS_OK;
}
extern "C" int vfsms_shading_free(vfsms_ctx *ctx, int64_t field)
{
    CTX_ENTER(ctx);
    auto it = ctx->shade_fields.find(field);
    if (it == ctx->shade_fields.end()) { vfsms_set_error("shading_free: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    TRY(it->second.gain.release(ctx->stream));
    ctx->shade_fields.erase(it);
    return VFSMS_OK;
}

// ---- focus stacking (Method.focusStack; focus_kernels.hip, specified by tests/focus_ref.py) ----------------------------------------------
// what a focus call enqueues between its checks and its read-back; d_out: the new tile's buffer or arena memory
static int focus_run(vfsms_ctx *ctx, const std::vector<TileView> &H, int mode, int radius, int median, uint8_t *d_out, uint8_t *d_pre, uint8_t *d_index,
                     unsigned long long *d_scores, uint32_t *d_partials, std::vector<unsigned long long> &S)
{
    const int n = (int)H.size(), h = H[0].h, w = H[0].w, ch = H[0].ch;
    FocusPlane *d_tab;
    TRY(focus_table_device(ctx, H.data(), n, &d_tab));
    int const_d = -1;
    if (mode == 0) TRY(focus_select_device(ctx, d_tab, n, h, w, ch, radius, d_pre, d_scores, d_partials));
    else TRY(focus_scores_device(ctx, H.data(), n, d_scores));
    HIP_TRY(hipMemcpyAsync(S.data(), d_scores, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream));
    if (mode == 1) {                                         // the plane of the largest score, the first of them
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        const_d = (int)(std::max_element(S.begin(), S.end()) - S.begin());
    }
    TRY(focus_compose_device(ctx, d_tab, d_pre, h, w, ch, median, const_d, d_out, w * ch, d_index));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_focus_stack(vfsms_ctx *ctx, int n, const int64_t *planes, int mode, int radius, int median, int64_t *out_tile, uint8_t *out_host,
                                 uint8_t *index, int64_t *scores)
{
    CTX_ENTER(ctx);
    if ((mode != 0 && mode != 1) || radius < 1 || radius > VFSMS_FOCUS_MAX_RADIUS || (median != 0 && median != 1)) {
        vfsms_set_error("focus_stack: mode %d / radius %d / median %d (0 pixel or 1 plane; 1..%d; 0 or 1)", mode, radius, median, VFSMS_FOCUS_MAX_RADIUS);
        return VFSMS_ERR_BAD_ARG;
    }
    std::vector<TileView> H;
    TRY(tile_list(ctx, "focus_stack", FOCUS_STACK, planes, n, H));
    const int h = H[0].h, w = H[0].w, ch = H[0].ch;
    const size_t px = (size_t)h * w, bytes = px * ch;
    const size_t pbytes = mode == 0 ? focus_partials_bytes(n, h, w) : 0;
    TRY(ctx_arena_reserve(ctx, 2 * px + (out_tile ? 0 : bytes) + pbytes + (sizeof(TileView) * 2 + 8) * (size_t)n + 65536));
    ctx->pinned_off = 0;
    uint8_t *d_pre = (uint8_t *)ctx_arena_alloc(ctx, px), *d_index = (uint8_t *)ctx_arena_alloc(ctx, px);
    unsigned long long *d_scores = (unsigned long long *)ctx_arena_alloc(ctx, sizeof(unsigned long long) * n);
    uint8_t *d_out = out_tile ? nullptr : (uint8_t *)ctx_arena_alloc(ctx, bytes);
    uint32_t *d_partials = (uint32_t *)ctx_arena_alloc(ctx, pbytes ? pbytes : 4);
    if (!d_pre || !d_index || !d_scores || !d_partials || (!out_tile && !d_out)) { vfsms_set_error("arena exhausted (focus_stack)"); return VFSMS_ERR_CAPACITY; }
    if (out_tile) TRY(tile_buffer(ctx, bytes, &d_out, ctx->stream));
    std::vector<unsigned long long> S(n);
    int rc = focus_run(ctx, H, mode, radius, median, d_out, d_pre, d_index, d_scores, d_partials, S);
    if (rc == VFSMS_OK && out_host && hipMemcpy(out_host, d_out, bytes, hipMemcpyDeviceToHost) != hipSuccess) { vfsms_set_error("focus_stack: the download failed"); rc = VFSMS_ERR_HIP; }
    if (rc == VFSMS_OK && index && hipMemcpy(index, d_index, px, hipMemcpyDeviceToHost) != hipSuccess) { vfsms_set_error("focus_stack: the download failed"); rc = VFSMS_ERR_HIP; }
    if (rc != VFSMS_OK) {
        hipStreamSynchronize(ctx->stream);                   // (nothing enqueued may still write the buffer that goes back to the pool)
        if (out_tile) (void)tile_pool_return(ctx, d_out, bytes, false);
        return rc;
    }
    if (scores) for (int i = 0; i < n; i++) scores[i] = (int64_t)S[i];
    if (out_tile) tile_register(ctx, tile_rec(d_out, h, w, ch, w * ch, true), out_tile);
    return VFSMS_OK;
}
extern "C" int vfsms_focus_scores(vfsms_ctx *ctx, int n, const int64_t *tiles, int64_t *scores)
{
    CTX_ENTER(ctx);
    if (!scores) { vfsms_set_error("focus_scores: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    std::vector<TileView> H;
    TRY(tile_list(ctx, "focus_scores", FOCUS_SCORES, tiles, n, H));
    TRY(ctx_arena_reserve(ctx, (sizeof(TileView) * 2 + 8) * (size_t)n + 65536));
    ctx->pinned_off = 0;
    unsigned long long *d_scores = (unsigned long long *)ctx_arena_alloc(ctx, sizeof(unsigned long long) * n);
    if (!d_scores) { vfsms_set_error("arena exhausted (focus_scores)"); return VFSMS_ERR_CAPACITY; }
    TRY(focus_scores_device(ctx, H.data(), n, d_scores));
    std::vector<unsigned long long> S(n);
    HIP_TRY(hipMemcpyAsync(S.data(), d_scores, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    for (int i = 0; i < n; i++) scores[i] = (int64_t)S[i];
    return VFSMS_OK;
}

// ---- 16-bit gray tiles (vfsms_deep_*; deep_kernels.hip, specified by tests/deep_ref.py) ----------------------------------------------------
// The deep tiles a call names: the count, then every handle known, in index order (a handle of another kind is unknown here, as a deep
// handle is unknown to every entry that takes tiles).  Reads arguments and records only
static int deep_list(vfsms_ctx *ctx, const char *who, int n, const int64_t *deeps, std::vector<DeepSrc> &out)
{
    if (n < 1 || n > VFSMS_DEEP_MAX_TILES || !deeps) { vfsms_set_error("%s: 1..%d deep tiles, got %d", who, VFSMS_DEEP_MAX_TILES, n); return VFSMS_ERR_BAD_ARG; }
    out.resize(n);
    for (int i = 0; i < n; i++) {
        auto it = ctx->deep_tiles.find(deeps[i]);
        if (it == ctx->deep_tiles.end()) { vfsms_set_error("%s: handle %d is not a deep tile of this context", who, i); return VFSMS_ERR_BAD_ARG; }
        out[i] = DeepSrc{it->second.pix.as<uint16_t>(), nullptr, it->second.h, it->second.w};
    }
    return VFSMS_OK;
}
extern "C" int vfsms_deep_upload(vfsms_ctx *ctx, const uint16_t *img, int h, int w, int stride_bytes, int64_t *deep)
{
    CTX_ENTER(ctx);
    if (!img || !deep || h < 1 || h > VFSMS_DEEP_MAX_SIDE || w < 1 || w > VFSMS_DEEP_MAX_SIDE || stride_bytes < 2 * w) {
        vfsms_set_error("deep_upload: %d x %d samples, rows %d bytes apart (sides 1..%d, rows at least 2 w bytes apart)", h, w, stride_bytes, VFSMS_DEEP_MAX_SIDE);
        return VFSMS_ERR_BAD_ARG;
    }
    DeepRec R;
    R.h = h; R.w = w;
    TRY(R.pix.reserve((size_t)h * w * 2, ctx->stream));
    if (hipMemcpy2D(R.pix.as<void>(), (size_t)w * 2, img, (size_t)stride_bytes, (size_t)w * 2, h, hipMemcpyHostToDevice) != hipSuccess) {
        vfsms_set_error("deep_upload: the upload failed"); return VFSMS_ERR_HIP;
    }
    *deep = ctx->next_handle++;
    ctx->deep_tiles.emplace(*deep, std::move(R));
    return VFSMS_OK;
}
extern "C" int vfsms_deep_free(vfsms_ctx *ctx, int64_t deep)
{
    CTX_ENTER(ctx);
    auto it = ctx->deep_tiles.find(deep);
    if (it == ctx->deep_tiles.end()) { vfsms_set_error("deep_free: unknown handle"); return VFSMS_ERR_BAD_ARG; }
    TRY(it->second.pix.release(ctx->stream));
    ctx->deep_tiles.erase(it);
    return VFSMS_OK;
}
extern "C" int vfsms_deep_window(vfsms_ctx *ctx, int n, const int64_t *deeps, int lo_ppm, int hi_ppm, int32_t *window)
{
    CTX_ENTER(ctx);
    std::vector<DeepSrc> T;
    TRY(deep_list(ctx, "deep_window", n, deeps, T));
    if (lo_ppm < 0 || lo_ppm > hi_ppm || hi_ppm > 1000000 || !window) {
        vfsms_set_error("deep_window: ppm %d, %d (0 <= lo_ppm <= hi_ppm <= 1000000)", lo_ppm, hi_ppm);
        return VFSMS_ERR_BAD_ARG;
    }
    unsigned long long N = 0;
    for (const DeepSrc &t : T) N += (unsigned long long)t.h * t.w;             // at most 2^42: (N - 1) * ppm stays below 2^62
    TRY(ctx_arena_reserve(ctx, deep_table_bytes(n) + 65536));
    ctx->pinned_off = 0;
    int lo = 0, hi = 0;
    TRY(deep_window_device(ctx, T.data(), n, (N - 1) * (unsigned long long)lo_ppm / 1000000ull, (N - 1) * (unsigned long long)hi_ppm / 1000000ull, &lo, &hi));
    if (hi == lo) { if (lo < 65535) hi = lo + 1; else lo = hi - 1; }
    window[0] = lo; window[1] = hi;
    return VFSMS_OK;
}
extern "C" int vfsms_deep_reduce(vfsms_ctx *ctx, int n, const int64_t *deeps, int lo, int hi, int64_t *tiles_out)
{
    CTX_ENTER(ctx);
    std::vector<DeepSrc> T;
    TRY(deep_list(ctx, "deep_reduce", n, deeps, T));
    if (lo < 0 || lo >= hi || hi > 65535 || !tiles_out) { vfsms_set_error("deep_reduce: window %d, %d (0 <= lo < hi <= 65535)", lo, hi); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_arena_reserve(ctx, deep_table_bytes(n) + 65536));
    ctx->pinned_off = 0;
    int rc = VFSMS_OK, got = 0;
    for (; got < n && rc == VFSMS_OK; got++) {
        rc = tile_buffer(ctx, (size_t)T[got].h * T[got].w, &T[got].dst, ctx->stream);
        if (rc != VFSMS_OK) break;
    }
    if (rc == VFSMS_OK) rc = deep_reduce_device(ctx, T.data(), n, lo, hi);
    if (rc == VFSMS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { vfsms_set_error("deep_reduce: the kernel failed"); rc = VFSMS_ERR_HIP; }
    if (rc != VFSMS_OK) {                                    // no tile is created: the buffers go back behind a synchronisation
        hipStreamSynchronize(ctx->stream);
        for (int i = 0; i < got; i++) (void)tile_pool_return(ctx, T[i].dst, (size_t)T[i].h * T[i].w, false);
        return rc;
    }
    for (int i = 0; i < n; i++) tile_register(ctx, tile_rec(T[i].dst, T[i].h, T[i].w, 1, T[i].w, true), &tiles_out[i]);
    return VFSMS_OK;
}
extern "C" int vfsms_deep_mosaic_rows(vfsms_ctx *ctx, int n, const int64_t *deeps, const int32_t *yx, int rows, int cols, int mode, int feather,
                                      int row0, int nrows, uint16_t *out)
{
    CTX_ENTER(ctx);
    std::vector<DeepSrc> T;
    TRY(deep_list(ctx, "deep_mosaic_rows", n, deeps, T));
    if (!yx || rows < 1 || cols < 1) { vfsms_set_error("deep_mosaic_rows: a canvas of %d x %d", rows, cols); return VFSMS_ERR_BAD_ARG; }
    std::vector<DeepRect> at(n);
    for (int i = 0; i < n; i++) {
        const long long y = yx[2 * i], x = yx[2 * i + 1];
        if (y < 0 || x < 0 || y + T[i].h > rows || x + T[i].w > cols) {
            vfsms_set_error("deep_mosaic_rows: tile %d (%d x %d at %lld, %lld) lies outside the %d x %d canvas", i, T[i].h, T[i].w, y, x, rows, cols);
            return VFSMS_ERR_BAD_ARG;
        }
        at[i] = DeepRect{(int)y, (int)x, T[i].h, T[i].w};
    }
    if ((mode != 0 && mode != 1) || feather < 0 || feather > 32767) {
        vfsms_set_error("deep_mosaic_rows: mode %d / feather %d (0 paste or 1 feather; 0..32767)", mode, feather);
        return VFSMS_ERR_BAD_ARG;
    }
    if (row0 < 0 || nrows < 1 || (long long)row0 + nrows > rows || (long long)nrows * cols > (1ll << 30) || !out) {
        vfsms_set_error("deep_mosaic_rows: rows %d..%d + %d of %d (inside the canvas, at most 2^30 samples)", row0, row0, nrows, rows);
        return VFSMS_ERR_BAD_ARG;
    }
    DeepBins B;
    if (!deep_bins_build(at.data(), n, cols, row0, nrows, VFSMS_DEEP_MAX_BIN_ENTRIES, &B)) {
        vfsms_set_error("deep_mosaic_rows: the band's bin table exceeds %zu entries (use shorter bands)", VFSMS_DEEP_MAX_BIN_ENTRIES);
        return VFSMS_ERR_CAPACITY;
    }
    const size_t bytes = (size_t)nrows * cols * sizeof(uint16_t);
    TRY(ctx_arena_reserve(ctx, bytes + deep_mosaic_table_bytes(n, B) + 65536));
    ctx->pinned_off = 0;
    uint16_t *d_out = (uint16_t *)ctx_arena_alloc(ctx, bytes);
    if (!d_out) { vfsms_set_error("arena exhausted (deep_mosaic_rows)"); return VFSMS_ERR_CAPACITY; }
    TRY(deep_mosaic_device(ctx, T.data(), at.data(), n, B, cols, row0, nrows, mode, feather, d_out));
    HIP_TRY(hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_deep_download(vfsms_ctx *ctx, int64_t deep, uint16_t *out, int stride_bytes)
{
    CTX_ENTER(ctx);
    auto it = ctx->deep_tiles.find(deep);
    if (it == ctx->deep_tiles.end()) { vfsms_set_error("deep_download: the handle is not a deep tile of this context"); return VFSMS_ERR_BAD_ARG; }
    const DeepRec &R = it->second;
    if (!out || stride_bytes < 2 * R.w) { vfsms_set_error("deep_download: rows %d bytes apart for %d samples (at least 2 w), or a null pointer", stride_bytes, R.w); return VFSMS_ERR_BAD_ARG; }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (hipMemcpy2D(out, (size_t)stride_bytes, R.pix.as<void>(), (size_t)R.w * 2, (size_t)R.w * 2, R.h, hipMemcpyDeviceToHost) != hipSuccess) {
        vfsms_set_error("deep_download: the download failed"); return VFSMS_ERR_HIP;
    }
    return VFSMS_OK;
}

// ---- shading correction of deep tiles (deep_shading_kernels.hip, specified by tests/deep_shading_ref.py) ------------------------------------
static int deep_field_new(vfsms_ctx *ctx, int h, int w, int pedestal, bool estimated, DeepShadeRec *F)
{
    const size_t P = (size_t)h * w, Pa = (P + 127) & ~(size_t)127;            // the three uint16 planes stay 256-byte aligned
    F->h = h; F->w = w; F->pedestal = pedestal; F->estimated = estimated;
    TRY(F->gain.reserve((estimated ? 3 : 1) * Pa * sizeof(uint16_t), ctx->stream));
    if (estimated) { F->smooth = F->gain.as<uint16_t>() + Pa; F->prof = F->smooth + Pa; }
    return VFSMS_OK;
}
extern "C" int vfsms_deep_shading_estimate(vfsms_ctx *ctx, int n, const int64_t *deeps, int percentile, int radius, int pedestal, int64_t *field)
{
    CTX_ENTER(ctx);
    std::vector<DeepSrc> T;
    TRY(deep_list(ctx, "deep_shading_estimate", n, deeps, T));
    for (int i = 1; i < n; i++)
        if (T[i].h != T[0].h || T[i].w != T[0].w) {
            vfsms_set_error("deep_shading_estimate: tile %d is %d x %d, tile 0 is %d x %d (one shape)", i, T[i].h, T[i].w, T[0].h, T[0].w);
            return VFSMS_ERR_BAD_ARG;
        }
    if (percentile < 0 || percentile > 100 || radius < 1 || radius > VFSMS_SHADE_MAX_RADIUS || pedestal < 0 || pedestal > 65535 || !field) {
        vfsms_set_error("deep_shading_estimate: percentile %d / radius %d / pedestal %d (0..100; 1..%d; 0..65535), or a null pointer", percentile, radius, pedestal, VFSMS_SHADE_MAX_RADIUS);
        return VFSMS_ERR_BAD_ARG;
    }
    TRY(shade_plane_fits("deep_shading_estimate", T[0].h, (size_t)T[0].w));
    TRY(ctx_arena_reserve(ctx, sizeof(void *) * (size_t)n + 65536));
    ctx->pinned_off = 0;
    DeepShadeRec F;
    TRY(deep_field_new(ctx, T[0].h, T[0].w, pedestal, true, &F));
    int rc = deep_shade_estimate_device(ctx, T.data(), n, F.h, F.w, percentile, radius, pedestal, F.gain.as<uint16_t>(), F.smooth, F.prof);
    if (rc == VFSMS_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) { vfsms_set_error("deep_shading_estimate: the kernels failed"); rc = VFSMS_ERR_HIP; }
    if (rc != VFSMS_OK) { hipStreamSynchronize(ctx->stream); return rc; }      // (the field goes with F; nothing enqueued may still write it)
    *field = ctx->next_handle++;
    ctx->deep_fields.emplace(*field, std::move(F));
    return VFSMS_OK;
}
extern "C" int vfsms_deep_shading_from_gain(vfsms_ctx *ctx, const uint16_t *gain, int h, int w, int pedestal, int64_t *field)
{
    CTX_ENTER(ctx);
    if (h < 1 || h > VFSMS_DEEP_MAX_SIDE || w < 1 || w > VFSMS_DEEP_MAX_SIDE || pedestal < 0 || pedestal > 65535 || !gain || !field) {
        vfsms_set_error("deep_shading_from_gain: %d x %d samples / pedestal %d (sides 1..%d; 0..65535), or a null pointer", h, w, pedestal, VFSMS_DEEP_MAX_SIDE);
        return VFSMS_ERR_BAD_ARG;
    }
    DeepShadeRec F;
    TRY(deep_field_new(ctx, h, w, pedestal, false, &F));
    if (hipMemcpy(F.gain.as<void>(), gain, sizeof(uint16_t) * (size_t)h * w, hipMemcpyHostToDevice) != hipSuccess) {
        vfsms_set_error("deep_shading_from_gain: the upload failed"); return VFSMS_ERR_HIP;
    }
    *field = ctx->next_handle++;
    ctx->deep_fields.emplace(*field, std::move(F));
    return VFSMS_OK;
}
extern "C" int vfsms_deep_shading_download(vfsms_ctx *ctx, int64_t field, uint16_t *gain, uint16_t *smooth, uint16_t *profile, int32_t *pedestal)
{
    CTX_ENTER(ctx);
    auto it = ctx->deep_fields.find(field);
    if (it == ctx->deep_fields.end()) { vfsms_set_error("deep_shading_download: the handle is not a deep shading field of this context"); return VFSMS_ERR_BAD_ARG; }
    if (!gain) { vfsms_set_error("deep_shading_download: a null pointer"); return VFSMS_ERR_BAD_ARG; }
    const DeepShadeRec &F = it->second;
    const size_t bytes = sizeof(uint16_t) * (size_t)F.h * F.w;
    HIP_TRY(hipMemcpyAsync(gain, F.gain.as<uint16_t>(), bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (smooth) { if (F.estimated) HIP_TRY(hipMemcpyAsync(smooth, F.smooth, bytes, hipMemcpyDeviceToHost, ctx->stream)); else memset(smooth, 0, bytes); }
    if (profile) { if (F.estimated) HIP_TRY(hipMemcpyAsync(profile, F.prof, bytes, hipMemcpyDeviceToHost, ctx->stream)); else memset(profile, 0, bytes); }
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    if (pedestal) *pedestal = F.pedestal;
    return VFSMS_OK;
}
extern "C" int vfsms_deep_shading_apply(vfsms_ctx *ctx, int64_t field, int n, const int64_t *deeps)
{
    CTX_ENTER(ctx);
    std::vector<DeepSrc> T;
    TRY(deep_list(ctx, "deep_shading_apply", n, deeps, T));
    auto it = ctx->deep_fields.find(field);
    if (it == ctx->deep_fields.end()) { vfsms_set_error("deep_shading_apply: the handle is not a deep shading field of this context"); return VFSMS_ERR_BAD_ARG; }
    const DeepShadeRec &F = it->second;
    for (int i = 0; i < n; i++)
        if (T[i].h != F.h || T[i].w != F.w) {
            vfsms_set_error("deep_shading_apply: tile %d is %d x %d, the field is %d x %d", i, T[i].h, T[i].w, F.h, F.w);
            return VFSMS_ERR_BAD_ARG;
        }
    std::vector<int64_t> seen(deeps, deeps + n);
    std::sort(seen.begin(), seen.end());
    if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { vfsms_set_error("deep_shading_apply: a tile is named twice (it would be corrected twice)"); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_arena_reserve(ctx, sizeof(void *) * (size_t)n + 65536));
    ctx->pinned_off = 0;
    TRY(deep_shade_apply_device(ctx, T.data(), n, F.h, F.w, F.pedestal, F.gain.as<uint16_t>()));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // the pointer table went through the pinned staging buffer: synchronous like every call that uses it
    return VFSMS_OK;
}
extern "C" int vfsms_deep_shading_free(vfsms_ctx *ctx, int64_t field)
{
    CTX_ENTER(ctx);
    auto it = ctx->deep_fields.find(field);
    if (it == ctx->deep_fields.end()) { vfsms_set_error("deep_shading_free: the handle is not a deep shading field of this context"); return VFSMS_ERR_BAD_ARG; }
    TRY(it->second.gain.release(ctx->stream));
    ctx->deep_fields.erase(it);
    return VFSMS_OK;
}

// ---- exposure compensation (Method.exposureCompensation; exposure_kernels.hip, specified by tests/exposure_ref.py) -----------------------
// vfsms_overlap_stats_batch: every launch of the batch is enqueued before the one synchronisation that brings the sums back
extern "C" int vfsms_overlap_stats_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int lo, int hi, int64_t *out3)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n > 0 && (!jobs || !out3))) { vfsms_set_error("overlap_stats: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (lo < 0 || hi > 255 || lo > hi) { vfsms_set_error("overlap_stats: band %d..%d (0 <= lo <= hi <= 255)", lo, hi); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    std::vector<ExpPairHost> H(n);
    for (int k = 0; k < n; k++) {
        TileRec *pA, *pB;
        TRY(resident_pair(ctx, "overlap_stats", k, jobs[k], &pA, &pB));
        const TileRec &A = *pA, &B = *pB;
        if (A.ch != B.ch) { vfsms_set_error("overlap_stats: the tiles of job %d have %d and %d channels", k, A.ch, B.ch); return VFSMS_ERR_BAD_ARG; }
        H[k] = ExpPairHost{A.ptr, B.ptr, A.stride, B.stride, A.h, A.w * A.ch, B.h, B.w * B.ch, A.ch, jobs[k].dx, jobs[k].dy};
    }
    const size_t out_bytes = sizeof(unsigned long long) * 3 * (size_t)n;
    TRY(ctx_arena_reserve(ctx, sizeof(ExpJob) * (size_t)n + out_bytes + 65536));
    ctx->pinned_off = 0;
    unsigned long long *d_out = (unsigned long long *)ctx_arena_alloc(ctx, out_bytes);
    if (!d_out) { vfsms_set_error("overlap_stats: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    TRY(overlap_stats_device(ctx, H.data(), n, lo, hi, d_out));
    HIP_TRY(hipMemcpyAsync(out3, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_exposure_apply(vfsms_ctx *ctx, int n, const int64_t *tiles, const uint16_t *gain_q12)
{
    CTX_ENTER(ctx);
    if (n < 1 || n > VFSMS_SHADE_MAX_TILES || !tiles || !gain_q12) { vfsms_set_error("exposure_apply: 1..%d tiles and a gain for each", VFSMS_SHADE_MAX_TILES); return VFSMS_ERR_BAD_ARG; }
    std::vector<TileView> H;
    TRY(tile_list(ctx, "exposure_apply", ANY_REWRITE, tiles, n, H));
    TRY(ctx_arena_reserve(ctx, sizeof(TileView) * 2 * (size_t)n + 65536));
    ctx->pinned_off = 0;
    TRY(exposure_apply_device(ctx, H.data(), n, gain_q12));
    HIP_TRY(hipStreamSynchronize(ctx->stream));            // the tile table went through the pinned staging buffer: synchronous like every call that uses it
    return VFSMS_OK;
}

// ---- lens correction (Method.lensCorrection; lens_kernels.hip, specified by tests/lens_ref.py) ---------------------------------------------
// vfsms_block_ncc_batch: the launch of the batch is enqueued before the one synchronisation that brings the results back
extern "C" int vfsms_block_ncc_batch(vfsms_ctx *ctx, const vfsms_ncc_job *jobs, int n, int block, int radius, const int64_t *first,
                                     int32_t *best4, int32_t *surface)
{
    CTX_ENTER(ctx);
    if (n < 0 || !first || (n > 0 && !jobs)) { vfsms_set_error("block_ncc: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (block < 8 || block > VFSMS_LENS_MAX_BLOCK || block % 8) { vfsms_set_error("block_ncc: block %d is no multiple of 8 in 8..%d", block, VFSMS_LENS_MAX_BLOCK); return VFSMS_ERR_BAD_ARG; }
    if (radius < 1 || radius > VFSMS_LENS_MAX_RADIUS) { vfsms_set_error("block_ncc: radius %d outside 1..%d", radius, VFSMS_LENS_MAX_RADIUS); return VFSMS_ERR_BAD_ARG; }
    std::vector<LensBlockHost> H(n);
    std::vector<long long> F(n + 1, 0);
    for (int k = 0; k < n; k++) {
        TileRec *pA, *pB;
        TRY(resident_pair(ctx, "block_ncc", k, jobs[k], &pA, &pB));
        const TileRec &A = *pA, &B = *pB;
        if (A.ch != B.ch || (A.ch != 1 && A.ch != 3)) { vfsms_set_error("block_ncc: the tiles of job %d have %d and %d channels (both 1 or both 3)", k, A.ch, B.ch); return VFSMS_ERR_BAD_ARG; }
        if (A.h != B.h || A.w != B.w) { vfsms_set_error("block_ncc: the tiles of job %d are %d x %d and %d x %d", k, A.h, A.w, B.h, B.w); return VFSMS_ERR_BAD_ARG; }
        H[k] = LensBlockHost{A.ptr, B.ptr, A.stride, B.stride, A.h, A.w, A.ch, jobs[k].dx, jobs[k].dy};
        int r0, c0, nby, nbx;
        lens_lattice(A.h, A.w, jobs[k].dx, jobs[k].dy, block, radius, &r0, &c0, &nby, &nbx);
        F[k + 1] = F[k] + (long long)nby * nbx;
    }
    for (int k = 0; k <= n; k++)
        if (first[k] != F[k]) { vfsms_set_error("block_ncc: first[%d] is %lld, the lattice gives %lld", k, (long long)first[k], F[k]); return VFSMS_ERR_BAD_ARG; }
    const size_t total = (size_t)F[n], CC = (size_t)(2 * radius + 1) * (2 * radius + 1);
    if (total == 0) return VFSMS_OK;
    if (!best4) { vfsms_set_error("block_ncc: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_arena_reserve(ctx, (sizeof(LensBlockHost) + 16) * ((size_t)n + 1) + sizeof(int32_t) * total * (4 + (surface ? CC : 0)) + 65536));
    ctx->pinned_off = 0;
    int32_t *d_best = (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * 4 * total);
    int32_t *d_surf = surface ? (int32_t *)ctx_arena_alloc(ctx, sizeof(int32_t) * CC * total) : nullptr;
    if (!d_best || (surface && !d_surf)) { vfsms_set_error("block_ncc: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    TRY(lens_blocks_device(ctx, H.data(), F.data(), n, block, radius, d_best, d_surf));
    HIP_TRY(hipMemcpyAsync(best4, d_best, sizeof(int32_t) * 4 * total, hipMemcpyDeviceToHost, ctx->stream));
    if (surface) HIP_TRY(hipMemcpyAsync(surface, d_surf, sizeof(int32_t) * CC * total, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
// what both resampling calls refuse of their map, for an h x w image; a centre coordinate below 0 is the image's own middle
static int lens_check_map(const char *who, int h, int w, int32_t a1_q30, int32_t a2_q30, int32_t cy2, int32_t cx2, int interp)
{
    if (interp != 0 && interp != 1) { vfsms_set_error("%s: interp %d (0 bilinear or 1 cubic)", who, interp); return VFSMS_ERR_BAD_ARG; }
    if (a1_q30 < -VFSMS_LENS_MAX_COEF || a1_q30 > VFSMS_LENS_MAX_COEF || a2_q30 < -VFSMS_LENS_MAX_COEF || a2_q30 > VFSMS_LENS_MAX_COEF) {
        vfsms_set_error("%s: coefficients %d, %d outside +-2^28 (Q30)", who, a1_q30, a2_q30); return VFSMS_ERR_BAD_ARG;
    }
    if (h > VFSMS_LENS_MAX_SIDE || w > VFSMS_LENS_MAX_SIDE) { vfsms_set_error("%s: an image of %d x %d (sides up to %d)", who, h, w, VFSMS_LENS_MAX_SIDE); return VFSMS_ERR_BAD_ARG; }
    const long long ey = cy2 < 0 ? 0 : 2ll * std::abs((long long)cy2 - (h - 1)), ex = cx2 < 0 ? 0 : 2ll * std::abs((long long)cx2 - (w - 1));
    if (ey > h - 1 || ex > w - 1) { vfsms_set_error("%s: the centre (%d, %d) / 2 lies outside the middle half of a %d x %d image", who, cy2, cx2, h, w); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}
extern "C" int vfsms_lens_apply(vfsms_ctx *ctx, int n, const int64_t *tiles, int32_t a1_q30, int32_t a2_q30, int32_t cy2, int32_t cx2, int interp)
{
    CTX_ENTER(ctx);
    TileRule rule = ANY_REWRITE;
    rule.pred = [=](int, const TileRec &t) { return lens_check_map("lens_apply", t.h, t.w, a1_q30, a2_q30, cy2, cx2, interp); };
    std::vector<TileView> H;
    TRY(tile_list(ctx, "lens_apply", rule, tiles, n, H));
    TRY(lens_apply_device(ctx, H.data(), n, a1_q30, a2_q30, cy2, cx2, interp));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}
extern "C" int vfsms_lens_remap_u8(vfsms_ctx *ctx, const uint8_t *src, int h, int w, int ch, int src_stride, int32_t a1_q30, int32_t a2_q30,
                                   int32_t cy2, int32_t cx2, int interp, uint8_t *dst)
{
    CTX_ENTER(ctx);
    if (!src || !dst || h <= 0 || w <= 0 || ch < 1 || ch > 4 || src_stride < w * ch) { vfsms_set_error("lens_remap: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(lens_check_map("lens_remap", h, w, a1_q30, a2_q30, cy2, cx2, interp));
    const size_t bytes = (size_t)h * w * ch;
    TRY(ctx_arena_reserve(ctx, 2 * bytes + 65536));
    ctx->pinned_off = 0;
    uint8_t *d_src, *d_dst = (uint8_t *)ctx_arena_alloc(ctx, bytes);
    if (!d_dst) { vfsms_set_error("lens_remap: arena exhausted"); return VFSMS_ERR_CAPACITY; }
    TRY(upload_image(ctx, src, h, w * ch, src_stride, &d_src));
    TRY(lens_remap_device(ctx, d_src, d_dst, w * ch, h, w, ch, a1_q30, a2_q30, cy2, cx2, interp));
    HIP_TRY(hipMemcpyAsync(dst, d_dst, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

// ---- ORB -------------------------------------------------------------------------------------------------------------------------
static void orb_caps(const vfsms_orb_params *p, int *cap1, int *cap2, int *cap)
{
    // level-0 quota bounds every level; FAST scores are integers, so ties can exceed 2 x quota -- leave generous room
    const float factor = 1.f / p->scale_factor;
    const int q0 = (int)lrintf(p->n_features * (1 - factor) / (1 - powf(factor, (float)p->n_levels)));
    *cap1 = 4 * q0 + 2048; *cap2 = 2 * q0 + 1024; *cap = 2 * p->n_features + 2048;
}
// after an overflow: capacities that hold every keypoint of the strip whose counters these are.  counters[4 + l] is the true number of
// survivors of level l's FAST-score cut (counted before any clamp); the quota cut keeps at most that many, the output at most their sum.
static void orb_grow_caps(const int *counters, int nlevels, int *cap1, int *cap2, int *cap)
{
    int m = 0; long long sum = 0;
    for (int l = 0; l < nlevels; l++) { m = std::max(m, counters[4 + l]); sum += counters[4 + l]; }
    *cap1 = std::max(*cap1, m); *cap2 = std::max(*cap2, m); *cap = (int)std::max<long long>(*cap, sum);
}

// ---- one ORB run: n sources detected and described in fused launches ----------------------------------------------------------------------
// The phases of a SURF run: orb_run_bytes into the caller's ONE ctx_arena_reserve, orb_run_carve (wires and uploads the records), orb_run_launch,
// then orb_run_retry's orb_run_readback, synchronisation and orb_run_overflow.  A source is a strip of a batch's table or a whole image.
// The one place that knows a run's arena block: the counters (64 ints per source: counters, thr1, n1, n2 at +0, +16, +32, +48), the
// sources' ROIs, the uploaded records
void orb_run_layout(ArenaWalk &a, OrbRun *run, const StripTable::Strip *S, int n, const vfsms_orb_params *p, int cap1, int cap2, int cap)
{
    run->R.resize(n);
    run->cblock = a.take<int>(64 * (size_t)n);
    for (int i = 0; i < n; i++) {
        OrbDev &r = run->R[i];
        orb_roi_layout(a, &r, S[i].p, S[i].stride, S[i].h, S[i].w, p, cap1, cap2, cap);
        if (run->cblock) { r.counters = run->cblock + 64 * i; r.thr1 = r.counters + 16; r.n1 = r.counters + 32; r.n2 = r.counters + 48; }
    }
    run->dR = a.take<OrbDev>(n);
}
static size_t orb_run_bytes(const vfsms_orb_params *p, const StripTable::Strip *S, int n, int cap1, int cap2, int cap)
{
    ArenaWalk a; OrbRun run; orb_run_layout(a, &run, S, n, p, cap1, cap2, cap); return a.off;
}
static int orb_run_carve(vfsms_ctx *ctx, OrbRun *run, const StripTable::Strip *S, int n, const vfsms_orb_params *p, int cap1, int cap2, int cap)
{
    ArenaWalk a = ctx_arena_walk(ctx);
    orb_run_layout(a, run, S, n, p, cap1, cap2, cap);
    TRY(ctx_arena_commit(ctx, a, "arena exhausted while carving an ORB run"));
    return ctx_copy_small(ctx, run->R.data(), sizeof(OrbDev) * n, run->dR);
}
// no prepare phase: k_orb_clear zeroes the counters
static int orb_run_launch(vfsms_ctx *ctx, const OrbRun &run, const vfsms_orb_params *p) { return launch_orb(ctx, run.dR, run.R.data(), (int)run.R.size(), p); }
static int orb_run_readback(vfsms_ctx *ctx, OrbRun *run)
{
    run->counters.resize(64 * run->R.size());
    HIP_TRY(hipMemcpyAsync(run->counters.data(), run->cblock, sizeof(int) * run->counters.size(), hipMemcpyDeviceToHost, ctx->stream));
    return VFSMS_OK;
}
// after the synchronisation: the last source whose keypoints exceeded a capacity, or -1; the capacities grow to hold every such source
static int orb_run_overflow(const OrbRun &run, int nlevels, int *cap1, int *cap2, int *cap)
{
    int over = -1;
    for (size_t i = 0; i < run.R.size(); i++)
        if (run.counters[64 * i + 2]) { over = (int)i; orb_grow_caps(&run.counters[64 * i], nlevels, cap1, cap2, cap); }
    return over;
}
// Ties can overflow the default capacities: the run happens once more with capacities that hold every keypoint, never a truncation.
// enqueue(cap1, cap2, cap) reserves, carves and launches `run` (and what reads it); *over: what orb_run_overflow says of the last run
template <typename Enqueue>
static int orb_run_retry(vfsms_ctx *ctx, const vfsms_orb_params *p, OrbRun *run, int *over, Enqueue enqueue)
{
    int c1, c2, c;
    orb_caps(p, &c1, &c2, &c);
    for (int pass = 0;; pass++) {
        TRY(enqueue(c1, c2, c));
        TRY(orb_run_readback(ctx, run));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
        *over = orb_run_overflow(*run, p->n_levels, &c1, &c2, &c);
        if (*over < 0 || pass > 0) return VFSMS_OK;
    }
}

extern "C" int vfsms_orb_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride,
                                         const vfsms_orb_params *params, float *kps_xy, uint8_t *desc,
                                         vfsms_keypoint *kps_full, int cap, int *n_out)
{
    CTX_ENTER(ctx);
    if (!img || !params || !n_out || h <= 0 || w <= 0 || stride < w || cap < 0) { vfsms_set_error("orb: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(ctx_prepare_orb(ctx, params));
    OrbRun run; int over;
    TRY(orb_run_retry(ctx, params, &run, &over, [&](int c1, int c2, int c) -> int {
        StripTable::Strip src{nullptr, w, h, w};
        TRY(ctx_arena_reserve(ctx, (size_t)h * w + orb_run_bytes(params, &src, 1, c1, c2, c) + 65536));
        ctx->pinned_off = 0;                                // entry points are synchronous: the staging buffer is free again
        uint8_t *d_img;
        TRY(upload_image(ctx, img, h, w, stride, &d_img));
        src.p = d_img;
        TRY(orb_run_carve(ctx, &run, &src, 1, params, c1, c2, c));
        return orb_run_launch(ctx, run, params);
    }));
    if (over >= 0) { vfsms_set_error("orb: internal keypoint capacity exceeded"); return VFSMS_ERR_CAPACITY; }
    const OrbDev &R = run.R[0];
    const int n = run.counters[1];
    *n_out = n;
    if (n > cap) { vfsms_set_error("orb: %d keypoints exceed the caller's capacity %d", n, cap); return VFSMS_ERR_CAPACITY; }
    if (n > 0) {
        if (kps_xy) HIP_TRY(hipMemcpyAsync(kps_xy, R.kps_xy, sizeof(float) * 2 * n, hipMemcpyDeviceToHost, ctx->stream));
        if (desc) HIP_TRY(hipMemcpyAsync(desc, R.desc, (size_t)32 * n, hipMemcpyDeviceToHost, ctx->stream));
        if (kps_full) HIP_TRY(hipMemcpyAsync(kps_full, R.kps_out, sizeof(vfsms_keypoint) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    return VFSMS_OK;
}

// ---- SIFT (sift_kernels.hip) -----------------------------------------------------------------------------------------------------
extern "C" int vfsms_sift_detect_describe(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, const vfsms_sift_params *params,
                                          float *kps_xy, float *desc, vfsms_keypoint *kps_full, int cap, int *n_out)
{
    CTX_ENTER(ctx);
    if (!img || !params || !n_out || h <= 0 || w <= 0 || stride < w || cap < 0) { vfsms_set_error("sift: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    *n_out = 0;
    TRY(sift_check_params(params));
    TRY(ctx_arena_reserve(ctx, (size_t)h * w + 65536));
    uint8_t *d_img;
    TRY(upload_image(ctx, img, h, w, stride, &d_img));
    return sift_detect_describe_device(ctx, d_img, h, w, params, kps_xy, desc, kps_full, cap, n_out);
}

extern "C" int vfsms_sift_pyramid(vfsms_ctx *ctx, const uint8_t *img, int h, int w, int stride, const vfsms_sift_params *params,
                                  float *gauss, float *dog, size_t cap_floats, int32_t *shapes, int shapes_cap, int *n_octaves)
{
    CTX_ENTER(ctx);
    if (!img || !params || !shapes || !n_octaves || h <= 0 || w <= 0 || stride < w) { vfsms_set_error("sift_pyramid: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(sift_check_params(params));
    TRY(ctx_arena_reserve(ctx, (size_t)h * w + 65536));
    uint8_t *d_img;
    TRY(upload_image(ctx, img, h, w, stride, &d_img));
    return sift_pyramid_device(ctx, d_img, h, w, params, gauss, dog, cap_floats, shapes, shapes_cap, n_octaves);
}

// ---- fused SIFT + BF + ratio + vote attempts --------------------------------------------------------------------------------------
// The distinct strips of the batch (build_strip_table) are detected and described once, shape run after shape run, in groups whose
// pyramids fit the context's byte budget (sift_group_strips); a group costs two host syncs whatever its size, and every array is sized
// from the counts read there, so nothing can overflow.  Only positions, descriptors and their packed int8 rows outlive a group
// (ctx->sift_pool).  The 2-NN search is the integer matrix-core kernel (k_bf_i8_d128, exact); VFSMS_BF_EXACT=1 takes k_bf_l2_gen<128>.
extern "C" int vfsms_attempt_sift_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                                        const vfsms_sift_params *params, double ratio, int offset_evaluate, int32_t *out)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!jobs || !out)) || !params) { vfsms_set_error("attempt_sift: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    TRY(sift_check_params(params));
    if (n == 0) return VFSMS_OK;
    const std::vector<int> ord = shape_order(jobs, n);
    StripTable T;
    TRY(build_strip_table(ctx, jobs, ord.data(), n, n, &T));
    const int u = (int)T.strips.size();
    ctx->pinned_off = 0;                                        // entry points are synchronous: the staging buffer is free again
    sift_pool_reset(ctx);
    int *cblock = (int *)sift_pool_alloc(ctx, sizeof(int) * 4 * u);          // per strip: candidates, keypoints before dedup, keypoints
    if (!cblock) return VFSMS_ERR_CAPACITY;
    std::vector<SiftStripOut> S(u);
    const bool exact = bf_force_exact();
    // detect + describe (+ pack): the strips are in shape order already
    for (const ShapeRun &q : shape_runs(T.strips.data(), u)) {
        const int h = q.h, w = q.w, i0 = q.first, i1 = q.first + q.count;
        int gmax = 1;
        TRY(sift_group_strips(ctx, h, w, params, &gmax));
        for (int a = i0; a < i1; a += gmax) {
            const int g = std::min(gmax, i1 - a);
            TRY(ctx_arena_reserve(ctx, (sizeof(SiftSrcHost) + 2 * 64 + sizeof(PackJob) + 1024) * (size_t)g + 65536));
            std::vector<SiftSrcHost> src(g);
            for (int k = 0; k < g; k++) { src[k].p = T.strips[a + k].p; src[k].stride = T.strips[a + k].stride; }
            ProfScope ps(ctx, "sift_group");
            TRY(sift_group_device(ctx, src.data(), g, h, w, params, cblock + 4 * a, &S[a], nullptr));
            if (!exact) {
                std::vector<PackJob> pj; int maxn = 0;
                for (int k = 0; k < g; k++) {
                    const SiftStripOut &o = S[a + k];
                    if (o.n == 0) continue;
                    pj.push_back(PackJob{o.desc, cblock + 4 * (a + k) + 2, o.d8, o.nrm});
                    maxn = std::max(maxn, o.n);
                }
                if (!pj.empty()) {
                    PackJob *dP;
                    TRY(ctx_upload_small(ctx, pj.data(), sizeof(PackJob) * pj.size(), (void **)&dP));
                    TRY(launch_pack_i8_d128(ctx, dP, (int)pj.size(), maxn));
                }
            }
        }
    }
    // match + vote: capacities are the exact counts
    HIP_TRY(hipStreamSynchronize(ctx->stream));                 // the last group's launch records have left the staging buffer, reset below
    int maxcap = 1, maxt = 1; long long waves = 0;
    std::vector<MatchJob> J(n, MatchJob{});
    for (int s_ = 0; s_ < n; s_++) {
        const int ia = T.a[s_], ib = T.b[s_];
        const SiftStripOut &A = S[ia], &B = S[ib];
        MatchJob &j = J[s_];
        j.q = A.desc; j.t = B.desc; j.kq = A.xy; j.kt = B.xy;
        j.q8 = A.d8; j.t8 = B.d8; j.qn2 = A.nrm; j.tn2 = B.nrm;
        j.nq_ptr = cblock + 4 * ia + 2; j.nt_ptr = cblock + 4 * ib + 2;
        j.capq = std::max(A.n, 1); j.capt = std::max(B.n, 1); j.row = ord[s_];
        j.sa = &T.strips[ia]; j.sb = &T.strips[ib];
        maxcap = std::max(maxcap, j.capq); maxt = std::max(maxt, B.n);
        waves += (j.capq + 63) / 64;
    }
    // a wave of the integer kernel owns 64 queries: its own split rule; the exhaustive float kernel keeps pick_nsplit
    MatchPlan P{false, 0, 0};
    P.ns = exact ? pick_nsplit(maxcap, maxt, n, 128) : pick_i8_nsplit(waves, maxt);
    TRY(ctx_arena_reserve(ctx, match_run_bytes(J.data(), n, P) + 65536));
    ctx->pinned_off = 0;
    MatchRun run;
    TRY(match_run_carve(ctx, &run, J.data(), n, 128, P));
    TRY(match_run_launch(ctx, run, 0, n, maxcap, maxt, exact ? SEARCH_FLOAT : SEARCH_I8_D128, MatchTail{TAIL_VOTE, ratio, -1, offset_evaluate}));
    TRY(match_run_readback(ctx, run, out));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
    return VFSMS_OK;
}

extern "C" int vfsms_attempt_orb_batch(vfsms_ctx *ctx, const vfsms_roi_pair *jobs, int n,
                                       const vfsms_orb_params *params, int max_dist, int offset_evaluate, int32_t *out)
{
    CTX_ENTER(ctx);
    if (n < 0 || (n && (!jobs || !out)) || !params) { vfsms_set_error("attempt_orb: bad arguments"); return VFSMS_ERR_BAD_ARG; }
    if (n == 0) return VFSMS_OK;
    TRY(ctx_prepare_orb(ctx, params));
    // ROIs of one shape next to each other: the image-sized kernels are launched per shape run (launch_orb); slot s holds job ord[s];
    // every distinct strip of the batch is carved and run once (build_strip_table)
    const std::vector<int> ord = shape_order(jobs, n);
    StripTable T;
    TRY(build_strip_table(ctx, jobs, ord.data(), n, n, &T));
    const int u = (int)T.strips.size();
    OrbRun orb; int over;
    TRY(orb_run_retry(ctx, params, &orb, &over, [&](int c1, int c2, int c) -> int {
        std::vector<MatchJob> J(n, MatchJob{});
        for (int s_ = 0; s_ < n; s_++) {
            J[s_].capq = J[s_].capt = c; J[s_].row = ord[s_];
            J[s_].sa = &T.strips[T.a[s_]]; J[s_].sb = &T.strips[T.b[s_]];
        }
        const MatchPlan P{false, pick_hamming_nsplit(c, n), 0};
        TRY(ctx_arena_reserve(ctx, orb_run_bytes(params, T.strips.data(), u, c1, c2, c) + match_run_bytes(J.data(), n, P) + 65536));
        ctx->pinned_off = 0;
        MatchRun match;
        TRY(orb_run_carve(ctx, &orb, T.strips.data(), u, params, c1, c2, c));
        for (int s_ = 0; s_ < n; s_++) {
            const OrbDev &A = orb.R[T.a[s_]], &B = orb.R[T.b[s_]];
            J[s_].q = (const float *)A.desc; J[s_].t = (const float *)B.desc; J[s_].kq = A.kps_xy; J[s_].kt = B.kps_xy;
            J[s_].nq_ptr = A.counters + 1; J[s_].nt_ptr = B.counters + 1;
        }
        TRY(match_run_carve(ctx, &match, J.data(), n, 32, P));
        TRY(orb_run_launch(ctx, orb, params));
        TRY(match_run_launch(ctx, match, 0, n, c, c, SEARCH_HAMMING, MatchTail{TAIL_VOTE, 0.0, max_dist, offset_evaluate, true}));
        return match_run_readback(ctx, match, out);       // results of all jobs, counters of all strips: two contiguous blocks, two D2H copies per run
    }));
    if (over >= 0) { vfsms_set_error("attempt_orb: internal keypoint capacity exceeded in strip %d of %d", over, u); return VFSMS_ERR_CAPACITY; }
    return VFSMS_OK;
}
