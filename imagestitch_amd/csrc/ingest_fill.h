// ingest_fill.h -- one hand-over of pixels to reserved tiles, from lookup to settlement (vfsms_tile_fill* of api.hip): the staging pools of
// the decoder threads and TileFill, the transaction that owns what a fill leases from them.  Host C++ over common.h and the runtime API, no
// kernels, no launchers: libvfsms and tools/ingest_fill_host_check.cpp (host sanitizers, failures injected) compile the same lines.
#pragma once
#include "common.h"
#include <string.h>

static inline int pad16(int x) { return (x + 15) & ~15; }       // a side on whole 16 x 16 iMCUs
// The two staging pools of the decoder threads (the tile pool belongs to the context thread), shared under stage_mu, first fit, at most 64
// entries each.  Pinned host staging: the decoder's own memory is pageable, and an asynchronous copy from pageable memory makes the runtime
// pin it on the fly (a trip through the kernel's memory-map lock per tile, contended by every decoder thread and by the registrar's
// launches); the rows are packed into a pinned buffer by the calling thread (a memcpy, in parallel across the decoders) and leave by true
// DMA.  Device staging: what a fill's kernels read and write before the tiles.
template <bool Pinned>
static hipError_t stage_get(vfsms_ctx *ctx, size_t need, StageBuf *out)
{
    std::vector<StageBuf> &pool = Pinned ? ctx->pin_pool : ctx->stage_pool;
    {
        std::lock_guard<std::mutex> lk(ctx->stage_mu);
        for (size_t k = 0; k < pool.size(); k++)
            if (pool[k].bytes >= need) { *out = pool[k]; pool.erase(pool.begin() + k); return hipSuccess; }
    }
    *out = StageBuf{nullptr, need};
    const hipError_t e = Pinned ? hipHostMalloc((void **)&out->ptr, need, hipHostMallocDefault) : hipMalloc((void **)&out->ptr, need);
    if (e != hipSuccess) out->ptr = nullptr;
    return e;
}
template <bool Pinned>
static void stage_put(vfsms_ctx *ctx, StageBuf b)
{
    if (!b.ptr) return;
    std::lock_guard<std::mutex> lk(ctx->stage_mu);
    std::vector<StageBuf> &pool = Pinned ? ctx->pin_pool : ctx->stage_pool;
    if (pool.size() < 64) pool.push_back(b); else if (Pinned) (void)hipHostFree(b.ptr); else (void)hipFree(b.ptr);
}
static void stage_pools_free(vfsms_ctx *ctx)                     // between fills the pools hold raw entries: freed here and nowhere else
{
    for (auto &sb : ctx->stage_pool) (void)hipFree(sb.ptr);
    for (auto &pb : ctx->pin_pool) (void)hipHostFree(pb.ptr);
    ctx->stage_pool.clear(); ctx->pin_pool.clear();
}
static void pack_rows(uint8_t *dst, const uint8_t *src, int stride, size_t row_bytes, int h)
{
    if ((size_t)stride == row_bytes) { memcpy(dst, src, row_bytes * h); return; }
    for (int y = 0; y < h; y++) memcpy(dst + (size_t)y * row_bytes, src + (size_t)y * stride, row_bytes);
}
// the end of a fill: its tiles filled, or given up
static void fill_pair_settle(vfsms_ctx *ctx, int64_t gray, int64_t color, bool ok)
{
    std::lock_guard<std::mutex> lk(ctx->tiles_mu);
    for (int64_t hd : { gray, color }) {
        if (!hd) continue;
        auto it = ctx->tiles.find(hd);
        if (it != ctx->tiles.end()) { it->second.fill = ok ? 0 : 2; it->second.pending = false; }   // (the work has landed: no stream wait needed)
    }
    ctx->tiles_cv.notify_all();
}

// One hand-over.  begin_*() looks the tiles up; host() / pack() / device() lease staging, and the object holds every lease to its end; copy()
// and run() enqueue on the copy stream and are skipped once `e` or `rc` tells of a failure.  It ends in one of three ways:
//   finish(), all well: the tiles' event is recorded and waited for, the leases go back, the tiles are FILLED;
//   finish() after a failure: the copy stream is synchronised -- nothing may still read a buffer that goes back to a pool -- the leases go
//     back, the tiles are GIVEN UP (fill = 2) and whoever waits for them is told;
//   refuse(): the file is handed back before a tile was touched.  The stream is synchronised if anything was enqueued, the leases go back,
//     the tiles STAY RESERVED: the caller fills them some other way.
// An object that is dropped unfinished refuses when nothing was enqueued and finishes as failed otherwise.
struct TileFill {
    vfsms_ctx *ctx; const char *who = "";
    int h = 0, w = 0, ch = 1; uint8_t *dg = nullptr, *dc = nullptr;     // the tiles' size in pixels; the gray (begin_one: the only) and the colour tile's pixels
    hipError_t e = hipSuccess; int rc = VFSMS_OK;
    explicit TileFill(vfsms_ctx *c) : ctx(c) {}
    TileFill(const TileFill &) = delete; TileFill &operator=(const TileFill &) = delete;
    ~TileFill() { if (open) { if (enqueued && ok()) rc = VFSMS_ERR_HIP; end(enqueued); } }
    bool ok() const { return e == hipSuccess && rc == VFSMS_OK; }
    // a reserved gray tile and / or a reserved 3-channel tile of one size (either handle may be 0), or an error and both as they were
    int begin_pair(int64_t gray, int64_t color, const char *who_, bool give_up)
    {
        who = who_; tile[0] = gray; tile[1] = color;
        std::lock_guard<std::mutex> lk(ctx->tiles_mu);
        TileRec *tg = nullptr, *tc = nullptr;
        if (gray) { auto it = ctx->tiles.find(gray); if (it != ctx->tiles.end() && it->second.fill == 1 && it->second.ch == 1) tg = &it->second; }
        if (color) { auto it = ctx->tiles.find(color); if (it != ctx->tiles.end() && it->second.fill == 1 && it->second.ch == 3) tc = &it->second; }
        if ((gray && !tg) || (color && !tc) || (!tg && !tc)) {
            vfsms_set_error("%s: needs a reserved 1-channel tile and / or a reserved 3-channel tile", who); return VFSMS_ERR_BAD_ARG;
        }
        if (give_up) { if (tg) tg->fill = 2; if (tc) tc->fill = 2; ctx->tiles_cv.notify_all(); return VFSMS_OK; }
        if (tg && tc && (tg->h != tc->h || tg->w != tc->w)) { vfsms_set_error("%s: the two tiles differ in size", who); return VFSMS_ERR_BAD_ARG; }
        h = tg ? tg->h : tc->h; w = tg ? tg->w : tc->w;
        ev = tg ? tg->ready : tc->ready; dg = tg ? tg->ptr : nullptr; dc = tc ? tc->ptr : nullptr;
        open = true;
        return VFSMS_OK;
    }
    // one reserved tile of any channel count: rows of w * ch bytes at dg
    int begin_one(int64_t handle, const char *who_, bool give_up)
    {
        who = who_; tile[0] = handle;
        std::lock_guard<std::mutex> lk(ctx->tiles_mu);
        auto it = ctx->tiles.find(handle);
        if (it == ctx->tiles.end() || it->second.fill != 1) { vfsms_set_error("%s: not a reserved tile", who); return VFSMS_ERR_BAD_ARG; }
        if (give_up) { it->second.fill = 2; ctx->tiles_cv.notify_all(); return VFSMS_OK; }
        h = it->second.h; w = it->second.w; ch = it->second.ch; ev = it->second.ready; dg = it->second.ptr;
        open = true;
        return VFSMS_OK;
    }
    // `cap` bytes of host staging: pinned from the pool, else (no pinned memory left) pageable memory of the object's own
    uint8_t *host(size_t cap, bool or_pageable = true)
    {
        if (stage_get<true>(ctx, cap, &pin) == hipSuccess) return pin.ptr;
        // the runtime's sticky "last error" must not outlive the fallback, or the launch check behind it (hipGetLastError behind
        // k_ingest_split) would report THIS failure and give the tiles up
        (void)hipGetLastError();
        if (!or_pageable) return nullptr;
        pageable.resize(cap);
        return pageable.data();
    }
    // the caller's rows, densely packed in host staging; without pinned memory rows that are dense already are taken where they lie
    const uint8_t *pack(const uint8_t *src, int stride, size_t row_bytes, int rows)
    {
        uint8_t *dst = host(row_bytes * rows, (size_t)stride != row_bytes);
        if (dst) pack_rows(dst, src, stride, row_bytes, rows);
        return dst ? dst : src;
    }
    // a device staging buffer (at most four a fill); nullptr after a failure, this one's included
    uint8_t *device(size_t bytes)
    {
        if (!ok()) return nullptr;
        e = ndev < 4 ? stage_get<false>(ctx, bytes, &dev[ndev]) : hipErrorOutOfMemory;
        return e == hipSuccess ? dev[ndev++].ptr : nullptr;
    }
    void copy(void *dst, const void *src, size_t bytes) { if (ok()) { enqueued = true; e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->copy_stream); } }
    template <typename Body> void run(Body body) { if (ok()) { enqueued = true; rc = body(); } }   // body: launches on the copy stream -> a VFSMS code
    int finish() { return end(true); }
    int refuse(int code) { rc = code; return end(e != hipSuccess); }   // (a runtime failure is never a refusal)
private:
    int64_t tile[2] = {0, 0}; hipEvent_t ev = nullptr;
    StageBuf pin{nullptr, 0}, dev[4]; int ndev = 0; std::vector<uint8_t> pageable;
    bool open = false, enqueued = false;
    int end(bool settle)
    {
        if (settle && ok()) e = hipEventRecord(ev, ctx->copy_stream);
        if (settle && ok()) e = hipEventSynchronize(ev);
        if (settle ? !ok() : enqueued) (void)hipStreamSynchronize(ctx->copy_stream);   // nothing may still read the staging buffers when they are reused
        for (int k = 0; k < ndev; k++) stage_put<false>(ctx, dev[k]);
        stage_put<true>(ctx, pin);
        ndev = 0; pin.ptr = nullptr; open = false;
        if (settle) fill_pair_settle(ctx, tile[0], tile[1], ok());
        if (e != hipSuccess) { vfsms_set_error("%s: %s", who, hipGetErrorString(e)); return VFSMS_ERR_HIP; }
        return rc;
    }
};
