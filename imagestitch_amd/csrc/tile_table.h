// tile_table.h -- the context's table of resident tiles (vfsms_ctx::tiles, tile_pool; the records are common.h's, beside the context that
// holds them): how a tile enters it, how a handle is looked up and handed over, how a buffer goes back to the pool, and what a call that
// takes a LIST of handles checks, in which order.  Host C++ over common.h and the runtime API, no kernels, no launchers: libvfsms and
// tools/tile_table_host_check.cpp (host sanitizers, failures injected) compile the same lines.
//
// Threads.  The map's structure (insert, erase, lookup), every member of a TileRec but two, the buffer pool, the event pool and the arena
// belong to the CONTEXT'S OWN THREAD: upload, reserve, wrap, free and every call that names a tile must come from it.  The two members are
// TileRec::fill and TileRec::pending: decoder threads write them (vfsms_tile_fill*, ingest_fill.h), so every thread reads and writes them
// under tiles_mu, and whoever changes `fill` notifies tiles_cv.  The decoder threads look their tiles up under the same mutex, which is why
// the inserts and erases of the context's thread take it too; its own lookups need not (nobody else changes the structure, and references
// into an unordered_map survive inserts).  ingest_fill.h and tile_is_filled (api.hip) are the lookups that run on other threads.
#pragma once
#include "common.h"
#include <algorithm>
#include <functional>

// a tile record of h x w x ch pixels at ptr, rows `stride` bytes apart; owned: the library's allocation (of h * w * ch bytes), else the
// caller's memory (vfsms_tile_wrap).  Filled, with no event and nothing pending: the caller sets what differs
static inline TileRec tile_rec(uint8_t *ptr, int h, int w, int ch, int stride, bool owned)
{
    TileRec t;
    t.ptr = ptr; t.h = h; t.w = w; t.ch = ch; t.stride = stride; t.owned = owned; t.bytes = owned ? (size_t)h * w * ch : 0;
    return t;
}
// the only place a tile enters the map
static inline void tile_register(vfsms_ctx *ctx, const TileRec &rec, int64_t *handle)
{
    std::lock_guard<std::mutex> lk(ctx->tiles_mu);             // (decoder threads look tiles up concurrently)
    *handle = ctx->next_handle++;
    ctx->tiles[*handle] = rec;
}
// The only place a buffer enters the pool.  The pool is capped by bytes (colour tiles of a mosaic are three times a gray one) and by
// entries; a buffer beyond the caps is freed behind a synchronisation.  in_use: work enqueued on the compute stream may still read the
// buffer (vfsms_tile_free: canvas paste / resident fuse return early), so the entry carries an event recorded there, and the stream that
// writes the buffer next waits for it (tile_buffer, api.hip).  An error leaves the buffer with the caller
static inline int tile_pool_return(vfsms_ctx *ctx, uint8_t *ptr, size_t bytes, bool in_use)
{
    if (ctx->tile_pool.size() < 256 && ctx->tile_pool_bytes + bytes <= ((size_t)8 << 30)) {
        PoolEnt e{bytes, ptr, nullptr};
        if (in_use) {
            if (!ctx->event_pool.empty()) { e.idle = ctx->event_pool.back(); ctx->event_pool.pop_back(); }
            else HIP_TRY(hipEventCreateWithFlags(&e.idle, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(e.idle, ctx->stream));
        }
        ctx->tile_pool.push_back(e);
        ctx->tile_pool_bytes += e.bytes;
    } else { HIP_TRY(hipStreamSynchronize(ctx->stream)); HIP_TRY(hipFree(ptr)); }
    return VFSMS_OK;
}
// the record behind a handle, on the context's thread; the pointer stays good until the tile is freed
static inline int tile_find(vfsms_ctx *ctx, const char *who, int64_t handle, TileRec **t)
{
    auto it = ctx->tiles.find(handle);
    if (it == ctx->tiles.end()) { vfsms_set_error("%s: unknown tile handle", who); return VFSMS_ERR_BAD_ARG; }
    *t = &it->second;
    return VFSMS_OK;
}
// the hand-over: wait for the decoder thread that owes a reserved tile its pixels, and make the compute stream wait for a tile's
// asynchronous upload (once)
static inline int tile_ready(vfsms_ctx *ctx, TileRec &t)
{
    std::unique_lock<std::mutex> lk(ctx->tiles_mu);
    if (t.fill) {                                            // reserved: block until its decoder thread has handed the pixels over
        ctx->tiles_cv.wait(lk, [&] { return t.fill != 1; });
        if (t.fill == 2) { vfsms_set_error("a reserved tile was never filled (its decoder reported a failure)"); return VFSMS_ERR_BAD_ARG; }
    }
    if (t.pending) { HIP_TRY(hipStreamWaitEvent(ctx->stream, t.ready, 0)); t.pending = false; }
    return VFSMS_OK;
}

// a handed-over tile as the launchers take it: pointer, row stride in bytes, rows, columns, channels
struct TileView { uint8_t *ptr; int stride, h, w, ch; };
static inline TileView tile_view(const TileRec &t) { return TileView{t.ptr, t.stride, t.h, t.w, t.ch}; }

// what a call asks of the tiles it is given as a list
struct TileRule {
    int lo, hi;                       // the count
    bool got;                         // the count's refusal says what it got
    const char *noun;                 // "tile" or "plane": what the shape refusal calls them
    bool gray_or_bgr;                 // 1 or 3 channels each
    bool same_shape;                  // every tile h x w x ch of tile 0
    bool rewritten;                   // the call writes the tiles: owned by the library (not from vfsms_tile_wrap), none named twice
    std::function<int(int, const TileRec &)> pred;   // (index, record) -> a VFSMS code, the error set: a rule of the caller's own, or empty
};
// The tiles a call names, judged and then handed over.  The order, for every caller:
//   1. the count and the null pointer;
//   2. every handle known, in index order;
//   3. per tile, in index order: channels, shape against tile 0, owned, the caller's predicate;
//   4. no handle twice;
//   5. tile_ready, in index order.
// 1 - 4 read arguments and tile records only.  A call that fails them has blocked on no decoder thread and enqueued nothing: no
// tile_ready runs before all of them have passed.  Of several faults the first in this order is the one reported.
static inline int tile_list(vfsms_ctx *ctx, const char *who, const TileRule &rule, const int64_t *tiles, int n, std::vector<TileView> &out)
{
    if (n < rule.lo || n > rule.hi || !tiles) {
        if (rule.got) vfsms_set_error("%s: %d..%d tiles, got %d", who, rule.lo, rule.hi, n);
        else vfsms_set_error("%s: %d..%d tiles", who, rule.lo, rule.hi);
        return VFSMS_ERR_BAD_ARG;
    }
    std::vector<TileRec *> T(n);
    for (int i = 0; i < n; i++) TRY(tile_find(ctx, who, tiles[i], &T[i]));
    for (int i = 0; i < n; i++) {
        const TileRec &t = *T[i], &t0 = *T[0];
        if (rule.gray_or_bgr && t.ch != 1 && t.ch != 3) { vfsms_set_error("%s: tile %d has %d channels (1 or 3)", who, i, t.ch); return VFSMS_ERR_BAD_ARG; }
        if (rule.same_shape && (t.h != t0.h || t.w != t0.w || t.ch != t0.ch)) {
            vfsms_set_error("%s: %s %d is %d x %d x %d, %s 0 is %d x %d x %d", who, rule.noun, i, t.h, t.w, t.ch, rule.noun, t0.h, t0.w, t0.ch);
            return VFSMS_ERR_BAD_ARG;
        }
        if (rule.rewritten && !t.owned) {
            vfsms_set_error("%s: tile %d comes from vfsms_tile_wrap: the library does not own its memory and does not rewrite it", who, i);
            return VFSMS_ERR_BAD_ARG;
        }
        if (rule.pred) TRY(rule.pred(i, t));
    }
    if (rule.rewritten) {
        std::vector<int64_t> seen(tiles, tiles + n);
        std::sort(seen.begin(), seen.end());
        if (std::adjacent_find(seen.begin(), seen.end()) != seen.end()) { vfsms_set_error("%s: a tile is named twice (it would be corrected twice)", who); return VFSMS_ERR_BAD_ARG; }
    }
    out.resize(n);
    for (int i = 0; i < n; i++) { TRY(tile_ready(ctx, *T[i])); out[i] = tile_view(*T[i]); }
    return VFSMS_OK;
}
