// canvas_band.h -- the band walk behind the four write-out routes of a canvas (vfsms_canvas_download_rows, .._download_rows_pyramid,
// .._encode_jpeg_rows, and the tile route .._encode_pyramid_tiles / .._encode_pyramid_tiles_deflate of api.hip; .._encode_png_rows uses the
// check and the flag alone: it keeps no state between bands): the one band check, the one reader of the sticky geometry flag, the
// operations of PyrPending, the rows of the reduced levels that wait between the bands of the tile route, and canvas_tile_band, the one
// driver of a band of that route -- begin to index, the capacity protocol included -- over a coder that api.hip supplies (JPEG, deflate).
// Host C++ over common.h and the runtime API, no kernels, no launchers: libvfsms and tools/canvas_band_host_check.cpp (host sanitizers,
// failures injected, a stub coder) compile the same lines.
#pragma once
#include "common.h"
#include <algorithm>
#include <initializer_list>

// The band contract: rows [row0, row0 + nrows) lie in the canvas; the band starts on a multiple of every unit and is a multiple of it long
// unless it ends at the last row.  `args_ok`: the entry's own pointers
struct BandUnit { int unit; const char *name; };
static int canvas_band_check(const char *who, bool args_ok, int rows, int row0, int nrows, std::initializer_list<BandUnit> units)
{
    if (!args_ok || row0 < 0 || nrows <= 0 || (long long)row0 + nrows > rows) { vfsms_set_error("%s: bad arguments", who); return VFSMS_ERR_BAD_ARG; }
    for (const BandUnit &u : units) {
        if (row0 % u.unit) { vfsms_set_error("%s: row0 = %d is not a multiple of %s = %d", who, row0, u.name, u.unit); return VFSMS_ERR_BAD_ARG; }
        if (nrows % u.unit && row0 + nrows != rows) {
            vfsms_set_error("%s: nrows = %d is not a multiple of %s = %d and the band does not end at the last row", who, nrows, u.name, u.unit);
            return VFSMS_ERR_BAD_ARG;
        }
    }
    return VFSMS_OK;
}

// The sticky "degenerate fuse geometry" flag of the fuses that ran without a readback leaves with the band: the copy is enqueued with the
// band's work, and behind the synchronisation that ends that work a set flag is the one error
static int canvas_flag_read(vfsms_ctx *ctx, const CanvasRec *cv, int *flag)
{
    HIP_TRY(hipMemcpyAsync(flag, cv->d_err.as<int>(), sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    return VFSMS_OK;
}
static int canvas_flag_verdict(int flag)
{
    if (!flag) return VFSMS_OK;
    vfsms_set_error("fuse: degenerate corner geometry in one of the fused tiles (the reference's getWeightsMatrix raises there)");
    return VFSMS_ERR_BAD_ARG;
}

// ---- PyrPending: the tile route's state between its bands ----------------------------------------------------------------------------------
// Level k's slot in the buffer for bands of up to `nrows` rows: the rows that may be pending (fewer than a tile row) and the band's share,
// tile - 1 + ceil(nrows / 2^k) rows, on a 256-byte boundary.  off[1 .. levels] = the slots; returns the buffer's size
static size_t pyr_pending_layout(const int *C, int ch, int tile, int levels, int nrows, size_t *off)
{
    size_t at = 0;
    for (int k = 1; k <= levels; k++) {
        off[k] = at;
        at += ((size_t)(tile - 1 + ((nrows + (1 << k) - 1) >> k)) * C[k] * ch + 255) & ~(size_t)255;
    }
    return at;
}

// what a band completes: the jobs of the levels with whole tile rows (level after level), and per level the rows at hand (`total`: pending
// plus the band's share, which the reduction writes at lvl[k]) and those of them that leave in tile rows now (`full`)
struct PyrPlan {
    JpegTileJob jobs[VFSMS_PYRAMID_MAX_LEVELS + 1]; int job_level[VFSMS_PYRAMID_MAX_LEVELS + 1], n_jobs = 0;
    int full[VFSMS_PYRAMID_MAX_LEVELS + 1] = {}, total[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
    uint8_t *lvl[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
    long long n_tiles = 0; int tile = 0, row_end = 0;
    // the records {level, tile number in the level, offset, bytes} of the planned tiles, given their offsets in the payload
    void index(const unsigned long long *tile_offs, int64_t *index) const
    {
        size_t g = 0;
        for (int j = 0; j < n_jobs; j++) {
            const int ntx = (jobs[j].cols + tile - 1) / tile;
            const long long first = (long long)(jobs[j].row0 / tile) * ntx;
            for (long long t = 0; t < (long long)jobs[j].tile_rows * ntx; t++, g++) {
                index[4 * g] = job_level[j]; index[4 * g + 1] = first + t;
                index[4 * g + 2] = (int64_t)tile_offs[g]; index[4 * g + 3] = (int64_t)(tile_offs[g + 1] - tile_offs[g]);
            }
        }
    }
};

// A band at row 0 starts a walk: nothing is pending, the buffer is sized for this band.  Any other band continues one: it is the band
// expected, with the walk's coder, tile and level count, or it is refused and the state stays as it was; a longer band than the buffer was sized
// for makes a larger buffer take the pending rows over (the record owns the old buffer with the old slots until the new one holds them)
inline int PyrPending::begin(const char *who, int rows, int cols, int ch_, int row0, int nrows, int tile_, int levels_, hipStream_t stream, int codec_)
{
    if (row0 == 0) {
        levels = -1;                                              // (no walk to continue if the buffer cannot be had)
        ch = ch_; R[0] = rows; C[0] = cols;
        for (int k = 1; k <= VFSMS_PYRAMID_MAX_LEVELS; k++) { R[k] = (R[k - 1] + 1) >> 1; C[k] = (C[k - 1] + 1) >> 1; }
        TRY(buf.reserve(pyr_pending_layout(C, ch, tile_, levels_, nrows, off), stream));
        for (int k = 1; k <= levels_; k++) base[k] = have[k] = 0;
        tile = tile_; levels = levels_; band = nrows; next = 0; codec = codec_;
    } else if (levels >= 0 && codec != codec_) {
        vfsms_set_error("%s: the walk in progress feeds the %s coder: a band of the other coder continues no walk (row0 = 0 starts one)", who, codec == VFSMS_PYR_CODEC_DEFLATE ? "deflate" : "JPEG");
        return VFSMS_ERR_BAD_ARG;
    } else if (tile != tile_ || levels != levels_ || next != row0) {
        vfsms_set_error("%s: bands arrive in order from row 0 with one tile and level count (expected row0 = %d, got %d)", who, levels < 0 ? 0 : next, row0);
        return VFSMS_ERR_BAD_ARG;
    } else if (nrows > band) {
        DevBuf grown; size_t noff[VFSMS_PYRAMID_MAX_LEVELS + 1] = {};
        TRY(grown.reserve(pyr_pending_layout(C, ch, tile, levels, nrows, noff), stream));
        for (int k = 1; k <= levels; k++)
            if (have[k]) HIP_TRY(hipMemcpyAsync(grown.as<uint8_t>() + noff[k], buf.as<uint8_t>() + off[k], (size_t)have[k] * C[k] * ch, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));                    // (the old buffer is freed by the move)
        buf = std::move(grown);
        for (int k = 1; k <= levels; k++) off[k] = noff[k];
        band = nrows;
    }
    return VFSMS_OK;
}

// Arithmetic only: level 0's tile rows of the band, and of level k the whole tile rows of its pending rows plus the band's share -- all of
// them when the band ends the canvas.  Nothing changes: the same band plans the same again
inline int PyrPending::plan(const char *who, const uint8_t *pix, int row0, int nrows, PyrPlan *p) const
{
    const bool last = row0 + nrows == R[0];
    *p = PyrPlan();
    p->tile = tile; p->row_end = row0 + nrows;
    long long mrows = 0;
    for (int k = 0; k <= levels; k++) {
        JpegTileJob J;
        const size_t pitch = (size_t)C[k] * ch;
        if (k == 0) { J = {pix, (size_t)R[0] * pitch, pitch, 0, R[0], C[0], row0, (nrows + tile - 1) / tile}; p->full[0] = p->total[0] = nrows; }
        else {
            uint8_t *slot = buf.as<uint8_t>() + off[k];
            p->lvl[k] = slot + (size_t)have[k] * pitch;
            p->total[k] = have[k] + (int)((((long long)row0 + nrows + (1 << k) - 1) >> k) - (row0 >> k));
            p->full[k] = last ? p->total[k] : p->total[k] / tile * tile;
            J = {slot, (size_t)p->total[k] * pitch, pitch, base[k], R[k], C[k], base[k], (p->full[k] + tile - 1) / tile};
        }
        if (J.tile_rows == 0) continue;
        p->jobs[p->n_jobs] = J; p->job_level[p->n_jobs++] = k;
        p->n_tiles += (long long)J.tile_rows * ((C[k] + tile - 1) / tile);
        mrows = std::max(mrows, (long long)J.tile_rows * (tile / 8));
    }
    if (mrows > 65535 || p->n_tiles > 0x7fffffff) { vfsms_set_error("%s: a band of %d rows is more tile rows than one call takes", who, nrows); return VFSMS_ERR_BAD_ARG; }
    return VFSMS_OK;
}

// The planned tile rows are encoded (the coefficients hold everything the streams need): the rows behind them move to the front of their
// slots for the next band
inline int PyrPending::commit(const PyrPlan &p, hipStream_t stream)
{
    for (int k = 1; k <= levels; k++) {
        const size_t pitch = (size_t)C[k] * ch;
        const int rem = p.total[k] - p.full[k];
        uint8_t *slot = buf.as<uint8_t>() + off[k];
        if (rem > 0 && p.full[k] > 0) HIP_TRY(hipMemcpyAsync(slot, slot + (size_t)p.full[k] * pitch, (size_t)rem * pitch, hipMemcpyDeviceToDevice, stream));
        base[k] += p.full[k]; have[k] = rem;
    }
    next = p.row_end;
    return VFSMS_OK;
}

// ---- the tile route's band: one driver, whichever coder ------------------------------------------------------------------------------------------
// A Coder is a small struct: `codec`, its VFSMS_PYR_CODEC_* tag; count(jobs, n_jobs, d_flag, &flag), the counting half, which leaves
// run.tile_offs[0 .. n_tiles] on the host and the int at d_flag in flag behind one synchronisation; write(out), the writing half.  reduce(lvl)
// forms the band's share of levels 1 .. levels where the plan says (the caller's launcher: none lives here).  The order of the steps is the
// contract: 1 begin (the band continues the walk or is refused with the walk as it was), 2 plan (arithmetic only), 3 *n_index, 4 reduce,
// 5 count, with the sticky geometry flag, 6 the flag's verdict, 7 *nbytes, 8 the capacity refusal -- both sizes reported, nothing written and
// NOTHING CONSUMED: the same band may come again and plans the same --, 9 commit, the only step that consumes rows, behind every refusal and
// in front of the write (the coder's scratch holds everything the streams need), 10 write, 11 index
template <class Coder, class Reduce>
static int canvas_tile_band(vfsms_ctx *ctx, CanvasRec *cv, const char *who, int row0, int nrows, int levels, int tile, Coder &coder, Reduce &&reduce,
                            uint8_t *out, size_t cap, size_t *nbytes, int64_t *index, int index_cap, int *n_index)
{
    PyrPending &P = cv->pend;
    PyrPlan plan;
    TRY(P.begin(who, cv->rows, cv->cols, cv->ch, row0, nrows, tile, levels, ctx->stream, coder.codec));
    TRY(P.plan(who, cv->pix.as<uint8_t>(), row0, nrows, &plan));
    *n_index = (int)plan.n_tiles;
    if (levels > 0) TRY(reduce(plan.lvl));
    int flag = 0;                                                  // the sticky geometry flag comes back with the sizes
    TRY(coder.count(plan.jobs, plan.n_jobs, cv->d_err.as<int>(), &flag));
    TRY(canvas_flag_verdict(flag));
    const unsigned long long bytes = coder.run.tile_offs[(size_t)plan.n_tiles];
    *nbytes = (size_t)bytes;
    if (!out || cap < bytes || !index || index_cap < plan.n_tiles) {
        vfsms_set_error("%s: the band takes %llu bytes in %lld tiles, the buffers hold %zu bytes and %d records", who, bytes, plan.n_tiles, out ? cap : (size_t)0, index ? index_cap : 0);
        return VFSMS_ERR_CAPACITY;
    }
    TRY(P.commit(plan, ctx->stream));
    TRY(coder.write(out));
    plan.index(coder.run.tile_offs.data(), index);
    return VFSMS_OK;
}
