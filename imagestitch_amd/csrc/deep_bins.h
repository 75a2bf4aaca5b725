// deep_bins.h -- the bin table of the 16-bit mosaic gather (vfsms_deep_mosaic_rows; deep_kernels.hip: k_deep_mosaic).
// Plain host C++, no HIP, no kernels: libvfsms and tools/deep_bins_host_check.cpp (host sanitizers, random layouts against a brute-force
// intersection) compile the same lines.
//
// A band is rows [row0, row0 + nrows) of a canvas `cols` wide, cut into blocks of DEEP_BIN_H x DEEP_BIN_W pixels, row-major: block
// (by, bx) holds band rows [by * DEEP_BIN_H, ...) and columns [bx * DEEP_BIN_W, ...).  One workgroup gathers one block, and the table tells
// it which tiles to walk: in CSR form, list[start[b] .. start[b + 1]) are the indices of the tiles whose rectangle meets block b, ASCENDING
// (the paste mode keeps the covering tile of the largest index, so the walk's order is part of the contract).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <vector>

#define DEEP_BIN_H 32
#define DEEP_BIN_W 256

struct DeepRect { int y0, x0, h, w; };                       // a tile on the canvas: top-left corner, rows, columns

struct DeepBins {
    int nby = 0, nbx = 0;                                    // blocks down and across the band
    std::vector<uint32_t> start;                             // nby * nbx + 1
    std::vector<uint32_t> list;
};

// blocks of the band that tile r meets: [by0, by1] x [bx0, bx1]; false: none (the tile misses the band).  64-bit throughout: y0 + h and
// row0 + nrows may reach 2^31
static inline bool deep_bins_span(const DeepRect &r, int row0, int nrows, int *by0, int *by1, int *bx0, int *bx1)
{
    const long long ya = r.y0 > row0 ? r.y0 : row0;
    const long long yb_t = (long long)r.y0 + r.h, yb_b = (long long)row0 + nrows;
    const long long yb = yb_t < yb_b ? yb_t : yb_b;          // exclusive
    if (ya >= yb || r.w <= 0) return false;
    *by0 = (int)((ya - row0) / DEEP_BIN_H); *by1 = (int)((yb - 1 - row0) / DEEP_BIN_H);
    *bx0 = r.x0 / DEEP_BIN_W; *bx1 = (int)(((long long)r.x0 + r.w - 1) / DEEP_BIN_W);
    return true;
}

// The table of n tiles (each inside the canvas: 0 <= x0, x0 + w <= cols; the caller has checked) for one band.  false, nothing usable in
// `out`: the table would hold more than max_entries list entries or blocks.
static inline bool deep_bins_build(const DeepRect *tiles, int n, int cols, int row0, int nrows, size_t max_entries, DeepBins *out)
{
    const long long nby = ((long long)nrows + DEEP_BIN_H - 1) / DEEP_BIN_H, nbx = ((long long)cols + DEEP_BIN_W - 1) / DEEP_BIN_W;
    if (nby <= 0 || nbx <= 0 || (unsigned long long)(nby * nbx) > max_entries) return false;
    out->nby = (int)nby; out->nbx = (int)nbx;
    const size_t nb = (size_t)(nby * nbx);
    out->start.assign(nb + 1, 0);
    unsigned long long total = 0;
    for (int t = 0; t < n; t++) {                            // counts, one slot ahead: start[b + 1] = entries of block b
        int by0, by1, bx0, bx1;
        if (!deep_bins_span(tiles[t], row0, nrows, &by0, &by1, &bx0, &bx1)) continue;
        total += (unsigned long long)(by1 - by0 + 1) * (unsigned long long)(bx1 - bx0 + 1);
        if (total > max_entries) return false;
        for (int by = by0; by <= by1; by++)
            for (int bx = bx0; bx <= bx1; bx++) out->start[(size_t)by * nbx + bx + 1]++;
    }
    for (size_t b = 0; b < nb; b++) out->start[b + 1] += out->start[b];
    out->list.assign((size_t)total, 0);
    std::vector<uint32_t> fill(out->start.begin(), out->start.end() - 1);
    for (int t = 0; t < n; t++) {                            // in tile order: every block's list ascends
        int by0, by1, bx0, bx1;
        if (!deep_bins_span(tiles[t], row0, nrows, &by0, &by1, &bx0, &bx1)) continue;
        for (int by = by0; by <= by1; by++)
            for (int bx = bx0; bx <= bx1; bx++) out->list[fill[(size_t)by * nbx + bx]++] = (uint32_t)t;
    }
    return true;
}
