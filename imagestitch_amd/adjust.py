"""Global tile placement from correlation-refined neighbour offsets (Method.globalAdjust = "ncc").

The registration paths measure the offsets of CONSECUTIVE tiles of the shooting path only, and the mosaic is laid out by summing them
(Stitcher._layout): two tiles side by side in neighbouring columns of a serpentine are linked through up to 2 * rows - 1 path pairs, their
shared edge is never looked at, and the +-1 px errors of the votes add up into seams between the columns.  Here

  1. neighbour_edges finds, from the path offsets, every pair of tiles that are SIDE neighbours -- also across the path;
  2. one engine call (Engine.ncc_search_batch, csrc/adjust_kernels.hip, specified by tests/ncc_search_ref.py) searches a window of
     offsets around each predicted one with the verifier's statistic (tests/verify_ref.py);
  3. solve_positions places all tiles by ONE unweighted least-squares fit over the measured edges;
  4. the rounded positions, differenced along the path, are the adjusted offsetList.

Everything but the engine call is numpy on the host: the solve is a dense n x n system for n tiles (a few thousand at most), not a hot
path.  All tiles must be resident on ONE device: the pair-sharded registration (GridRegistrar.register_sharded) keeps only a rank's chunk
there and is out of scope.
"""
import numpy as np

FIXED_ONE = 1 << 20          # the engine reports scores as floor(score * 2^20 + 0.5) (include/vfsms.h: VFSMS_VERIFY_FIXED_ONE)


def _common_shape(shapes):
    hw = {(int(s[0]), int(s[1])) for s in shapes}
    if len(hw) != 1:
        raise ValueError("global adjustment needs tiles of one size, got %s" % sorted(hw))
    return hw.pop()


def path_positions(offsets):
    """int64 [n, 2]: tile origins as the cumulative sum of the path offsets, tile 0 at (0, 0)"""
    off = np.asarray(offsets, np.int64).reshape(-1, 2)
    return np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(off, axis=0)])


def neighbour_edges(shapes, offsets, radius, min_overlap=16):
    """Every pair a < b of tiles that are side neighbours under the positions the path offsets predict -> int64 [E, 4] = (a, b, dx, dy),
    sorted by (a, b), (dx, dy) = position of b minus position of a (the offset convention of offsetList).  With h_o = h - |dx| and
    w_o = w - |dy|: (h_o >= h / 2 and w_o - radius >= min_overlap) or (w_o >= w / 2 and h_o - radius >= min_overlap) -- a strip along a
    whole side that is still min_overlap wide at the far end of the search window; corner neighbours are not edges.  The pairs of the
    path (b = a + 1) are always included."""
    h, w = _common_shape(shapes)
    P = path_positions(offsets)
    n = len(P)
    if n != len(shapes):
        raise ValueError("neighbour_edges: %d offsets for %d tiles" % (n - 1, len(shapes)))
    d = P[None, :, :] - P[:, None, :]                        # d[a, b] = P[b] - P[a]
    ho, wo = h - np.abs(d[..., 0]), w - np.abs(d[..., 1])
    R = int(radius)
    side = ((2 * ho >= h) & (wo - R >= min_overlap)) | ((2 * wo >= w) & (ho - R >= min_overlap))
    idx = np.arange(n)
    side |= idx[None, :] == idx[:, None] + 1
    side &= idx[None, :] > idx[:, None]
    a, b = np.nonzero(side)                                  # row-major: sorted by (a, b)
    return np.stack([a, b, d[a, b, 0], d[a, b, 1]], axis=1).astype(np.int64)


def solve_positions(n, edges):
    """Unweighted least squares over sum |P_b - P_a - d_e|^2 with P_0 = 0: edges = rows (a, b, dx, dy) -> float64 [n, 2].  The reduced
    normal equations (the graph Laplacian without tile 0) through np.linalg.solve.  When the edges are consistent -- the rounded solution
    meets every one of them exactly, so it IS the minimiser -- the integers themselves are returned."""
    e = np.asarray(edges, np.float64).reshape(-1, 4)
    a, b = e[:, 0].astype(np.int64), e[:, 1].astype(np.int64)
    L = np.zeros((n, n), np.float64)
    rhs = np.zeros((n, 2), np.float64)
    np.add.at(L, (a, a), 1.0); np.add.at(L, (b, b), 1.0)
    np.add.at(L, (a, b), -1.0); np.add.at(L, (b, a), -1.0)
    np.add.at(rhs, b, e[:, 2:4]); np.add.at(rhs, a, -e[:, 2:4])
    P = np.zeros((n, 2), np.float64)
    if n > 1:
        P[1:] = np.linalg.solve(L[1:, 1:], rhs[1:])
    Pr = np.rint(P)
    if len(e) and np.array_equal(Pr[b] - Pr[a], e[:, 2:4]):
        return Pr
    return P


def _residuals(P, edges):
    """(max, rms) of the Euclidean residual |P_b - P_a - d_e| over the edges"""
    if not len(edges):
        return 0.0, 0.0
    e = np.asarray(edges, np.float64)
    r = P[e[:, 1].astype(np.int64)] - P[e[:, 0].astype(np.int64)] - e[:, 2:4]
    m = np.sqrt((r * r).sum(axis=1))
    return float(m.max()), float(np.sqrt((m * m).mean()))


def adjust_offsets(engine, handles, shapes, offsets, radius=4, threshold=0.5, min_pixels=4096, min_overlap=16):
    """The adjusted offsetList of one registered path whose gray tiles are resident on `engine` -> (offsets [[dx, dy], ...], report).

    One ncc_search_batch call over all neighbour_edges, centred on the offsets the path predicts.  An edge is MEASURED when its best
    score reaches `threshold` (compared as the fixed-point integers the engine reports) and the peak is bracketed by the window
    (|i| < radius and |j| < radius): its offset is then the refined one.  An unmeasured edge across the path is dropped; an unmeasured
    pair of the path keeps its voted offset, so the graph stays connected.  The positions of solve_positions are rounded half up
    (floor(P + 0.5)) and differenced along the path.
    report: edges, measured, dropped, kept_votes, and the maximum / RMS edge residual (px, over the edges that entered the fit) of the
    voted positions (`residual_before`) and of the rounded adjusted ones (`residual_after`).
    All tiles on one device: the sharded registration is out of scope."""
    n = len(shapes)
    off = np.asarray(offsets, np.int64).reshape(-1, 2)
    if len(handles) != n or len(off) != n - 1:
        raise ValueError("adjust_offsets: %d handles, %d shapes, %d offsets" % (len(handles), n, len(off)))
    R = int(radius)
    edges = neighbour_edges(shapes, off, R, min_overlap)
    best = np.asarray(engine.ncc_search_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in edges.tolist()], R, int(min_pixels)),
                      np.int64).reshape(-1, 4)
    on_path = edges[:, 1] == edges[:, 0] + 1
    measured = (best[:, 2] >= int(np.floor(float(threshold) * FIXED_ONE + 0.5))) & (np.abs(best[:, 0]) < R) & (np.abs(best[:, 1]) < R)
    used = edges[measured | on_path].copy()
    used[:, 2:4] += np.where(measured[:, None], best[:, 0:2], 0)[measured | on_path]
    P0 = path_positions(off).astype(np.float64)
    P = np.floor(solve_positions(n, used) + 0.5)
    adjusted = (P[1:] - P[:-1]).astype(np.int64)
    before, after = _residuals(P0, used), _residuals(P, used)
    report = dict(edges=int(len(edges)), measured=int(measured.sum()), dropped=int((~measured & ~on_path).sum()),
                  kept_votes=int((~measured & on_path).sum()), radius=R,
                  residual_before=dict(max=before[0], rms=before[1]), residual_after=dict(max=after[0], rms=after[1]))
    return [[int(v[0]), int(v[1])] for v in adjusted], report
