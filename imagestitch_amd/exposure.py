"""Per-tile exposure compensation from overlap statistics (Method.exposureCompensation = "gain").

Lamps warm up, auto-exposure steps and detector gain wanders while a grid is scanned: the tiles of a mosaic differ in brightness by a
factor each, and a blend only smears the step over the overlap.  Here

  1. overlap_edges finds, from the offsets the mosaic is laid out by, every pair of tiles that share pixels -- corner neighbours too;
  2. one engine call (Engine.overlap_stats_batch, csrc/exposure_kernels.hip, specified by tests/exposure_ref.py) counts the samples of
     every overlap that are unclipped in both tiles and sums them on either side;
  3. solve_gains fits one gain per tile by ONE weighted least-squares fit in the log domain over the measured edges -- the same kind of
     fit as adjust.solve_positions, without a prior and without tuning constants;
  4. one engine call (Engine.exposure_apply) multiplies the resident tiles in place by their Q12 gains.

Everything but the two engine calls is numpy on the host: the solve is a dense system per connected component of the tile graph (a few
thousand tiles at most), not a hot path.  All tiles must be resident on ONE device: the pair-sharded registration is out of scope, as it
is for adjust.adjust_offsets.
"""
import numpy as np

from .adjust import path_positions

GAIN_ONE = 4096              # Q12


def overlap_edges(shapes, offsets, min_pixels):
    """Every pair a < b of tiles whose rectangles, under path_positions(offsets), share at least min_pixels pixels (and at least one)
    -> int64 [E, 4] = (a, b, dx, dy), sorted by (a, b), (dx, dy) = position of b minus position of a: tile b's pixel (r, c) meets tile
    a's pixel (r + dx, c + dy).  Tiles may differ in size."""
    P = path_positions(offsets)
    n = len(P)
    if n != len(shapes):
        raise ValueError("overlap_edges: %d offsets for %d tiles" % (n - 1, len(shapes)))
    hw = np.array([[int(s[0]), int(s[1])] for s in shapes], np.int64)
    d = P[None, :, :] - P[:, None, :]                        # d[a, b] = P[b] - P[a]
    # along one axis tile a covers [0, len_a), tile b [d, d + len_b)
    shared = np.minimum(hw[:, None, :], d + hw[None, :, :]) - np.maximum(d, 0)
    both = np.maximum(shared, 0).prod(axis=2)
    idx = np.arange(n)
    a, b = np.nonzero((both > 0) & (both >= int(min_pixels)) & (idx[None, :] > idx[:, None]))      # row-major: sorted by (a, b)
    return np.stack([a, b, d[a, b, 0], d[a, b, 1]], axis=1).astype(np.int64)


def _components(n, a, b):
    """label [n] of the connected components of the graph with edges (a_k, b_k): union-find"""
    root = list(range(n))

    def find(i):
        while root[i] != i:
            root[i] = root[root[i]]
            i = root[i]
        return i
    for u, v in zip(a.tolist(), b.tolist()):
        ru, rv = find(u), find(v)
        if ru != rv:
            root[max(ru, rv)] = min(ru, rv)
    return np.array([find(i) for i in range(n)], np.int64)


def measured_edges(stats, min_samples):
    """bool [E]: the edges whose statistic carries an exposure ratio: N >= min_samples, Sa > 0 and Sb > 0"""
    s = np.asarray(stats, np.int64).reshape(-1, 3)
    return (s[:, 0] >= int(min_samples)) & (s[:, 1] > 0) & (s[:, 2] > 0)


def solve_gains(n, edges, stats, min_samples, max_gain):
    """One gain per tile from the overlap statistics (N, Sa, Sb) of the edges (a, b, dx, dy) -> (g float64 [n], Q12 uint16 [n]).

    With l = log g, the minimiser of sum_e N_e (l_a - l_b - log(Sb_e / Sa_e))^2 over the measured edges whose log gains have mean 0 in
    every connected component (the minimum-norm solution of the weighted Laplacian): per component, the normal equations with its first
    tile held at 0 through np.linalg.solve, then the component's mean taken off.  A tile without a measured edge keeps g = 1.  g is
    clipped to [1 / max_gain, max_gain]; Q = floor(g * 4096 + 0.5)."""
    if not 1.0 <= float(max_gain) < 16.0:
        raise ValueError("solve_gains: max_gain must be in [1, 16) (a Q12 gain is a uint16)")
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    s = np.asarray(stats, np.int64).reshape(-1, 3)
    if len(e) != len(s):
        raise ValueError("solve_gains: %d edges, %d statistics" % (len(e), len(s)))
    m = measured_edges(s, min_samples)
    a, b = e[m, 0], e[m, 1]
    wgt = s[m, 0].astype(np.float64)
    t = np.log(s[m, 2].astype(np.float64) / s[m, 1].astype(np.float64))
    L = np.zeros((n, n), np.float64)
    rhs = np.zeros(n, np.float64)
    np.add.at(L, (a, a), wgt); np.add.at(L, (b, b), wgt)
    np.add.at(L, (a, b), -wgt); np.add.at(L, (b, a), -wgt)
    np.add.at(rhs, a, wgt * t); np.add.at(rhs, b, -wgt * t)
    logg = np.zeros(n, np.float64)
    label = _components(n, a, b)
    for c in np.unique(label):
        members = np.nonzero(label == c)[0]
        if len(members) < 2:
            continue
        rest = members[1:]
        x = np.zeros(len(members), np.float64)
        x[1:] = np.linalg.solve(L[np.ix_(rest, rest)], rhs[rest])
        logg[members] = x - x.mean()
    g = np.clip(np.exp(logg), 1.0 / float(max_gain), float(max_gain))
    return g, np.floor(g * float(GAIN_ONE) + 0.5).astype(np.uint16)


def edge_residual(edges, stats, g, min_samples):
    """the largest |log(g_a Sa / (g_b Sb))| over the measured edges; 0.0 when there is none"""
    e = np.asarray(edges, np.int64).reshape(-1, 4)
    s = np.asarray(stats, np.int64).reshape(-1, 3)
    m = measured_edges(s, min_samples)
    if not m.any():
        return 0.0
    g = np.asarray(g, np.float64)
    ra = np.log(g[e[m, 0]]) + np.log(s[m, 1].astype(np.float64))
    rb = np.log(g[e[m, 1]]) + np.log(s[m, 2].astype(np.float64))
    return float(np.abs(ra - rb).max())


def compensate(engine, handles, shapes, offsets, band=(1, 254), min_pixels=4096, max_gain=2.0):
    """Exposure compensation of one laid-out path whose tiles are resident on `engine`, in place -> (gains_q12 uint16 [n], report).

    handles[k] / shapes[k]: tile k of the path; offsets: the n - 1 path offsets the mosaic is laid out by.  A handle listed more than
    once is ONE tile: it gets one gain (its first listing stands for it in the graph) and is corrected once.  One overlap_stats_batch
    call over all overlap_edges with at least min_pixels shared pixels and the band (lo, hi); an edge is measured with at least
    min_pixels unclipped samples; one exposure_apply call.
    report: edges, measured, components (of the measured graph, tiles without an edge included), gain_min / gain_max (float),
    residual_before / residual_after: the largest |log(g_a Sa / (g_b Sb))| over the measured edges with g = 1 and with the gains the
    tiles were multiplied by (the Q12 values)."""
    n = len(shapes)
    off = np.asarray(offsets, np.int64).reshape(-1, 2)
    if len(handles) != n or len(off) != n - 1:
        raise ValueError("compensate: %d handles, %d shapes, %d offsets" % (len(handles), n, len(off)))
    lo, hi = int(band[0]), int(band[1])
    first = {}
    for k, h in enumerate(handles):
        first.setdefault(h, k)
    rep = np.array([first[h] for h in handles], np.int64)    # the listing that stands for tile k
    edges = overlap_edges(shapes, off, min_pixels)
    edges = edges[(rep[edges[:, 0]] == edges[:, 0]) & (rep[edges[:, 1]] == edges[:, 1])]
    stats = np.asarray(engine.overlap_stats_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in edges.tolist()], lo, hi),
                       np.int64).reshape(-1, 3)
    g, q = solve_gains(n, edges, stats, min_pixels, max_gain)
    g, q = g[rep], q[rep]
    m = measured_edges(stats, min_pixels)
    uniq = sorted(first.values())
    if uniq:
        engine.exposure_apply([handles[k] for k in uniq], q[uniq])
    label = _components(n, edges[m, 0], edges[m, 1])
    report = dict(edges=int(len(edges)), measured=int(m.sum()), components=int(len(np.unique(label[uniq]))),
                  gain_min=float(g.min()) if n else 1.0, gain_max=float(g.max()) if n else 1.0, band=[lo, hi],
                  residual_before=edge_residual(edges, stats, np.ones(n), min_pixels),
                  residual_after=edge_residual(edges, stats, q.astype(np.float64) / GAIN_ONE, min_pixels))
    return q, report
