"""Radial lens correction estimated from the overlaps of the registered tiles (Method.lensCorrection; no reference counterpart,
tests/lens_ref.py is the specification).

Every registration path here measures ONE translation per pair and every fuse assumes that a translation is all that separates two
tiles.  An objective, and more so an SEM column, adds radial distortion: along a shared side the true displacement then bows
quadratically, and the blend smears what the translation leaves into ghosting at both ends of every overlap.  Here

  1. block_first / one engine call (Engine.block_ncc_batch, csrc/lens_kernels.hip) measure the displacement of every block x block
     square of every overlap of adjust.neighbour_edges with the verifier's statistic (tests/verify_ref.py);
  2. fit_radial fits ONE undistorting function u(s) = s (1 + b1 rho^2) per dataset from them -- no calibration target;
  3. one engine call (Engine.lens_apply) resamples the resident tiles in place under the series inverse of it;
  4. a second block_ncc_batch on the corrected tiles moves the path offsets by the median displacement that is left.

Everything but the engine calls is numpy on the host: the fit has one unknown besides the per-edge translations, not a hot path.
All tiles must be resident on ONE device and of one shape: the pair-sharded registration and per-tile models are out of scope.
"""
import numpy as np

from .adjust import neighbour_edges

FIXED_ONE = 1 << 20          # the engine reports scores as floor(score * 2^20 + 0.5) (include/vfsms.h: VFSMS_VERIFY_FIXED_ONE)
Q30 = 1 << 30
MAX_COEFFICIENT = 0.25       # |a| the resampling takes (Q30 coefficients up to 2^28)
MODES = ("estimate", "given")
INTERPOLATIONS = ("bilinear", "cubic")


def check_options(mode, block, radius, interpolation, coefficients=None):
    """Method.lensCorrection / lensBlock / lensRadius / lensInterpolation / lensCoefficients, judged before anything is measured"""
    if mode not in MODES:
        raise ValueError("lensCorrection must be 'none', 'estimate' or 'given'")
    if not 8 <= int(block) <= 128 or int(block) % 8:
        raise ValueError("lensBlock must be a multiple of 8 in 8..128, got %r" % (block,))
    if not 1 <= int(radius) <= 16:
        raise ValueError("lensRadius must lie in 1..16, got %r" % (radius,))
    if interpolation not in INTERPOLATIONS:
        raise ValueError("lensInterpolation must be 'bilinear' or 'cubic', got %r" % (interpolation,))
    if mode == "given":
        if coefficients is None or len(coefficients) != 2:
            raise ValueError("lensCorrection 'given' needs lensCoefficients = (a1, a2)")
        coefficients_q30(*coefficients)


def coefficients_q30(a1, a2):
    """(a1, a2) as the Q30 integers the resampling takes: floor(a * 2^30 + 0.5); |a| <= 0.25"""
    q = [int(np.floor(float(a) * Q30 + 0.5)) for a in (a1, a2)]
    if max(abs(v) for v in q) > Q30 // 4:
        raise ValueError("lens coefficients (%r, %r) lie outside +-%g" % (a1, a2, MAX_COEFFICIENT))
    return q[0], q[1]


def centre_half_pixels(centre):
    """Method.lensCentre (cy, cx) in pixels, or None for every tile's own middle -> (cy2, cx2) in half pixels as the engine takes them"""
    if centre is None:
        return (-1, -1)
    cy2, cx2 = (int(np.floor(2.0 * float(v) + 0.5)) for v in centre)
    if cy2 < 0 or cx2 < 0:
        raise ValueError("lensCentre %r lies outside the tile" % (centre,))
    return (cy2, cx2)


def block_lattice(shape, dx, dy, block, radius):
    """(r0, c0, nby, nbx): the overlap of an h x w pair under (dx, dy) in B's coordinates (verify_ref.overlap), shrunk by `radius` on
    all four sides and cut into whole block x block squares from its top-left corner (r0, c0); nby = nbx = 0 when none fits"""
    h, w = int(shape[0]), int(shape[1])
    dx, dy, block, radius = int(dx), int(dy), int(block), int(radius)
    r0, r1 = max(0, -dx) + radius, min(h, h - dx) - radius
    c0, c1 = max(0, -dy) + radius, min(w, w - dy) - radius
    nby, nbx = max(0, r1 - r0) // block, max(0, c1 - c0) // block
    if nby == 0 or nbx == 0:
        nby = nbx = 0
    return min(r0, h), min(c0, w), nby, nbx


def block_first(shape, offsets, block, radius):
    """int64 [n + 1] for n jobs on tiles of one shape with the offsets [(dx, dy), ...]: the index of every job's first block and the total"""
    first = np.zeros(len(offsets) + 1, np.int64)
    for k, (dx, dy) in enumerate(offsets):
        _r0, _c0, nby, nbx = block_lattice(shape, dx, dy, block, radius)
        first[k + 1] = first[k] + nby * nbx
    return first


def block_centres(shape, offsets, block, radius):
    """float64 [blocks, 2]: the centre (row, column) of every block in B's coordinates, and int64 [blocks] the job it belongs to"""
    cen, job = [], []
    for k, (dx, dy) in enumerate(offsets):
        r0, c0, nby, nbx = block_lattice(shape, dx, dy, block, radius)
        for by in range(nby):
            for bx in range(nbx):
                cen.append((r0 + by * block + (block - 1) / 2.0, c0 + bx * block + (block - 1) / 2.0))
                job.append(k)
    return np.array(cen, np.float64).reshape(-1, 2), np.array(job, np.int64)


def measured_blocks(best4, radius, threshold):
    """bool [blocks]: the best fixed-point score reaches the threshold (compared as integers) and the peak is bracketed by the window"""
    b = np.asarray(best4, np.int64).reshape(-1, 4)
    R = int(radius)
    return (b[:, 2] >= int(np.floor(float(threshold) * FIXED_ONE + 0.5))) & (np.abs(b[:, 0]) < R) & (np.abs(b[:, 1]) < R)


def subpixel(best4, surface, radius, measured):
    """float64 [blocks, 2]: (i, j) of the best candidate plus, for a measured block, the vertex of the parabola through the fixed-point
    scores on either side of it, per axis; a neighbour pair that is not concave (s- - 2 s0 + s+ >= 0) contributes 0"""
    b = np.asarray(best4, np.int64).reshape(-1, 4)
    S = np.asarray(surface, np.int64)
    R = int(radius)
    d = b[:, 0:2].astype(np.float64)
    for k in np.nonzero(measured)[0]:
        i, j = int(b[k, 0]) + R, int(b[k, 1]) + R
        s0 = float(S[k, i, j])
        for axis, (lo, hi) in enumerate(((S[k, i - 1, j], S[k, i + 1, j]), (S[k, i, j - 1], S[k, i, j + 1]))):
            den = float(lo) - 2.0 * s0 + float(hi)
            if den < 0.0:
                d[k, axis] += 0.5 * (float(lo) - float(hi)) / den
    return d


def _edge_means(values, job, use):
    """values [blocks, 2] minus the mean over the used blocks of their job"""
    out = np.zeros_like(values)
    for k in np.unique(job[use]):
        m = use & (job == k)
        out[m] = values[m] - values[m].mean(axis=0)
    return out


def _with_three(job, use):
    """the used blocks whose job has at least 3 of them"""
    cnt = np.bincount(job[use], minlength=int(job.max()) + 1 if len(job) else 1)
    return use & (cnt[job] >= 3) if len(job) else use


def displacement_spread(disp, job, measured):
    """the RMS, over the measured blocks of jobs with at least 3 of them, of the displacement about its own job's mean, in px"""
    use = _with_three(job, np.asarray(measured, bool))
    if not use.any():
        return 0.0
    r = _edge_means(disp, job, use)[use]
    return float(np.sqrt((r * r).sum(axis=1).mean()))


def fit_radial(shape, offsets, best4, surface, block, radius, threshold, min_blocks=32, min_shift=0.25, centre=None):
    """One radial model from the block displacement field of n jobs on tiles of one shape -> report.

    offsets: the jobs' (dx, dy); best4 / surface: what block_ncc_batch returned for them.  With c the centre ((h - 1) / 2, (w - 1) / 2)
    or `centre`, D^2 = ((h - 1)^2 + (w - 1)^2) / 4, s_b = block centre - c, s_a = s_b + (dx, dy) + displacement and rho^2 = |s|^2 / D^2,
    every measured block of job e says u(s_a) - u(s_b) = t_e for u(s) = s (1 + b1 rho^2): linear in b1 and t_e.  The t_e go with the
    per-job means (jobs with at least 3 measured blocks), b1 is the least-squares solution over both components; blocks whose residual
    exceeds max(0.5 px, 3 RMS) are dropped, once, and the fit repeated.  The resampling takes the inverse s(u) = u (1 + a1 rho_u^2 +
    a2 rho_u^4), a1 = -b1, a2 = 3 b1^2 (the series inverse, exact to O(b1^3)).
    report: edges, blocks, measured, trimmed, b1, a1, a2, corner_px = (a1 + a2) D, spread_before (displacement_spread), apply (bool)
    and, when not, reason: fewer than min_blocks measured blocks, or |corner_px| < min_shift (resampling would only blur)."""
    h, w = int(shape[0]), int(shape[1])
    c = np.array([(h - 1) / 2.0, (w - 1) / 2.0]) if centre is None else np.array([float(centre[0]), float(centre[1])])
    D2 = ((h - 1) ** 2 + (w - 1) ** 2) / 4.0
    D = float(np.sqrt(D2))
    cen, job = block_centres(shape, offsets, block, radius)
    b = np.asarray(best4, np.int64).reshape(-1, 4)
    if len(b) != len(cen):
        raise ValueError("fit_radial: %d blocks measured, the lattice has %d" % (len(b), len(cen)))
    measured = measured_blocks(b, radius, threshold)
    disp = subpixel(b, surface, radius, measured)
    off = np.asarray(offsets, np.float64).reshape(-1, 2)
    report = dict(edges=int(len(off)), blocks=int(len(b)), measured=int(measured.sum()), trimmed=0, b1=0.0, a1=0.0, a2=0.0, corner_px=0.0,
                  spread_before=displacement_spread(disp, job, measured), apply=False, reason=None)
    if report["measured"] < int(min_blocks):
        report["reason"] = "%d measured blocks, lensMinBlocks is %d" % (report["measured"], int(min_blocks))
        return report
    s_b = cen - c
    d = off[job] + disp if len(job) else disp                # s_a - s_b
    s_a = s_b + d
    g = s_a * ((s_a * s_a).sum(axis=1) / D2)[:, None] - s_b * ((s_b * s_b).sum(axis=1) / D2)[:, None]

    def solve(use):
        use = _with_three(job, use)
        dt, gt = _edge_means(d, job, use)[use], _edge_means(g, job, use)[use]
        den = float((gt * gt).sum())
        b1 = -float((gt * dt).sum()) / den if den > 0.0 else 0.0
        res = np.zeros(len(job), np.float64)
        res[use] = np.sqrt(((dt + b1 * gt) ** 2).sum(axis=1))
        return b1, res, use

    b1, res, use = solve(measured)
    if use.any():
        rms = float(np.sqrt((res[use] ** 2).mean()))
        keep = use & (res <= max(0.5, 3.0 * rms))
        report["trimmed"] = int(use.sum() - keep.sum())
        if report["trimmed"]:
            b1, res, use = solve(keep)
    a1, a2 = -b1, 3.0 * b1 * b1
    report.update(b1=b1, a1=a1, a2=a2, corner_px=(a1 + a2) * D)
    if abs(report["corner_px"]) < float(min_shift):
        report["reason"] = "a corner shift of %.3f px, lensMinShift is %g" % (report["corner_px"], float(min_shift))
        return report
    report["apply"] = True
    return report


def path_moves(n_tiles, edges, first, best4, radius, threshold):
    """{path pair k: (mi, mj)} for the edges (k, k + 1) with at least 3 measured blocks: the component-wise lower median of their measured
    integer (i, j)"""
    b = np.asarray(best4, np.int64).reshape(-1, 4)
    measured = measured_blocks(b, radius, threshold)
    moves = {}
    for e, (a, bb, _dx, _dy) in enumerate(np.asarray(edges, np.int64).reshape(-1, 4).tolist()):
        if bb != a + 1:
            continue
        sel = b[int(first[e]):int(first[e + 1])][measured[int(first[e]):int(first[e + 1])]]
        if len(sel) >= 3:
            moves[a] = tuple(int(np.sort(sel[:, q])[(len(sel) - 1) // 2]) for q in (0, 1))
    return moves


def correct(engine, handles, shapes, offsets, mode="estimate", coefficients=None, centre=None, block=64, radius=8, threshold=0.5,
            min_blocks=32, min_shift=0.25, interpolation="cubic"):
    """Lens correction of one registered path whose tiles (gray or B G R, one shape) are resident on `engine`, in place
    -> (offsets [[dx, dy], ...], (a1, a2) or None, report).

    One block_ncc_batch over adjust.neighbour_edges centred on the offsets the path predicts, fit_radial ("estimate") or the
    coefficients given, one lens_apply over all tiles (a handle listed more than once is ONE tile: corrected once), a second
    block_ncc_batch on the corrected tiles: every path pair with at least 3 measured blocks moves its offset by the lower median of its
    measured (i, j), the others keep theirs.  Without a correction (fit_radial's report says why) the tiles and the offsets stay as they are and
    (a1, a2) is None.  report: fit_radial's, plus spread_after and moved (the path pairs whose offset changed)."""
    check_options(mode, block, radius, interpolation, coefficients)
    n = len(shapes)
    off = np.asarray(offsets, np.int64).reshape(-1, 2)
    if len(handles) != n or len(off) != n - 1:
        raise ValueError("lens.correct: %d handles, %d shapes, %d offsets" % (len(handles), n, len(off)))
    shape = (int(shapes[0][0]), int(shapes[0][1]))
    R, B = int(radius), int(block)
    centre2 = centre_half_pixels(centre)
    edges = neighbour_edges(shapes, off, R)
    jobs = [(handles[a], handles[b], dx, dy) for a, b, dx, dy in edges.tolist()]
    eoff = [(dx, dy) for _a, _b, dx, dy in edges.tolist()]
    first = block_first(shape, eoff, B, R)
    if mode == "estimate":
        best, surface = engine.block_ncc_batch(jobs, first, B, R, want_surface=True)
        report = fit_radial(shape, eoff, best, surface, B, R, threshold, min_blocks, min_shift,
                            None if centre is None else (centre2[0] / 2.0, centre2[1] / 2.0))
        if not report["apply"]:
            report.update(spread_after=None, moved=0)
            return [[int(v[0]), int(v[1])] for v in off], None, report
        pair = (report["a1"], report["a2"])
    else:
        pair = (float(coefficients[0]), float(coefficients[1]))
        D = float(np.sqrt(((shape[0] - 1) ** 2 + (shape[1] - 1) ** 2) / 4.0))
        report = dict(edges=int(len(edges)), blocks=int(first[-1]), a1=pair[0], a2=pair[1], corner_px=(pair[0] + pair[1]) * D, apply=True, reason=None)
    q1, q2 = coefficients_q30(*pair)
    engine.lens_apply(list(dict.fromkeys(handles)), q1, q2, centre2, interpolation)
    best, surface = engine.block_ncc_batch(jobs, first, B, R, want_surface=True)
    measured = measured_blocks(best, R, threshold)
    _cen, job = block_centres(shape, eoff, B, R)
    report["spread_after"] = displacement_spread(subpixel(best, surface, R, measured), job, measured)
    moves = path_moves(n, edges, first, best, R, threshold)
    out = [[int(v[0]) + moves.get(k, (0, 0))[0], int(v[1]) + moves.get(k, (0, 0))[1]] for k, v in enumerate(off)]
    report["moved"] = sum(1 for m in moves.values() if m != (0, 0))
    return out, pair, report


def undistort(img, coefficients, centre=None, interpolation="cubic", engine=None):
    """One image, (h, w) or (h, w, ch) uint8, resampled under the radial map s(u) = u (1 + a1 rho^2 + a2 rho^4) about `centre` ((cy, cx) in
    pixels; None: the middle) on the device (Engine.lens_remap) -> a new array.  coefficients = (a1, a2), |a| <= 0.25, as
    Stitcher.lensCoefficients holds them after an "estimate" run."""
    if engine is None:
        from ._lib import default_engine
        engine = default_engine()
    q1, q2 = coefficients_q30(*coefficients)
    return engine.lens_remap(img, q1, q2, centre_half_pixels(centre), interpolation)
