"""The specification of the stage model behind Method.failedPairRepair = "stage", restated in plain Python on host arrays.

The reference has no such step (a pair that cannot be registered ends the mosaic, Stitcher.py:64-79); imagestitch_amd/stage.py equals this
row for row and report for report.

Inputs: the tiles of a path (uint8, ONE shape h x w), the result table of its pairs -- rows (status, dx, dy, direction, i, votes) -- an
optional hint (one class per pair) and radius, factor, peaks, threshold, min_pixels, blank_ratio.

Class of an offset.  |dx| * w >= |dy| * h: 1 for dx > 0, else 3.  Otherwise 2 for dy > 0, else 4 (the codes of
SyntheticGrid.true_directions and grid.serpentine_directions).

Model.  M[c] = the component-wise LOWER median (element (n - 1) // 2 of the sorted values) of the accepted offsets of class c.  A class
without an accepted pair takes the negated M of the opposite class (1 <-> 3, 2 <-> 4); a class is unavailable when both are empty.

Measured.  A failed pair gets one wide search (ncc_wide_ref) per available class c, centred on M[c].  A candidate counts when its
fixed-point score reaches floor(threshold * 2^20 + 0.5) and |ti| < R and |tj| < R.  The best score wins, ties go to the smaller c; the row
becomes (1, M[c] + (ti, tj), c, 0, 0).

Predicted.  Only for a pair that is still failed.  Its class is hint[k] when the hint has one entry per pair and names an available class;
else the period rule over the classes of the accepted and measured pairs: T is the smallest T >= 1 with no k where pairs k and k + T are
both known and differ and at least T such k where both are known and equal; the pair's class is the one class of the known pairs
congruent to it mod T, if there is exactly one (and it is available).  The prediction stands only when the overlap at M[c] is blank:
N >= min_pixels and min(sigma_a, sigma_b) < blank_ratio * ref, sigma = sqrt(max(0, Saa - Sa * Sa / N) / N) in float64 from
verify_ref.sums, ref = the median (numpy's: the mean of the two middle values) over the accepted pairs of their own
min(sigma_a, sigma_b) at their accepted offsets.  Then the row becomes (1, M[c], c, 0, 0).

Everything else stays failed.
"""
import math

import numpy as np

import ncc_wide_ref
import verify_ref

OPPOSITE = {1: 3, 3: 1, 2: 4, 4: 2}


def offset_class(dx, dy, h, w):
    if abs(dx) * w >= abs(dy) * h:
        return 1 if dx > 0 else 3
    return 2 if dy > 0 else 4


def lower_median(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2]


def model(table, h, w):
    """-> ({class: (mx, my) or None}, {class: accepted pairs})"""
    by = {c: [] for c in (1, 2, 3, 4)}
    for r in table:
        if int(r[0]) == 1:
            by[offset_class(int(r[1]), int(r[2]), h, w)].append((int(r[1]), int(r[2])))
    own = {c: (lower_median(o[0] for o in by[c]), lower_median(o[1] for o in by[c])) if by[c] else None for c in by}
    M = {}
    for c in by:
        if own[c] is not None:
            M[c] = own[c]
        elif own[OPPOSITE[c]] is not None:
            M[c] = (-own[OPPOSITE[c]][0], -own[OPPOSITE[c]][1])
        else:
            M[c] = None
    return M, {c: len(by[c]) for c in by}


def period(known):
    """known: a class or None per pair -> the T of the period rule, or None"""
    P = len(known)
    for T in range(1, P):
        same = 0
        ok = True
        for k in range(P - T):
            a, b = known[k], known[k + T]
            if a is None or b is None:
                continue
            if a != b:
                ok = False
                break
            same += 1
        if ok and same >= T:
            return T
    return None


def period_class(known, T, k):
    if T is None:
        return None
    seen = set(known[q] for q in range(k % T, len(known), T) if known[q] is not None)
    return seen.pop() if len(seen) == 1 else None


def sigma_min(s):
    N, Sa, Sb, Saa, Sbb, _Sab = (int(v) for v in s)
    if N <= 0:
        return 0.0
    sa = math.sqrt(max(0.0, float(Saa) - float(Sa) * float(Sa) / float(N)) / float(N))
    sb = math.sqrt(max(0.0, float(Sbb) - float(Sb) * float(Sb) / float(N)) / float(N))
    return min(sa, sb)


def repair(tiles, table, hint=None, radius=32, factor=4, peaks=2, threshold=0.5, min_pixels=4096, blank_ratio=0.25,
           wide=ncc_wide_ref.search, sums=verify_ref.sums):
    """-> (int32 table [P, 6], report); `wide` and `sums` stand for ncc_wide_ref.search and verify_ref.sums (tests pass cached ones)"""
    table = np.array(table, np.int32).reshape(-1, 6)
    P = len(table)
    h, w = tiles[0].shape
    R = int(radius)
    M, counts = model(table, h, w)
    avail = [c for c in (1, 2, 3, 4) if M[c] is not None]
    thr = int(math.floor(float(threshold) * float(verify_ref.FIXED_ONE) + 0.5))
    out = table.copy()
    accepted = [k for k in range(P) if int(table[k, 0]) == 1]
    known = [offset_class(int(r[1]), int(r[2]), h, w) if int(r[0]) == 1 else None for r in table]
    entries = {}
    for k in range(P):
        if int(table[k, 0]) == 1:
            continue
        best = None
        for c in avail:
            o8, _seeds = wide(tiles[k], tiles[k + 1], M[c][0], M[c][1], R, factor, peaks, min_pixels)
            ti, tj, fx = int(o8[0]), int(o8[1]), int(o8[2])
            if fx >= thr and abs(ti) < R and abs(tj) < R and (best is None or fx > best[0]):
                best = (fx, c, ti, tj)
        if best is not None:
            fx, c, ti, tj = best
            out[k] = (1, M[c][0] + ti, M[c][1] + tj, c, 0, 0)
            known[k] = c
            entries[k] = {"pair": k, "kind": "measured", "class": c, "score": fx / float(verify_ref.FIXED_ONE), "displacement": [ti, tj]}
    T = period(known)
    sig = [sigma_min(sums(tiles[k], tiles[k + 1], int(table[k, 1]), int(table[k, 2]))) for k in accepted]
    ref = float(np.median(np.array(sig, np.float64))) if sig else None
    use_hint = hint is not None and len(hint) == P
    for k in range(P):
        if int(out[k, 0]) == 1:
            continue
        c = int(hint[k]) if use_hint and int(hint[k]) in avail else None
        if c is None:
            c = period_class(known, T, k)
            if c not in avail:
                c = None
        kind = "unresolved"
        if c is not None and ref is not None:
            s = sums(tiles[k], tiles[k + 1], M[c][0], M[c][1])
            if int(s[0]) >= int(min_pixels) and sigma_min(s) < float(blank_ratio) * ref:
                out[k] = (1, M[c][0], M[c][1], c, 0, 0)
                kind = "predicted"
        entries[k] = {"pair": k, "kind": kind, "class": c if kind == "predicted" else 0, "score": None, "displacement": [0, 0] if kind == "predicted" else None}
    pairs = [entries[k] for k in sorted(entries)]
    report = dict(model={c: dict(offset=list(M[c]) if M[c] is not None else None, count=counts[c]) for c in (1, 2, 3, 4)},
                  period=T, ref_sigma=ref, pairs=pairs,
                  counts={kind: sum(1 for e in pairs if e["kind"] == kind) for kind in ("measured", "predicted", "unresolved")})
    return out, report
