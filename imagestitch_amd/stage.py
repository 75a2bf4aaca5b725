"""Repair of the pairs a path could not register, from a stage model (Method.failedPairRepair = "stage").

The reference ends a mosaic at the first pair that cannot be registered (Stitcher.py:64-79), and one featureless tile -- empty mounting
medium, a hole in the section, the slide margin -- makes two consecutive pairs fail.  A motorised stage repeats its steps, so the pairs that
DID register say where the others must be:

  1. model: per scan direction (class 1 down, 2 right, 3 up, 4 left) the lower median of the accepted offsets; a direction nobody
     travelled takes the negated offset of the opposite one;
  2. measured: every failed pair is searched by correlation in a wide window around the model's offset of each direction
     (Engine.ncc_wide_batch, csrc/wide_kernels.hip); a score that reaches the threshold inside the window's rim is a measurement;
  3. predicted: a pair whose overlap carries no signal (the standard deviation of a side is below blank_ratio x the median of the accepted
     pairs') takes the model's offset of the direction the operator's hint or the path's period gives it;
  4. everything else stays failed: the mosaic breaks there, as it always did.

Specification: tests/stage_ref.py (this module equals it row for row and report for report).  At most three engine calls per table: the
wide searches, the overlap sums of the accepted pairs and of the candidates for a prediction.
"""
import numpy as np

FIXED_ONE = 1 << 20          # the engine reports scores as floor(score * 2^20 + 0.5) (include/vfsms.h: VFSMS_VERIFY_FIXED_ONE)
CLASSES = (1, 2, 3, 4)
KINDS = ("measured", "predicted", "unresolved")


def classes_of(offsets, h, w):
    """the scan direction of each [dx, dy]: the dominant axis relative to the tile's shape, then its sign"""
    o = np.asarray(offsets, np.int64).reshape(-1, 2)
    vertical = np.abs(o[:, 0]) * int(w) >= np.abs(o[:, 1]) * int(h)
    return np.where(vertical, np.where(o[:, 0] > 0, 1, 3), np.where(o[:, 1] > 0, 2, 4)).astype(np.int64)


def stage_model(offsets, classes):
    """-> (int64[5, 2] M indexed by class, bool[5] available, int[5] accepted pairs per class)"""
    M = np.zeros((5, 2), np.int64)
    own = np.zeros(5, bool)
    count = np.zeros(5, np.int64)
    for c in CLASSES:
        sel = np.sort(offsets[classes == c], axis=0)
        count[c] = len(sel)
        if len(sel):
            M[c] = sel[(len(sel) - 1) // 2]
            own[c] = True
    avail = own.copy()
    for c in CLASSES:
        opp = (c + 1) % 4 + 1
        if not own[c] and own[opp]:
            M[c] = -M[opp]
            avail[c] = True
    return M, avail, count


def path_period(known):
    """known: int[P], 0 where the class of a pair is not known -> the smallest T >= 1 such that no two known pairs T apart differ and at
    least T such pairs agree; None when there is none"""
    known = np.asarray(known, np.int64)
    for T in range(1, len(known)):
        a, b = known[:-T], known[T:]
        both = (a != 0) & (b != 0)
        if not np.any(both & (a != b)) and int(np.count_nonzero(both)) >= T:
            return T
    return None


def _sigma_min(s6):
    """min(sigma_a, sigma_b) per row of int64[n, 6] = (N, Sa, Sb, Saa, Sbb, Sab); 0 for an empty overlap"""
    s = np.asarray(s6, np.int64).reshape(-1, 6).astype(np.float64)
    n = np.where(s[:, 0] > 0, s[:, 0], 1.0)
    va = np.maximum(0.0, s[:, 3] - s[:, 1] * s[:, 1] / n) / n
    vb = np.maximum(0.0, s[:, 4] - s[:, 2] * s[:, 2] / n) / n
    return np.where(s[:, 0] > 0, np.minimum(np.sqrt(va), np.sqrt(vb)), 0.0)


def repair_table(engine, handles, shapes, table, hint=None, radius=32, factor=4, peaks=2, threshold=0.5, min_pixels=4096, blank_ratio=0.25):
    """`table`: the int32[P, 6] result table of GridRegistrar.register(stop_on_fail=False) over the resident gray tiles `handles` (one
    shape) -> (the table with the repaired rows filled in -- (1, dx, dy, class, 0, 0) -- and report): report["model"][c] = the offset and
    the accepted pairs of class c, ["period"], ["ref_sigma"], ["pairs"] = per failed pair its kind ("measured" / "predicted" /
    "unresolved"), class, score and displacement from the model's offset, ["counts"] per kind."""
    table = np.array(table, np.int32).reshape(-1, 6)
    P = len(table)
    if len(handles) != P + 1 or len(shapes) != P + 1:
        raise ValueError("repair_table: %d pairs need %d tiles" % (P, P + 1))
    if len(set((int(s[0]), int(s[1])) for s in shapes)) > 1:
        raise ValueError("repair_table: the stage model takes tiles of one shape")
    if not hasattr(engine, "ncc_wide_batch") or not hasattr(engine, "overlap_sums_batch"):
        raise NotImplementedError("this engine has no wide correlation search (failedPairRepair = 'stage')")
    h, w = (int(shapes[0][0]), int(shapes[0][1])) if P + 1 else (0, 0)
    R = int(radius)
    ok = table[:, 0] == 1
    offsets = table[:, 1:3].astype(np.int64)
    known = np.zeros(P, np.int64)
    known[ok] = classes_of(offsets[ok], h, w)
    M, avail, count = stage_model(offsets[ok], known[ok])
    cands = [c for c in CLASSES if avail[c]]
    failed = [int(k) for k in np.flatnonzero(~ok)]
    out = table.copy()
    entries = {}

    # measured: one wide search per (failed pair, available class), all in one call
    jobs = [(handles[k], handles[k + 1], int(M[c, 0]), int(M[c, 1])) for k in failed for c in cands]
    if jobs:
        res = np.asarray(engine.ncc_wide_batch(jobs, R, int(factor), int(peaks), int(min_pixels)), np.int64).reshape(len(failed), len(cands), 8)
        good = (res[:, :, 2] >= int(np.floor(float(threshold) * FIXED_ONE + 0.5))) & (np.abs(res[:, :, 0]) < R) & (np.abs(res[:, :, 1]) < R)
        for n, k in enumerate(failed):
            if not good[n].any():
                continue
            q = int(np.argmax(np.where(good[n], res[n, :, 2], -(1 << 40))))      # the first of equal scores: the smaller class
            c, ti, tj = cands[q], int(res[n, q, 0]), int(res[n, q, 1])
            out[k] = (1, M[c, 0] + ti, M[c, 1] + tj, c, 0, 0)
            known[k] = c
            entries[k] = {"pair": k, "kind": "measured", "class": c, "score": int(res[n, q, 2]) / float(FIXED_ONE), "displacement": [ti, tj]}

    # predicted: the class from the hint, else from the period of what is known; it stands only on a blank overlap
    T = path_period(known)
    use_hint = hint is not None and len(hint) == P
    want = {}
    for k in failed:
        if k in entries:
            continue
        c = int(hint[k]) if use_hint and int(hint[k]) in cands else 0
        if not c and T is not None:
            seen = np.unique(known[k % T::T])
            seen = seen[seen != 0]
            c = int(seen[0]) if len(seen) == 1 and int(seen[0]) in cands else 0
        want[k] = c
    acc = [int(k) for k in np.flatnonzero(ok)]
    ask = [k for k in want if want[k]] if acc else []
    ref = None
    if acc:
        sjobs = [(handles[k], handles[k + 1], int(offsets[k, 0]), int(offsets[k, 1])) for k in acc]
        sjobs += [(handles[k], handles[k + 1], int(M[want[k], 0]), int(M[want[k], 1])) for k in ask]
        s6 = np.asarray(engine.overlap_sums_batch(sjobs), np.int64).reshape(-1, 6)
        sig = _sigma_min(s6)
        ref = float(np.median(sig[:len(acc)]))
        for n, k in enumerate(ask):
            row = len(acc) + n
            if int(s6[row, 0]) >= int(min_pixels) and float(sig[row]) < float(blank_ratio) * ref:
                c = want[k]
                out[k] = (1, M[c, 0], M[c, 1], c, 0, 0)
                entries[k] = {"pair": k, "kind": "predicted", "class": c, "score": None, "displacement": [0, 0]}
    for k in want:
        if k not in entries:
            entries[k] = {"pair": k, "kind": "unresolved", "class": 0, "score": None, "displacement": None}
    pairs = [entries[k] for k in sorted(entries)]
    report = dict(model={c: dict(offset=[int(M[c, 0]), int(M[c, 1])] if avail[c] else None, count=int(count[c])) for c in CLASSES},
                  period=T, ref_sigma=ref, pairs=pairs, counts={kind: sum(1 for e in pairs if e["kind"] == kind) for kind in KINDS})
    return out, report
