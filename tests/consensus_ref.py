"""The specification of Method.getOffsetByRansac (offsetCaculate = "ransac"), restated in numpy.

The reference's getOffsetByRansac (ImageUtility.py:180-210) fits a homography and then breaks, so it cannot specify anything; this
file does.  csrc/consensus_kernels.hip (vfsms_consensus_offset and the consensus vote tail of every fused path) equals it bit for bit.

Inputs are getOffsetByMode's: kpsA, kpsB float32 (x, y); matches = [(trainIdx, queryIdx)], kpsA indexed by queryIdx and kpsB by
trainIdx; one integer tolerance t (Method.ransacThreshold, 0..64).

1. votes: v_k = (int(float32(ay - by)), int(float32(ax - bx))) per match -- getOffsetByMode's vote; V = the votes that are not (0, 0),
   in match order (the list the mode votes over).
2. support(k) = #{j in V : |dx_j - dx_k| <= t and |dy_j - dy_k| <= t} (a Chebyshev window on the integer votes).
3. the winner k* is the smallest index of largest support.
4. the inliers are the votes in the window of v_k*; the offset is the lower median of their dx and of their dy, taken separately
   (ascending, element (n - 1) // 2).
5. count = support(k*), status = count >= offsetEvaluate.  No matches: (False, (0, 0), 0).  Matches but V empty: offset (0, 0), count 1.

At t = 0 this is getOffsetByMode: support(k) is the count of v_k's tuple, the first vote of the largest count is the first occurrence
of the earliest-seen most frequent tuple (the mode's tie-break), and the median of equal votes is the vote.
"""
import numpy as np

MAX_TOL = 64


def votes(kpsA, kpsB, matches):
    """-> int64[n, 2] of (dx, dy): every match's vote, (0, 0) included, in match order"""
    kA = np.ascontiguousarray(kpsA, np.float32).reshape(-1, 2)
    kB = np.ascontiguousarray(kpsB, np.float32).reshape(-1, 2)
    m = np.asarray(matches, np.int64).reshape(-1, 2)
    tr, q = m[:, 0], m[:, 1]
    dx = (kA[q, 1] - kB[tr, 1]).astype(np.float32).astype(np.int64)      # float32 difference, truncated toward zero
    dy = (kA[q, 0] - kB[tr, 0]).astype(np.float32).astype(np.int64)
    return np.stack([dx, dy], 1)


def support(V, t, chunk=1024):
    """int64[n]: the support of every vote of V (int[n, 2]) at tolerance t"""
    V = np.asarray(V, np.int32).reshape(-1, 2)
    x, y = V[:, 0], V[:, 1]
    out = np.zeros(len(V), np.int64)
    for a in range(0, len(V), chunk):
        inx = np.abs(x[a:a + chunk, None] - x[None, :]) <= t
        iny = np.abs(y[a:a + chunk, None] - y[None, :]) <= t
        out[a:a + chunk] = np.count_nonzero(inx & iny, axis=1)
    return out


def lower_median(a):
    a = np.sort(np.asarray(a, np.int64))
    return int(a[(len(a) - 1) // 2])


def consensus_from_votes(all_votes, t, offset_evaluate=3):
    """the estimator on the votes of every match (step 1's list before the (0, 0) votes are dropped) -> (status, [dx, dy], count)"""
    if not 0 <= int(t) <= MAX_TOL:
        raise ValueError("tolerance %r outside 0..%d" % (t, MAX_TOL))
    all_votes = np.asarray(all_votes, np.int64).reshape(-1, 2)
    if len(all_votes) == 0:
        return False, [0, 0], 0
    V = all_votes[~((all_votes[:, 0] == 0) & (all_votes[:, 1] == 0))]
    if len(V) == 0:
        return bool(1 >= offset_evaluate), [0, 0], 1
    s = support(V, t)
    k = int(np.argmax(s))                                  # the first index of the largest support
    c = V[k]
    inl = V[(np.abs(V[:, 0] - c[0]) <= t) & (np.abs(V[:, 1] - c[1]) <= t)]
    count = int(s[k])
    assert len(inl) == count
    return bool(count >= offset_evaluate), [lower_median(inl[:, 0]), lower_median(inl[:, 1])], count


def consensus_offset(kpsA, kpsB, matches, t=3, offset_evaluate=3):
    """-> (status, [dx, dy], count): what Engine.consensus_offset returns"""
    if len(matches) == 0:
        return False, [0, 0], 0
    return consensus_from_votes(votes(kpsA, kpsB, matches), t, offset_evaluate)


def mode_from_votes(all_votes, offset_evaluate=3):
    """getOffsetByMode restated on the same votes (for the t = 0 identity): the most frequent tuple, ties to the first seen"""
    all_votes = np.asarray(all_votes, np.int64).reshape(-1, 2)
    if len(all_votes) == 0:
        return False, [0, 0], 0
    counts, first = {}, {}
    for i, (dx, dy) in enumerate(all_votes.tolist()):
        if dx == 0 and dy == 0:
            continue
        counts[(dx, dy)] = counts.get((dx, dy), 0) + 1
        first.setdefault((dx, dy), i)
    if not counts:
        return bool(1 >= offset_evaluate), [0, 0], 1
    best = min(counts, key=lambda k: (-counts[k], first[k]))
    return bool(counts[best] >= offset_evaluate), [best[0], best[1]], counts[best]


def keypoints_for_votes(all_votes, seed=0):
    """(kpsA, kpsB, matches) whose votes are exactly `all_votes`: fractional keypoints (truncation toward zero is exercised) and B's
    keypoints in another order than A's (trainIdx != queryIdx)"""
    rng = np.random.default_rng(seed)
    V = np.asarray(all_votes, np.int64).reshape(-1, 2)
    n = len(V)
    bx = rng.integers(100, 900, n).astype(np.float32) + rng.uniform(0.0, 0.5, n).astype(np.float32)
    by = rng.integers(100, 900, n).astype(np.float32) + rng.uniform(0.0, 0.5, n).astype(np.float32)
    # a = b + v + f with 0 < |f| < 0.5 of the sign of v: int(float32(a - b)) = v (v = 0: either sign truncates to 0)
    fx = rng.uniform(0.05, 0.45, n).astype(np.float32) * np.where(V[:, 1] < 0, -1, 1).astype(np.float32)
    fy = rng.uniform(0.05, 0.45, n).astype(np.float32) * np.where(V[:, 0] < 0, -1, 1).astype(np.float32)
    ax = (bx + V[:, 1].astype(np.float32) + fx).astype(np.float32)
    ay = (by + V[:, 0].astype(np.float32) + fy).astype(np.float32)
    perm = rng.permutation(n)
    kpsB = np.empty((n, 2), np.float32)
    kpsB[perm, 0], kpsB[perm, 1] = bx, by
    kpsA = np.stack([ax, ay], 1)
    matches = np.stack([perm, np.arange(n)], 1).astype(np.int32)
    assert np.array_equal(votes(kpsA, kpsB, matches), V), "keypoints do not reproduce the votes"
    return kpsA, kpsB, matches
