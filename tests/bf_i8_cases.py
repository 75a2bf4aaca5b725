"""Seeded inputs for the integer 128-d 2-NN search (k_pack_i8_d128 + k_bf_i8_d128), shared by tests/test_bf_i8_host.py (which asserts,
from the reference alone, that the cases contain what they are built for) and tests/test_bf_i8_gpu.py.  case(kind, nq, nt) -> (q, t) as
uint8 arrays (nq, 128), (nt, 128).

Shapes: the smallest counts that reach every edge of the 16-column tile, the 64-query wave and the 256-query workgroup on the query side;
the 16-train tile, the 4-train lane group inside it and the 64-row pad on the train side; and, with 8 splits, both empty splits and splits
of one partial tile.

Where a train sits in the kernel: train j is row j & 15 of tile j >> 4, held by lane group (j & 15) >> 2; a column's four lane groups
are merged by (distance, index), and the group that writes the result is group 0.  With nsplit splits a split covers
ceil(ceil(nt / 16) / nsplit) whole tiles."""
import functools

import numpy as np

NQ = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)
NT = (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 129)
SHAPES = tuple((nq, nt) for nq in NQ for nt in NT)
KINDS = ("sift_like", "extremes", "duplicates", "near_ties", "pad_bait", "zero_rows", "far")
NSPLITS = (0, 1, 2, 3, 8)
DIM = 128
SEED = 20250


def split_trains(nt, nsplit):
    """trains per split of k_bf_i8_d128: whole 16-train tiles"""
    tiles = (nt + 15) // 16
    return 16 * ((tiles + nsplit - 1) // nsplit)


def lane_group(j):
    return (j & 15) >> 2


def _rng(kind, nq, nt):
    return np.random.default_rng([SEED, KINDS.index(kind), nq, nt])


def _sift_rows(rng, n):
    """sparse small integers with a few saturated 255s, the look of a SIFT descriptor"""
    a = rng.integers(0, 48, (n, DIM))
    a[rng.random((n, DIM)) < 0.55] = 0
    a[rng.random((n, DIM)) < 0.02] = 255
    return a


def _noisy(rng, rows):
    return np.clip(rows + rng.integers(-1, 2, rows.shape), 0, 255)


def _sift_like(rng, nq, nt):
    t = _sift_rows(rng, nt)
    q = _sift_rows(rng, nq)
    half = np.arange(0, nq, 2)
    q[half] = _noisy(rng, t[rng.integers(0, nt, len(half))])
    return q, t


def _extremes(rng, nq, nt):
    t = 255 * rng.integers(0, 2, (nt, DIM))
    q = 255 * rng.integers(0, 2, (nq, DIM))
    third = np.arange(0, nq, 3)
    q[third] = t[rng.integers(0, nt, len(third))]                  # distance 0
    flip = np.arange(1, nq, 3)
    q[flip] = 255 - t[rng.integers(0, nt, len(flip))]              # the largest distance there is: 128 * 255^2
    return q, t


# ---- duplicates ---------------------------------------------------------------------------------------------------------------------
def duplicate_pairs(nt):
    """{placement: [(lower, upper) train indices that hold one row]} for a train count.  within_lane: 1 apart inside a 4-train lane group;
    cross_lane: 4 or 8 apart inside a tile, the lower index in the lower lane group; cross_lane_up: the lower index in a HIGHER lane group
    than the upper one, which then sits in the next tile (a merge that kept its own side on equal distances would still be right for
    cross_lane, never for these); cross_tile: 16 apart, same lane group; cross_split: further apart than a split is long with 2 splits,
    hence with 3 and 8 as well."""
    P = {"within_lane": [(0, 1), (18, 19)], "cross_lane": [(2, 6), (3, 11)], "cross_lane_up": [(13, 17), (7, 16), (10, 20)],
         "cross_tile": [(5, 21), (40, 56)], "cross_split": []}
    gap = split_trains(nt, 2)
    P["cross_split"] = [(8, 8 + gap + 1), (12, 12 + gap + 4)]
    return {k: [(a, b) for a, b in v if b < nt] for k, v in P.items()}


def _duplicates(rng, nq, nt):
    t = rng.integers(3, 253, (nt, DIM))
    placed = duplicate_pairs(nt)
    taken = set()
    members = []                                                    # (placement, lower, upper)
    for name, pairs in placed.items():
        for a, b in pairs:
            assert a not in taken and b not in taken
            taken |= {a, b}
            t[b] = t[a]
            members.append((name, a, b))
    for j in range(1, nt):                                          # every other row is a copy of its predecessor's class
        if j not in taken and (j - 1) not in taken:
            t[j] = t[j - 1]; taken |= {j, j - 1}
    for j in range(nt):                                             # a leftover single between two classes joins the one in front of it
        if j not in taken and j > 0:
            t[j] = t[j - 1]; taken.add(j)
    q = np.empty((nq, DIM), np.int64)
    for i in range(nq):
        # the queries walk the placed pairs first, two each (the upper copy's row, which equals the lower one's), then any train
        j = members[(i // 2) % len(members)][2] if members and i < 8 * len(members) else int(rng.integers(0, nt))
        q[i] = t[j]
        if i & 1:                                                   # equal non-zero distance to every copy: +-1..3 on a few elements
            k = rng.choice(DIM, 1 + i % 5, replace=False)
            q[i, k] += rng.choice([-3, -2, -1, 1, 2, 3], len(k))
    assert q.min() >= 0 and q.max() <= 255
    return q, t


# ---- near ties ----------------------------------------------------------------------------------------------------------------------
def _near_ties(rng, nq, nt):
    """trains in families around a base row: member m differs from the base by 1 on 3 + m elements, so the squared distances of a family
    to its base are 3, 4, 5, ...: neighbours differ by exactly 1.  The train order is shuffled; the queries are the bases."""
    nbase = max(1, nt // 4)
    base = rng.integers(60, 196, (nbase, DIM))
    t = np.empty((nt, DIM), np.int64)
    order = rng.permutation(nt)
    for n, j in enumerate(order):
        b, m = n % nbase, n // nbase
        row = base[b].copy()
        k = rng.choice(DIM, 3 + m, replace=False)
        row[k] += rng.choice([-1, 1], len(k))
        t[j] = row
    q = base[np.arange(nq) % nbase]
    return q, t


# ---- pad bait -----------------------------------------------------------------------------------------------------------------------
def _pad_bait(rng, nq, nt):
    """every third query is all 128 -- the value a zero pad row stands for -- and the trains keep every element at least 87 away from it"""
    lo = rng.integers(0, 41, (nt, DIM)); hi = rng.integers(215, 256, (nt, DIM))
    t = np.where(rng.random((nt, DIM)) < 0.5, lo, hi)
    q = _noisy(rng, t[rng.integers(0, nt, nq)])
    q[::3] = 128
    return q, t


def _zero_rows(rng, nq, nt):
    q, t = _sift_like(rng, nq, nt)
    t[::5] = 0
    q[::4] = 0
    if nt > 3:
        t[3] = 0
    return q, t


def _far(rng, nq, nt):
    """dsq = 112 * 255^2 = 7 282 800 plus a spread of about 100: float32 roots near 2698.7 are 2^-12 apart and a step of 1 in dsq moves the
    root by 1.9e-4, so neighbouring integers often share their sqrtf"""
    q = np.zeros((nq, DIM), np.int64); t = np.full((nt, DIM), 255, np.int64)
    q[:, :16] = rng.integers(0, 4, (nq, 16)); t[:, :16] = rng.integers(0, 4, (nt, 16))
    return q, t


_BUILD = {"sift_like": _sift_like, "extremes": _extremes, "duplicates": _duplicates, "near_ties": _near_ties, "pad_bait": _pad_bait,
          "zero_rows": _zero_rows, "far": _far}


@functools.lru_cache(maxsize=None)
def case(kind, nq, nt):
    q, t = _BUILD[kind](_rng(kind, nq, nt), nq, nt)
    assert q.shape == (nq, DIM) and t.shape == (nt, DIM) and min(q.min(), t.min()) >= 0 and max(q.max(), t.max()) <= 255
    q = q.astype(np.uint8); t = t.astype(np.uint8)
    q.setflags(write=False); t.setflags(write=False)
    return q, t


@functools.lru_cache(maxsize=None)
def reference(kind, nq, nt):
    """bf_i8_ref.knn2 of a case, computed once per process and read-only"""
    import bf_i8_ref
    out = bf_i8_ref.knn2(*case(kind, nq, nt))
    for a in out:
        a.setflags(write=False)
    return out
