"""GPU tests (-m gpu) of the trimmed fp16 candidate filter of the 64-d 2-NN search (csrc/match_kernels.hip: |t|^2 as the initial value
of the accumulator, pass 0 on every BFM_P0_STRIDE-th tile of a chunk plus its last) through the engine's entry point vfsms_bf_l2_knn2:
(i1, d1, d2) must equal the oracle's exhaustive exact search (oracle.bf_l2_knn2), bit for bit.

  - train counts on the edges of the 32-train tile (1, 2, 31, 32, 33, 64, 65, 97: one to four tiles, last tiles of 1, 31 and 32 rows)
    times query counts on the edges of the 64-query wave and the 256-query workgroup (1, 63, 64, 65, 257);
  - planted neighbours: every query's two nearest trains sit in tiles that pass 0 skips at strides 2 and 4 (odd position in the chunk,
    not its last), the third nearest, 0.05 further away, in a tile it visits at either stride (every fourth of the chunk, or its last), the rest far
    away -- so pass 0's bound comes from the third nearest and pass 1 must still list the two.  300 x 300 lays this out for ONE
    chunk of ten tiles; the engine cuts so few trains into chunks of two tiles (pick_filter_nsplit: eight chunks for small query
    counts), which are swept whole, so 300 x 1280 repeats it on the eight chunks of five tiles the engine makes of 1280 trains,
    where tiles are skipped for real;
  - exact duplicate train rows: a tie goes to the lower index."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
NT = (1, 2, 31, 32, 33, 64, 65, 97)
NQ = (1, 63, 64, 65, 257)


def _unit(a):
    a = np.asarray(a, np.float64)
    return (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)


def _same(engine, oracle, q, t):
    i1, d1, d2 = engine.bf_l2_knn2(q, t)
    oi1, od1, _oi2, od2 = oracle.bf_l2_knn2(q, t)
    assert len(i1) == len(q)
    assert np.array_equal(i1, oi1) and np.array_equal(d1, od1) and np.array_equal(d2, od2)
    return i1


@pytest.mark.parametrize("nt", NT)
def test_tile_and_wave_edges(engine, oracle, nt):
    for nq in NQ:
        rng = np.random.default_rng(100 * nt + nq)
        q, t = _unit(rng.normal(size=(nq, 64))), _unit(rng.normal(size=(nt, 64)))
        q[::2] = _unit(t[rng.integers(0, nt, len(q[::2]))] + 0.05 * rng.normal(size=(len(q[::2]), 64)))     # half the queries have a near train
        _same(engine, oracle, q, t)


def _planted(nq, nt, tchunk, seed):
    """(q, t, rows of the two planted nearest trains per query, row of the third): chunks of `tchunk` tiles"""
    rng = np.random.default_rng(seed)
    ntiles = (nt + 31) // 32
    skipped, visited = [], []
    for tile0 in range(0, ntiles, tchunk):
        tile1 = min(ntiles, tile0 + tchunk)
        for tl in range(tile0, tile1):
            k = tl - tile0
            if k % 2 == 1 and tl != tile1 - 1:
                skipped.append(tl)                                # no multiple of 2 or 4, not the last: skipped at strides 2 and 4
            elif (k % 4 == 0 or tl == tile1 - 1) and tl * 32 + 32 <= nt:
                visited.append(tl)                                # a multiple of 4, or the last: visited at any stride
    near_rows = np.concatenate([np.arange(32 * tl, 32 * tl + 32) for tl in skipped])
    third_rows = np.concatenate([np.arange(32 * tl, 32 * tl + 32) for tl in visited])
    nc = len(near_rows) // 2
    assert nc >= 32 and len(third_rows) >= nc
    rng.shuffle(near_rows); rng.shuffle(third_rows)
    centres = _unit(rng.normal(size=(nc, 64)))
    t = _unit(rng.normal(size=(nt, 64)))                          # the rest: distance ~1.4 from every centre

    def at(dist):                                                 # unit rows at chord distance `dist` from their centres
        e = rng.normal(size=(nc, 64)); e -= (e * centres).sum(1, keepdims=True) * centres
        e /= np.linalg.norm(e, axis=1, keepdims=True)
        c = 1.0 - dist * dist / 2.0
        return (c * centres + np.sqrt(1.0 - c * c) * e).astype(np.float32)
    n1, n2, n3 = near_rows[:nc], near_rows[nc:2 * nc], third_rows[:nc]
    t[n1], t[n2], t[n3] = at(0.10), at(0.15), at(0.20)
    which = rng.integers(0, nc, nq)
    q = _unit(centres[which] + 0.0002 * rng.normal(size=(nq, 64)))
    return q, t, n1[which], n2[which], n3[which]


@pytest.mark.parametrize("nq,nt,tchunk", [(300, 300, 10), (300, 1280, 5)])
def test_nearest_two_in_tiles_pass0_skips(engine, oracle, nq, nt, tchunk):
    q, t, n1, n2, n3 = _planted(nq, nt, tchunk, seed=nt)
    d = np.linalg.norm(q.astype(np.float64)[:, None, :] - t.astype(np.float64)[None, :, :], axis=2)
    order = np.argsort(d, axis=1)[:, :4]
    rows = np.arange(nq)
    assert np.array_equal(order[:, 0], n1) and np.array_equal(order[:, 1], n2) and np.array_equal(order[:, 2], n3)      # the construction holds
    assert (np.abs(d[rows, n3] - d[rows, n2] - 0.05) < 0.01).all() and (d[rows, order[:, 3]] > 0.7).all()       # everything else is far
    i1 = _same(engine, oracle, q, t)
    assert np.array_equal(i1, n1)


def test_duplicate_train_rows_keep_the_lower_index(engine, oracle):
    rng = np.random.default_rng(7)
    base = _unit(rng.normal(size=(50, 64)))
    src = rng.integers(0, 50, 200)
    t = base[src]                                                 # 200 rows out of 50: every row occurs about four times, across tiles
    q = t[rng.integers(0, 200, 130)].copy()                       # distance 0 to several trains
    q[::3] = _unit(q[::3] + 0.02 * rng.normal(size=(len(q[::3]), 64)))      # and equal non-zero distances to several trains
    i1 = _same(engine, oracle, q, t)
    first = np.array([np.flatnonzero(src == s)[0] if (src == s).any() else -1 for s in range(50)])
    assert np.array_equal(i1, first[src[i1]])                     # the winner is the first occurrence of its row
