"""The 2-NN of 128-d rows with integer elements 0..255 under the matcher's rule, written in numpy on integers: the reference that
tests/test_bf_i8_host.py checks against two independent float references and tests/test_bf_i8_gpu.py holds k_pack_i8_d128 + k_bf_i8_d128
(csrc/match_kernels.hip) to.  Never loads the library.

The rule (knn_update over ascending train indices, csrc/match_kernels.hip): distances are compared in the sqrt domain, d = sqrtf(dsq) in
float32; the best train is the FIRST index attaining the smallest d; the second-best distance is the second smallest of the row's multiset
of d (so d2 == d1 when two trains share the smallest d).  Where sqrtf maps two distinct dsq to one float -- above about 2^22 -- the
lowest index of the collision class wins, even when a later train has the smaller integer dsq."""
import numpy as np

DIM = 128


def dsq(q, t):
    """int64 (nq, nt): the squared distances, formed on integers"""
    q = np.asarray(q); t = np.asarray(t)
    assert q.ndim == 2 and t.ndim == 2 and q.shape[1] == t.shape[1] == DIM
    assert q.dtype.kind in "iu" and t.dtype.kind in "iu"
    qi, ti = q.astype(np.int32), t.astype(np.int32)
    out = np.empty((len(q), len(t)), np.int64)
    for i0 in range(0, len(q), 64):                                # blocks of queries: the differences of a block stay small in memory
        e = qi[i0:i0 + 64, None, :] - ti[None, :, :]
        out[i0:i0 + 64] = (e * e).sum(axis=2, dtype=np.int64)
    assert out.size == 0 or int(out.max()) < 2 ** 24
    return out


def knn2(q, t):
    """(i1 int32, d1 float32, d2 float32) per query row; nt == 0: (-1, inf, inf)"""
    s = dsq(q, t)
    nq, nt = s.shape
    if nt == 0:
        return np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32), np.full(nq, np.inf, np.float32)
    d = np.sqrt(s.astype(np.float32))
    assert d.dtype == np.float32
    i1 = np.argmin(d, axis=1).astype(np.int32)                     # the first index of the minimum
    d1 = d[np.arange(nq), i1]
    d2 = np.partition(d, 1, axis=1)[:, 1] if nt >= 2 else np.full(nq, np.inf, np.float32)
    return i1, d1, d2
