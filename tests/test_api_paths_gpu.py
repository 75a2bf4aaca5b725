"""GPU tests (-m gpu) that pin what the entry points of csrc/api.hip share: the single-tile and the batch form of the resident SURF
feature sets, of their match + vote and of the fused attempts must give the same bytes, a feature set's handle must die with its free
whichever way it was allocated, a batch of mixed ROI shapes must come back in the caller's order, and the four int64 fuse entry points
must give what their references give.  Three resident tiles of 256 x 320: two textured neighbours and a constant one (no keypoints)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd._lib import VFSMS_ERR_BAD_ARG
from imagestitch_amd.synthetic import SyntheticGrid

import multiband_ref as MB
import seam_ref as SR

pytestmark = pytest.mark.gpu

H, W = 256, 320
SUB = (32, 48, 160, 200)                                 # a strict sub-rectangle (y0, x0, h, w)
WHOLE = (0, 0, H, W)


@pytest.fixture(scope="module")
def tiles(oracle):
    a, b = SyntheticGrid(2, 1, H, W, overlap=0.5).tiles(threads=1)
    flat = np.full((H, W), 97, np.uint8)
    y0, x0, h, w = SUB
    for t in (a, b, np.ascontiguousarray(a[y0:y0 + h, x0:x0 + w])):     # the oracle sees texture: no case below passes on empty sets
        assert len(oracle.surf_detect_describe(t)[0]) >= 64
    assert len(oracle.surf_detect_describe(flat)[0]) == 0
    return a, b, flat


@pytest.fixture(scope="module")
def handles(engine, tiles):
    hs = [engine.tile_upload(t) for t in tiles]
    yield hs
    for h in hs:
        engine.tile_free(h)


def _download_and_free(engine, feat, n):
    out = engine.features_download(feat, n)
    engine.features_free(feat)
    return out


def _same(x, y):
    return all(p.shape == q.shape and p.tobytes() == q.tobytes() for p, q in zip(x, y))


@pytest.mark.parametrize("enhance", [(0, 0.0, 0), (1, 0.0, 0)], ids=["plain", "equalize"])
def test_single_set_equals_batch_set(engine, handles, enhance):
    for k in (0, 1, 2):
        f1, n1 = engine.features_surf(handles[k], WHOLE, enhance=enhance)
        (f2,), (n2,) = engine.features_surf_batch([handles[k]], enhance=enhance)
        one, two = _download_and_free(engine, f1, n1), _download_and_free(engine, f2, n2)
        assert n1 == n2 == len(one[0]) and (n1 >= 64 if k < 2 else n1 == 0), (k, n1, n2)
        assert _same(one, two), k


def test_sub_rectangle_set_equals_the_host_buffer_call(engine, tiles, handles):
    y0, x0, h, w = SUB
    f, n = engine.features_surf(handles[0], SUB)
    got = _download_and_free(engine, f, n)
    want = engine.surf_detect_describe(np.ascontiguousarray(tiles[0][y0:y0 + h, x0:x0 + w]))
    assert n >= 64 and _same(got, want)


def test_match_rows_single_and_batch(engine, handles):
    (fa, na), (fb, nb), (fe, ne) = [engine.features_surf(h, WHOLE) for h in handles]
    try:
        ab, ba = engine.features_match_offset(fa, fb).tolist(), engine.features_match_offset(fb, fa).tolist()
        assert ne == 0 and ab[0] == 1 and ab[4:6] == [na, nb] and ab[6] >= ab[3] > 0, ab
        assert engine.features_match_offset_batch([fa], [fb])[0].tolist() == ab
        rows = engine.features_match_offset_batch([fa, fe, fb], [fb, fb, fa]).tolist()
        assert rows == [ab, [0, 0, 0, 0, 0, nb, 0, 0], ba]
        assert engine.features_match_offset(fe, fb).tolist() == rows[1]
    finally:
        for f in (fa, fb, fe):
            engine.features_free(f)


def _refused(engine, feat):
    n, d = C.c_int(), C.c_int()
    return engine.lib.vfsms_features_download(engine.ctx, C.c_int64(feat), None, None, 0, C.byref(n), C.byref(d)) == VFSMS_ERR_BAD_ARG


def test_feature_handles_die_with_their_free_in_any_order(engine, handles):
    first = None
    for order in itertools.permutations(range(3)):
        single = [engine.features_surf(h, WHOLE) for h in handles]                  # the third set is empty
        batch = list(zip(*engine.features_surf_batch(handles)))                      # one shared allocation
        kept = [engine.features_download(f, n) for f, n in single + batch]
        first = first or kept
        assert all(_same(x, y) for x, y in zip(kept, first))
        for sets in (single, batch):
            for pos, k in enumerate(order):
                engine.features_free(sets[k][0])
                assert _refused(engine, sets[k][0])
                with pytest.raises(isa.VfsmsError):
                    engine.features_free(sets[k][0])
                for j in order[pos + 1:]:                                            # the sets still alive keep their bytes
                    assert _same(engine.features_download(*sets[j]), first[j]), (order, k, j)
    f, n = engine.features_surf(handles[0], WHOLE)                                  # after the last free the single path still allocates
    assert _same(_download_and_free(engine, f, n), first[0]) and _refused(engine, f)


def _mixed_jobs(hs):
    a, b = hs[0], hs[1]
    col = (a, b, 0, W - 64, 0, 0, H, 64)                 # 256 x 64: right edge of a, left edge of b
    row = (a, b, H - 64, 0, 0, 0, 64, W)                 # 64 x 320: bottom of a, top of b
    back = (b, a, 0, 0, 0, W - 64, H, 64)                # 256 x 64 again: its two strips are col's, swapped
    return [col, row, back, row]


def test_mixed_shape_phase_batch_keeps_the_callers_order(engine, handles):
    jobs = _mixed_jobs(handles)
    rows = engine.attempt_phase_batch(jobs)
    alone = np.concatenate([engine.attempt_phase_batch([j]) for j in jobs])
    print("phase rows", rows.tolist(), "alone", alone.tolist())
    assert rows.tobytes() == alone.tobytes()
    assert rows[1].tolist() == rows[3].tolist() and rows[0].tolist() != rows[1].tolist()


def test_mixed_shape_surf_batch_keeps_the_callers_order(engine, handles):
    jobs = _mixed_jobs(handles)
    rows = engine.attempt_surf_batch(jobs).tolist()
    alone = [engine.attempt_surf_batch([j])[0].tolist() for j in jobs]
    assert rows == alone
    assert all(r[4] > 0 and r[5] > 0 for r in rows) and rows[0][4:6] == rows[2][5:3:-1] and rows[0] != rows[1]


@pytest.mark.parametrize("ch", [1, 3])
def test_int64_fuse_entry_points_against_their_references(engine, oracle, ch):
    from fakes import OracleEngine
    rng = np.random.default_rng(11 + ch)
    r, c = 24, 40
    shape = (r, c) if ch == 1 else (r, c, ch)
    for hole in (False, True):                            # strip geometry; corner geometry (an L-shaped hole in A)
        A = rng.integers(0, 256, shape).astype(np.int64); B = rng.integers(0, 256, shape).astype(np.int64)
        if hole:
            A[:r // 2 + 4, :c // 2 + 6] = -1                # 57 % of A is left: under the 65 % that decides for a strip
        for dx, dy in ((3, 5), (-3, -5)):
            tag = (ch, hole, dx, dy)
            want, winfo = oracle.fuse_fade(A, B, dx, dy, return_info=True)
            got, info = engine.fuse_fade_i64(A, B, dx, dy, return_info=True)
            assert got.tobytes() == want.tobytes() and info.tolist() == winfo.tolist() and info[0] == int(hole), tag
            d = np.abs(engine.fuse_trig_i64(A, B, dx, dy).astype(np.int16) - OracleEngine(oracle).fuse_trig_i64(A, B, dx, dy).astype(np.int16))
            print("trig", tag, "max", int(d.max()), "differing", int(np.count_nonzero(d)), "of", d.size)
            assert d.max() <= 1 and np.count_nonzero(d) * 1000 < d.size, tag       # include/vfsms.h: |diff| <= 1 on < 0.1 % of the bytes
            for levels in (1, 4):
                got, info = engine.fuse_multiband_i64(A, B, dx, dy, levels=levels, return_info=True)
                assert got.tobytes() == MB.multiband(A, B, dx, dy, levels, oracle.corner_ramps).tobytes() and info.tolist() == winfo.tolist(), tag
            for blend in ("none", "multiBandBlending"):
                want, wseam = SR.seam_fuse(A, B, dx, dy, blend, 4, oracle.corner_ramps, return_seam=True)
                got, info, seam = engine.fuse_seam_i64(A, B, dx, dy, blend=blend, return_info=True, return_seam=True)
                assert got.tobytes() == want.tobytes() and seam.tolist() == wseam.tolist() and info.tolist() == winfo.tolist(), tag
                assert engine.fuse_seam_i64(A, B, dx, dy, blend=blend).tobytes() == want.tobytes(), tag     # without a seam buffer


def test_refused_seam_geometry_leaves_a_clean_result(engine, oracle):
    A = np.full((2, 2), -1, np.int64); A[0, 0] = 9
    B = np.full((2, 2), 50, np.int64)
    with pytest.raises(IndexError):
        oracle.fuse_fade(A, B, 1, 1)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for blend in (0, 1):
        out = np.full((2, 2), 7, np.uint8); info = np.full(4, 5, np.int32); seam = np.full(4, 3, np.int32)
        rc = engine.lib.vfsms_fuse_seam_i64(engine.ctx, p(A), p(B), 2, 2, 1, 1, 1, blend, 4, p(out), p(info), p(seam))
        assert rc == VFSMS_ERR_BAD_ARG and info[0] == -1 and not out.any() and seam.tolist() == [-1] * 4, (blend, rc, info, out, seam)
    for call in (engine.fuse_fade_i64, engine.fuse_trig_i64, engine.fuse_multiband_i64):
        with pytest.raises(isa.VfsmsError):
            call(A, B, 1, 1)
