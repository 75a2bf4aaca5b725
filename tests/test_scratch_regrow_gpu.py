"""The library's long-lived device memory in the orders a session can meet it: every grow-only scratch buffer small, large, small again on
ONE engine, each call byte for byte what a brand-new engine returns for it (growth loses nothing, stale capacity changes nothing, no shape
reads another's leftovers); the canvas lifecycle through the spare slot; and handles that share or outlive an allocation."""
import numpy as np
import pytest

import imagestitch_amd as isa

pytestmark = pytest.mark.gpu


def _same(got, want, tag):
    got = got if isinstance(got, (tuple, list)) else (got,)
    want = want if isinstance(want, (tuple, list)) else (want,)
    assert len(got) == len(want), tag
    for k, (g, w) in enumerate(zip(got, want)):
        if isinstance(g, (tuple, list)):
            _same(g, w, tag + (k,))
            continue
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, tag + (k, g.dtype, g.shape, w.dtype, w.shape)
        assert g.tobytes() == w.tobytes(), tag + (k, "%d bytes differ" % int(np.count_nonzero(g.view(np.uint8) != w.view(np.uint8))))


def _regrow(name, call, small, large, setup=None):
    """call(engine, state, case) for case = small, large, small on one engine (state = setup(engine), once per engine), each against the same
    call on an engine that has done nothing else -> the three results of the one engine"""
    setup = setup or (lambda eng: None)

    def run(cases):
        eng = isa.Engine(0)
        try:
            state = setup(eng)
            return [call(eng, state, c) for c in cases]
        finally:
            eng.close()

    got = run([small, large, small])
    fresh = {id(c): run([c])[0] for c in (small, large)}
    for k, c in enumerate((small, large, small)):
        _same(got[k], fresh[id(c)], (name, ("small", "large", "small again")[k]))
    return got


def _regions(seed, r, c, ch):
    rng = np.random.default_rng(seed)
    shape = (r, c) if ch == 1 else (r, c, ch)
    A = rng.integers(0, 256, shape).astype(np.int64); B = rng.integers(0, 256, shape).astype(np.int64)
    A[r // 3:, c // 4:] = -1
    return A, B


def _texture(seed, h, w):
    """random blobs of about 4 px, smoothed: corners and blobs at the scales SURF and SIFT look at"""
    rng = np.random.default_rng(seed)
    t = np.kron(rng.integers(0, 256, (h // 4 + 2, w // 4 + 2)).astype(np.float64), np.ones((4, 4)))[:h + 4, :w + 4]
    for _ in range(2):
        t = (t[:-2] + 2 * t[1:-1] + t[2:]) / 4
        t = (t[:, :-2] + 2 * t[:, 1:-1] + t[:, 2:]) / 4
    assert t.shape == (h, w)
    return np.ascontiguousarray(np.rint(t).astype(np.uint8))


def test_multiband_scratch():
    small, large = _regions(1, 24, 24, 1) + (2,), _regions(2, 96, 80, 3) + (4,)
    got = _regrow("fuse_multiband_i64", lambda eng, _s, c: eng.fuse_multiband_i64(c[0], c[1], 5, 7, levels=c[2], return_info=True), small, large)
    assert all(len(np.unique(out)) > 2 for out, _info in got)


def test_seam_scratch():
    small, large = _regions(3, 24, 24, 1), _regions(4, 96, 80, 3)
    got = _regrow("fuse_seam_i64", lambda eng, _s, c: eng.fuse_seam_i64(c[0], c[1], 5, 7, blend="none", return_seam=True), small, large)
    assert all(len(np.unique(out)) > 2 and (seam >= 0).any() for out, seam in got)


def test_shading_scratch():
    rng = np.random.default_rng(5)
    small = [rng.integers(0, 256, (32, 32)).astype(np.uint8) for _ in range(2)]
    large = [rng.integers(0, 256, (96, 64, 3)).astype(np.uint8) for _ in range(3)]

    def call(eng, _s, tiles):
        handles = [eng.tile_upload_color(t) if t.ndim == 3 else eng.tile_upload(t) for t in tiles]
        f = eng.shading_estimate(handles, 50, 3)
        try:
            return eng.shading_download(f, with_profile=True)
        finally:
            eng.shading_free(f)
            for h in handles:
                eng.tile_free(h)

    got = _regrow("shading_estimate", call, small, large)
    assert all(len(np.unique(gain)) > 2 and prof.any() for gain, _q8, prof in got)


def test_sift_scratch():
    small, large = _texture(6, 64, 64), _texture(7, 128, 160)
    got = _regrow("sift_detect_describe", lambda eng, _s, img: eng.sift_detect_describe(img, full=True), small, large)
    assert all(len(xy) >= 1 for xy, _desc, _kps in got), [len(g[0]) for g in got]
    assert len(got[1][0]) > len(got[0][0])


def test_surf_arena():
    small, large = _texture(8, 64, 64), _texture(9, 256, 256)
    got = _regrow("surf_detect_describe", lambda eng, _s, img: eng.surf_detect_describe(img, full=True), small, large)
    assert all(len(xy) >= 1 for xy, _desc, _kps in got), [len(g[0]) for g in got]
    assert len(got[1][0]) > len(got[0][0])


def test_jpeg_scratch():
    rng = np.random.default_rng(10)
    small, large = rng.integers(0, 256, (16, 16)).astype(np.uint8), rng.integers(0, 256, (48, 80, 3)).astype(np.uint8)
    got = _regrow("jpeg_encode_device", lambda eng, _s, img: eng.jpeg_encode_device(img), small, large)
    assert all(out[:2].tolist() == [0xFF, 0xD8] and out[-2:].tolist() == [0xFF, 0xD9] for out in got) and got[1].size > got[0].size


def test_canvas_pyramid_scratch():
    """one 64 x 48 canvas: an 8-row band with 2 levels, the whole canvas with 3, the band again"""
    rows, cols = 64, 48
    img = np.random.default_rng(11).integers(0, 256, (rows, cols)).astype(np.uint8)

    def setup(eng):
        cv = eng.canvas_create(rows, cols, 1)
        eng.canvas_paste(cv, img, 0, 0)
        return cv

    def call(eng, cv, case):
        if case == "band":
            r0, band, levels = next(eng.canvas_download_pyramid_bands(cv, rows, cols, 1, 2, band_rows=8))
            return (np.array(band),) + tuple(np.array(lv) for lv in levels)
        return tuple(np.array(lv) for lv in eng.canvas_pyramid(cv, rows, cols, 1, 3))

    got = _regrow("canvas_pyramid", call, "band", "whole", setup)
    assert np.array_equal(got[0][0], img[:8]) and [lv.shape for lv in got[0][1:]] == [(4, 24), (2, 12)]
    assert [lv.shape for lv in got[1]] == [(32, 24), (16, 12), (8, 6)] and all(lv.any() for lv in got[1])


# ---- canvas lifecycle -------------------------------------------------------------------------------------------------------------------
def _two_tiles(seed, h, w, ch, off):
    """two h x w tiles, the second `off` = (dx, dy) from the first -> tiles, canvas size, the second tile's placement and fuse ROI"""
    rng = np.random.default_rng(seed)
    tiles = [np.ascontiguousarray(rng.integers(0, 256, (h, w) if ch == 1 else (h, w, ch)).astype(np.uint8)) for _ in range(2)]
    place, rx, ry, rows, cols = isa.Stitcher._layout([(h, w), (h, w)], [[0, 0], list(off)])
    oy, ox = place[1]
    roi = (max(oy, rx[0][0]), max(ox, ry[0][0]), min(oy + h, rx[0][1]), min(ox + w, ry[0][1]))
    return tiles, rows, cols, (oy, ox), roi


def _paste_and_fuse(eng, cv, tiles, at, roi, off, rows, cols, ch):
    eng.canvas_paste(cv, tiles[0], 0, 0)
    eng.canvas_fuse_tile(cv, tiles[1], at[0], at[1], roi, off[0], off[1], method=0)
    return eng.canvas_download(cv, rows, cols, ch)


def test_canvas_lifecycle_through_the_spare_slot():
    tiles, rows, cols, at, roi = _two_tiles(12, 36, 32, 1, (4, 24))
    assert (rows, cols) == (40, 56)
    tiles3, rows3, cols3, at3, roi3 = _two_tiles(13, 20, 18, 3, (4, 6))
    assert (rows3, cols3) == (24, 24)
    fresh = isa.Engine(0)
    try:
        cv = fresh.canvas_create(rows, cols, 1)
        want = _paste_and_fuse(fresh, cv, tiles, at, roi, (4, 24), rows, cols, 1)
        fresh.canvas_free(cv)
    finally:
        fresh.close()
    assert want[:36, :24].tobytes() == tiles[0][:, :24].tobytes() and want[36:, 24:].tobytes() == tiles[1][32:].tobytes() and not want[36:, :24].any()
    eng = isa.Engine(0)
    try:
        cv = eng.canvas_create(rows, cols, 1)
        eng.canvas_paste(cv, tiles[0], 2, 3)
        first = eng.canvas_download(cv, rows, cols, 1)
        assert first[2:38, 3:35].tobytes() == tiles[0].tobytes() and int(np.count_nonzero(first)) == int(np.count_nonzero(tiles[0]))
        eng.canvas_free(cv)
        cv = eng.canvas_create(rows, cols, 1)                      # the spare's buffers
        assert not eng.canvas_download(cv, rows, cols, 1).any()
        _same(_paste_and_fuse(eng, cv, tiles, at, roi, (4, 24), rows, cols, 1), want, ("spare reused",))
        eng.canvas_free(cv)
        cv = eng.canvas_create(rows3, cols3, 3)                    # another size: the spare is released, not kept beside it
        assert not eng.canvas_download(cv, rows3, cols3, 3).any()
        eng.canvas_paste(cv, tiles3[0], 4, 6)
        expect = np.zeros((rows3, cols3, 3), np.uint8); expect[4:24, 6:24] = tiles3[0]
        _same(eng.canvas_download(cv, rows3, cols3, 3), expect, ("other size",))
        eng.canvas_free(cv)
        cv = eng.canvas_create(rows, cols, 1)
        assert not eng.canvas_download(cv, rows, cols, 1).any()
        eng.canvas_free(cv)
        with pytest.raises(isa.VfsmsError, match="canvas_free: unknown canvas handle"):
            eng.canvas_free(cv)
        again = eng.canvas_create(rows, cols, 1)                   # the refused call touched nothing: the spare is still there and clean
        _same(_paste_and_fuse(eng, again, tiles, at, roi, (4, 24), rows, cols, 1), want, ("after the refused free",))
        eng.canvas_free(again)
    finally:
        eng.close()


# ---- handles that share or outlive an allocation --------------------------------------------------------------------------------------------
def test_feature_sets_of_one_block_are_freed_one_by_one():
    eng = isa.Engine(0)
    try:
        hs = [eng.tile_upload(_texture(14 + k, 128, 128)) for k in range(2)]
        (f0, f1), (n0, n1) = eng.features_surf_batch(hs)           # two sets, one shared allocation
        assert n0 >= 1 and n1 >= 1
        before = eng.features_download(f1, n1)
        first = eng.features_download(f0, n0)
        assert len(before[0]) == n1 and before[1].any() and first[0].tobytes() != before[0].tobytes()
        eng.features_free(f0)
        _same(eng.features_download(f1, n1), before, ("the other set of the block",))
        out = eng.features_match_offset(f1, f1)
        assert int(out[4]) == n1 and int(out[5]) == n1
        eng.features_free(f1)
        with pytest.raises(isa.VfsmsError, match="unknown handle"):
            eng.features_download(f1, n1)
    finally:
        eng.close()


def test_a_shading_field_outlives_another():
    rng = np.random.default_rng(16)
    tiles = [rng.integers(0, 256, (32, 40)).astype(np.uint8) for _ in range(3)]

    def applied(eng, field):
        handles = [eng.tile_upload(t) for t in tiles]
        try:
            eng.shading_apply(field, handles)
            out = []
            for h in handles:
                cv = eng.canvas_create(32, 40, 1)
                eng.canvas_paste_tile(cv, h, 0, 0)
                out.append(eng.canvas_download(cv, 32, 40, 1))
                eng.canvas_free(cv)
            return out
        finally:
            for h in handles:
                eng.tile_free(h)

    eng = isa.Engine(0)
    try:
        handles = [eng.tile_upload(t) for t in tiles]
        f1, f2 = eng.shading_estimate(handles, 50, 3), eng.shading_estimate(handles, 20, 2)
        gain2 = eng.shading_download(f2)
        assert eng.shading_download(f1).tobytes() != gain2.tobytes()
        both = applied(eng, f2)
        assert any(b.tobytes() != t.tobytes() for b, t in zip(both, tiles))
        eng.shading_free(f1)
        _same(eng.shading_download(f2), gain2, ("gain",))
        _same(applied(eng, f2), both, ("applied",))
        eng.shading_free(f2)
    finally:
        eng.close()
