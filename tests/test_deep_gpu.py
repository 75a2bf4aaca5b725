"""The 16-bit path on the device (csrc/deep_kernels.hip, vfsms_deep_*) against its specification tests/deep_ref.py: the exact window
selection and the 8-bit views over tile sets of mixed shapes, the mosaic gather over the layouts of tests/deep_cases.py in every band
size, and every refusal of the C ABI.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import imagestitch_amd as isa

import deep_cases as DC
import deep_ref as DR

pytestmark = pytest.mark.gpu


def _tile_bytes(engine, handle, shape):
    """the bytes of a resident 8-bit tile, read back the way test_focus_gpu._tile_bytes does it"""
    cv = engine.canvas_create(shape[0], shape[1], 1)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, shape[0], shape[1], 1)
    finally:
        engine.canvas_free(cv)


def _handle_counter(engine):
    """the context hands out handles of every kind from one counter: the handle of a fresh 1 x 1 tile (freed again) tells where it stands, so
    two readings that differ by one had no handle created between them"""
    h = engine.tile_upload(np.zeros((1, 1), np.uint8))
    engine.tile_free(h)
    return h


@pytest.fixture(scope="module")
def sets(engine):
    """kind -> (tiles, deep handles), uploaded once; one tile of the "full" set goes up from a strided view with an odd element offset"""
    out = {}
    for kind in DC.KINDS:
        tiles = DC.tile_set(kind)
        handles = []
        for k, t in enumerate(tiles):
            if kind == "full" and k == 3:
                big = np.zeros((t.shape[0], 2 * t.shape[1] + 7), np.uint16)
                view = big[:, 3:3 + t.shape[1]]               # rows 2 w + 7 samples apart, starting 3 samples (6 bytes) in
                view[:] = t
                assert not view.flags["C_CONTIGUOUS"]
                handles.append(engine.deep_upload(view))
            else:
                handles.append(engine.deep_upload(t))
        out[kind] = (tiles, handles)
    yield out
    for _tiles, handles in out.values():
        for h in handles:
            engine.deep_free(h)


@pytest.mark.parametrize("kind", DC.KINDS)
def test_window_is_exact(engine, sets, kind):
    tiles, handles = sets[kind]
    for lo_ppm, hi_ppm in DC.PPM_PAIRS:
        assert engine.deep_window(handles, lo_ppm, hi_ppm) == DR.window(tiles, lo_ppm, hi_ppm), (kind, lo_ppm, hi_ppm)
    for k in (0, 2, 3):                                      # single tiles: one sample, less than a chunk, more than one chunk
        assert engine.deep_window(handles[k:k + 1], 1000, 999000) == DR.window(tiles[k:k + 1], 1000, 999000), (kind, k)
    assert engine.deep_window(handles + handles[::-1], 250000, 750000) == DR.window(tiles + tiles, 250000, 750000)      # a handle may be named twice


@pytest.mark.parametrize("kind", DC.KINDS)
def test_reduce_is_exact(engine, sets, kind):
    tiles, handles = sets[kind]
    k = int(tiles[2][5, 7])
    k = min(max(k, 0), 65534)
    windows = [(0, 65535), (k, k + 1), (100, 4195), (65534, 65535), DR.window(tiles, 1000, 999000)]
    for lo, hi in windows:
        before = _handle_counter(engine)
        views = engine.deep_reduce(handles, lo, hi)
        try:
            assert len(views) == len(tiles) and _handle_counter(engine) - before == len(tiles) + 1
            for t, v in zip(tiles, views):
                got = _tile_bytes(engine, v, t.shape)
                want = DR.reduce(t, lo, hi)
                assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want), (kind, lo, hi, t.shape, int(np.count_nonzero(got != want)))
        finally:
            for v in views:
                engine.tile_free(v)


def test_reduce_division_over_every_numerator(engine):
    """every sample value through windows whose D is small, large, a power of two and not: the reciprocal-and-fix-up division of the kernel
    against the reference's integer division (65536 samples: four chunks)"""
    t = np.arange(65536, dtype=np.uint16).reshape(256, 256)
    h = engine.deep_upload(t)
    try:
        for lo, hi in ((0, 1), (0, 2), (0, 3), (0, 255), (0, 256), (0, 257), (1, 65535), (0, 65535), (0, 65534), (12345, 12352), (2003, 5069), (300, 33068)):
            (v,) = engine.deep_reduce([h], lo, hi)
            try:
                assert np.array_equal(_tile_bytes(engine, v, t.shape), DR.reduce(t, lo, hi)), (lo, hi)
            finally:
                engine.tile_free(v)
    finally:
        engine.deep_free(h)


@pytest.fixture(scope="module")
def placed(engine):
    """layout name -> the deep handles of its placed tiles (a tile used twice is ONE handle named twice)"""
    out, owned = {}, []
    for name, c in DC.layouts().items():
        hs = [engine.deep_upload(t) for t in c["tiles"]]
        owned += hs
        out[name] = [hs[u] for u in c["use"]]
    yield out
    for h in owned:
        engine.deep_free(h)


@pytest.mark.parametrize("name", sorted(DC.layouts()))
def test_mosaic_equals_the_reference_in_every_band(engine, placed, name):
    c = DC.layouts()[name]
    rows, cols, handles = c["rows"], c["cols"], placed[name]
    configs = [(0, 0)] + [(1, f) for f in DC.FEATHERS]
    for mode, feather in configs:
        want = DC.reference(name, mode, feather)
        got = engine.deep_mosaic_rows(handles, c["yx"], rows, cols, mode, feather)
        assert got.dtype == np.uint16 and got.shape == want.shape and np.array_equal(got, want), (name, mode, feather, int(np.count_nonzero(got != want)))
        for band in ((1, 7, 64) if (mode, feather) in ((0, 0), (1, 5)) else (7, 64)):
            for r0 in range(0, rows, band):
                n = min(band, rows - r0)                     # the last band is ragged
                got = engine.deep_mosaic_rows(handles, c["yx"], rows, cols, mode, feather, r0, n)
                assert got.shape == (n, cols) and np.array_equal(got, want[r0:r0 + n]), (name, mode, feather, band, r0)
    if name == "gap":                                        # bands no tile touches
        assert not DC.reference(name, 1, 0)[33:50].any() and not engine.deep_mosaic_rows(handles, c["yx"], rows, cols, 1, 0, 34, 15).any()
    if name == "all_max":
        want = DC.reference(name, 1, 0)
        assert set(np.unique(want).tolist()) == {0, 65535}


def test_mosaic_does_not_depend_on_the_order_of_the_tiles(engine, placed):
    c = DC.layouts()["jitter3x3"]
    handles = placed["jitter3x3"]
    order = [4, 8, 0, 2, 6, 1, 7, 3, 5]
    a = engine.deep_mosaic_rows(handles, c["yx"], c["rows"], c["cols"], "feather", 5)
    b = engine.deep_mosaic_rows([handles[k] for k in order], [c["yx"][k] for k in order], c["rows"], c["cols"], "feather", 5)
    assert np.array_equal(a, b)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_with_nothing_written(engine):
    lib, ctx = engine.lib, engine.ctx
    BAD = -1
    t = np.arange(40 * 60, dtype=np.uint16).reshape(40, 60)
    deep = engine.deep_upload(t)
    tile = engine.tile_upload(np.zeros((40, 60), np.uint8))
    one = np.array([deep], np.int64)
    many = np.full(4097, deep, np.int64)
    wrong = np.array([tile], np.int64)
    unknown = np.array([deep + 100000], np.int64)
    yx = np.zeros((4097, 2), np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    try:
        def refused(call, *outputs):
            """the call returns BAD_ARG, its output arrays keep their sentinel, no handle was created"""
            before = _handle_counter(engine)
            keep = [o.copy() for o in outputs]
            assert call() == BAD
            for o, k in zip(outputs, keep):
                assert np.array_equal(o, k)
            assert _handle_counter(engine) - before == 1

        # upload: a side outside 1..32768, a stride below 2 w
        hd = C.c_int64(-7)
        for h, w, stride in ((0, 60, 120), (40, 0, 120), (32769, 60, 120), (40, 32769, 65538), (40, 60, 119)):
            before = _handle_counter(engine)
            assert lib.vfsms_deep_upload(ctx, p(t), h, w, stride, C.byref(hd)) == BAD and hd.value == -7
            assert _handle_counter(engine) - before == 1
        # window
        win = np.array([-5, -6], np.int32)
        for n, hs in ((0, one), (4097, many), (1, wrong), (1, unknown)):
            refused(lambda: lib.vfsms_deep_window(ctx, n, p(hs), 1000, 999000, p(win)), win)
        for lo_ppm, hi_ppm in ((-1, 5), (10, 5), (0, 1000001)):
            refused(lambda: lib.vfsms_deep_window(ctx, 1, p(one), lo_ppm, hi_ppm, p(win)), win)
        # reduce
        out = np.full(4097, -9, np.int64)
        for n, hs in ((0, one), (4097, many), (1, wrong), (1, unknown)):
            refused(lambda: lib.vfsms_deep_reduce(ctx, n, p(hs), 0, 65535, p(out)), out)
        for lo, hi in ((5, 5), (6, 5), (-1, 5), (0, 65536)):
            refused(lambda: lib.vfsms_deep_reduce(ctx, 1, p(one), lo, hi, p(out)), out)
        # mosaic
        band = np.full((40, 60), 0xABCD, np.uint16)

        def mosaic(n=1, hs=one, at=(0, 0), rows=40, cols=60, mode=1, feather=0, row0=0, nrows=40):
            yx[0] = at
            return lambda: lib.vfsms_deep_mosaic_rows(ctx, n, p(hs), p(yx), rows, cols, mode, feather, row0, nrows, p(band))
        assert mosaic()() == 0 and np.array_equal(band, t)       # (the arguments the refusals vary are good ones)
        band[:] = 0xABCD
        for kw in (dict(n=0), dict(n=4097, hs=many), dict(hs=wrong), dict(hs=unknown),
                   dict(at=(1, 0)), dict(at=(0, 1)), dict(at=(-1, 0)), dict(at=(0, -1)), dict(rows=39), dict(cols=59),
                   dict(mode=2), dict(mode=-1), dict(feather=-1), dict(feather=32768),
                   dict(row0=-1), dict(nrows=0), dict(row0=1, nrows=40), dict(row0=40, nrows=1),
                   dict(rows=40000, cols=40000, nrows=30000)):
            refused(mosaic(**kw), band)
        # the first fault in argument order is the one reported: a bad count before a bad handle before a bad mode before a bad band
        msg = C.create_string_buffer(512)
        assert mosaic(n=0, hs=wrong, mode=7, nrows=0)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"1..4096" in msg.value
        assert mosaic(hs=wrong, mode=7, nrows=0)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"not a deep tile" in msg.value
        assert mosaic(mode=7, nrows=0)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"mode" in msg.value
        # a deep handle is no tile to the 8-bit entries, and freeing is by kind
        with pytest.raises(isa.VfsmsError):
            engine.tile_free(deep)
        with pytest.raises(isa.VfsmsError):
            engine.focus_scores([deep])
        with pytest.raises(isa.VfsmsError):
            engine.deep_free(tile)
        cv = engine.canvas_create(40, 60, 1)
        try:
            with pytest.raises(isa.VfsmsError):
                engine.canvas_paste_tile(cv, deep, 0, 0)
        finally:
            engine.canvas_free(cv)
        assert engine.deep_window([deep], 0, 1000000) == (0, 2399)      # both handles are alive and well after all of it
    finally:
        engine.deep_free(deep)
        engine.tile_free(tile)
