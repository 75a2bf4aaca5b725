"""The 16-bit shading correction on the device (csrc/deep_shading_kernels.hip and the box / level / gain kernels it shares with the 8-bit
path, vfsms_deep_shading_*) against its specification tests/deep_shading_ref.py, over the sets of tests/deep_shading_cases.py, and every
refusal of the C ABI.  Every comparison is np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import imagestitch_amd as isa

import deep_cases as DC
import deep_ref as DR
import deep_shading_cases as DSC
import deep_shading_ref as DSR

pytestmark = pytest.mark.gpu


def _handle_counter(engine):
    """the context hands out handles of every kind from one counter (test_deep_gpu.py): the handle of a fresh 1 x 1 tile, freed again, tells
    where it stands, so two readings that differ by one had no handle created between them"""
    h = engine.tile_upload(np.zeros((1, 1), np.uint8))
    engine.tile_free(h)
    return h


def _same(got, want):
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.parametrize("name", sorted(DSC.SETS))
def test_estimate_and_apply_equal_the_reference(engine, name):
    tiles, other = DSC.tiles(name)
    n = len(tiles)
    named = [k for k in range(n) if k != 1]                  # tile 1 (where there is one) is estimated from but never corrected
    handles = [engine.deep_upload(t) for t in tiles]
    bystander = engine.deep_upload(other)                    # a tile of the same shape that no call names
    try:
        for percentile, radius, pedestal in DSC.combos(name):
            tag = (name, percentile, radius, pedestal)
            G, F, P = DSC.reference(name, percentile, radius, pedestal)
            before = _handle_counter(engine)
            field = engine.deep_shading_estimate(handles, percentile, radius, pedestal)
            try:
                assert _handle_counter(engine) - before == 2, tag                # the field, and nothing else
                g, f, p, d = engine.deep_shading_download(field)
                assert _same(p, P), tag + ("profile", int(np.count_nonzero(p != P)))
                assert _same(f, F), tag + ("smooth", int(np.count_nonzero(f != F)))
                assert _same(g, G), tag + ("gain", int(np.count_nonzero(g != G)))
                assert d == pedestal, tag
                for k in range(n):                           # the estimate only read
                    assert _same(engine.deep_download(handles[k]), tiles[k]), tag + (k,)
                engine.deep_shading_apply(field, [handles[k] for k in named])
                for k in range(n):
                    want = DSR.apply(tiles[k], G, pedestal) if k in named else tiles[k]
                    got = engine.deep_download(handles[k])
                    assert _same(got, want), tag + ("tile", k, int(np.count_nonzero(got != want)))
                assert _same(engine.deep_download(bystander), other), tag
            finally:
                engine.deep_shading_free(field)
            for k in named:                                  # fresh samples for the next combination
                engine.deep_free(handles[k])
                handles[k] = engine.deep_upload(tiles[k])
    finally:
        for h in handles + [bystander]:
            engine.deep_free(h)


@pytest.mark.parametrize("name", ["1x1-full-1", "3x5-12bit-7", "33x131-full-2", "70x257-12bit-7"])
def test_a_gain_from_the_host_is_applied_as_it_is(engine, name):
    tiles, _ = DSC.tiles(name)
    rng = np.random.default_rng(21)
    gain = rng.integers(0, 65536, tiles[0].shape).astype(np.uint16)
    gain.reshape(-1)[::3] = rng.integers(3000, 6000, gain.reshape(-1)[::3].shape)         # gains near one among the extremes
    for pedestal in DSC.PEDESTALS:
        handles = [engine.deep_upload(t) for t in tiles]
        field = engine.deep_shading_from_gain(gain, pedestal)
        try:
            g, f, p, d = engine.deep_shading_download(field)
            assert _same(g, gain) and d == pedestal
            assert f.dtype == np.uint16 and p.dtype == np.uint16 and f.shape == gain.shape and not f.any() and not p.any()
            engine.deep_shading_apply(field, handles)
            for t, h in zip(tiles, handles):
                assert _same(engine.deep_download(h), DSR.apply(t, gain, pedestal)), (name, pedestal)
        finally:
            engine.deep_shading_free(field)
            for h in handles:
                engine.deep_free(h)


def test_download_returns_what_was_uploaded(engine):
    rng = np.random.default_rng(22)
    for h, w in DSC.SHAPES:
        t = rng.integers(0, 65536, (h, w)).astype(np.uint16)
        big = np.zeros((h, 2 * w + 7), np.uint16)
        view = big[:, 3:3 + w]                               # rows 2 w + 7 samples apart, starting 3 samples (6 bytes) in
        view[:] = t
        for src in (t, view):
            d = engine.deep_upload(src)
            try:
                assert _same(engine.deep_download(d), t)
                out = np.full((h, 2 * w + 5), 0xABCD, np.uint16)
                engine.deep_download(d, out=out[:, 2:2 + w])
                assert np.array_equal(out[:, 2:2 + w], t)
                out[:, 2:2 + w] = 0xABCD
                assert (out == 0xABCD).all()                 # nothing written between the rows of the view
            finally:
                engine.deep_free(d)


def test_corrected_tiles_compose_with_the_mosaic(engine):
    c = DC.layouts()["jitter3x3"]
    tiles = [c["tiles"][u] for u in c["use"]]
    pedestal = 2000
    handles = [engine.deep_upload(t) for t in tiles]
    field = engine.deep_shading_estimate(handles, 50, 4, pedestal)
    try:
        engine.deep_shading_apply(field, handles)
        got = engine.deep_mosaic_rows(handles, c["yx"], c["rows"], c["cols"], "feather", 0)
        want = DR.mosaic(DSR.correct(tiles, 50, 4, pedestal), c["yx"], c["rows"], c["cols"], 1, 0)
        assert _same(got, want)
    finally:
        engine.deep_shading_free(field)
        for h in handles:
            engine.deep_free(h)


def test_flatfield16_equals_correct(engine):
    tiles, _ = DSC.tiles("33x131-12bit-7")
    before = _handle_counter(engine)
    out, gain = isa.flatfield16(engine, tiles, percentile=37, radius=4, pedestal=2000)
    assert _handle_counter(engine) - before == len(tiles) + 2                    # the tiles and the field, all freed again:
    with pytest.raises(isa.VfsmsError):
        engine.deep_free(before + len(tiles))                                    # the last tile's handle is gone
    with pytest.raises(isa.VfsmsError):
        engine.deep_shading_free(before + len(tiles) + 1)                        # and so is the field's
    want = DSR.correct(tiles, 37, 4, 2000)
    assert _same(gain, DSR.estimate(tiles, 37, 4, 2000)[0])
    assert len(out) == len(tiles) and all(_same(a, b) for a, b in zip(out, want))
    given = np.full(tiles[0].shape, 5000, np.uint16)
    out, gain = isa.flatfield16(engine, tiles, pedestal=100, gain=given)
    assert _same(gain, given) and all(_same(a, DSR.apply(t, given, 100)) for a, t in zip(out, tiles))
    with pytest.raises(ValueError):
        isa.flatfield16(engine, [tiles[0], tiles[0][:, :5]])
    with pytest.raises(ValueError):
        isa.flatfield16(engine, [tiles[0].astype(np.uint8)])


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_every_bad_argument_is_refused_with_nothing_written(engine):
    lib, ctx = engine.lib, engine.ctx
    BAD = -1
    rng = np.random.default_rng(23)
    t = [rng.integers(0, 65536, (40, 60)).astype(np.uint16) for _ in range(3)]
    small = rng.integers(0, 65536, (40, 59)).astype(np.uint16)
    deeps = [engine.deep_upload(a) for a in t]
    odd = engine.deep_upload(small)
    tile = engine.tile_upload(np.zeros((40, 60), np.uint8))
    field = engine.deep_shading_estimate(deeps, 50, 4, 2000)
    field8 = engine.shading_from_gain(np.full((40, 60), 4096, np.uint16))
    p = lambda a: a.ctypes.data_as(C.c_void_p)             # noqa: E731
    arr = lambda *hs: np.array(hs, np.int64)               # noqa: E731
    three, many = arr(*deeps), np.full(4097, deeps[0], np.int64)
    try:
        def refused(call, *outputs):
            """the call returns BAD_ARG (or the binding raises VfsmsError), its output arrays keep their sentinel, no handle was created and
            every tile still holds its samples"""
            before = _handle_counter(engine)
            keep = [o.copy() for o in outputs]
            try:
                assert call() == BAD
            except isa.VfsmsError:
                pass
            for o, k in zip(outputs, keep):
                assert np.array_equal(o, k)
            assert _handle_counter(engine) - before == 1
            for a, d in zip(t + [small], deeps + [odd]):
                assert np.array_equal(engine.deep_download(d), a)

        # estimate
        out = C.c_int64(-7)
        est = lambda n, hs, pc=50, r=4, d=0, f=C.byref(out): (lambda: lib.vfsms_deep_shading_estimate(ctx, n, p(hs), pc, r, d, f))      # noqa: E731
        for n, hs in ((0, three), (4097, many), (1, arr(tile)), (1, arr(deeps[0] + 100000)), (1, arr(field)), (3, arr(deeps[0], tile, deeps[1])),
                      (2, arr(deeps[0], odd)), (4, arr(deeps[0], deeps[1], deeps[2], odd))):
            refused(est(n, hs))
            assert out.value == -7
        for kw in (dict(pc=-1), dict(pc=101), dict(r=0), dict(r=128), dict(d=-1), dict(d=65536), dict(f=None)):
            refused(est(3, three, **kw))
            assert out.value == -7
        assert lib.vfsms_deep_shading_estimate(ctx, 3, None, 50, 4, 0, C.byref(out)) == BAD and out.value == -7
        with pytest.raises(isa.VfsmsError):
            engine.deep_shading_estimate([deeps[0], odd])
        with pytest.raises(isa.VfsmsError):
            engine.deep_shading_estimate([tile])
        # the first fault in argument order is the one reported: the count before the handle before the shape before the parameters
        msg = C.create_string_buffer(512)
        assert est(0, arr(tile), pc=101)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"1..4096" in msg.value
        assert est(2, arr(tile, odd), pc=101)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"not a deep tile" in msg.value
        assert est(2, arr(deeps[0], odd), pc=101)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"one shape" in msg.value
        assert est(3, three, pc=101)() == BAD and lib.vfsms_last_error(msg, 512) == 0 and b"percentile" in msg.value
        # from_gain
        gain = np.full((40, 60), 4096, np.uint16)
        for h, w, d, g, f in ((0, 60, 0, p(gain), C.byref(out)), (40, 0, 0, p(gain), C.byref(out)), (32769, 60, 0, p(gain), C.byref(out)),
                              (40, 32769, 0, p(gain), C.byref(out)), (40, 60, -1, p(gain), C.byref(out)), (40, 60, 65536, p(gain), C.byref(out)),
                              (40, 60, 0, None, C.byref(out)), (40, 60, 0, p(gain), None)):
            refused(lambda: lib.vfsms_deep_shading_from_gain(ctx, g, h, w, d, f))
            assert out.value == -7
        # apply
        app = lambda f, n, hs: (lambda: lib.vfsms_deep_shading_apply(ctx, C.c_int64(f), n, p(hs)))      # noqa: E731
        for f, n, hs in ((field, 0, three), (field, 4097, many), (field, 1, arr(tile)), (field, 1, arr(deeps[0] + 100000)), (field, 1, arr(field)),
                         (field, 2, arr(deeps[0], tile)), (field, 1, arr(odd)), (field, 2, arr(deeps[0], odd)),
                         (field, 2, arr(deeps[0], deeps[0])), (field, 3, arr(deeps[1], deeps[0], deeps[1])),
                         (field8, 3, three), (deeps[0], 3, three), (tile, 3, three), (field + 100000, 3, three)):
            refused(app(f, n, hs))
        assert lib.vfsms_deep_shading_apply(ctx, C.c_int64(field), 3, None) == BAD
        with pytest.raises(isa.VfsmsError):
            engine.deep_shading_apply(field8, deeps)         # an 8-bit field is no deep field
        with pytest.raises(isa.VfsmsError):
            engine.deep_shading_apply(field, deeps + [deeps[0]])
        # download of a field
        g = np.full((40, 60), 0xABCD, np.uint16); s = g.copy(); q = g.copy()
        ped = C.c_int32(-7)
        for f, gp in ((field8, p(g)), (deeps[0], p(g)), (tile, p(g)), (field + 100000, p(g)), (field, None)):
            refused(lambda: lib.vfsms_deep_shading_download(ctx, C.c_int64(f), gp, p(s), p(q), C.byref(ped)), g, s, q)
            assert ped.value == -7
        assert lib.vfsms_deep_shading_download(ctx, C.c_int64(field), p(g), None, None, None) == 0 and not (g == 0xABCD).all()      # the planes after the gain may be NULL
        # download of a tile
        buf = np.full((40, 64), 0xABCD, np.uint16)
        for d, o, stride in ((tile, p(buf), 128), (field, p(buf), 128), (deeps[0] + 100000, p(buf), 128), (deeps[0], None, 128), (deeps[0], p(buf), 119),
                             (deeps[0], p(buf), 0), (deeps[0], p(buf), -128)):
            refused(lambda: lib.vfsms_deep_download(ctx, C.c_int64(d), o, stride), buf)
        assert lib.vfsms_deep_download(ctx, C.c_int64(deeps[0]), p(buf), 128) == 0 and np.array_equal(buf[:, :60], t[0]) and (buf[:, 60:] == 0xABCD).all()
        # a deep field is no field to the 8-bit entries, an 8-bit field none to the deep ones, and freeing is by kind
        u8 = engine.tile_upload(np.zeros((40, 60), np.uint8))
        try:
            for call in (lambda: engine.shading_apply(field, [u8]), lambda: engine.shading_free(field), lambda: engine.deep_shading_free(field8),
                         lambda: engine.deep_shading_free(deeps[0]), lambda: engine.deep_free(field), lambda: engine.tile_free(field),
                         lambda: engine.shading_estimate(deeps), lambda: engine.shading_apply(field8, deeps)):
                before = _handle_counter(engine)
                with pytest.raises(isa.VfsmsError):
                    call()
                assert _handle_counter(engine) - before == 1
            refused(lambda: lib.vfsms_shading_download(ctx, C.c_int64(field), p(g), None, None), g)
        finally:
            engine.tile_free(u8)
        # everything is alive and well after all of it
        G = DSR.estimate(t, 50, 4, 2000)[0]
        assert np.array_equal(engine.deep_shading_download(field)[0], G)
        assert np.array_equal(engine.shading_download(field8), np.full((40, 60), 4096, np.uint16))
        engine.deep_shading_apply(field, deeps)
        for a, d in zip(t, deeps):
            assert np.array_equal(engine.deep_download(d), DSR.apply(a, G, 2000))
    finally:
        engine.deep_shading_free(field)
        engine.shading_free(field8)
        engine.tile_free(tile)
        for d in deeps + [odd]:
            engine.deep_free(d)
