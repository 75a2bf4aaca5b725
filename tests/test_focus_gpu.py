"""Method.focusStack on the device against tests/focus_ref.py, exactly (np.array_equal of out, D and S): shapes down to one pixel, rows that
are no multiple of four bytes, several blocks with ragged edges, radii beyond the tile, 2 .. 64 planes, ties, both modes, the new resident
tile, strided tiles behind an odd base address, the refusals of the C ABI, and the two-step call through Stitcher."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import imagestitch_amd as isa

import focus_cases as FC
import focus_ref as FR

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (3, 5), (5, 7, 3), (33, 130, 3), (70, 257), (97, 201, 3)]


def _upload(engine, tiles):
    return [engine.tile_upload_color(t) if t.ndim == 3 else engine.tile_upload(t) for t in tiles]


def _free(engine, handles):
    for h in handles:
        engine.tile_free(h)


def _stack(rng, kind, n, shape):
    if kind == "random":
        return [rng.integers(0, 256, shape).astype(np.uint8) for _ in range(n)]
    if kind == "ties":
        return [rng.choice(np.array([0, 17, 255], np.uint8), shape) for _ in range(n)]
    if kind == "flat":
        return [np.full(shape, 10 * k + 3, np.uint8) for k in range(n)]
    one = rng.integers(0, 256, shape).astype(np.uint8)
    return [one.copy() for _ in range(n)]


def _tile_bytes(engine, handle, shape):
    ch = shape[2] if len(shape) == 3 else 1
    cv = engine.canvas_create(shape[0], shape[1], ch)
    try:
        engine.canvas_paste_tile(cv, handle, 0, 0)
        return engine.canvas_download(cv, shape[0], shape[1], ch)
    finally:
        engine.canvas_free(cv)


def _check(engine, handles, tiles, R, median, mode="pixel", tag=None):
    out, D, S = engine.focus_stack(handles, mode=mode, radius=R, median=median)
    wout, wD, wS = FR.fuse(tiles, R, median, mode)
    assert S.dtype == np.int64 and np.array_equal(S, wS), (tag, S, wS)
    assert D.dtype == np.uint8 and D.shape == wD.shape and np.array_equal(D, wD), (tag, int(np.count_nonzero(D != wD)))
    assert out.dtype == np.uint8 and out.shape == wout.shape and np.array_equal(out, wout), (tag, int(np.count_nonzero(out != wout)))
    return out, D, S


@pytest.mark.parametrize("R", [1, 4, 31])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_pixel_mode(engine, shape, R):
    """(33, 130, 3): rows of 390 bytes, no multiple of 4; (70, 257) and (97, 201, 3): several blocks, ragged on both axes; R = 31: the
    window is larger than the small tiles and the kernel takes its 32-row block.  N in {2, 3, 64}, median in {0, 1}, every stack kind."""
    rng = np.random.default_rng(sum(shape) + R)
    tiles = _stack(rng, "random", 64, shape)
    handles = _upload(engine, tiles)
    try:
        for n in (2, 3, 64):
            for median in (0, 1):
                _check(engine, handles[:n], tiles[:n], R, median, tag=(n, median))
    finally:
        _free(engine, handles)
    for kind, n in (("ties", 3), ("ties", 64), ("equal", 3), ("flat", 3)):
        tiles = _stack(rng, kind, n, shape)
        handles = _upload(engine, tiles)
        try:
            for median in (0, 1):
                out, D, _S = _check(engine, handles, tiles, R, median, tag=(kind, n, median))
                if kind in ("equal", "flat"):
                    assert not D.any() and np.array_equal(out, tiles[0])
        finally:
            _free(engine, handles)


@pytest.mark.parametrize("shape", [(48, 80), (64, 64, 3)], ids=("gray", "colour"))
def test_synthetic_series(engine, shape):
    """a focus_cases stack: the device picks the planes the specification picks, and they are the right ones"""
    tiles, sharp, depth = FC.stack(shape, 4, "quad", seed=3)
    handles = _upload(engine, tiles)
    try:
        out, D, _S = _check(engine, handles, tiles, 4, 1)
        assert np.mean(D == depth) >= 0.95
        best = min(np.abs(t.astype(np.int32) - sharp).mean() for t in tiles)
        assert np.abs(out.astype(np.int32) - sharp).mean() <= best / 10
        _check(engine, handles, tiles, 4, 1, mode="plane")
    finally:
        _free(engine, handles)


@pytest.mark.parametrize("shape", [(5, 7, 3), (70, 257), (33, 130, 3)], ids=lambda s: "x".join(map(str, s)))
def test_plane_mode_and_scores(engine, shape):
    rng = np.random.default_rng(shape[1])
    tiles = _stack(rng, "random", 5, shape)
    tiles[1][...] = np.where(rng.random(shape) < 0.5, 0, 255).astype(np.uint8)
    tiles[3] = tiles[1].copy()                                # two planes of one score, the largest: the lower index is taken
    handles = _upload(engine, tiles)
    try:
        out, D, S = _check(engine, handles, tiles, 4, 1, mode="plane")
        assert S[1] == S[3] == S.max() and (D == 1).all() and np.array_equal(out, tiles[1])
        assert np.array_equal(engine.focus_scores(handles), FR.scores(tiles))
    finally:
        _free(engine, handles)


def test_scores_of_mixed_shapes(engine):
    rng = np.random.default_rng(8)
    tiles = [rng.integers(0, 256, s).astype(np.uint8) for s in ((1, 1), (3, 5), (33, 130, 3), (70, 257), (9, 4, 3), (1, 300))]
    handles = _upload(engine, tiles)
    try:
        got = engine.focus_scores(handles)
        assert got.dtype == np.int64 and np.array_equal(got, FR.scores(tiles))
        assert np.array_equal(engine.focus_scores(handles[2:3]), FR.scores(tiles[2:3]))
    finally:
        _free(engine, handles)


@pytest.mark.parametrize("shape", [(33, 130, 3), (70, 257)], ids=("colour", "gray"))
def test_out_tile(engine, shape):
    """want_tile: a NEW resident tile that holds `out`, can be placed on a canvas and freed; the planes are unchanged afterwards"""
    rng = np.random.default_rng(4)
    tiles = _stack(rng, "random", 3, shape)
    handles = _upload(engine, tiles)
    try:
        tile, D, S = engine.focus_stack(handles, radius=2, median=1, want_tile=True)
        try:
            wout, wD, wS = FR.fuse(tiles, 2, 1)
            assert tile not in handles and np.array_equal(D, wD) and np.array_equal(S, wS)
            assert np.array_equal(_tile_bytes(engine, tile, shape), wout)
            again = engine.focus_stack(handles + [tile], radius=2, median=0)          # the new tile is a tile like any other
            assert np.array_equal(again[0], FR.fuse(tiles + [wout], 2, 0)[0])
        finally:
            engine.tile_free(tile)
        with pytest.raises(isa.VfsmsError):
            engine.tile_free(tile)
        for k, h in enumerate(handles):
            assert np.array_equal(_tile_bytes(engine, h, shape), tiles[k]), k
    finally:
        _free(engine, handles)


def test_strided_tiles_behind_an_odd_base(engine):
    """rows 41 bytes apart for w = 37 behind an odd base address (tile_wrap): neither the stride nor the alignment of the dword path holds,
    and the alignment differs from row to row"""
    rng = np.random.default_rng(11)
    h, w, stride, n = 12, 37, 41, 5
    tiles = [rng.integers(0, 256, (h, w)).astype(np.uint8) for _ in range(n)]
    padded = rng.integers(0, 256, (n, h, stride)).astype(np.uint8)      # the padding holds other bytes: none of them may be read as pixels
    for k, t in enumerate(tiles):
        padded[k, :, :w] = t
    loaded = [ln.split()[-1] for ln in open("/proc/self/maps") if "libamdhip64.so" in ln.split()[-1]]
    hip = C.CDLL(loaded[0] if loaded else "libamdhip64.so")            # the HIP runtime the library itself runs on
    buf = C.c_void_p()
    assert hip.hipMalloc(C.byref(buf), C.c_size_t(padded.size + 1)) == 0
    handles = []
    try:
        assert hip.hipMemcpy(C.c_void_p(buf.value + 1), padded.ctypes.data_as(C.c_void_p), C.c_size_t(padded.size), 1) == 0
        handles = [engine.tile_wrap(buf.value + 1 + k * h * stride, h, w, stride) for k in range(n)]
        for R in (1, 4, 31):
            for median in (0, 1):
                _check(engine, handles, tiles, R, median, tag=(R, median))
        _check(engine, handles, tiles, 4, 1, mode="plane")
        assert np.array_equal(engine.focus_scores(handles), FR.scores(tiles))
        back = np.empty_like(padded)
        engine.sync()
        assert hip.hipMemcpy(back.ctypes.data_as(C.c_void_p), C.c_void_p(buf.value + 1), C.c_size_t(padded.size), 2) == 0
        assert np.array_equal(back, padded)
    finally:
        _free(engine, handles)
        engine.sync()
        hip.hipFree(buf)


def test_refusals_create_no_tile(engine):
    """every refusal of vfsms_focus_stack / vfsms_focus_scores is VFSMS_ERR_BAD_ARG (-1 is not assumed: the code is read from the header's
    enum through the message of VfsmsError), writes nothing and creates no tile: the handle counter of the context has not moved"""
    rng = np.random.default_rng(2)
    tiles = _stack(rng, "random", 3, (16, 24))
    handles = _upload(engine, tiles)
    ho = engine.tile_upload(rng.integers(0, 256, (16, 25)).astype(np.uint8))
    hc = engine.tile_upload_color(rng.integers(0, 256, (16, 24, 3)).astype(np.uint8))
    h2 = [engine.tile_upload_color(rng.integers(0, 256, (16, 24, 2)).astype(np.uint8)) for _ in range(2)]
    lib, ctx = engine.lib, engine.ctx
    out = np.full((16, 24), 7, np.uint8); D = np.full((16, 24), 7, np.uint8); S = np.full(70, -5, np.int64)
    tile = C.c_int64(-9)

    def raw(hs, mode=0, radius=4, median=1):
        th = np.ascontiguousarray(hs, np.int64)
        return lib.vfsms_focus_stack(ctx, len(th), th.ctypes.data_as(C.c_void_p), mode, radius, median, C.byref(tile),
                                     out.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p))

    def raw_scores(hs):
        th = np.ascontiguousarray(hs, np.int64)
        return lib.vfsms_focus_scores(ctx, len(th), th.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p))
    BAD_ARG = raw([], 0, 4, 1)
    assert BAD_ARG != 0
    try:
        with pytest.raises(isa.VfsmsError) as e:
            engine.focus_stack(handles, radius=0)
        assert "error %d:" % BAD_ARG in str(e.value)           # the code the binding reports for a bad argument
        def said():
            buf = C.create_string_buffer(512)
            lib.vfsms_last_error(buf, 512)
            return buf.value.decode()
        # (the call, what the library says): one fault each, then two at once -- an unknown handle is reported before any tile is judged
        for call, says in ((lambda: raw(handles[:1]), "focus_stack: 2..64 tiles, got 1"),                       # n outside 2..64
                           (lambda: raw([handles[k % 3] for k in range(65)]), "focus_stack: 2..64 tiles, got 65"),
                           (lambda: raw([]), "focus_stack: 2..64 tiles, got 0"),
                           (lambda: raw(handles + [987654321]), "focus_stack: unknown tile handle"),
                           (lambda: raw(handles + [ho]), "focus_stack: plane 3 is 16 x 25 x 1, plane 0 is 16 x 24 x 1"),   # another shape
                           (lambda: raw(handles + [hc]), "focus_stack: plane 3 is 16 x 24 x 3, plane 0 is 16 x 24 x 1"),   # another channel count
                           (lambda: raw(h2), "focus_stack: tile 0 has 2 channels (1 or 3)"),
                           (lambda: raw(handles, radius=0), "focus_stack: mode 0 / radius 0 / median 1 (0 pixel or 1 plane; 1..31; 0 or 1)"),
                           (lambda: raw(handles, radius=32), "focus_stack: mode 0 / radius 32 / median 1"),
                           (lambda: raw(handles, median=2), "focus_stack: mode 0 / radius 4 / median 2"),
                           (lambda: raw(handles, median=-1), "focus_stack: mode 0 / radius 4 / median -1"),
                           (lambda: raw(handles, mode=2), "focus_stack: mode 2 / radius 4 / median 1"),
                           (lambda: raw(handles, mode=-1), "focus_stack: mode -1 / radius 4 / median 1"),
                           (lambda: raw_scores([]), "focus_scores: 1..4096 tiles, got 0"),
                           (lambda: raw_scores([handles[0]] * 4097), "focus_scores: 1..4096 tiles, got 4097"),
                           (lambda: raw_scores([handles[0], 987654321]), "focus_scores: unknown tile handle"),
                           (lambda: raw_scores([handles[0], h2[0]]), "focus_scores: tile 1 has 2 channels (1 or 3)"),
                           (lambda: raw([handles[0], handles[0], 987654321]), "focus_stack: unknown tile handle"),
                           (lambda: raw([h2[0], 987654321]), "focus_stack: unknown tile handle"),
                           (lambda: raw_scores([h2[0], handles[0], handles[0], 987654321]), "focus_scores: unknown tile handle")):
            assert call() == BAD_ARG and says in said(), (says, said())
        assert tile.value == -9 and (out == 7).all() and (D == 7).all() and (S == -5).all()
        nxt = engine.tile_upload(tiles[0])                     # handles are consecutive: none was taken in between
        assert nxt == h2[1] + 1
        engine.tile_free(nxt)
        for bad, says in ((lambda: engine.focus_stack([]), "focus_stack: 2..64 tiles, got 0"),
                          (lambda: engine.focus_stack([987654321, handles[0]]), "focus_stack: unknown tile handle"),
                          (lambda: engine.focus_stack(handles + [ho]), "focus_stack: plane 3 is 16 x 25 x 1, plane 0 is 16 x 24 x 1"),
                          (lambda: engine.focus_scores([]), "focus_scores: 1..4096 tiles, got 0")):
            with pytest.raises(isa.VfsmsError, match=re.escape(says)):
                bad()
        with pytest.raises(ValueError):
            engine.focus_stack(handles, mode="voxel")
        assert raw([handles[0], handles[0]]) == 0              # a plane named twice is only read twice
        assert tile.value > 0 and np.array_equal(out, tiles[0]) and not D.any()
        engine.tile_free(tile.value)
    finally:
        _free(engine, handles + [ho, hc] + h2)


# ---- through Stitcher ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("color", (False, True), ids=("gray", "colour"))
def test_two_step_call(engine, tmp_path, color):
    """a 2 x 2 grid of 256 x 256 tiles, each a 3-plane series on disk: imageSetFocusStack's files decode to exactly the specification's
    fusion of the decoded planes, and imageSetStitchWithMutiple on that folder gives the offsets and the mosaic of the same run on tiles
    fused by the specification"""
    from PIL import Image
    from imagestitch_amd.ingest import _imread, _list_images
    from imagestitch_amd.synthetic import SyntheticGrid
    g = SyntheticGrid(2, 2, 256, overlap=0.25)
    proj = tmp_path / "series"; (proj / "1").mkdir(parents=True)
    spec = tmp_path / "spec"; (spec / "1").mkdir(parents=True)
    for k, t in enumerate(g.tiles(threads=2)):
        f = t.astype(np.float32)
        sharp = np.clip(np.stack([0.6 * f + 30, f, 255 - 0.7 * f], -1), 0, 255).astype(np.uint8) if color else t
        planes, _sharp, _depth = FC.stack_of(sharp, 3, "quad" if k % 2 else "ramp")
        for z, p in enumerate(planes):
            Image.fromarray(p[:, :, ::-1] if color else p).save(str(proj / "1" / ("1_%02d_z%d.png" % (k, z))))
    names = ("direction", "directIncre", "roiRatio", "isColorMode", "featureMethod", "fuseMethod", "offsetEvaluate")
    old = {n: getattr(isa.Stitcher, n) for n in names}
    runs = {}
    try:
        isa.Stitcher.directIncre, isa.Stitcher.roiRatio, isa.Stitcher.isColorMode = 1, 0.3, color
        isa.Stitcher.featureMethod, isa.Stitcher.fuseMethod, isa.Stitcher.offsetEvaluate = "surf", "fadeInAndFadeOut", 3
        st = isa.Stitcher(); st._engine = engine
        msgs = []
        st.printAndWrite = msgs.append
        st.focusStack, st.focusPlanes, st.focusDepthMaps = "pixel", 3, True
        written = st.imageSetFocusStack(str(proj), str(tmp_path / "fused"), 1, fileExtension="png")
        files = _list_images(str(proj / "1"), "png")
        assert [os.path.basename(p) for p in written[0]] == ["1_%02d_z0.png" % k for k in range(4)]
        assert _list_images(str(tmp_path / "fused" / "1"), "png") == written[0] and len(msgs) == 4
        for k, path in enumerate(written[0]):
            decoded = [_imread(f, color) for f in files[3 * k:3 * k + 3]]
            wout, wD, _wS = FR.fuse(decoded, 4, 1)
            assert np.array_equal(_imread(path, color), wout), k
            depth = os.path.join(str(tmp_path / "fused" / "1"), "depth", "1_%02d_z0_depth.png" % k)
            assert np.array_equal(_imread(depth, False), wD)
            assert msgs[k] == "  focus stack 1_%02d_z0: pixels per plane %s" % (k, [int(v) for v in np.bincount(wD.reshape(-1), minlength=3)])
            Image.fromarray(wout[:, :, ::-1] if color else wout).save(str(spec / "1" / os.path.basename(path)))
        for tag, folder in (("device", tmp_path / "fused"), ("spec", spec)):
            st = isa.Stitcher(); st._engine = engine
            isa.Stitcher.direction = 1; st.direction = 1
            st.printAndWrite = lambda c: None
            offsets, real = [], st.getStitchByOffset

            def grab(fl, offs, offsets=offsets, real=real):
                offsets.append([[int(v) for v in o] for o in offs])
                return real(fl, offs)
            st.getStitchByOffset = grab
            out = tmp_path / ("out_" + tag)
            st.imageSetStitchWithMutiple(str(folder), str(out) + os.sep, 1, st.calculateOffsetForFeatureSearchIncre,
                                         startNum=1, fileExtension="png", outputfileExtension="npy")
            runs[tag] = ([np.load(str(out / f)) for f in sorted(os.listdir(str(out))) if f.endswith(".npy")], offsets)
    finally:
        for n, v in old.items():
            setattr(isa.Stitcher, n, v)
        isa.Stitcher.tempImageFeature.isBreak = True
    assert runs["device"][1] and runs["device"][1] == runs["spec"][1]
    assert len(runs["device"][0]) == len(runs["spec"][0]) >= 1
    for a, b in zip(runs["device"][0], runs["spec"][0]):
        assert a.shape == b.shape and a.ndim == (3 if color else 2) and np.array_equal(a, b)
