"""The lossless tile coder on the device (csrc/deflate_kernels.hip over csrc/deflate_core.h; Method.pyramidCompression = "deflate-device")
against its specification, tests/deflate_ref.py, byte for byte: the operator at the smallest shapes at which each mechanism can go wrong,
capacity, the canvas path with pending rows carried across bands, its contract -- the walk it shares with the JPEG tiles included -- and the
driver.  There is no tolerance anywhere."""
import os
import re
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import deflate_ref as ref                 # noqa: E402
from test_pyramid_gpu import _canvas      # noqa: E402
from test_deflate_host import depth_limit_tile, check_file, check_pillow_reads      # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kernel_constant(name):
    src = open(os.path.join(ROOT, "imagestitch_amd", "csrc", "deflate_kernels.hip")).read()
    return int(re.search(r"^#define %s (\d+)\s" % name, src, re.M).group(1))


PER_THREAD = _kernel_constant("DFL_PER_THREAD")                 # consecutive bytes a thread
THREADS = _kernel_constant("DFL_THREADS")                       # threads a workgroup: one workgroup a chunk
CHUNK = PER_THREAD * THREADS


def _image(h, w, ch, seed, noise=False):
    rng = np.random.default_rng(seed)
    shape = (h, w, 3) if ch == 3 else (h, w)
    if noise:
        return rng.integers(0, 256, shape, dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    base = 128 + 80 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.normal(0, 2, (h, w))
    img = np.stack([base, 0.7 * base + 30, 255 - base], -1) if ch == 3 else base
    return (np.clip(img, 0, 255).astype(np.uint8) >> 2) << 2     # (quantised: runs of equal differences among the literals)


def _split(payload, offsets):
    payload = bytes(payload)
    assert int(offsets[0]) == 0 and int(offsets[-1]) == len(payload)
    return [payload[int(a):int(b)] for a, b in zip(offsets[:-1], offsets[1:])]


def boundary_runs_image():
    """a gray image of 128 x 128 tiles (16384 predicted bytes: several chunks) whose predicted bytes hold zero runs of 3 .. 520 that start and
    that end one byte in front of, at, and one byte behind a boundary between two threads, two waves and two workgroups of the symbol pass;
    everything else is a filler without runs.  -> (image, number of runs placed)"""
    T = 128
    N = T * T
    assert N % CHUNK == 0 and N // CHUNK >= 2 and CHUNK % 2048 == 0, "the test's layout assumes chunks of a few KB"
    wave = 64 * PER_THREAD
    kinds = {"workgroup": [b for b in range(2048, N, 2048) if b % CHUNK == 0],
             "wave": [b for b in range(2048, N, 2048) if b % CHUNK and b % wave == 0],
             "thread": [b + 3 * PER_THREAD for b in range(2048, N, 2048)]}
    assert all(kinds.values()) and all(b % PER_THREAD == 0 and b % wave for b in kinds["thread"])
    filler = (np.arange(N) * 7 % 251 + 1).astype(np.uint8)
    assert (filler[1:] != filler[:-1]).all()
    tiles, placed = [], 0
    for kind, slots in kinds.items():
        todo = [(L, ends, d) for L in (3, 4, 5, 259, 260, 261, 262, 517, 520) for ends in (False, True) for d in (-1, 0, 1)]
        while todo:
            pred = filler.copy()
            for B in slots:
                if not todo:
                    break
                L, ends, d = todo.pop()
                a = B + d - L if ends else B + d
                assert 1 <= a and a + L < N
                pred[a:a + L] = 0
                placed += 1
            tile = np.cumsum(pred.reshape(T, T).astype(np.uint32), 1).astype(np.uint8)
            assert np.array_equal(ref.predict(tile).reshape(-1), pred)
            tiles.append(tile)
    return np.hstack(tiles), placed


def _depth_tile():
    img, pred = depth_limit_tile()
    assert ref.unlimited_depth(ref.histogram(ref.tokens(pred.tobytes()))) == 16
    return img


def _long_runs_tile():
    """one gray 1040 x 1040 tile: more chunks than the threads of the workgroup that scans them, the last chunk half empty; all zeros -- one
    run over most of the tile, through the scan's step -- but for a few rows of noise, among them the first and the last"""
    T = 1040
    assert T * T > THREADS * CHUNK and (T * T) % CHUNK
    img = np.zeros((T, T), np.uint8)
    rng = np.random.default_rng(9)
    for y in (0, 500, 501, 1008, T - 1):
        img[y] = rng.integers(0, 256, T, dtype=np.uint8)
    img[700, 300:] = 77                                          # (a non-zero run, and a zero run that starts in mid-row)
    return img


# (what, image, T): the image is made when the case runs
OPERATOR = [
    ("one pixel, the rest padding: runs longer than 258 across tile rows", lambda: np.full((1, 1, 3), 201, np.uint8), 16),
    ("edge tiles in both directions", lambda: _image(17, 33, 3, 1), 16),
    ("tiles all padding but one row or column, gray", lambda: _image(65, 65, 1, 2, noise=True), 64),
    ("tiles all padding but one row or column, colour", lambda: _image(65, 65, 3, 3, noise=True), 64),
    ("zero runs at every offset around thread, wave and workgroup boundaries", lambda: boundary_runs_image()[0], 128),
    ("noise: no run, 256 near-equal literals", lambda: _image(64, 64, 1, 4, noise=True), 64),
    ("smooth colour: matches among literals, several tiles", lambda: _image(70, 100, 3, 5), 32),
    ("the depth limit", _depth_tile, 112),
    ("more chunks a tile than the run scans take in one step, the last one short; runs across the steps", lambda: _long_runs_tile(), 1040),
    ("a 512 x 512 x 3 tile of 255s: the Adler sums", lambda: np.full((512, 512, 3), 255, np.uint8), 512),
    ("a 512 x 512 x 3 tile of noise", lambda: _image(512, 512, 3, 6, noise=True), 512),
]


@pytest.mark.parametrize("case", OPERATOR, ids=[c[0] for c in OPERATOR])
def test_operator_equals_the_specification(engine, case):
    what, make, T = case
    img = make()
    h, w = img.shape[:2]
    want = ref.tile_streams(img, T, True)
    payload, offsets = engine.deflate_encode_tiles_device(img, T, bgr=True)
    got = _split(payload, offsets)
    assert len(got) == len(want) == -(-h // T) * -(-w // T)
    for t, (g, x) in enumerate(zip(got, want)):
        assert g == x, (what, "tile", t, len(g), len(x))
    assert len(zlib.decompress(got[0])) == T * T * (3 if img.ndim == 3 else 1)
    if h * w <= 128 * 128 * 8:
        wide = np.zeros((h, w + 5) + img.shape[2:], np.uint8)
        wide[:, 3:3 + w] = img
        view = wide[:, 3:3 + w]                                 # rows strided, the first pixel at an odd byte
        assert h == 1 or not view.flags.c_contiguous
        p2, o2 = engine.deflate_encode_tiles_device(view, T, bgr=True)
        assert bytes(p2) == bytes(payload) and np.array_equal(o2, offsets), (what, "strided")
        if img.ndim == 3:
            p3, o3 = engine.deflate_encode_tiles_device(np.ascontiguousarray(img[:, :, ::-1]), T, bgr=False)
            assert bytes(p3) == bytes(payload) and np.array_equal(o3, offsets), (what, "rgb")


def test_the_boundary_image_places_every_run():
    img, placed = boundary_runs_image()
    assert placed == 3 * 9 * 2 * 3 and img.shape[0] == 128 and img.shape[1] % 128 == 0


def test_operator_refusals(engine):
    img = np.zeros((40, 40, 3), np.uint8)
    for what, kw in (("tile no multiple of 16", dict(tile=24)), ("tile 0", dict(tile=0)), ("negative tile", dict(tile=-16))):
        with pytest.raises(_lib.VfsmsError) as e:
            engine.deflate_encode_tiles_device(img, **kw)
        assert "deflate_encode_tiles_device" in str(e.value), what
        with pytest.raises(ValueError):
            ref.check_geometry(kw["tile"], 3)
    with pytest.raises(_lib.VfsmsError):
        engine.deflate_encode_tiles_device(np.zeros((40, 40, 2), np.uint8), 32)


def test_operator_capacity(engine):
    import ctypes as C
    img = _image(70, 100, 3, 5)
    payload, offsets = engine.deflate_encode_tiles_device(img, 32)
    need = len(payload)
    fn = engine.lib.vfsms_deflate_encode_tiles_device
    offs = np.zeros(offsets.size, np.uint64)

    def call(out, n_offs=offs.size):
        n = C.c_size_t()
        rc = fn(engine.ctx, img.ctypes.data_as(C.c_void_p), 70, 100, 3, img.strides[0], 1, 32, out.ctypes.data_as(C.c_void_p), C.c_size_t(out.size - 64),
                C.byref(n), offs.ctypes.data_as(C.c_void_p), n_offs)
        return rc, n.value
    small = np.full(need - 1 + 64, 0xAB, np.uint8)              # (64 guard bytes behind the capacity handed over)
    rc, n = call(small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and n == need and (small == 0xAB).all()
    exact = np.full(need + 64, 0xAB, np.uint8)
    rc, n = call(exact)
    assert rc == _lib.VFSMS_OK and n == need and bytes(exact[:need]) == bytes(payload) and (exact[need:] == 0xAB).all()
    assert np.array_equal(offs, offsets)
    assert call(exact, offs.size - 1)[0] == _lib.VFSMS_ERR_BAD_ARG


# ---- the canvas path ------------------------------------------------------------------------------------------------------------------
ROWS, COLS = 150, 201


@pytest.fixture(scope="module", params=[1, 3], ids=["gray", "colour"])
def canvas(engine, request):
    ch = request.param
    cv = _canvas(engine, ROWS, COLS, ch, 31 + ch)
    img = engine.canvas_download(cv, ROWS, COLS, ch)
    assert (img == 0).any() and img.any()
    yield cv, img, ch, {}
    engine.canvas_free(cv)


def _want(canvas, levels, T):
    _cv, img, _ch, cache = canvas
    if (levels, T) not in cache:
        cache[(levels, T)] = ref.file_tiles(img, levels, T)
    return cache[(levels, T)]


def _walk(engine, cv, ch, levels, T, band_rows):
    """-> per level {tile number: stream}, checking the index as it comes"""
    got = [dict() for _ in range(levels + 1)]
    for r0, n, payload, index in engine.canvas_encode_pyramid_tiles_deflate(cv, ROWS, COLS, ch, levels, T, band_rows):
        payload = bytes(payload)
        assert [(int(k), int(t)) for k, t, _o, _c in index] == engine.pyramid_tiles_index(ROWS, COLS, levels, T, r0, n)
        pos = 0
        for k, t, off, cnt in index.tolist():                    # file order: back to back, level after level, tiles ascending
            assert off == pos and cnt > 0 and t not in got[k]
            got[k][t] = payload[off:off + cnt]
            pos += cnt
        assert pos == len(payload)
    return got


# levels 1 .. 3 of 150 rows are 75, 38 and 19 rows: with bands of 32 rows and T = 32 level 1 gets 16 rows a band, so a tile row waits for a
# second band, levels 2 and 3 for more, and the short last band (22 rows) flushes short tile rows of every level; T = 64 with bands of 64
# likewise; levels = 0 is level 0 alone
@pytest.mark.parametrize("levels,T,band_rows", [(3, 32, 32), (3, 32, 64), (2, 64, 64), (1, 64, 128), (0, 32, 32)])
def test_canvas_bands_give_the_files_tiles(engine, canvas, levels, T, band_rows):
    cv, img, ch, _cache = canvas
    want = _want(canvas, levels, T)
    got = _walk(engine, cv, ch, levels, T, band_rows)
    for k in range(levels + 1):
        assert sorted(got[k]) == list(range(len(want[k]))), ("level", k)
        for t, x in enumerate(want[k]):
            assert got[k][t] == x, ("level", k, "tile", t, band_rows)
    if (levels, T) == (3, 32):
        assert [len(w) for w in want] == [5 * 7, 3 * 4, 2 * 2, 1]


def test_canvas_band_contract_and_the_shared_walk(engine, canvas):
    cv, img, ch, _cache = canvas
    LEVELS, TILE = 3, 32
    want = _want(canvas, LEVELS, TILE)
    out, index = np.empty(1 << 21, np.uint8), np.empty((256, 4), np.int64)

    def call(row0, nrows, levels=LEVELS, tile=TILE, handle=None, out=out, index=index):
        return engine.canvas_encode_pyramid_tiles_deflate_rows(cv if handle is None else handle, row0, nrows, levels, tile, out, index)

    def jpeg(row0, nrows):
        return engine.canvas_encode_pyramid_tiles_rows(cv, row0, nrows, LEVELS, TILE, 90, 4, out, index)
    for what, kw in (("row0 no multiple of 2^levels", dict(row0=4, nrows=32, tile=16, levels=3)), ("nrows no multiple of 2^levels", dict(row0=0, nrows=16, tile=16, levels=5)),
                     ("row0 no multiple of the tile", dict(row0=16, nrows=32)), ("nrows no multiple of the tile", dict(row0=0, nrows=48)),
                     ("levels 11", dict(row0=0, nrows=ROWS, levels=11)), ("rows beyond the canvas", dict(row0=128, nrows=32)),
                     ("tile no multiple of 16", dict(row0=0, nrows=24, tile=24)), ("unknown canvas", dict(row0=0, nrows=32, handle=cv + 12345))):
        with pytest.raises(_lib.VfsmsError) as e:
            call(**kw)
        assert "canvas_encode_pyramid_tiles_deflate" in str(e.value), (what, str(e.value))
    # a short buffer consumes nothing: the same band again succeeds, and the walk goes on from it
    rc, need, ni = call(0, 64)
    assert rc == _lib.VFSMS_OK and ni == 2 * 7 + 1 * 4
    small = np.full(need - 1, 0xAB, np.uint8)
    rc, need2, ni2 = call(0, 64, out=small)
    assert rc == _lib.VFSMS_ERR_CAPACITY and (need2, ni2) == (need, ni) and (small == 0xAB).all()
    rc, need2, ni2 = call(0, 64, index=np.empty((ni - 1, 4), np.int64))
    assert rc == _lib.VFSMS_ERR_CAPACITY and (need2, ni2) == (need, ni)
    first = bytes(out[:need])
    rc, need3, _ = call(0, 64)
    assert rc == _lib.VFSMS_OK and bytes(out[:need3]) == first
    with pytest.raises(_lib.VfsmsError) as e:                    # a band out of order: the next one is row 64
        call(32, 32)
    assert "expected row0 = 64" in str(e.value)
    with pytest.raises(_lib.VfsmsError) as e:                    # a JPEG band into the deflate walk: refused, the walk intact
        jpeg(64, 32)
    assert "deflate" in str(e.value) and "canvas_encode_pyramid_tiles" in str(e.value)
    rc, need4, ni4 = call(64, 86)                                # .. to the last row, in a band longer than the first: the pending buffer grows
    assert rc == _lib.VFSMS_OK and ni4 == 3 * 7 + 2 * 4 + 2 * 2 + 1
    tiles = {(int(k), int(t)): bytes(out[o:o + c]) for k, t, o, c in index[:ni4].tolist()}
    assert tiles[(0, 34)] == want[0][34] and tiles[(3, 0)] == want[3][0] and tiles[(1, 11)] == want[1][11] and (1, 0) not in tiles
    # the reverse: a deflate band into a JPEG walk
    rc, _need, ni = jpeg(0, 64)
    assert rc == _lib.VFSMS_OK and ni == 2 * 7 + 1 * 4
    with pytest.raises(_lib.VfsmsError) as e:
        call(64, 86)
    assert "JPEG" in str(e.value)
    rc, _need, ni = jpeg(64, 86)                                 # the JPEG walk is intact
    assert rc == _lib.VFSMS_OK and ni == 3 * 7 + 2 * 4 + 2 * 2 + 1
    rc, need5, _ = call(0, 64)                                   # row0 = 0 starts over, with either coder
    assert rc == _lib.VFSMS_OK and bytes(out[:need5]) == first


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_stitcher_writes_deflate_tiles_end_to_end(engine, tmp_path, colour):
    from PIL import Image
    from test_pyramid_host import read_tiff
    rng = np.random.default_rng(8)
    proj = tmp_path / "proj"; (proj / "1").mkdir(parents=True)
    yy, xx = np.mgrid[0:192, 0:192]
    for k in range(9):
        base = 128 + 90 * np.sin((xx + 31 * k) / 11.0) * np.cos((yy + 17 * k) / 13.0) + rng.normal(0, 5, (192, 192))
        tile = np.clip(np.stack([base, 0.8 * base + 20, 255 - base], -1) if colour else base, 0, 255).astype(np.uint8)
        Image.fromarray(tile).save(str(proj / "1" / ("t%d.png" % k)))
    old = (isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod)
    outs = {}
    try:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = colour, "fadeInAndFadeOut"
        for comp in ("deflate", "deflate-device"):
            s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.mosaicBandRows = 64
            s.outputPyramid, s.pyramidTile, s.pyramidCompression = True, 64, comp
            # a 3 x 3 serpentine arrangement with overlaps and holes: the same offsets for both runs
            offsets = iter([[6, 160], [-4, 165], [158, 5], [3, -162], [-5, -160], [161, -3], [4, 163], [-2, 158]])
            out = tmp_path / ("o_" + comp)
            s.imageSetStitchWithMutiple(str(proj), str(out) + os.sep, 1, lambda images: (True, next(offsets)), fileExtension="png", outputfileExtension="tif")
            assert os.listdir(str(out)) == ["stitching_result_1.tif"]
            outs[comp] = str(out / "stitching_result_1.tif")
    finally:
        isa.Stitcher.isColorMode, isa.Stitcher.fuseMethod = old
    host = read_tiff(outs["deflate"])
    mosaic = host[0]["image"]
    mosaic = np.ascontiguousarray(mosaic[:, :, ::-1]) if colour else mosaic            # B G R, as the canvas held it
    assert min(mosaic.shape[:2]) > 400 and (mosaic == 0).any()
    K = isa.io.default_levels(mosaic.shape[0], mosaic.shape[1], 64)
    assert K >= 3 and len(host) == K + 1
    pages = check_file(outs["deflate-device"], mosaic, K, 64, big=False)        # the parser: tags 259 = 8 and 317 = 2, every tile the specification's
    check_pillow_reads(outs["deflate-device"], mosaic, K)
    for mine, pg in zip(pages, host):                                            # the pages of the "deflate" run of the same mosaic, padding included
        assert np.array_equal(mine, pg["padded"])
