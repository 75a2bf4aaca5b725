"""fuseMethod "multiBandBlending" on the device against tests/multiband_ref.py, byte for byte: the int64 operator on the fade fixtures
and on random regions, and the device canvas (host tiles, resident tiles, one-call assembly) against the reference's int64 / -1
canvas walk with the numpy blend."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

import multiband_ref as MB

pytestmark = pytest.mark.gpu


def _ref(oracle, A, B, dx, dy, levels):
    """the reference bytes, or None where the fade's geometry is refused (the reference's getWeightsMatrix raises)"""
    try:
        return MB.multiband(A, B, dx, dy, levels, oracle.corner_ramps)
    except IndexError:
        return None


def _check_operator(engine, oracle, A, B, dx, dy, levels, tag):
    want = _ref(oracle, A, B, dx, dy, levels)
    if want is None:
        with pytest.raises(isa.VfsmsError):
            engine.fuse_multiband_i64(A, B, dx, dy, levels=levels)
        return False
    got = engine.fuse_multiband_i64(A, B, dx, dy, levels=levels)
    assert got.dtype == np.uint8 and got.shape == want.shape, tag
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d bytes differ, first at %s: %d vs %d" % (tag, len(d), d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))
    return True


def test_multiband_operator_on_the_fade_fixtures(engine, oracle, golden_dir):
    """all 249 fade fixtures (gray and colour, both strip orientations, the four corner cases): equal bytes, the fade's error where the
    fade refuses the geometry; the fade's info comes back unchanged"""
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    n_ok = n_err = 0
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        A, B = g["f%d_A" % i], g["f%d_B" % i]
        for levels in ((4, 1, 2) if i % 7 == 0 else (4,)):
            if _check_operator(engine, oracle, A, B, int(dx), int(dy), levels, "fixture %d, N = %d" % (i, levels)):
                n_ok += 1
            else:
                n_err += 1
        if _ref(oracle, A, B, int(dx), int(dy), 4) is not None:
            _, info = engine.fuse_multiband_i64(A, B, dx, dy, return_info=True)
            _, finfo = engine.fuse_fade_i64(A, B, dx, dy, return_info=True)
            assert info.tolist() == finfo.tolist(), i
    assert n_ok > 200, (n_ok, n_err)


def _random_region(rng, r, c, ch, hole):
    shape = (r, c) if ch == 1 else (r, c, ch)
    A = rng.integers(0, 256, shape).astype(np.int64); B = rng.integers(0, 256, shape).astype(np.int64)
    if hole == "tl":
        A[:r // 2 + 37, :] = -1
        keep = np.arange(r)[:, None] < r - 90
        cols = A[:, :c // 2 + 11]
        A[:, :c // 2 + 11] = np.where(keep if ch == 1 else keep[:, :, None], -1, cols)
    if hole == "br":
        A[r // 3:, c // 4:] = -1
    return A, B


def test_multiband_operator_on_random_regions(engine, oracle):
    """sizes from 1 x 1 to whole tiles, holes top-left / bottom-right, both signs of dx / dy, N = 1..6, gray and colour"""
    rng = np.random.default_rng(11)
    k = 0
    for (r, c) in ((1, 1), (1, 7), (2, 3), (5, 7), (33, 1025), (409, 2048), (2048, 300), (1200, 1500)):
        small = r * c < 50000
        for ch in (1, 3):
            for hole in (None, "tl", "br"):
                for dx, dy in ((5, 7), (-5, -7)):
                    A, B = _random_region(rng, r, c, ch, hole)
                    for levels in (range(1, 7) if small else (1 + k % 6,)):
                        _check_operator(engine, oracle, A, B, dx, dy, levels, "%dx%dx%d %s (%d, %d) N = %d" % (r, c, ch, hole, dx, dy, levels))
                    k += 1


def test_multiband_identical_inputs_return_the_input(engine):
    rng = np.random.default_rng(5)
    for shape in ((37, 53), (64, 48, 3), (300, 41)):
        A = rng.integers(0, 256, shape).astype(np.int64)
        for levels in range(1, 7):
            assert np.array_equal(engine.fuse_multiband_i64(A, A.copy(), 3, 4, levels=levels), A.astype(np.uint8)), (shape, levels)


def _color(t):
    t = t.astype(np.int32)
    return np.ascontiguousarray(np.stack([t, 255 - t, (t * 7 + 31) & 255], -1).astype(np.uint8))


def _host_walk(oracle, files, offs, color, levels):
    """getStitchByOffset through the reference's int64 / -1 canvas walk (_stitchWithHostFuse -> fuseImage), blend = the numpy reference"""
    from fakes import OracleEngine

    class RefEngine(OracleEngine):
        def fuse_multiband_i64(self, A, B, dx, dy, levels=4, return_info=False):
            assert not return_info
            return MB.multiband(A, B, dx, dy, levels, oracle.corner_ramps)

    s = isa.Stitcher(); s._engine = RefEngine(oracle); s.isPrintLog = False; s.isColorMode = color
    s.fuseMethod = "multiBandBlending"; s.multiBandLevels = levels
    return s.getStitchByOffset(files, [list(o) for o in offs])


def _device_paths(engine, files, offs, color, levels):
    """the same mosaic on the device canvas three ways: host tiles per call, resident tiles per call, one assemble call"""
    from imagestitch_amd.stitcher import _imread
    tiles = [np.ascontiguousarray(_imread(f, color)) for f in files]
    shapes = [t.shape for t in tiles]
    origin = [[0, 0]] + [list(o) for o in offs]
    offsetList, rangeX, rangeY, rows, cols = isa.Stitcher._layout(shapes, origin)
    ch = 3 if color else 1
    geom = []
    for i, t in enumerate(tiles):
        oy, ox = offsetList[i]
        if i == 0:
            geom.append((oy, ox, 0, 0, 0, 0, 0, 0, -1))
        else:
            geom.append((oy, ox, max(oy, rangeX[i - 1][0]), max(ox, rangeY[i - 1][0]), min(oy + t.shape[0], rangeX[i - 1][1]),
                         min(ox + t.shape[1], rangeY[i - 1][1]), origin[i][0], origin[i][1], 6))
    outs = []
    handles = [engine.tile_upload_color(t) if color else engine.tile_upload(t) for t in tiles]
    try:
        for way in ("host", "resident", "assemble"):
            cv = engine.canvas_create(rows, cols, ch)
            try:
                engine.canvas_set_multiband_levels(cv, levels)
                if way == "assemble":
                    engine.canvas_assemble_resident(cv, handles, np.array(geom, np.int32))
                for i, g in enumerate(geom if way != "assemble" else ()):
                    if g[8] < 0:
                        if way == "host":
                            engine.canvas_paste(cv, tiles[i], g[0], g[1])
                        else:
                            engine.canvas_paste_tile(cv, handles[i], g[0], g[1])
                    elif way == "host":
                        engine.canvas_fuse_tile(cv, tiles[i], g[0], g[1], g[2:6], g[6], g[7], method=2)
                    else:
                        engine.canvas_fuse_tile_resident(cv, handles[i], g[0], g[1], g[2:6], g[6], g[7], method=2)
                outs.append(engine.canvas_download(cv, rows, cols, ch))
            finally:
                engine.canvas_free(cv)
    finally:
        for h in handles:
            engine.tile_free(h)
    return outs


def _mosaic_case(engine, oracle, tmp_path, rows, cols, tile, color, levels=4, tag="mb"):
    from test_host_logic import _write_tiles
    g = SyntheticGrid(rows, cols, tile, blobs=tile <= 2048)
    tiles = g.tiles(threads=4)
    if color:
        tiles = [_color(t) for t in tiles]
    offs = [list(map(int, o)) for o in g.true_offsets()]
    files = _write_tiles(tmp_path, tiles, "%s%d%d%d%d" % (tag, rows, cols, tile, int(color)))
    old = isa.Stitcher.isColorMode
    try:
        isa.Stitcher.isColorMode = color
        want = _host_walk(oracle, files, offs, color, levels)
        got = _device_paths(engine, files, offs, color, levels)
        s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.isColorMode = color
        s.fuseMethod = "multiBandBlending"; s.multiBandLevels = levels
        got.append(s.getStitchByOffset(files, [list(o) for o in offs]))
    finally:
        isa.Stitcher.isColorMode = old
    for way, out in zip(("host tiles", "resident tiles", "one-call assembly", "Stitcher"), got):
        assert out.shape == want.shape, (way, out.shape, want.shape)
        assert np.array_equal(out, want), (way, int(np.count_nonzero(out != want)))
    return want


@pytest.mark.parametrize("color", [False, True])
def test_multiband_canvas_3x3_serpentine(engine, oracle, tmp_path, color):
    _mosaic_case(engine, oracle, tmp_path, 3, 3, 640, color)


@pytest.mark.parametrize("color", [False, True])
def test_multiband_canvas_2x2_production_tiles(engine, oracle, tmp_path, color):
    _mosaic_case(engine, oracle, tmp_path, 2, 2, 2048, color)


def test_multiband_canvas_config4_tile_size(engine, oracle, tmp_path):
    """4096 x 4096 tiles (BASELINE configs[4]), gray"""
    _mosaic_case(engine, oracle, tmp_path, 2, 2, 4096, False)


def test_multiband_levels_reach_the_canvas(engine, oracle, tmp_path):
    a = _mosaic_case(engine, oracle, tmp_path, 2, 2, 640, False, levels=2, tag="l2")
    b = _mosaic_case(engine, oracle, tmp_path, 2, 2, 640, False, levels=4, tag="l4")
    assert not np.array_equal(a, b)


def test_multiband_refuses_what_the_fade_refuses(engine, oracle):
    """a corner geometry where the reference's getWeightsMatrix raises: the operator fails like the fade, and on the canvas the one-call
    assembly enqueues and the download reports the latched error"""
    A = np.full((2, 2), -1, np.int64); A[0, 0] = 9
    B = np.full((2, 2), 50, np.int64)
    assert _ref(oracle, A, B, 1, 1, 4) is None
    with pytest.raises(isa.VfsmsError):
        engine.fuse_fade_i64(A, B, 1, 1)
    with pytest.raises(isa.VfsmsError):
        engine.fuse_multiband_i64(A, B, 1, 1)
    t0 = np.full((1, 1), 9, np.uint8); t1 = np.full((2, 2), 50, np.uint8)
    h0, h1 = engine.tile_upload(t0), engine.tile_upload(t1)
    cv = engine.canvas_create(2, 2, 1)
    try:
        engine.canvas_assemble_resident(cv, [h0, h1], np.array([(0, 0, 0, 0, 0, 0, 0, 0, -1), (0, 0, 0, 0, 2, 2, 1, 1, 6)], np.int32))
        with pytest.raises(isa.VfsmsError):
            engine.canvas_download(cv, 2, 2, 1)
    finally:
        engine.canvas_free(cv)
        engine.tile_free(h0); engine.tile_free(h1)
