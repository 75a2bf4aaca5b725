"""fuseMethod "optimalSeamLine" on the device against tests/seam_ref.py, exactly: the int64 operator's bytes AND its seam on the fade
fixtures, on random regions, at the widths where the register path changes shape and at production sizes; the device canvas (host tiles,
resident tiles, one-call assembly, Stitcher) against the reference's int64 / -1 canvas walk with the numpy seam."""
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd.synthetic import SyntheticGrid

import seam_ref as SR

pytestmark = pytest.mark.gpu

BLENDS = ("none", "multiBandBlending")


def _check_operator(engine, oracle, A, B, dx, dy, blend, levels, tag):
    """bytes and seam equal the reference's; where the fade's geometry is refused the operator fails like the fade -> False"""
    try:
        want, wseam = SR.seam_fuse(A, B, dx, dy, blend, levels, oracle.corner_ramps, return_seam=True)
    except IndexError:
        with pytest.raises(isa.VfsmsError):
            engine.fuse_seam_i64(A, B, dx, dy, blend=blend, levels=levels)
        return False
    got, seam = engine.fuse_seam_i64(A, B, dx, dy, blend=blend, levels=levels, return_seam=True)
    assert seam.dtype == np.int32 and seam.shape == wseam.shape, tag
    if not np.array_equal(seam, wseam):
        d = np.flatnonzero(seam != wseam)
        raise AssertionError("%s: %d seam entries differ, first at %d: %d vs %d" % (tag, len(d), d[0], seam[d[0]], wseam[d[0]]))
    assert got.dtype == np.uint8 and got.shape == want.shape, tag
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError("%s: %d bytes differ, first at %s: %d vs %d" % (tag, len(d), d[0].tolist(), got[tuple(d[0])], want[tuple(d[0])]))
    return True


def test_seam_operator_on_the_fade_fixtures(engine, oracle, golden_dir):
    """all fade fixtures (gray and colour, both strip orientations, the four corner cases), both blends; the fade's info comes back"""
    g = np.load(os.path.join(golden_dir, "fuse_cases.npz"))
    n_ok = 0
    for i, (dx, dy, _c) in enumerate(g["meta"]):
        A, B = g["f%d_A" % i], g["f%d_B" % i]
        for blend in BLENDS:
            for levels in ((4, 1) if i % 7 == 0 and blend != "none" else (4,)):
                ok = _check_operator(engine, oracle, A, B, int(dx), int(dy), blend, levels, "fixture %d, %s, N = %d" % (i, blend, levels))
                n_ok += ok
        if ok:
            _, info = engine.fuse_seam_i64(A, B, dx, dy, return_info=True)
            _, finfo = engine.fuse_fade_i64(A, B, dx, dy, return_info=True)
            assert info.tolist() == finfo.tolist(), i
    assert n_ok > 400, n_ok


def _random_region(rng, r, c, ch, hole, levels=256):
    shape = (r, c) if ch == 1 else (r, c, ch)
    A = rng.integers(0, levels, shape).astype(np.int64); B = rng.integers(0, levels, shape).astype(np.int64)
    cut = {"tl": (slice(0, r // 2 + 1), slice(0, c // 2 + 2)), "tr": (slice(0, r // 2 + 1), slice(c // 3, c)),
           "bl": (slice(r // 3, r), slice(0, c // 2 + 2)), "br": (slice(r // 3, r), slice(c // 4, c))}.get(hole)
    if cut is not None:
        A[cut] = -1
    if hole == "dots":
        A[rng.random((r, c)) < 0.05] = -1
        B[rng.random((r, c)) < 0.05] = -1
    return A, B


def test_seam_operator_on_random_regions(engine, oracle):
    """gray and colour, scattered holes and the four L-shaped corner patterns, tall and wide strips, both signs of dx / dy, few grey
    levels (ties everywhere) and many"""
    rng = np.random.default_rng(31)
    n = {True: 0, False: 0}
    for (r, c) in ((1, 1), (1, 7), (7, 1), (2, 3), (5, 7), (33, 300), (300, 41), (129, 130), (409, 600), (700, 300)):
        for ch in (1, 3):
            for hole in (None, "dots", "tl", "tr", "bl", "br"):
                for dx, dy in ((5, 7), (-5, -7)):
                    for levels in (3, 256):
                        A, B = _random_region(rng, r, c, ch, hole, levels)
                        blend = BLENDS[(n[True] + n[False]) % 2] if r * c > 50000 else None
                        for b in (BLENDS if blend is None else (blend,)):
                            n[_check_operator(engine, oracle, A, B, dx, dy, b, 3, "%dx%dx%d %s (%d, %d) L%d %s" % (r, c, ch, hole, dx, dy, levels, b))] += 1
    assert n[True] > 500, n


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65, 255, 256, 257, 513])
def test_seam_widths_around_the_lane_boundaries(engine, oracle, width):
    """the forward pass picks its positions per lane from the seam's own width (4 up to 256 positions, 8 up to 512, ...): 1, 2 and 63 / 64 /
    65 leave lanes idle or fill them exactly, 255 / 256 / 257 and 513 cross the switches to the next register shape"""
    rng = np.random.default_rng(width)
    for (r, c) in ((width + 70, width), (width, width + 70)):          # a vertical seam over `width` columns, a horizontal one over `width` rows
        for ch, levels in ((1, 4), (3, 256)):
            A, B = _random_region(rng, r, c, ch, "dots", levels)
            for dx, dy in ((2, 3), (-2, -3)):
                assert _check_operator(engine, oracle, A, B, dx, dy, "none", 4, "%dx%dx%d (%d, %d)" % (r, c, ch, dx, dy))


def test_seam_wider_than_the_register_path(engine, oracle):
    """4097 positions: one above the 64 lanes x 64 registers of k_seam_dp -> k_seam_dp_wide"""
    rng = np.random.default_rng(41)
    A, B = _random_region(rng, 4100, 4097, 1, None, 6)
    A[5, 9] = -1
    assert _check_operator(engine, oracle, A, B, 3, 4, "none", 4, "4100x4097")


def test_wide_kernel_on_varied_regions(engine, oracle, monkeypatch):
    """the same kernel forced on small regions (VFSMS_SEAM_REG_CAP=0), corner mode included"""
    monkeypatch.setenv("VFSMS_SEAM_REG_CAP", "0")
    rng = np.random.default_rng(43)
    for (r, c) in ((1, 1), (5, 7), (300, 41), (64, 1500), (409, 600)):
        for hole in (None, "dots", "tl", "br"):
            A, B = _random_region(rng, r, c, 1 + 2 * (r % 2), hole, 5)
            _check_operator(engine, oracle, A, B, 5, -7, "none", 4, "wide %dx%d %s" % (r, c, hole))
    monkeypatch.setenv("VFSMS_SEAM_REG_CAP", "8")                       # positions per lane capped at 8: 600 positions go wide, 41 stay in registers
    A, B = _random_region(rng, 700, 600, 1, None, 5)
    assert _check_operator(engine, oracle, A, B, 1, 1, "none", 4, "cap 8")


@pytest.mark.parametrize("shape", [(2048, 410), (4096, 819), (410, 2048)])
def test_seam_at_production_strip_sizes(engine, oracle, shape):
    rng = np.random.default_rng(shape[0])
    A, B = _random_region(rng, shape[0], shape[1], 1, "dots", 256)
    for blend in BLENDS:
        assert _check_operator(engine, oracle, A, B, 4, 9, blend, 4, "%dx%d %s" % (shape + (blend,)))
    A, B = _random_region(rng, shape[0], shape[1], 3, None, 8)
    assert _check_operator(engine, oracle, A, B, -4, -9, "none", 4, "%dx%dx3" % shape)


def test_seam_identical_inputs_and_repeatability(engine):
    rng = np.random.default_rng(5)
    for shape in ((37, 53), (64, 48, 3), (300, 41)):
        A = rng.integers(0, 256, shape).astype(np.int64)
        for blend in BLENDS:
            assert np.array_equal(engine.fuse_seam_i64(A, A.copy(), 3, 4, blend=blend), A.astype(np.uint8)), (shape, blend)
    A, B = _random_region(rng, 900, 333, 3, "dots", 7)
    first = engine.fuse_seam_i64(A, B, 1, 2, return_seam=True)
    second = engine.fuse_seam_i64(A, B, 1, 2, return_seam=True)
    assert np.array_equal(first[0], second[0]) and np.array_equal(first[1], second[1])


# ---- the device canvas --------------------------------------------------------------------------------------------------------------------
def _color(t):
    t = t.astype(np.int32)
    return np.ascontiguousarray(np.stack([t, 255 - t, (t * 7 + 31) & 255], -1).astype(np.uint8))


def _host_walk(oracle, files, offs, color, blend, levels):
    """getStitchByOffset through the reference's int64 / -1 canvas walk (_stitchWithHostFuse -> fuseImage), fuse = the numpy seam"""
    from fakes import OracleEngine

    class RefEngine(OracleEngine):
        def fuse_seam_i64(self, A, B, dx, dy, blend="none", levels=4, return_info=False, return_seam=False):
            assert not return_info and not return_seam
            return SR.seam_fuse(A, B, dx, dy, blend, levels, oracle.corner_ramps)

    s = isa.Stitcher(); s._engine = RefEngine(oracle); s.isPrintLog = False; s.isColorMode = color
    s.fuseMethod = "optimalSeamLine"; s.seamLineBlend = blend; s.multiBandLevels = levels
    return s.getStitchByOffset(files, [list(o) for o in offs])


def _device_paths(engine, files, offs, color, blend, levels):
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
                         min(ox + t.shape[1], rangeY[i - 1][1]), origin[i][0], origin[i][1], 7))
    outs = []
    handles = [engine.tile_upload_color(t) if color else engine.tile_upload(t) for t in tiles]
    try:
        for way in ("host", "resident", "assemble"):
            cv = engine.canvas_create(rows, cols, ch)
            try:
                engine.canvas_set_seam_blend(cv, blend)
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
                        engine.canvas_fuse_tile(cv, tiles[i], g[0], g[1], g[2:6], g[6], g[7], method=3)
                    else:
                        engine.canvas_fuse_tile_resident(cv, handles[i], g[0], g[1], g[2:6], g[6], g[7], method=3)
                outs.append(engine.canvas_download(cv, rows, cols, ch))
            finally:
                engine.canvas_free(cv)
    finally:
        for h in handles:
            engine.tile_free(h)
    return outs


def _mosaic_case(engine, oracle, tmp_path, rows, cols, tile, color, blend="none", levels=4, tag="sm"):
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
        want = _host_walk(oracle, files, offs, color, blend, levels)
        got = _device_paths(engine, files, offs, color, blend, levels)
        s = isa.Stitcher(); s._engine = engine; s.isPrintLog = False; s.isColorMode = color
        s.fuseMethod = "optimalSeamLine"; s.seamLineBlend = blend; s.multiBandLevels = levels
        got.append(s.getStitchByOffset(files, [list(o) for o in offs]))
    finally:
        isa.Stitcher.isColorMode = old
    for way, out in zip(("host tiles", "resident tiles", "one-call assembly", "Stitcher"), got):
        assert out.shape == want.shape, (way, out.shape, want.shape)
        assert np.array_equal(out, want), (way, blend, int(np.count_nonzero(out != want)))
    return want


@pytest.mark.parametrize("color", [False, True])
def test_seam_canvas_3x3_serpentine(engine, oracle, tmp_path, color):
    _mosaic_case(engine, oracle, tmp_path, 3, 3, 640, color)


@pytest.mark.parametrize("color", [False, True])
def test_seam_canvas_2x2_production_tiles(engine, oracle, tmp_path, color):
    _mosaic_case(engine, oracle, tmp_path, 2, 2, 2048, color)


def test_seam_blend_and_levels_reach_the_canvas(engine, oracle, tmp_path):
    """each setting gives the reference's bytes for that setting (asserted inside), and the settings differ from each other"""
    a = _mosaic_case(engine, oracle, tmp_path, 2, 2, 640, False, "none", 4, tag="bn")
    b = _mosaic_case(engine, oracle, tmp_path, 2, 2, 640, False, "multiBandBlending", 2, tag="b2")
    c = _mosaic_case(engine, oracle, tmp_path, 2, 2, 640, False, "multiBandBlending", 4, tag="b4")
    assert not np.array_equal(a, b) and not np.array_equal(b, c)


def test_seam_canvas_without_the_host_strip_shortcut(engine, oracle, tmp_path, monkeypatch):
    """VFSMS_FUSE_ANALYTIC=0: the geometry of every ROI comes from the statistics kernel's records on the device"""
    monkeypatch.setenv("VFSMS_FUSE_ANALYTIC", "0")
    _mosaic_case(engine, oracle, tmp_path, 2, 3, 320, False, tag="na")


def test_seam_refuses_what_the_fade_refuses(engine, oracle):
    A = np.full((2, 2), -1, np.int64); A[0, 0] = 9
    B = np.full((2, 2), 50, np.int64)
    with pytest.raises(IndexError):
        SR.seam_fuse(A, B, 1, 1, "none", 4, oracle.corner_ramps)
    with pytest.raises(isa.VfsmsError):
        engine.fuse_fade_i64(A, B, 1, 1)
    for blend in BLENDS:
        with pytest.raises(isa.VfsmsError):
            engine.fuse_seam_i64(A, B, 1, 1, blend=blend)
    with pytest.raises(ValueError):
        engine.fuse_seam_i64(A, B, 1, 1, blend="average")
    with pytest.raises(isa.VfsmsError):
        engine.fuse_seam_i64(B, B, 1, 1, blend="multiBandBlending", levels=9)
    t0 = np.full((1, 1), 9, np.uint8); t1 = np.full((2, 2), 50, np.uint8)
    h0, h1 = engine.tile_upload(t0), engine.tile_upload(t1)
    cv = engine.canvas_create(2, 2, 1)
    try:
        engine.canvas_assemble_resident(cv, [h0, h1], np.array([(0, 0, 0, 0, 0, 0, 0, 0, -1), (0, 0, 0, 0, 2, 2, 1, 1, 7)], np.int32))
        with pytest.raises(isa.VfsmsError):
            engine.canvas_download(cv, 2, 2, 1)
        with pytest.raises(isa.VfsmsError):
            engine.canvas_fuse_tile_resident(cv, h1, 0, 0, (0, 0, 2, 2), 1, 1, method=4)
        with pytest.raises(isa.VfsmsError):
            engine.canvas_assemble_resident(cv, [h0], np.array([(0, 0, 0, 0, 0, 0, 0, 0, 8)], np.int32))
    finally:
        engine.canvas_free(cv)
        engine.tile_free(h0); engine.tile_free(h1)
