"""The canvas kernels of csrc/fuse_kernels.hip (k_fuse_apply fade and trigonometric, k_fuse_simple, k_fuse_stats_weights, k_fuse_counts_pick) and
the host geometry beside them (corner_picks, canvas_valid_area) against the reference walk, on the irregular layouts of tests/canvas_cases.py:
random placements (all four corner quadrants, ROIs off the lane-quad grid, sub-rectangle ROIs, black and saturated pixels, gray and colour) and
the edge list (ROI sizes around the wave-layout switch, one workgroup's columns, FUSE_SB and the lane quad; tile widths with a second column
block; ROIs on the canvas border).  Public Engine methods only; the reference is the oracle's fuseByFadeInAndFadeOut walk, the numpy
restatement of fuseByTrigonometric in tests/fakes.py, and the numpy walk of average / maximum / minimum.  Every test runs with
VFSMS_FUSE_ANALYTIC unset (strips and corners from the host's rectangle list) and "0" (the statistics kernel for every tile).
tests/test_canvas_cases_host.py states what the cases contain."""
import numpy as np
import pytest

import imagestitch_amd as isa
import canvas_cases as cc
from fakes import OracleEngine
from test_canvas_paths_gpu import _Analytic, _upload

FLAGS = [None, "0"]
_refs = {}


def _cases(which, colour):
    return cc.random_cases(colour) if which == "random" else [tuple(e[1:]) for e in cc.edge_canvases(colour)]


def _fade_refs(oracle, which, colour):
    """(bytes, infos, first tile the reference raises on or None) per case, computed once per process"""
    key = ("fade", which, colour)
    if key not in _refs:
        _refs[key] = [cc.reference_fade_walk(oracle, *case) for case in _cases(which, colour)]
    return _refs[key]


def _simple_refs(which, colour, mode):
    key = (mode, which, colour)
    if key not in _refs:
        _refs[key] = [cc.reference_simple_walk(tiles, geom, rows, cols, mode) for rows, cols, tiles, geom in _cases(which, colour)]
    return _refs[key]


def _channels(tiles):
    return tiles[0].shape[2] if tiles[0].ndim == 3 else 1


def _free(engine, handles):
    for h in handles:
        engine.tile_free(h)


def _assemble(engine, handles, rows, cols, ch, geom):
    """the one-call walk -> the canvas bytes, or "degenerate" when the download refuses"""
    cv = engine.canvas_create(rows, cols, ch)
    try:
        engine.canvas_assemble_resident(cv, handles[:len(geom)], geom)
        try:
            return engine.canvas_download(cv, rows, cols, ch)
        except isa.VfsmsError as e:
            assert "degenerate" in str(e), e
            return "degenerate"
    finally:
        engine.canvas_free(cv)


def _equal(got, want):
    return not isinstance(got, str) and got.shape == want.shape and np.array_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("which", ["random", "edge"])
def test_fade_canvas_bytes_equal_the_oracle_walk(engine, oracle, which, colour, flag):
    """canvas_assemble_resident + canvas_download == the oracle walk, byte for byte.  Where the reference raises at tile k the library refuses
    with its "degenerate" error, and the canvas of the tiles in front of k still equals the oracle's."""
    refs = _fade_refs(oracle, which, colour)
    refused = 0
    with _Analytic(flag):
        for n, ((rows, cols, tiles, geom), (want, _infos, stop)) in enumerate(zip(_cases(which, colour), refs)):
            handles = _upload(engine, tiles)
            try:
                got = _assemble(engine, handles, rows, cols, _channels(tiles), geom)
                if stop is None:
                    assert _equal(got, want), (which, colour, flag, n)
                else:
                    refused += 1
                    assert isinstance(got, str) and got == "degenerate", (which, colour, flag, n, stop)
                    assert _equal(_assemble(engine, handles, rows, cols, _channels(tiles), geom[:stop]), want), (which, colour, flag, n, stop)
            finally:
                _free(engine, handles)
        if which == "edge":
            for e in cc.edge_verdict_only(colour):
                handles = _upload(engine, e.tiles)
                try:
                    got = _assemble(engine, handles, e.rows, e.cols, _channels(e.tiles), e.geom)
                    assert isinstance(got, str) and got == "degenerate", (e.name, colour, flag)
                finally:
                    _free(engine, handles)
    assert refused == sum(r[2] is not None for r in refs) and (which == "edge") == (refused == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("colour", [False, True])
def test_fade_info_rows_equal_the_oracle_on_the_edge_list(engine, oracle, colour, flag):
    """the per-tile resident call: (mode, quadrant, rowIndex, colIndex) as the oracle reports them, and the same bytes as the one-call walk"""
    refs = _fade_refs(oracle, "edge", colour)
    with _Analytic(flag):
        for e, (want, infos, _stop) in zip(cc.edge_canvases(colour) + cc.edge_verdict_only(colour), refs + [(None, None, None)] * 99):
            ch = _channels(e.tiles)
            handles = _upload(engine, e.tiles)
            cv = engine.canvas_create(e.rows, e.cols, ch)
            try:
                for k, (h, g) in enumerate(zip(handles, e.geom)):
                    y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
                    if mode == cc.PASTE:
                        engine.canvas_paste_tile(cv, h, y0, x0)
                    elif infos is None and k == len(handles) - 1:                  # verdict only: the reference raises on the last tile
                        with pytest.raises(isa.VfsmsError, match="degenerate"):
                            engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True)
                    else:
                        info = engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True)
                        assert tuple(int(v) for v in info) == infos[k], (e.name, colour, flag, k, info, infos[k])
                if infos is not None:
                    assert np.array_equal(engine.canvas_download(cv, e.rows, e.cols, ch), want), (e.name, colour, flag)
            finally:
                engine.canvas_free(cv)
                _free(engine, handles)


def _expected_trig_tile(ref, prev, placed, tile, g):
    """-> (the canvas the reference gives after this tile from the canvas `prev` with the placed-mask `placed`, the ROI as slices or None)"""
    y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
    want = prev.copy()
    want[y0:y0 + tile.shape[0], x0:x0 + tile.shape[1]] = tile
    if mode == cc.PASTE or ry1 <= ry0 or rx1 <= rx0:
        return want, None
    A = prev[ry0:ry1, rx0:rx1].astype(np.int64)
    A[~placed[ry0:ry1, rx0:rx1]] = -1
    B = tile[ry0 - y0:ry1 - y0, rx0 - x0:rx1 - x0].astype(np.int64)
    want[ry0:ry1, rx0:rx1] = ref.fuse_trig_i64(A, B, dx, dy)                           # IndexError where getWeightsMatrix raises
    return want, (slice(ry0, ry1), slice(rx0, rx1))


@pytest.mark.gpu
@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("which", ["random", "edge"])
def test_trigonometric_canvas_tiles_equal_the_reference_formula(engine, oracle, which, colour, flag):
    """fuseByTrigonometric on the canvas path, tile by tile: after every canvas_fuse_tile_resident(method=1) the downloaded canvas against the
    numpy restatement of ImageFusion.py:246-293 applied to the library's OWN previous canvas (-1 where the rectangle list has placed nothing),
    so that a one-level difference never feeds the next tile's input.  Tolerance as include/vfsms.h and
    test_fuse_trigonometric_operator_vs_reference_formula state it: at most one grey level, on fewer than 0.1 % of the compared ROI bytes over
    the whole test; everything outside the ROI exact.  Where the reference's getWeightsMatrix raises, the library refuses and the canvas ends."""
    ref = OracleEngine(oracle)
    nbytes = ndiff = refused = 0
    with _Analytic(flag):
        cases = _cases(which, colour) + ([tuple(e[1:]) for e in cc.edge_verdict_only(colour)] if which == "edge" else [])
        for n, (rows, cols, tiles, geom) in enumerate(cases):
            ch = _channels(tiles)
            handles = _upload(engine, tiles)
            cv = engine.canvas_create(rows, cols, ch)
            try:
                prev = np.zeros((rows, cols) + tiles[0].shape[2:], np.uint8)
                placed = np.zeros((rows, cols), bool)
                for k, (h, t, g) in enumerate(zip(handles, tiles, geom)):
                    y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
                    try:
                        want, roi = _expected_trig_tile(ref, prev, placed, t, g)
                    except IndexError:
                        refused += 1
                        with pytest.raises(isa.VfsmsError, match="degenerate"):
                            engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True, method=1)
                        break
                    if mode == cc.PASTE:
                        engine.canvas_paste_tile(cv, h, y0, x0)
                    else:
                        engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True, method=1)
                    got = engine.canvas_download(cv, rows, cols, ch)
                    if roi is not None:
                        d = np.abs(got[roi].astype(np.int16) - want[roi].astype(np.int16))
                        assert d.max() <= 1, (which, colour, flag, n, k, int(d.max()))
                        nbytes += d.size; ndiff += int(np.count_nonzero(d))
                        want[roi] = got[roi]
                    assert np.array_equal(got, want), (which, colour, flag, n, k)                 # outside the ROI: exact
                    prev = got
                    placed[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = True
            finally:
                engine.canvas_free(cv)
                _free(engine, handles)
    print("trigonometric %s colour=%s analytic=%s: %d of %d ROI bytes one level off (%.5f %%), %d canvases ended by a refusal"
          % (which, colour, flag, ndiff, nbytes, 100.0 * ndiff / nbytes, refused))
    assert nbytes > 100000 and (refused == len(cc.edge_verdict_only(colour)) if which == "edge" else refused >= 1)
    assert ndiff < 1e-3 * nbytes, (ndiff, nbytes)


@pytest.mark.gpu
@pytest.mark.parametrize("flag", FLAGS)
@pytest.mark.parametrize("colour", [False, True])
@pytest.mark.parametrize("mode", [cc.AVERAGE, cc.MAXIMUM, cc.MINIMUM])
def test_simple_blends_equal_the_reference_walk_on_irregular_layouts(engine, mode, colour, flag):
    """average / maximum / minimum (k_fuse_simple) against the numpy walk with fuseImage's fill-in (Stitcher.py:498-504; the black pixels of
    the tiles are what exercise it): the one-call walk on the random canvases and the edge list, and on the edge list the per-tile calls with
    a resident tile and with a host tile."""
    with _Analytic(flag):
        for which in ("random", "edge"):
            for n, ((rows, cols, tiles, geom0), want) in enumerate(zip(_cases(which, colour), _simple_refs(which, colour, mode))):
                ch = _channels(tiles)
                geom = cc.with_mode(geom0, mode)
                handles = _upload(engine, tiles)
                try:
                    assert _equal(_assemble(engine, handles, rows, cols, ch, geom), want), (which, mode, colour, flag, n)
                    for form in (("resident", "host") if which == "edge" else ()):
                        cv = engine.canvas_create(rows, cols, ch)
                        try:
                            for h, t, g in zip(handles, tiles, geom):
                                y0, x0, ry0, rx0, ry1, rx1 = [int(v) for v in g[:6]]
                                if g[8] == cc.PASTE:
                                    engine.canvas_paste_tile(cv, h, y0, x0) if form == "resident" else engine.canvas_paste(cv, t, y0, x0)
                                elif form == "resident":
                                    engine.canvas_blend_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), mode - cc.AVERAGE)
                                else:
                                    engine.canvas_blend_tile(cv, t, y0, x0, (ry0, rx0, ry1, rx1), mode - cc.AVERAGE)
                            assert np.array_equal(engine.canvas_download(cv, rows, cols, ch), want), (form, mode, colour, flag, n)
                        finally:
                            engine.canvas_free(cv)
                finally:
                    _free(engine, handles)
