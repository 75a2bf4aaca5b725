"""The four write-out routes of a canvas share more than their band contract (csrc/canvas_band.h): the two encode routes share the canvas's
encoder scratch, all of them the reader of the sticky geometry flag, and the tile route keeps rows between its calls.  So the routes are
taken in turn on ONE canvas and must give what each gives alone, and a canvas with a degenerate fuse must be refused by every one of them,
the tile route without consuming a row."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import canvas_cases as cc                 # noqa: E402
import tiff_jpeg_ref as ref               # noqa: E402
from test_canvas_paths_gpu import _upload   # noqa: E402
from test_pyramid_gpu import _canvas      # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402

pytestmark = pytest.mark.gpu

ROWS, COLS, TILE, LEVELS, Q, R = 150, 200, 32, 3, 90, 4      # the canvas of tests/test_tiff_jpeg_gpu.py
_want = {}


def _file_tiles(img, ch):
    """the specification's tiles of the canvas of `ch` channels (both tests build the same one), computed once"""
    if ch not in _want:
        _want[ch] = (img.copy(), ref.file_tiles(img, LEVELS, TILE, Q, R))
    assert np.array_equal(_want[ch][0], img)
    return _want[ch][1]


def _tile_band(eng, cv, r0, n, levels=LEVELS, tile=TILE, rows=ROWS, cols=COLS):
    """one band of the tile route -> {(level, tile number): stream}"""
    out = np.empty(1 << 20, np.uint8)
    index = np.empty((len(eng.pyramid_tiles_index(rows, cols, levels, tile, r0, n)), 4), np.int64)
    rc, _need, ni = eng.canvas_encode_pyramid_tiles_rows(cv, r0, n, levels, tile, Q, R, out, index)
    assert rc == _lib.VFSMS_OK and ni == len(index)
    return {(int(k), int(t)): bytes(out[o:o + c]) for k, t, o, c in index.tolist()}


def _jpeg_rows(eng, cv, r0, n):
    out = np.empty(1 << 20, np.uint8)
    rc, need = eng.canvas_encode_jpeg_rows(cv, r0, n, Q, 1, out)
    assert rc == _lib.VFSMS_OK
    return bytes(out[:need])


def _pyramid_band(eng, cv, ch, which):
    """band number `which` of the pyramid download with bands of 64 rows and two levels -> (row0, the band's bytes, its levels' bytes)"""
    r0, band, levels = list(eng.canvas_download_pyramid_bands(cv, ROWS, COLS, ch, 2, 64))[which]
    return r0, band.tobytes(), [lv.tobytes() for lv in levels]


def _jpeg_walk(eng, cv, ch):
    return [(r0, n, bytes(p)) for r0, n, p in eng.canvas_encode_jpeg_bands(cv, ROWS, COLS, ch, Q, 1, 64)]


@pytest.mark.parametrize("ch", [1, 3], ids=["gray", "colour"])
def test_routes_taken_in_turn_on_one_canvas_give_what_each_gives_alone(engine, ch):
    fresh = isa.Engine(0)                                        # every route by itself, on an engine that did nothing else
    try:
        cv = _canvas(fresh, ROWS, COLS, ch, 21 + ch)
        img = fresh.canvas_download(cv, ROWS, COLS, ch)
        alone_rows = fresh.canvas_download_rows(cv, 32, 64, COLS, ch).tobytes()
        alone_tiles = [_tile_band(fresh, cv, r0, min(32, ROWS - r0)) for r0 in range(0, ROWS, 32)]
        alone_jpeg_rows = _jpeg_rows(fresh, cv, 64, 86)
        alone_pyramid = _pyramid_band(fresh, cv, ch, 1)
        alone_jpeg = _jpeg_walk(fresh, cv, ch)
        fresh.canvas_free(cv)
    finally:
        fresh.close()
    assert (img == 0).any() and img.any()
    cv = _canvas(engine, ROWS, COLS, ch, 21 + ch)
    try:
        assert engine.canvas_download_rows(cv, 32, 64, COLS, ch).tobytes() == alone_rows
        tiles = {}
        for b, r0 in enumerate(range(0, ROWS, 32)):
            got = _tile_band(engine, cv, r0, min(32, ROWS - r0))
            assert got == alone_tiles[b], ("tile route, band", b)
            assert not set(got) & set(tiles)
            tiles.update(got)
            # between the bands: the other encode route on the same scratch, and a pixel route on the same flag
            assert _jpeg_rows(engine, cv, 64, 86) == alone_jpeg_rows, ("jpeg rows behind tile band", b)
            assert _pyramid_band(engine, cv, ch, 1) == alone_pyramid, ("pyramid band behind tile band", b)
        assert _jpeg_walk(engine, cv, ch) == alone_jpeg
    finally:
        engine.canvas_free(cv)
    want = _file_tiles(img, ch)                                  # and the interleaved tile walk is still the specification's
    assert sorted(tiles) == [(k, t) for k in range(LEVELS + 1) for t in range(len(want[k]))]
    for (k, t), stream in tiles.items():
        assert stream == want[k][t], ("level", k, "tile", t)


@pytest.mark.parametrize("colour", [False, True], ids=["gray", "colour"])
def test_every_route_refuses_a_canvas_with_a_degenerate_fuse(engine, oracle, colour):
    e = cc.edge_verdict_only(colour)[0]
    assert cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom)[2] is not None      # the reference raises on it
    ch = 3 if colour else 1
    out, index = np.empty(1 << 20, np.uint8), np.empty((256, 4), np.int64)
    handles = _upload(engine, e.tiles)
    cv = engine.canvas_create(e.rows, e.cols, ch)
    try:
        engine.canvas_assemble_resident(cv, handles, e.geom)
        routes = (("canvas_download", lambda: engine.canvas_download(cv, e.rows, e.cols, ch)),
                  ("canvas_download_rows", lambda: engine.canvas_download_rows(cv, 0, e.rows, e.cols, ch)),
                  ("the pyramid download", lambda: engine.canvas_pyramid(cv, e.rows, e.cols, ch, 1)),
                  ("canvas_encode_jpeg_rows", lambda: engine.canvas_encode_jpeg_rows(cv, 0, e.rows, Q, 1, out)),
                  ("canvas_encode_pyramid_tiles_rows", lambda: engine.canvas_encode_pyramid_tiles_rows(cv, 0, e.rows, 1, 16, Q, 1, out, index)))
        for what, call in routes:
            with pytest.raises(isa.VfsmsError, match="degenerate"):
                call()
    finally:
        engine.canvas_free(cv)
        for h in handles:
            engine.tile_free(h)
    # the refused tile call consumed nothing: a sound canvas built afterwards on this engine walks from row 0 to the specification's tiles
    cv = _canvas(engine, ROWS, COLS, ch, 21 + ch)
    try:
        img = engine.canvas_download(cv, ROWS, COLS, ch)
        tiles = {}
        for r0 in range(0, ROWS, 64):
            tiles.update(_tile_band(engine, cv, r0, min(64, ROWS - r0)))
    finally:
        engine.canvas_free(cv)
    want = _file_tiles(img, ch)
    assert tiles == {(k, t): x for k in range(LEVELS + 1) for t, x in enumerate(want[k])}
