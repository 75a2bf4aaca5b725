"""What tests/canvas_cases.py generates, stated with the oracle alone: the conditions tests/test_canvas_reference_gpu.py relies on when it holds the
canvas kernels to the reference on these cases.  A change to a generator that empties a share (no more corner ROIs of some quadrant, every
canvas degenerate, a wanted size gone) fails here, on a machine without a GPU."""
import numpy as np
import pytest

import canvas_cases as cc
from fakes import OracleEngine


def _oracle_engine_walk(oracle, rows, cols, tiles, geom):
    """the same walk through tests/fakes.OracleEngine's canvas calls (what the GPU test compares the library with)"""
    ref = OracleEngine(oracle)
    ch = tiles[0].shape[2] if tiles[0].ndim == 3 else 1
    cv = ref.canvas_create(rows, cols, ch)
    for t, g in zip(tiles, geom):
        y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
        if mode == cc.PASTE:
            ref.canvas_paste(cv, t, y0, x0)
        else:
            ref.canvas_fuse_tile(cv, t, y0, x0, (ry0, rx0, ry1, rx1), dx, dy)
    return ref.canvas_download(cv, rows, cols, ch)


@pytest.mark.parametrize("colour", [False, True])
def test_random_canvases_hold_the_shares_the_gpu_test_relies_on(oracle, colour):
    cases = cc.random_cases(colour)
    assert len(cases) == 40
    degenerate = fused = strips = offgrid = black = saturated = 0
    quadrant = [0, 0, 0, 0]
    for n, (rows, cols, tiles, geom) in enumerate(cases):
        assert all(t.dtype == np.uint8 and t.shape[2:] == ((3,) if colour else ()) for t in tiles)
        assert geom.shape == (len(tiles), 9) and geom.dtype == np.int32
        want, infos, stop = cc.reference_fade_walk(oracle, rows, cols, tiles, geom)
        degenerate += stop is not None
        fused += int(np.count_nonzero(geom[:, 8] != cc.PASTE))
        black += any(np.count_nonzero(t == 0) > 0.2 * t.size for t in tiles)
        saturated += any(np.count_nonzero(t == 255) > 0.2 * t.size for t in tiles)
        for g, info in zip(geom, infos):
            if info is None:
                continue
            if info[0] == 0:
                strips += 1
            else:
                quadrant[info[1]] += 1
            offgrid += int((g[3] - g[1]) % 4 != 0)
        k = len(tiles) if stop is None else stop          # the module's walk and the OracleEngine's are the same walk
        assert np.array_equal(want, _oracle_engine_walk(oracle, rows, cols, tiles[:k], geom[:k])), n
    print("seed %d colour %s: %d degenerate canvases, %d fused tiles, %d strips, corner tiles per quadrant %s, %d ROI left edges off the quad grid, "
          "%d canvases with black and %d with saturated tiles" % (cc.RANDOM_SEEDS[colour], colour, degenerate, fused, strips, quadrant, offgrid, black, saturated))
    assert 1 <= degenerate <= 10          # at most a quarter; at least one, so that the refusal and the tiles in front of it are checked
    assert fused >= 100
    assert strips >= 40
    assert min(quadrant) >= 4, quadrant
    assert offgrid >= 30
    assert black >= 8 and saturated >= 8


def test_the_gray_seed_is_the_existing_random_placements_test_generator():
    """draw for draw the canvases of test_random_placements_fused_from_the_rectangle_list_equal_the_statistics_path (first canvas restated here)"""
    rng = np.random.default_rng(20190158)
    rows, cols = int(rng.integers(500, 900)), int(rng.integers(500, 900))
    ntile = int(rng.integers(3, 8))
    th, tw = int(rng.integers(90, 320)), int(rng.integers(90, 320))
    y0, x0 = int(rng.integers(0, rows - th)), int(rng.integers(0, cols - tw))
    t = rng.integers(0, 256, (th, tw), dtype=np.uint8)
    t[rng.random((th, tw)) < 0.3] = 0
    r, c, tiles, geom = next(iter(cc.random_canvases(20190158, 1, False)))
    assert (r, c, len(tiles)) == (rows, cols, ntile) and tuple(geom[0]) == (y0, x0, 0, 0, 0, 0, 0, 0, cc.PASTE) and np.array_equal(tiles[0], t)


@pytest.mark.parametrize("colour", [False, True])
def test_edge_canvases_walk_and_cover_every_listed_boundary(oracle, colour):
    cases = cc.edge_canvases(colour)
    widths, heights, tile_widths, pairs, lo_hi, offset_x0 = set(), set(), set(), set(), set(), set()
    border = set()
    for e in cases:
        assert 2 <= len(e.tiles) <= 3 and e.rows * e.cols <= 1500000, e.name
        assert all(t.shape[2:] == ((3,) if colour else ()) for t in e.tiles)
        want, infos, stop = cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom)
        assert stop is None, (e.name, stop)
        assert np.array_equal(want, _oracle_engine_walk(oracle, e.rows, e.cols, e.tiles, e.geom)), e.name
        for t, g, info in zip(e.tiles, e.geom, infos):
            if info is None:
                continue
            y0, x0, ry0, rx0, ry1, rx1 = [int(v) for v in g[:6]]
            r, c = ry1 - ry0, rx1 - rx0
            widths.add(c); heights.add(r)
            pairs.add((cc.layout_of(c), "strip" if info[0] == 0 else info[1]))
            if x0 % 4:
                tile_widths.add(t.shape[1])
                offset_x0.add(x0 % 4)
            lo_hi.add(((rx0 - x0) % 4, (rx1 - x0) % 4))
            if ry0 == 0 and rx0 == 0 and ry1 == e.rows and rx1 == e.cols:
                border.add("strip" if info[0] == 0 else "corner")
    assert set(cc.ROI_WIDTHS) <= widths, set(cc.ROI_WIDTHS) - widths
    assert set(cc.ROI_HEIGHTS) <= heights, set(cc.ROI_HEIGHTS) - heights
    assert set(cc.TILE_WIDTHS) <= tile_widths, tile_widths                       # each on a tile column offset x0 with x0 % 4 != 0
    assert offset_x0 == {1, 2, 3}
    want_pairs = {(layout, kind) for layout in (1, 2, 4) for kind in ("strip", 0, 1, 2, 3)}
    assert want_pairs <= pairs, want_pairs - pairs
    assert {lo for lo, hi in lo_hi} >= {1, 2, 3} and {hi for lo, hi in lo_hi} >= {1, 2, 3}
    assert {(1, 2), (2, 3), (3, 1)} <= lo_hi
    assert border == {"strip", "corner"}
    print("edge canvases colour %s: %d walked, %d verdict only" % (colour, len(cases), len(cc.edge_verdict_only(colour))))


@pytest.mark.parametrize("colour", [False, True])
def test_verdict_only_canvases_are_those_the_reference_raises_on(oracle, colour):
    cases = cc.edge_verdict_only(colour)
    assert len(cases) >= 2
    for e in cases:
        _want, _infos, stop = cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom)
        assert stop == len(e.tiles) - 1, (e.name, stop)
        # and so does the trigonometric operator, which takes its corner geometry from the same getWeightsMatrix
        assert len(e.tiles) == 2
        g = e.geom[1]
        y0, x0 = [int(v) for v in e.geom[0][:2]]
        cv = np.zeros((e.rows, e.cols) + e.tiles[0].shape[2:], np.int64) - 1
        cv[y0:y0 + e.tiles[0].shape[0], x0:x0 + e.tiles[0].shape[1]] = e.tiles[0]
        A = cv[g[2]:g[4], g[3]:g[5]]
        with pytest.raises(IndexError):
            OracleEngine(oracle).fuse_trig_i64(A, np.zeros_like(A), int(g[6]), int(g[7]))
