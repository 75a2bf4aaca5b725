"""CPU tests of Method.lensCorrection: the integer resampling of tests/lens_ref.py against a float64 evaluation of the same map, the
block lattice and the block field against verify_ref.py, the radial fit of imagestitch_amd/lens.py against the specification's and
against the injected distortion of tests/lens_cases.py, and Stitcher._correctLens on a CPU double of its own."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import lens
from imagestitch_amd.adjust import neighbour_edges
from imagestitch_amd.synthetic import texture_window

import lens_cases as LC
import lens_ref as LR
import verify_ref


# ---- the resampling ----------------------------------------------------------------------------------------------------------------------
def _smooth(shape, seed=3):
    t = 128.0 + 45.0 * texture_window(50, 70, shape[0], shape[1], seed=seed).astype(np.float64)
    if len(shape) == 3:
        t = np.stack([t, 0.8 * t + 20.0, 255.0 - t], axis=-1)
    return np.clip(np.rint(t), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("interp", [0, 1])
def test_zero_coefficients_are_the_identity(interp):
    rng = np.random.default_rng(1)
    for shape in ((1, 1), (1, 9), (5, 7), (33, 40, 3), (70, 57)):
        img = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(LR.remap(img, 0, 0, None, None, interp), img)
        h, w = shape[:2]
        assert np.array_equal(LR.remap(img, 0, 0, (h - 1) - (h - 1) // 2, (w - 1) + (w - 1) // 2, interp), img)


def test_catmull_rom_weights_sum_to_one():
    W = LR.cubic_weights(np.arange(256))
    assert W.shape == (256, 4) and W.dtype == np.int64 and (W.sum(axis=1) == 1 << 25).all()
    assert W[0].tolist() == [0, 1 << 25, 0, 0]
    f = np.arange(256) / 256.0                               # the float Catmull-Rom kernel (a = -1/2), exactly representable here
    F = np.stack([(-f ** 3 + 2 * f ** 2 - f) / 2, (3 * f ** 3 - 5 * f ** 2 + 2) / 2, (-3 * f ** 3 + 4 * f ** 2 + f) / 2, (f ** 3 - f ** 2) / 2], axis=1)
    assert np.array_equal(W.astype(np.float64) / (1 << 25), F)
    assert np.abs(W).sum(axis=1).max() <= 1.27 * (1 << 25)     # the accumulator bound of the specification: 255 (1.27 2^25)^2 < 2^59


def _remap_f64(img, a1, a2, cy, cx, interp):
    """the same map and the same weights in float64, without any quantisation of positions or weights"""
    h, w = img.shape[:2]
    p = img.astype(np.float64).reshape(h, w, -1)
    y, x = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    D2 = max(1.0, ((h - 1) ** 2 + (w - 1) ** 2) / 4.0)
    rho = ((y - cy) ** 2 + (x - cx) ** 2) / D2
    f = a1 * rho + a2 * rho * rho
    sy, sx = y + (y - cy) * f, x + (x - cx) * f
    iy, ix = np.floor(sy), np.floor(sx)
    fy, fx = (sy - iy)[..., None], (sx - ix)[..., None]
    iy, ix = iy.astype(np.int64), ix.astype(np.int64)

    def at(yy, xx):
        return p[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)]

    def cr(t):
        return [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2]
    if interp == 0:
        out = (1 - fy) * ((1 - fx) * at(iy, ix) + fx * at(iy, ix + 1)) + fy * ((1 - fx) * at(iy + 1, ix) + fx * at(iy + 1, ix + 1))
    else:
        wy, wx = cr(fy), cr(fx)
        out = sum(wy[t] * sum(wx[u] * at(iy - 1 + t, ix - 1 + u) for u in range(4)) for t in range(4))
    return np.clip(out, 0.0, 255.0).reshape(img.shape)


@pytest.mark.parametrize("interp", [0, 1])
@pytest.mark.parametrize("shape,a1,a2,dc", [((96, 128), 0.03, 0.0027, (0, 0)), ((96, 128), -0.25, 0.125, (0, 0)), ((70, 57, 3), 0.25, -0.125, (17, -14)),
                                            ((33, 130), -0.02, 0.0012, (-8, 32))])
def test_integer_remap_within_one_level_of_float64(shape, a1, a2, dc, interp):
    """positions are quantised to 1 / 256 px and the sums are exact: on a smooth scene (a few grey levels per pixel) the integer output
    stays within 1 grey level of the float64 evaluation"""
    img = _smooth(shape)
    h, w = shape[:2]
    cy2, cx2 = h - 1 + 2 * dc[0], w - 1 + 2 * dc[1]
    q1, q2 = LR.coefficients_q30(a1, a2)
    got = LR.remap(img, q1, q2, cy2, cx2, interp).astype(np.float64)
    want = _remap_f64(img, a1, a2, cy2 / 2.0, cx2 / 2.0, interp)
    assert np.abs(got - want).max() <= 1.0
    assert not np.array_equal(got, img)


def test_the_map_is_refused_outside_its_limits():
    assert LR.check_map(96, 128, 1 << 28, -(1 << 28), 95 + 47, 127 - 63, 1)
    assert not LR.check_map(96, 128, (1 << 28) + 1, 0, 95, 127, 1) and not LR.check_map(96, 128, 0, 0, 95 + 48, 127, 0)
    assert not LR.check_map(96, 128, 0, 0, 95, 127 - 64, 0) and not LR.check_map(96, 128, 0, 0, 95, 127, 2)
    assert not LR.check_map(16385, 8, 0, 0, 16384, 7, 0)
    assert lens.coefficients_q30(0.25, -0.25) == (1 << 28, -(1 << 28)) == LR.coefficients_q30(0.25, -0.25)
    with pytest.raises(ValueError):
        lens.coefficients_q30(0.2500001, 0.0)
    assert lens.centre_half_pixels(None) == (-1, -1) and lens.centre_half_pixels((47.5, 63.25)) == (95, 127)


# ---- the block lattice and the block field -----------------------------------------------------------------------------------------------
def _brute_lattice(h, w, dx, dy, block, R):
    """the B rows / columns that lie R inside the overlap on both sides (r - R and r + R are rows of B whose partner is a row of A),
    counted one by one"""
    rows = [r for r in range(h) if all(0 <= r + i < h and 0 <= r + i + dx < h for i in (-R, R))]
    cols = [c for c in range(w) if all(0 <= c + j < w and 0 <= c + j + dy < w for j in (-R, R))]
    nby, nbx = len(rows) // block, len(cols) // block
    return (rows[0] if rows else None, cols[0] if cols else None, nby, nbx) if nby and nbx else (None, None, 0, 0)


def test_lattice_agrees_with_a_brute_count():
    offsets = [(dx, dy) for dx in (-95, -72, -40, -3, 0, 5, 41, 70, 96, 200) for dy in (-128, -100, -33, 0, 2, 64, 99, 127)]
    for block, R in ((16, 1), (16, 3), (16, 16), (8, 2), (64, 2)):
        counts = []
        for dx, dy in offsets:
            want = _brute_lattice(96, 128, dx, dy, block, R)
            for got in (lens.block_lattice((96, 128), dx, dy, block, R), LR.block_lattice(96, 128, dx, dy, block, R)):
                assert got[2:] == want[2:] and (want[2] == 0 or got[:2] == want[:2]), (block, R, dx, dy, got, want)
            counts.append(want[2] * want[3])
        assert 0 in counts and max(counts) > (1 if block < 64 else 0)
        first = lens.block_first((96, 128), offsets, block, R)
        assert np.array_equal(first, np.concatenate([[0], np.cumsum(counts)])) and np.array_equal(first, LR.block_first((96, 128), offsets, block, R))


@pytest.mark.parametrize("color", [False, True])
def test_block_field_is_verify_ref_block_by_block(color):
    tiles, offs = LC.grid("s+", color)
    A, B = LR.luma(tiles[0]), LR.luma(tiles[1])
    dx, dy = offs[0][0] + 1, offs[0][1] - 2
    block, R = 16, 2
    best4, surface = LR.block_ncc(tiles[0], tiles[1], dx, dy, block, R)
    r0, c0, nby, nbx = LR.block_lattice(A.shape[0], A.shape[1], dx, dy, block, R)
    assert nby * nbx == len(best4) >= 8
    for k in range(len(best4)):
        y, x = r0 + (k // nbx) * block, c0 + (k % nbx) * block
        b = B[y:y + block, x:x + block]
        keys = []
        for i in range(-R, R + 1):
            for j in range(-R, R + 1):
                a = A[y + dx + i:y + dx + i + block, x + dy + j:x + dy + j + block]
                sc = verify_ref.score(verify_ref.sums(a, b, 0, 0), 0)
                assert surface[k, i + R, j + R] == verify_ref.fixed(sc)
                keys.append((-sc, i * i + j * j, i, j))
        top = min(keys)
        assert best4[k].tolist() == [top[2], top[3], verify_ref.fixed(-top[0]), block * block]
    assert (best4[:, 2] > 0.9 * verify_ref.FIXED_ONE).all() and (best4[:, 1] == 2).all()                    # the perturbed column offset is found
    flat = np.full_like(A, 77)
    fb, fs = LR.block_ncc(flat, B, dx, dy, block, R)
    assert (fb == [0, 0, 0, block * block]).all() and not fs.any()


# ---- the fit -----------------------------------------------------------------------------------------------------------------------------
def _field(name, color):
    tiles, offs = LC.grid(name, color)
    shapes = [t.shape for t in tiles]
    edges = neighbour_edges(shapes, np.asarray(offs), LC.RADIUS)
    eoff = [(e[2], e[3]) for e in edges.tolist()]
    first, best4, surface = LR.block_ncc_batch(tiles, [tuple(e) for e in edges.tolist()], LC.BLOCK, LC.RADIUS)
    return shapes[0][:2], edges, eoff, first, best4, surface


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("name", sorted(LC.CASES))
def test_fit_equals_the_specification(name, color):
    shape, edges, eoff, first, best4, surface = _field(name, color)
    assert np.array_equal(first, lens.block_first(shape, eoff, LC.BLOCK, LC.RADIUS)) and len(edges) == 4
    got = lens.fit_radial(shape, eoff, best4, surface, LC.BLOCK, LC.RADIUS, LC.THRESHOLD, min_blocks=8)
    want = LR.fit_radial(shape, eoff, best4, surface, LC.BLOCK, LC.RADIUS, LC.THRESHOLD)
    assert (got["measured"], got["trimmed"]) == (want["measured"], want["trimmed"]) and got["blocks"] == len(best4) and got["edges"] == 4
    for key in ("b1", "a1", "a2", "corner_px", "spread_before"):
        assert abs(got[key] - want[key]) <= 1e-9 * max(1.0, abs(want[key])), key
    assert got["a1"] == -got["b1"] and got["a2"] == 3.0 * got["b1"] * got["b1"]
    off_centre = lens.fit_radial(shape, eoff, best4, surface, LC.BLOCK, LC.RADIUS, LC.THRESHOLD, min_blocks=8, centre=(60.0, 85.5))
    want = LR.fit_radial(shape, eoff, best4, surface, LC.BLOCK, LC.RADIUS, LC.THRESHOLD, centre=(60.0, 85.5))
    assert abs(off_centre["b1"] - want["b1"]) <= 1e-9


@pytest.mark.parametrize("color", [False, True])
@pytest.mark.parametrize("name", ["s+", "s-", "m+", "m-"])
def test_fit_recovers_the_injected_distortion(name, color):
    """the whole chain of lens.correct on the specification's engine: the fitted corner coefficient a1 + a2 within 15 % of the injected
    one, and the spread of the displacement about its edge's mean at most half of what it was.  (The integer reference gave
    a1 + a2 = 0.0321 / -0.0284 for +-0.03, 0.0195 / -0.0192 for +-0.02, and spreads of 0.42 .. 0.46 -> 0.05 .. 0.07 px.)"""
    tiles, offs = LC.grid(name, color)
    eng = LC.SpecEngine(tiles)
    out, pair, rep = lens.correct(eng, [0, 1, 2, 3], [t.shape for t in tiles], offs, block=LC.BLOCK, radius=LC.RADIUS, threshold=LC.THRESHOLD,
                                  min_blocks=8)
    a1 = LC.CASES[name][2]
    print(name, color, pair, rep)
    assert rep["apply"] and pair == (rep["a1"], rep["a2"]) and eng.calls == ["block_ncc_batch", "lens_apply", "block_ncc_batch"]
    assert abs((pair[0] + pair[1]) / a1 - 1.0) <= 0.15
    assert rep["spread_after"] <= rep["spread_before"] / 2
    assert out == [list(o) for o in offs] and rep["moved"] == 0          # the offsets were the true ones
    assert not any(np.array_equal(eng.tiles[k], tiles[k]) for k in range(4))


@pytest.mark.parametrize("color", [False, True])
def test_undistorted_tiles_are_left_alone(color):
    tiles, offs = LC.grid("s0", color)
    eng = LC.SpecEngine(tiles)
    out, pair, rep = lens.correct(eng, [0, 1, 2, 3], [t.shape for t in tiles], offs, block=LC.BLOCK, radius=LC.RADIUS, min_blocks=8)
    assert pair is None and not rep["apply"] and "lensMinShift" in rep["reason"] and abs(rep["corner_px"]) < 0.25 and abs(rep["a1"]) < 0.002
    assert rep["spread_before"] < 0.1 and rep["spread_after"] is None
    assert eng.calls == ["block_ncc_batch"] and all(np.array_equal(eng.tiles[k], tiles[k]) for k in range(4)) and out == [list(o) for o in offs]
    eng = LC.SpecEngine(tiles)                               # the default lensMinBlocks: these grids have 46 blocks at most
    _out, pair, rep = lens.correct(eng, [0, 1, 2, 3], [t.shape for t in tiles], offs, block=LC.BLOCK, radius=LC.RADIUS, min_blocks=64)
    assert pair is None and "lensMinBlocks" in rep["reason"] and eng.calls == ["block_ncc_batch"]


def test_options_are_judged_first():
    for kw in (dict(mode="auto"), dict(block=12), dict(block=136), dict(radius=0), dict(radius=17), dict(interpolation="lanczos"),
               dict(mode="given"), dict(mode="given", coefficients=(0.3, 0.0))):
        args = dict(mode="estimate", block=64, radius=8, interpolation="cubic")
        args.update(kw)
        with pytest.raises(ValueError):
            lens.check_options(**args)
    lens.check_options("given", 64, 8, "bilinear", (0.01, 0.0003))
    with pytest.raises(ValueError):
        lens.correct(LC.SpecEngine([]), [0, 1], [(8, 8)], [[0, 4]])


# ---- the Stitcher --------------------------------------------------------------------------------------------------------------------------
class HookEngine(LC.SpecEngine):
    """the specification's engine with what getStitchByOffset needs to reach its hooks on resident tiles"""

    def tile_free(self, handle):
        self.calls.append("tile_free")


class BareEngine:
    """an engine without the lens calls"""

    def tile_free(self, handle):
        pass


class _Reached(Exception):
    pass


def _stitcher(engine, **settings):
    s = isa.Stitcher(); s._engine = engine; s.isColorMode = False; s.fuseMethod = "fadeInAndFadeOut"
    msgs = []
    s.printAndWrite = lambda c, msgs=msgs: msgs.append(c)
    for k, v in settings.items():
        setattr(s, k, v)
    return s, msgs


def _run_to_layout(s, tiles, offsets):
    """getStitchByOffset on resident tiles up to _layout -> (the order of the hooks, the offsets the mosaic would be laid out by)"""
    files = ["t%d.png" % k for k in range(len(tiles))]
    s._resident = {f: (k, t.shape) for k, (f, t) in enumerate(zip(files, tiles))}
    order, seen = [], {}
    for name in ("_correctShading", "_correctLens", "_compensateExposure"):
        real = getattr(s, name)
        setattr(s, name, lambda *a, _n=name, _r=real: (order.append(_n), _r(*a) if _n == "_correctLens" else None)[1])

    def layout(shapes, originOffsetList):
        seen["offsets"] = [list(o) for o in originOffsetList]
        raise _Reached()
    s._layout = layout
    with pytest.raises(_Reached):
        s.getStitchByOffset(files, [list(o) for o in offsets])
    return order, seen["offsets"]


def test_stitcher_hook_order_offsets_and_coefficients():
    tiles, true = LC.grid("s+")
    settings = dict(lensBlock=LC.BLOCK, lensRadius=LC.RADIUS, lensMinBlocks=8)
    moved = [[true[0][0] + 1, true[0][1] - 2], list(true[1]), [true[2][0] - 1, true[2][1] + 1]]
    eng = HookEngine(tiles)
    s, msgs = _stitcher(eng, lensCorrection="estimate", shadingCorrection="estimate", exposureCompensation="gain", **settings)
    assert s.lensCoefficients is None
    order, laid = _run_to_layout(s, tiles, moved)
    assert order == ["_correctShading", "_correctLens", "_compensateExposure"]
    assert eng.calls[:3] == ["block_ncc_batch", "lens_apply", "block_ncc_batch"]
    # every path pair moved by the lower median of its measured (i, j): back onto the true offsets
    assert laid == [[0, 0]] + [list(o) for o in true] and s.lensReport["moved"] == 2
    # ... which is what the specification's chain gives from the same inputs
    edges = neighbour_edges([t.shape for t in tiles], np.asarray(moved), LC.RADIUS)
    fixed, want, _rep = LR.chain(tiles, edges.tolist(), moved, LC.BLOCK, LC.RADIUS, 0.5, 8, 0.25, 1, lens.fit_radial)
    assert laid[1:] == want and all(np.array_equal(eng.tiles[k], fixed[k]) for k in range(4))
    pair, rep = s.lensCoefficients, s.lensReport
    assert pair == (rep["a1"], rep["a2"]) and abs((pair[0] + pair[1]) / 0.03 - 1.0) <= 0.15
    assert msgs == ["  lens correction: a1 %.6f, a2 %.6f, %.3f px at the corner, %.3f -> %.3f px spread over 4 edges, 2 offsets moved" %
                    (pair[0], pair[1], rep["corner_px"], rep["spread_before"], rep["spread_after"])]
    # "given" with the pair left behind: the same tiles and offsets, no fit
    eng2 = HookEngine(tiles)
    s2, _ = _stitcher(eng2, lensCorrection="given", lensCoefficients=pair, **settings)
    order, laid2 = _run_to_layout(s2, tiles, moved)
    assert order == ["_correctLens"] and eng2.calls[:2] == ["lens_apply", "block_ncc_batch"] and laid2 == laid
    assert all(np.array_equal(eng2.tiles[k], eng.tiles[k]) for k in range(4)) and s2.lensCoefficients == pair
    # "none": the hook is never entered
    s3, msgs3 = _stitcher(HookEngine(tiles))
    order, laid3 = _run_to_layout(s3, tiles, moved)
    assert order == [] and laid3 == [[0, 0]] + moved and msgs3 == []


def test_stitcher_skips_and_says_why():
    tiles, true = LC.grid("s0")
    eng = HookEngine(tiles)
    s, msgs = _stitcher(eng, lensCorrection="estimate", lensBlock=LC.BLOCK, lensRadius=LC.RADIUS, lensMinBlocks=8)
    _order, laid = _run_to_layout(s, tiles, true)
    assert laid == [[0, 0]] + [list(o) for o in true] and s.lensCoefficients is None and eng.calls[0] == "block_ncc_batch" and "lens_apply" not in eng.calls
    assert len(msgs) == 1 and msgs[0].startswith("  lens correction skipped: a corner shift of")


def test_refusals_through_the_stitcher():
    tiles, true = LC.grid("s0")
    for engine, setting, error in ((BareEngine(), "estimate", NotImplementedError), (BareEngine(), "auto", ValueError),
                                   (HookEngine(tiles), "Estimate", ValueError)):
        s, _ = _stitcher(engine, lensCorrection=setting)
        with pytest.raises(error):
            _run_to_layout_raises(s, tiles, true)
    s, _ = _stitcher(HookEngine(tiles), lensCorrection="estimate")       # the calls, but no resident tiles
    with pytest.raises(NotImplementedError):
        s._correctLens(None, [t.shape for t in tiles], [[0, 0]] + true)
    s, _ = _stitcher(HookEngine(tiles), lensCorrection="estimate")       # tiles of several shapes
    with pytest.raises(ValueError, match="tiles of one shape"):
        s._correctLens([0, 1, 2, 3], [(128, 160), (128, 160), (128, 161), (128, 160)], [[0, 0]] + true)
    s, _ = _stitcher(HookEngine(tiles), lensCorrection="given")          # "given" without coefficients
    with pytest.raises(ValueError, match="lensCoefficients"):
        s._correctLens([0, 1, 2, 3], [t.shape for t in tiles], [[0, 0]] + true)


def _run_to_layout_raises(s, tiles, offsets):
    files = ["t%d.png" % k for k in range(len(tiles))]
    s._resident = {f: (k, t.shape) for k, (f, t) in enumerate(zip(files, tiles))}
    s._layout = lambda *a: (_ for _ in ()).throw(AssertionError("the layout was reached"))
    s.getStitchByOffset(files, [list(o) for o in offsets])


def test_public_surface():
    m = isa.Method()
    assert (m.lensCorrection, m.lensCoefficients, m.lensCentre, m.lensBlock, m.lensRadius, m.lensThreshold, m.lensMinBlocks, m.lensMinShift,
            m.lensInterpolation) == ("none", None, None, 64, 8, 0.5, 32, 0.25, "cubic")
    assert "undistort" in isa.__all__ and isa.undistort is lens.undistort
    for name in ("block_ncc_batch", "lens_apply", "lens_remap"):
        assert callable(getattr(isa.Engine, name))

    class Remap:
        def lens_remap(self, img, a1, a2, centre2, interpolation):
            return ("remap", a1, a2, centre2, interpolation)
    assert isa.undistort(np.zeros((4, 4), np.uint8), (0.25, -0.125), centre=(1.5, 2.0), interpolation="bilinear", engine=Remap()) == \
        ("remap", 1 << 28, -(1 << 27), (3, 4), "bilinear")
