"""2- and 4-channel images through every kernel whose entry point takes ch 1..4, each against the reference of its operation, exactly
(np.array_equal; the trigonometric fuse keeps the tolerance of test_fuse_trigonometric_operator_vs_reference_formula): the pyramid reduce, the
multiband blend, the seam, the fade / trigonometric / ramps operators, the canvas kernels, the lens resampling, the shading field and the
exposure statistics -- and the documented refusal of every entry that takes 1 or 3 channels only.  The inputs are those of
tests/channel_cases.py; tests/test_channel_counts_host.py states what they contain.  The instantiations and branches this reaches for the
first time: k_pyramid<2,128,64>, <4,64,64>, <2,16,16>, <4,16,16>; cases 2 and 4 of the multiband switches (k_mb_down, k_mb_up, k_mb_up_canvas,
k_mb_up_i64); k_lens_remap<0,2> and <0,4>; k_shade_box_h with its LDS segment exactly full; the seam's uint16 energy at its maximum of
5100; the ch != 1 branches of the fuse kernels at element counts valid * ch other than * 3."""
import ctypes as C

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import lens
from imagestitch_amd._lib import NccJob, VFSMS_ERR_BAD_ARG

import canvas_cases as cc
import channel_cases as X
import exposure_ref as ER
import lens_ref as LR
import multiband_ref as MB
import pyramid_ref as PR
import seam_ref as SR
import shading_ref as SH
from fakes import OracleEngine
from test_canvas_paths_gpu import _Analytic
from test_canvas_reference_gpu import _assemble, _equal, _expected_trig_tile
from test_lens_gpu import COEFFICIENTS, INTERP, _centres
from test_multiband_gpu import _check_operator as _check_multiband, _random_region as _mb_region
from test_pyramid_gpu import _canvas, _equal as _levels_equal
from test_seam_gpu import BLENDS, _check_operator as _check_seam
from test_shading_gpu import _free, _tile_bytes, _upload

pytestmark = pytest.mark.gpu

CH = pytest.mark.parametrize("ch", X.CHANNELS)


# ---- pyramid -------------------------------------------------------------------------------------------------------------------------------------
PYRAMIDS = {2: [(1, 1, 2), (3, 2, 2), (70, 131, 5), (130, 259, 7)],            # (130, 259): two regions of 128 px and 3, and the 16 x 16 second launch
            4: [(130, 131, 7), (66, 200, 5)]}                                  # rows always start dword-aligned: pyr_load4's sh == 0 branch only


@CH
def test_pyramid_levels_equal_the_reference(engine, ch):
    for rows, cols, levels in PYRAMIDS[ch]:
        cv = _canvas(engine, rows, cols, ch, rows + cols + ch)
        try:
            img = engine.canvas_download(cv, rows, cols, ch)
            assert img.shape == (rows, cols, ch)
            if rows > 8:
                assert (img == 0).any() and img.any()            # holes and content
            want = PR.pyramid_levels(img, levels)
            _levels_equal(engine.canvas_pyramid(cv, rows, cols, ch, levels), want, (rows, cols, ch))
        finally:
            engine.canvas_free(cv)


@CH
def test_pyramid_band_by_band(engine, ch):
    rows, cols, levels, band = {2: (130, 259, 6, 64), 4: (130, 131, 5, 64)}[ch]
    cv = _canvas(engine, rows, cols, ch, 11 + ch)
    try:
        img = engine.canvas_download(cv, rows, cols, ch)
        want = PR.pyramid_levels(img, levels)
        bands, parts = [], [[] for _ in range(levels)]
        for r0, b, lv in engine.canvas_download_pyramid_bands(cv, rows, cols, ch, levels, band):
            assert r0 == sum(x.shape[0] for x in bands) and len(lv) == levels
            bands.append(b.copy())
            for k in range(levels):
                assert lv[k].shape[0] == PR.band_of_level(r0, b.shape[0], rows, k + 1)[1]
                parts[k].append(lv[k].copy())
        assert len(bands) == 3 and np.array_equal(np.concatenate(bands, 0), img)
        _levels_equal([np.concatenate(p, 0) for p in parts], want, "bands")
    finally:
        engine.canvas_free(cv)


# ---- multiband -----------------------------------------------------------------------------------------------------------------------------------
@CH
def test_multiband_operator_equals_the_reference(engine, oracle, ch):
    rng = np.random.default_rng(11 + ch)
    n_ok = n_plain = 0
    for (r, c) in ((1, 1), (2, 3), (5, 7), (17, 67), (40, 133)):
        for hole in (None, "tl", "br"):
            for dx, dy in ((5, 7), (-5, -7)):
                A, B = _mb_region(rng, r, c, ch, hole)
                for levels in (range(1, 7) if r * c < 100 else (3, 6)):
                    n_ok += _check_multiband(engine, oracle, A, B, dx, dy, levels, "%dx%dx%d %s (%d, %d) N = %d" % (r, c, ch, hole, dx, dy, levels))
                    n_plain += hole is None
    assert n_ok >= n_plain > 40                                  # a region without a hole is a strip: the reference never refuses it
    for name, A, B, dx, dy in X.fuse_cases(ch):                  # strips of both kinds and the four corners, with empty pixels
        assert _check_multiband(engine, oracle, A, B, dx, dy, 3, name), name


@CH
def test_multiband_identical_inputs_return_the_input(engine, ch):
    rng = np.random.default_rng(5 + ch)
    for shape in ((37, 53, ch), (5, 7, ch)):
        A = rng.integers(0, 256, shape).astype(np.int64)
        for levels in range(1, 7):
            assert np.array_equal(engine.fuse_multiband_i64(A, A.copy(), 3, 4, levels=levels), A.astype(np.uint8)), (shape, levels)


@CH
def test_multiband_canvas_route_equals_the_int64_walk(engine, oracle, ch):
    """canvas_fuse_tile(method 2) tile by tile and one canvas_assemble_resident against the reference's int64 / -1 canvas walk with the numpy blend"""
    rows, cols, tiles, geom = X.multiband_layout(ch)
    for levels in (2, 4):
        want, fused = X.reference_fuse_walk(tiles, geom, rows, cols, lambda A, B, dx, dy: MB.multiband(A, B, dx, dy, levels, oracle.corner_ramps))
        assert len(fused) == 3
        handles = _upload(engine, tiles)
        try:
            for way in ("host", "assemble"):
                cv = engine.canvas_create(rows, cols, ch)
                try:
                    engine.canvas_set_multiband_levels(cv, levels)
                    if way == "assemble":
                        engine.canvas_assemble_resident(cv, handles, geom)
                    else:
                        for t, g in zip(tiles, geom):
                            if g[8] == cc.PASTE:
                                engine.canvas_paste(cv, t, g[0], g[1])
                            else:
                                engine.canvas_fuse_tile(cv, t, g[0], g[1], g[2:6], g[6], g[7], method=2)
                    got = engine.canvas_download(cv, rows, cols, ch)
                    assert np.array_equal(got, want), (way, levels, int(np.count_nonzero(got != want)))
                finally:
                    engine.canvas_free(cv)
        finally:
            _free(engine, handles)


# ---- seam ----------------------------------------------------------------------------------------------------------------------------------------
@CH
def test_seam_operator_equals_the_reference(engine, oracle, ch):
    """pixels and seam; none of the cases is refused (tests/test_channel_counts_host.py), so every check must come back True"""
    for name, A, B, dx, dy in X.seam_cases(ch):
        for blend in BLENDS:
            assert _check_seam(engine, oracle, A, B, dx, dy, blend, 3, "%s x%d %s" % (name, ch, blend)), name
    A, B = X.max_energy_region(ch)
    assert SR.energy(A, B).max() == 1275 * ch


@CH
def test_seam_refuses_a_region_too_long_for_int32_costs(engine, ch):
    r, c = X.SEAM_TOO_LONG
    A = np.zeros((r, c, ch), np.int64); B = np.ones((r, c, ch), np.int64)
    with pytest.raises(ValueError):
        SR.seam_fuse(A, B, 1, 1, corner_ramps=lambda A: None)
    with pytest.raises(isa.VfsmsError, match="too long for int32") as e:
        engine.fuse_seam_i64(A, B, 1, 1)
    assert e.value.code == VFSMS_ERR_BAD_ARG


# ---- fade, trigonometric, ramps ------------------------------------------------------------------------------------------------------------------
@CH
def test_fade_trig_and_ramps_operators_equal_the_oracle(engine, oracle, ch):
    """fade: the oracle's bytes and info, and the same info from the multiband and the seam operator.  ramps: getWeightsMatrix's factors in
    corner mode, the strip ramps of multiband_ref.fade_weights otherwise.  trigonometric: the tolerance include/vfsms.h states and
    test_fuse_trigonometric_operator_vs_reference_formula holds -- at most one grey level, on at most 0.1 % of the bytes over the test."""
    ref = OracleEngine(oracle)
    nbytes = ndiff = 0
    for name, A, B, dx, dy in X.fuse_cases(ch):
        want, winfo = oracle.fuse_fade(A, B, dx, dy, return_info=True)
        got, info = engine.fuse_fade_i64(A, B, dx, dy, return_info=True)
        assert info.tolist() == winfo.tolist(), (name, info, winfo)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (name, int(np.count_nonzero(got != want)))
        assert engine.fuse_multiband_i64(A, B, dx, dy, return_info=True)[1].tolist() == info.tolist(), name
        assert engine.fuse_seam_i64(A, B, dx, dy, return_info=True)[1].tolist() == info.tolist(), name
        (wAr, wBr, wAc, wBc), rinfo = engine.fuse_ramps_i64(A, dx, dy)
        assert rinfo[0] == winfo[0] and (not winfo[0] or rinfo.tolist() == winfo.tolist()), (name, rinfo, winfo)
        wA, wB = MB.fade_weights(A, dx, dy, oracle.corner_ramps)
        if winfo[0]:
            wr, wc, _cinfo = oracle.corner_ramps(A)
            assert np.array_equal(wBr, wr) and np.array_equal(wBc, wc), name
        else:
            assert np.array_equal(wAr[:, None] * wAc[None, :], wA), name
        assert np.array_equal(wBr[:, None] * wBc[None, :], wB), name
        try:                                                     # getWeightsMatrix forced on every case, the strips included
            wr, wc, cinfo = oracle.corner_ramps(A)
        except IndexError:
            with pytest.raises(isa.VfsmsError):
                engine.fuse_ramps_i64(A, dx, dy, force_corner=True)
        else:
            (_a, fBr, _b, fBc), finfo = engine.fuse_ramps_i64(A, dx, dy, force_corner=True)
            assert np.array_equal(fBr, wr) and np.array_equal(fBc, wc) and finfo[1:].tolist() == cinfo[1:].tolist(), name
        twant = ref.fuse_trig_i64(A, B, dx, dy)
        tgot, tinfo = engine.fuse_trig_i64(A, B, dx, dy, return_info=True)
        assert tinfo.tolist() == winfo.tolist(), name
        d = np.abs(tgot.astype(np.int16) - twant.astype(np.int16))
        assert d.max() <= 1, (name, int(d.max()))
        nbytes += d.size; ndiff += int(np.count_nonzero(d))
    print("trigonometric operator ch = %d: %d of %d bytes one level off" % (ch, ndiff, nbytes))
    assert ndiff <= 1e-3 * nbytes, (ndiff, nbytes)


# ---- the canvas kernels --------------------------------------------------------------------------------------------------------------------------
_refs = {}


def _fade_refs(oracle, ch):
    if ch not in _refs:
        _refs[ch] = [cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom) for e in X.edge_canvases(ch)]
    return _refs[ch]


@pytest.mark.parametrize("flag", [None, "0"])
@CH
def test_canvas_fade_equals_the_oracle_walk_and_its_verdicts(engine, oracle, ch, flag):
    """the one-call walk, the per-tile resident call (with the oracle's info rows) and the per-tile host call; where the reference raises,
    the library refuses with its "degenerate" error"""
    with _Analytic(flag):
        for e, (want, infos, stop) in zip(X.edge_canvases(ch), _fade_refs(oracle, ch)):
            assert stop is None
            handles = _upload(engine, e.tiles)
            try:
                assert _equal(_assemble(engine, handles, e.rows, e.cols, ch, e.geom), want), (e.name, flag)
                for form in ("resident", "host"):
                    cv = engine.canvas_create(e.rows, e.cols, ch)
                    try:
                        for k, (h, t, g) in enumerate(zip(handles, e.tiles, e.geom)):
                            y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
                            if mode == cc.PASTE:
                                engine.canvas_paste_tile(cv, h, y0, x0) if form == "resident" else engine.canvas_paste(cv, t, y0, x0)
                                continue
                            info = (engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True) if form == "resident"
                                    else engine.canvas_fuse_tile(cv, t, y0, x0, (ry0, rx0, ry1, rx1), dx, dy))
                            assert tuple(int(v) for v in info) == infos[k], (e.name, flag, form, k, info, infos[k])
                        assert np.array_equal(engine.canvas_download(cv, e.rows, e.cols, ch), want), (e.name, flag, form)
                    finally:
                        engine.canvas_free(cv)
            finally:
                _free(engine, handles)
        for e in X.edge_verdict_only(ch):
            handles = _upload(engine, e.tiles)
            try:
                got = _assemble(engine, handles, e.rows, e.cols, ch, e.geom)
                assert isinstance(got, str) and got == "degenerate", (e.name, flag)
                for method in (0, 1):
                    cv = engine.canvas_create(e.rows, e.cols, ch)
                    try:
                        engine.canvas_paste_tile(cv, handles[0], *[int(v) for v in e.geom[0][:2]])
                        y0, x0, ry0, rx0, ry1, rx1, dx, dy, _mode = [int(v) for v in e.geom[1]]
                        with pytest.raises(isa.VfsmsError, match="degenerate"):
                            engine.canvas_fuse_tile_resident(cv, handles[1], y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True, method=method)
                    finally:
                        engine.canvas_free(cv)
            finally:
                _free(engine, handles)


@pytest.mark.parametrize("flag", [None, "0"])
@CH
def test_canvas_trigonometric_tiles_equal_the_reference_formula(engine, oracle, ch, flag):
    """tile by tile against the numpy restatement applied to the library's own previous canvas, as
    test_trigonometric_canvas_tiles_equal_the_reference_formula does for 1 and 3 channels, with its tolerance: at most one grey level, on
    fewer than 0.1 % of the compared ROI bytes over the whole test; everything outside the ROI exact"""
    ref = OracleEngine(oracle)
    nbytes = ndiff = 0
    with _Analytic(flag):
        for e in X.edge_canvases(ch):
            handles = _upload(engine, e.tiles)
            cv = engine.canvas_create(e.rows, e.cols, ch)
            try:
                prev = np.zeros((e.rows, e.cols, ch), np.uint8)
                placed = np.zeros((e.rows, e.cols), bool)
                for k, (h, t, g) in enumerate(zip(handles, e.tiles, e.geom)):
                    y0, x0, ry0, rx0, ry1, rx1, dx, dy, mode = [int(v) for v in g]
                    want, roi = _expected_trig_tile(ref, prev, placed, t, g)             # (an IndexError here fails the test: none is refused)
                    if mode == cc.PASTE:
                        engine.canvas_paste_tile(cv, h, y0, x0)
                    else:
                        engine.canvas_fuse_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), dx, dy, want_info=True, method=1)
                    got = engine.canvas_download(cv, e.rows, e.cols, ch)
                    if roi is not None:
                        d = np.abs(got[roi].astype(np.int16) - want[roi].astype(np.int16))
                        assert d.max() <= 1, (e.name, flag, k, int(d.max()))
                        nbytes += d.size; ndiff += int(np.count_nonzero(d))
                        want[roi] = got[roi]
                    assert np.array_equal(got, want), (e.name, flag, k)
                    prev = got
                    placed[y0:y0 + t.shape[0], x0:x0 + t.shape[1]] = True
            finally:
                engine.canvas_free(cv)
                _free(engine, handles)
    print("trigonometric canvas ch = %d analytic = %s: %d of %d ROI bytes one level off" % (ch, flag, ndiff, nbytes))
    assert nbytes > 100000 and ndiff < 1e-3 * nbytes, (ndiff, nbytes)


@pytest.mark.parametrize("flag", [None, "0"])
@pytest.mark.parametrize("mode", [cc.AVERAGE, cc.MAXIMUM, cc.MINIMUM, cc.PASTE])
@CH
def test_canvas_simple_blends_and_paste_equal_the_reference_walk(engine, ch, mode, flag):
    """average / maximum / minimum (k_fuse_simple; the tiles' elements that are black in one channel only exercise the fill-in) and the plain
    paste: the one-call walk and the per-tile calls with a resident and with a host tile"""
    with _Analytic(flag):
        for e in X.edge_canvases(ch):
            if mode == cc.PASTE:
                geom = np.array(e.geom, np.int32)
                geom[:, 2:8] = 0; geom[:, 8] = cc.PASTE
                want = X.paste_walk(e.tiles, geom, e.rows, e.cols)
            else:
                geom = cc.with_mode(e.geom, mode)
                want = cc.reference_simple_walk(e.tiles, geom, e.rows, e.cols, mode)
            handles = _upload(engine, e.tiles)
            try:
                assert _equal(_assemble(engine, handles, e.rows, e.cols, ch, geom), want), (e.name, mode, flag)
                for form in ("resident", "host"):
                    cv = engine.canvas_create(e.rows, e.cols, ch)
                    try:
                        for h, t, g in zip(handles, e.tiles, geom):
                            y0, x0, ry0, rx0, ry1, rx1 = [int(v) for v in g[:6]]
                            if g[8] == cc.PASTE:
                                engine.canvas_paste_tile(cv, h, y0, x0) if form == "resident" else engine.canvas_paste(cv, t, y0, x0)
                            elif form == "resident":
                                engine.canvas_blend_tile_resident(cv, h, y0, x0, (ry0, rx0, ry1, rx1), mode - cc.AVERAGE)
                            else:
                                engine.canvas_blend_tile(cv, t, y0, x0, (ry0, rx0, ry1, rx1), mode - cc.AVERAGE)
                        assert np.array_equal(engine.canvas_download(cv, e.rows, e.cols, ch), want), (e.name, form, mode, flag)
                    finally:
                        engine.canvas_free(cv)
            finally:
                _free(engine, handles)


# ---- lens ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", [0, 1])
@CH
def test_lens_remap_and_apply_equal_the_reference(engine, ch, interp):
    """k_lens_remap<0, CH>, every tap clamped: host arrays (one strided view) and resident tiles, the three coefficient pairs, the default
    centre and both ends of its allowed range"""
    tiles = [X.tiles_u8(23, 1, s + (ch,))[0] for s in X.LENS_SHAPES]
    for coef in COEFFICIENTS:
        for t in tiles:
            for cy2, cx2 in _centres(t.shape):
                want = LR.remap(t, coef[0], coef[1], cy2, cx2, interp)
                got = engine.lens_remap(t, coef[0], coef[1], (cy2, cx2), INTERP[interp])
                assert got.dtype == np.uint8 and np.array_equal(got, want), (t.shape, coef, (cy2, cx2), interp, int(np.count_nonzero(got != want)))
                if coef == (0, 0):
                    assert np.array_equal(got, t)
                h = _upload(engine, [t])
                try:
                    engine.lens_apply(h, coef[0], coef[1], (cy2, cx2), INTERP[interp])
                    assert np.array_equal(_tile_bytes(engine, h[0], t.shape), want), (t.shape, coef, (cy2, cx2), interp)
                finally:
                    _free(engine, h)
        src = X.tiles_u8(6, 1, (33, 150, ch))[0][:, 7:137]
        assert not src.flags["C_CONTIGUOUS"]
        assert np.array_equal(engine.lens_remap(src, coef[0], coef[1], (-1, -1), INTERP[interp]),
                              LR.remap(np.ascontiguousarray(src), coef[0], coef[1], None, None, interp)), (coef, interp)


# ---- shading ---------------------------------------------------------------------------------------------------------------------------------------
def _check_shading(engine, tiles, R, pct=50):
    """estimate -> profile, field and gain; the apply in place; the same gain handed back through shading_from_gain"""
    wg, wq, wp = SH.estimate(tiles, pct, R)
    want = [SH.apply(t, wg) for t in tiles]
    for source in ("estimate", "from_gain"):
        handles = _upload(engine, tiles)
        try:
            f = engine.shading_estimate(handles, pct, R) if source == "estimate" else engine.shading_from_gain(wg)
            try:
                gain, q8, prof = engine.shading_download(f, with_profile=True)
                if source == "estimate":
                    assert np.array_equal(prof, wp), (R, "profile")
                    assert q8.dtype == np.uint16 and np.array_equal(q8, wq), (R, "field", int(np.count_nonzero(q8 != wq)))
                else:
                    assert not q8.any() and not prof.any()
                assert gain.dtype == np.uint16 and np.array_equal(gain, wg), (R, source, int(np.count_nonzero(gain != wg)))
                engine.shading_apply(f, handles)
            finally:
                engine.shading_free(f)
            for k, h in enumerate(handles):
                got = _tile_bytes(engine, h, tiles[k].shape)
                assert np.array_equal(got, want[k]), (R, source, k, int(np.count_nonzero(got != want[k])))
        finally:
            _free(engine, handles)


@pytest.mark.parametrize("R", X.SHADING_RADII)
@CH
def test_shading_estimate_and_apply_equal_the_reference(engine, ch, R):
    for shape in X.SHADING_SHAPES:
        tiles = [t.copy() for t in X.tiles_u8(R, 5, shape + (ch,))]
        for t in tiles[:-1]:
            t[:2] = np.minimum(t[:2], 60)                         # a dark band in the profile: gains above one, and the last tile saturates in it
        _check_shading(engine, tiles, R)


@CH
def test_shading_at_the_capacity_of_the_horizontal_segment(engine, ch):
    """R = 127 on a row of at least 1024 samples: at ch = 4 the first workgroup of k_shade_box_h stages 1024 + 2 * 127 * 4 = 2040 samples, its whole
    LDS segment (the highest index read is 2039); the second one stages the row's last samples with the halo clamped on the right"""
    shape = X.SHADING_CAPACITY[ch]
    assert X.shading_staged(shape, 127) == 1024 + 2 * 127 * ch
    _check_shading(engine, X.tiles_u8(127, 3, shape), 127, 37)


# ---- exposure --------------------------------------------------------------------------------------------------------------------------------------
@CH
def test_overlap_statistics_and_exposure_apply_equal_the_reference(engine, ch):
    tiles = X.tiles_u8(41, 3, X.EXPOSURE_SHAPE + (ch,))
    jobs = [(a, b, dx, dy) for a, b in ((0, 1), (1, 2), (2, 2)) for dx, dy in X.EXPOSURE_OFFSETS]
    handles = _upload(engine, tiles)
    try:
        for band in ((0, 255), (1, 254), (100, 140)):
            want = np.array([ER.stats(tiles[a], tiles[b], dx, dy, *band) for a, b, dx, dy in jobs], np.int64)
            assert (want[:, 0] > 0).sum() >= 20 and (want[:, 0] == 0).sum() >= 6
            got = engine.overlap_stats_batch([(handles[a], handles[b], dx, dy) for a, b, dx, dy in jobs], *band)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert np.array_equal(got, want), [(jobs[k], got[k].tolist(), want[k].tolist()) for k in bad[:5]]
        gains = [0, 4097, 65535]
        engine.exposure_apply(handles, gains)
        for k, h in enumerate(handles):
            assert np.array_equal(_tile_bytes(engine, h, tiles[k].shape), ER.apply(tiles[k], gains[k])), gains[k]
    finally:
        _free(engine, handles)


def test_overlap_statistics_refuse_a_job_of_two_and_four_channels(engine):
    t2, t4 = X.tiles_u8(3, 1, X.EXPOSURE_SHAPE + (2,))[0], X.tiles_u8(3, 1, X.EXPOSURE_SHAPE + (4,))[0]
    handles = _upload(engine, [t2, t4])
    try:
        out = np.full((2, 3), -7, np.int64)
        for pair in ((0, 1), (1, 0)):
            arr = (NccJob * 2)(NccJob(handles[0], handles[0], 0, 0), NccJob(handles[pair[0]], handles[pair[1]], 1, -1))
            assert engine.lib.vfsms_overlap_stats_batch(engine.ctx, arr, 2, 0, 255, out.ctypes.data_as(C.c_void_p)) == VFSMS_ERR_BAD_ARG
            assert (out == -7).all()
        with pytest.raises(isa.VfsmsError, match="2 and 4 channels"):
            engine.overlap_stats_batch([(handles[0], handles[1], 0, 0)], 0, 255)
        assert engine.overlap_stats_batch([(handles[1], handles[1], 0, 0)], 0, 255)[0].tolist() == list(ER.stats(t4, t4, 0, 0, 0, 255))
    finally:
        _free(engine, handles)


# ---- the entries that take 1 or 3 channels only ------------------------------------------------------------------------------------------------
@CH
def test_entries_for_one_or_three_channels_refuse_and_write_nothing(engine, ch):
    """VFSMS_ERR_BAD_ARG from the JPEG, PNG and deflate-TIFF encoders (canvas routes, and the host-array operators at ch = 4: their ch = 2
    refusals are in the encoders' own tests), vfsms_focus_scores, vfsms_focus_stack (ch = 4; ch = 2 is in tests/test_focus_gpu.py) and
    vfsms_block_ncc_batch (ch = 2; ch = 4 is in tests/test_lens_gpu.py); every output buffer keeps its sentinel"""
    rows, cols = 64, 64
    img = X.tiles_u8(9, 1, (rows, cols, ch))[0]
    out = np.full(1 << 16, 0x5A, np.uint8)
    index = np.full((64, 4), -7, np.int64)

    def refused(call):
        with pytest.raises(isa.VfsmsError, match="channels") as e:
            call()
        assert e.value.code == VFSMS_ERR_BAD_ARG, e.value
        assert (out == 0x5A).all() and (index == -7).all()

    cv = engine.canvas_create(rows, cols, ch)
    try:
        engine.canvas_paste(cv, img, 0, 0)
        refused(lambda: engine.canvas_encode_jpeg_rows(cv, 0, rows, 95, 0, out))
        refused(lambda: engine.canvas_encode_png_rows(cv, 0, rows, 16, out))
        refused(lambda: engine.canvas_encode_pyramid_tiles_rows(cv, 0, rows, 1, 32, 95, 0, out, index))
        refused(lambda: engine.canvas_encode_pyramid_tiles_deflate_rows(cv, 0, rows, 1, 32, out, index))
        assert np.array_equal(engine.canvas_download(cv, rows, cols, ch), img)       # and the canvas is as it was
    finally:
        engine.canvas_free(cv)
    if ch == 4:
        refused(lambda: engine.jpeg_encode_device(img))
        refused(lambda: engine.png_encode_device(img, 16))
        refused(lambda: engine.jpeg_encode_tiles_device(img, 32))
        refused(lambda: engine.deflate_encode_tiles_device(img, 32))
    handles = _upload(engine, [img, img.copy()])
    try:
        S = np.full(2, -5, np.int64)
        th = np.ascontiguousarray(handles, np.int64)
        assert engine.lib.vfsms_focus_scores(engine.ctx, 2, th.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p)) == VFSMS_ERR_BAD_ARG
        assert (S == -5).all()
        refused(lambda: engine.focus_scores(handles))
        if ch == 4:
            fused, D = np.full(img.shape, 7, np.uint8), np.full(img.shape[:2], 7, np.uint8)
            tile = C.c_int64(-9)
            assert engine.lib.vfsms_focus_stack(engine.ctx, 2, th.ctypes.data_as(C.c_void_p), 0, 4, 1, C.byref(tile), fused.ctypes.data_as(C.c_void_p),
                                                D.ctypes.data_as(C.c_void_p), S.ctypes.data_as(C.c_void_p)) == VFSMS_ERR_BAD_ARG
            assert tile.value == -9 and (fused == 7).all() and (D == 7).all() and (S == -5).all()
            refused(lambda: engine.focus_stack(handles))
        if ch == 2:
            first = lens.block_first((rows, cols), [(8, 3)], 16, 3)
            best = np.full((int(first[-1]), 4), -7, np.int32); surf = np.full((int(first[-1]), 7, 7), -7, np.int32)
            assert first[-1] > 0
            arr = (NccJob * 1)(NccJob(handles[0], handles[1], 8, 3))
            assert engine.lib.vfsms_block_ncc_batch(engine.ctx, arr, 1, 16, 3, np.ascontiguousarray(first, np.int64).ctypes.data_as(C.c_void_p),
                                                    best.ctypes.data_as(C.c_void_p), surf.ctypes.data_as(C.c_void_p)) == VFSMS_ERR_BAD_ARG
            assert (best == -7).all() and (surf == -7).all()
            refused(lambda: engine.block_ncc_batch([(handles[0], handles[1], 8, 3)], first, 16, 3))
        for h in handles:
            assert np.array_equal(_tile_bytes(engine, h, img.shape), img)
    finally:
        _free(engine, handles)
