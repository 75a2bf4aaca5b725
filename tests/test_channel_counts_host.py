"""What tests/channel_cases.py generates, stated with the references alone: the conditions tests/test_channel_counts_gpu.py relies on when it runs
2- and 4-channel images through the kernels.  A change that empties a share (no strip of one kind, no corner geometry, a region the reference
refuses, the max-energy region below 5100, the shading row short of its LDS segment) fails here, on a machine without a GPU -- and so does a
return of the pixel-validity rule to the reference's literal "sum != -3", which counts every empty pixel of 2 or 4 channels as valid."""
import numpy as np
import pytest

import canvas_cases as cc
import channel_cases as X
import multiband_ref as MB
import seam_ref as SR
from fakes import OracleEngine


def _kind(oracle, A):
    """1 / 2: a strip of that kind; ("corner", index): corner mode with getWeightsMatrix's quadrant.  An IndexError from the oracle propagates:
    a case the reference refuses is a failure of the case list"""
    r, c = A.shape[:2]
    if np.count_nonzero(A > -1) / A.size > 0.65:
        return 1 if c <= r else 2
    _wr, _wc, info = oracle.corner_ramps(A)
    return ("corner", int(info[1]))


@pytest.mark.parametrize("ch", X.CHANNELS)
def test_fuse_and_seam_cases_hold_both_strip_kinds_and_corners_and_none_is_refused(oracle, ch):
    ref = OracleEngine(oracle)
    for what, cases in (("fuse", X.fuse_cases(ch)), ("seam", X.seam_cases(ch))):
        kinds = set()
        for name, A, B, dx, dy in cases:
            assert A.shape == B.shape and A.shape[2] == ch and A.dtype == np.int64, name
            kind = _kind(oracle, A)
            kinds.add(kind)
            out, info = oracle.fuse_fade(A, B, dx, dy, return_info=True)          # raises where the reference refuses
            assert (info[0] == 1) == isinstance(kind, tuple) and (not info[0] or info[1] == kind[1]), (name, info, kind)
            if what == "fuse":
                assert ref.fuse_trig_i64(A, B, dx, dy).shape == A.shape
                assert MB.multiband(A, B, dx, dy, 3, oracle.corner_ramps).shape == A.shape
            else:
                for blend in ("none", "multiBandBlending"):
                    got, seam = SR.seam_fuse(A, B, dx, dy, blend, 3, oracle.corner_ramps, return_seam=True)
                    assert got.shape == A.shape and seam.shape == (A.shape[0] + A.shape[1],), name
        assert {1, 2} <= kinds and any(isinstance(k, tuple) for k in kinds), (what, ch, kinds)
        if what == "fuse":
            assert {("corner", q) for q in range(4)} <= kinds, kinds
    # empty pixels and pixels black in one channel only are there
    for name, A, B, dx, dy in X.fuse_cases(ch):
        if A.shape[0] * A.shape[1] > 7:
            assert (A == -1).all(axis=2).any(), name
            assert ((A == 0).any(axis=2) & (A > 0).any(axis=2)).any(), name
    # an element is -1 only where its whole pixel is: the representation the canvas path's validity plane stands for
    for name, A, B, dx, dy in X.fuse_cases(ch) + X.seam_cases(ch):
        for Z in (A, B):
            assert np.array_equal((Z == -1).any(axis=2), (Z == -1).all(axis=2)), name


@pytest.mark.parametrize("ch", X.CHANNELS)
def test_the_validity_rule_is_every_channel_empty_and_not_the_literal_bgr_sum(oracle, ch):
    """for every region with an all-empty pixel the old rule (sum != -3) and the rule in force give different validity planes; the rule in
    force is "not every channel is -1", in seam_ref and in the oracle's scans"""
    n = 0
    for name, A, B, dx, dy in X.fuse_cases(ch) + X.seam_cases(ch):
        empty = (A == -1).all(axis=2)
        assert np.array_equal(SR.pixel_valid(A), ~empty), name
        if empty.any():
            n += 1
            assert not np.array_equal(X.old_rule_valid(A), SR.pixel_valid(A)), name
            assert X.old_rule_valid(A)[empty].all(), name                             # the old rule counts every empty pixel as valid
    assert n >= 20, n
    # the oracle's own scan: a region whose left 20 columns are empty.  Under the old rule getWeightsMatrix found a "valid" pixel in column 0
    # (a wrong corner at ch = 2, an IndexError at ch = 4); under the rule in force the first valid column is 20, so colIndex = 19
    rng = np.random.default_rng(ch)
    A = rng.integers(1, 256, (40, 50, ch)).astype(np.int64)
    A[:, :20] = -1
    B = rng.integers(1, 256, (40, 50, ch)).astype(np.int64)
    _wr, _wc, info = oracle.corner_ramps(A)
    A3 = np.repeat(A[:, :, :1], 3, axis=2)
    _wr3, _wc3, info3 = oracle.corner_ramps(A3)
    assert info[1:].tolist() == info3[1:].tolist() and int(info[3]) == 19, (info, info3)
    want = oracle.fuse_fade(A3, np.repeat(B[:, :, :1], 3, axis=2), 30, 0)
    assert np.array_equal(oracle.fuse_fade(A, B, 30, 0)[:, :, 0], want[:, :, 0])
    # three channels: both rules are one rule
    assert np.array_equal(X.old_rule_valid(A3), SR.pixel_valid(A3))


def test_the_max_energy_region_reaches_5100():
    A, B = X.max_energy_region(4)
    E = SR.energy(A, B)
    assert E.max() == SR.E_MAX == 5100 and (E[2:-2, 2:-2] == 5100).all() and E.min() < 5100
    assert SR.energy(*X.max_energy_region(2)).max() == 2550
    assert any(name.startswith("max energy") for name, *_ in X.seam_cases(4))
    # and the region the int32 cost bound refuses
    r, c = X.SEAM_TOO_LONG
    assert 5100 * max(r, c) > 2 ** 31 - 1 >= 5100 * (max(r, c) - 1) and r * c * 4 * 8 * 2 < 64 << 20
    with pytest.raises(ValueError):
        SR.seam_fuse(np.zeros((r, c, 2), np.int64), np.zeros((r, c, 2), np.int64), 1, 1, corner_ramps=lambda A: None)


@pytest.mark.parametrize("ch", X.CHANNELS)
def test_edge_canvases_walk_and_cover_the_listed_sizes(oracle, ch):
    cases = X.edge_canvases(ch)
    widths, heights, tile_widths, kinds = set(), set(), set(), set()
    for e in cases:
        assert all(t.shape[2:] == (ch,) and t.dtype == np.uint8 for t in e.tiles), e.name
        want, infos, stop = cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom)
        assert stop is None, (e.name, stop)
        for t, g, info in zip(e.tiles, e.geom, infos):
            if info is None:
                continue
            y0, x0, ry0, rx0, ry1, rx1 = [int(v) for v in g[:6]]
            widths.add(rx1 - rx0); heights.add(ry1 - ry0)
            kinds.add((cc.layout_of(rx1 - rx0), "strip" if info[0] == 0 else info[1]))
            if x0 % 4:
                tile_widths.add(t.shape[1])
        assert any(((t == 0).any(axis=2) & (t > 0).any(axis=2)).any() for t in e.tiles if t.size > 40), e.name
    assert set(X.ROI_WIDTHS) <= widths and set(X.ROI_HEIGHTS) <= heights and set(X.TILE_WIDTHS) <= tile_widths, (widths, heights, tile_widths)
    assert {(layout, kind) for layout in (1, 2, 4) for kind in ("strip", 0, 1, 2, 3)} <= kinds, kinds
    verdict = X.edge_verdict_only(ch)
    assert len(verdict) == 2
    for e in verdict:
        assert cc.reference_fade_walk(oracle, e.rows, e.cols, e.tiles, e.geom)[2] == len(e.tiles) - 1, e.name


@pytest.mark.parametrize("ch", X.CHANNELS)
def test_the_multiband_layout_fuses_two_strips_and_a_corner(oracle, ch):
    rows, cols, tiles, geom = X.multiband_layout(ch)
    want, fused = X.reference_fuse_walk(tiles, geom, rows, cols, lambda A, B, dx, dy: MB.multiband(A, B, dx, dy, 3, oracle.corner_ramps))
    assert want.shape == (rows, cols, ch) and len(fused) == 3
    assert [_kind(oracle, A) if not isinstance(_kind(oracle, A), tuple) else "corner" for A, _B, _dx, _dy in fused] == [1, 2, "corner"]


def test_the_shading_capacity_case_fills_the_staged_segment():
    shape = X.SHADING_CAPACITY[4]
    assert shape[2] == 4 and shape[1] * shape[2] >= X.SHADE_SEG and X.shading_staged(shape, 127) == X.SHADE_LDS == 2040
    assert X.shading_staged(X.SHADING_CAPACITY[2], 127) == 1024 + 2 * 127 * 2 and X.SHADING_CAPACITY[2][1] * 2 >= X.SHADE_SEG
