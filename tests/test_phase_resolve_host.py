"""CPU tests of Stitcher.phaseResolve = "ncc": the specification (phase_resolve_ref.py) recovers true offsets -- wrapped, of either
sign, on odd surfaces, behind a burned-in pattern -- and refuses what it should; the library's state machine over it registers a grid;
the committed real crops; the host plumbing refuses engines without the resolver.  No GPU."""
import json
import os

import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd._lib import Engine, pairs_offsets_eval
from imagestitch_amd.grid import GridRegistrar
from imagestitch_amd.utility import roi_rect

import phase_resolve_cases as PC
import phase_resolve_ref as PR
import verify_ref as V
from phase_numpy import optimal_dft_size


# ---- truth on strips cut from one smooth random field ------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(PC.SHIFTS))
def test_reference_recovers_the_true_offset(shape):
    """both signs, zero, and shifts beyond half the padded size on each axis; 45 x 75 has odd M and N (the reading is taken before
    fftShift, so an odd size needs no rule of its own); 49 x 97 is padded to 50 x 100, so the wrap period is not the strip size"""
    h, w = shape
    M, N = optimal_dft_size(h), optimal_dft_size(w)
    assert (M, N) == {(48, 160): (48, 160), (160, 48): (160, 48), (45, 75): (45, 75), (49, 97): (50, 100)}[shape]
    wrapped = [0, 0]
    for (dx, dy) in PC.SHIFTS[shape]:
        A, B = PC.cut(h, w, dx, dy)
        for K in (1, 2):
            r = PR.resolve(A, B, K, PC.THRESHOLD, PC.MIN_PIXELS)
            assert list(r["row"][:6]) == [1, dx, dy, 0, 1, 1], (shape, (dx, dy), K, r["row"], r["peaks"])
            assert tuple(r["peaks"][0]) == (dx % M, dy % N) and r["row"][6] < 4          # the first peak carries it
            c = r["row"][6]
            assert r["cands"][c, 3] == (h - abs(dx)) * (w - abs(dy)) and r["scores"][c] > 0.9
            others = [s for k, s in enumerate(r["scores"]) if k != c]
            assert max(others) < r["scores"][c] - 0.5                                    # the other readings are nowhere near
        wrapped[0] += 2 * abs(dx) > M; wrapped[1] += 2 * abs(dy) > N
    assert wrapped[0] >= 2 and wrapped[1] >= 2


def test_the_four_shifts_of_the_issue_table():
    for (dx, dy) in ((5, -7), (33, 10), (-35, 100), (20, -120)):
        assert (dx, dy) in PC.SHIFTS[(48, 160)]
    A, B = PC.cut(48, 160, 33, 10)
    r = PR.resolve(A, B, 1, PC.THRESHOLD, PC.MIN_PIXELS)
    # the reading the reference's arg-max amounts to, (uy - M, ux) = (-15, 10), is among the candidates and scores nothing
    assert tuple(r["peaks"][0]) == (33, 10) and list(r["cands"][1, :2]) == [-15, 10] and r["scores"][1] < 0.2 and r["row"][6] == 0


# ---- a shift only the second peak carries ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,shift", [((48, 160), (5, -7)), ((160, 48), (-7, 5)), ((45, 75), (4, -6)), ((49, 97), (5, -7))])
def test_second_peak_behind_a_burned_in_bar(shape, shift):
    h, w = shape
    A, B = PC.bar_pair(h, w, shift[0], shift[1], 2)
    M, N = optimal_dft_size(h), optimal_dft_size(w)
    r = PR.resolve(A, B, 2, PC.THRESHOLD, PC.MIN_PIXELS)
    assert tuple(r["peaks"][0]) == (0, 0)                                                 # the bar does not move
    assert tuple(r["peaks"][1]) == (shift[0] % M, shift[1] % N)
    assert 4 <= r["row"][6] < 8 and list(r["row"][:3]) == [1, shift[0], shift[1]]
    r1 = PR.resolve(A, B, 1, PC.THRESHOLD, PC.MIN_PIXELS)
    assert list(r1["row"][1:3]) != list(shift) and list(r1["row"][1:3]) == [0, 0]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", sorted(PC.SHIFTS))
def test_refusals(shape):
    h, w = shape
    r = PR.resolve(*PC.disjoint(h, w), 2, PC.THRESHOLD, PC.MIN_PIXELS)
    assert r["row"][0] == 0 and max(r["scores"]) < 0.4 and r["row"][7] == V.fixed(max(s for s, c in zip(r["scores"], r["cands"]) if c[3] > 0))
    A, B = PC.flat(h, w)
    R = PR.surface(A, B)
    assert not R.any()                                                                    # exactly zero: (0, 0) is the only peak
    r = PR.resolve(A, B, 2, PC.THRESHOLD, PC.MIN_PIXELS, R=R)
    assert list(r["row"]) == [0, 0, 0, 0, 1, 1, 0, 0] and r["peaks"].tolist() == [[0, 0], [-1, -1]] and not r["cands"][4:].any()
    assert r["cands"][0].tolist() == [0, 0, 0, h * w]
    # an overlap under min_pixels scores 0: the same true shift, accepted with a small minimum and refused with a large one
    dx, dy = PC.SHIFTS[shape][2]
    A, B = PC.cut(h, w, dx, dy)
    n = (h - abs(dx)) * (w - abs(dy))
    assert PR.resolve(A, B, 2, PC.THRESHOLD, n)["row"][0] == 1
    r = PR.resolve(A, B, 2, PC.THRESHOLD, n + 1)
    assert r["row"][0] == 0 and r["cands"][r["row"][6], 2] == 0 or list(r["row"][1:3]) != [dx, dy]
    k = [tuple(c[:2]) for c in r["cands"]].index((dx, dy))
    assert r["cands"][k].tolist() == [dx, dy, 0, n]


def test_candidate_rules():
    # a peak's readings, the kept ones, the absent peak; M < 2 h, so every present peak keeps a reading
    c = PR.candidates([(49, 3), (-1, -1)], 50, 100, 49, 97)
    assert c == [(49, 3, False), (-1, 3, True), (49, -97, False), (-1, -97, False)] + [(0, 0, False)] * 4
    for (h, w) in ((49, 97), (45, 75), (409, 2048), (7, 5)):
        M, N = optimal_dft_size(h), optimal_dft_size(w)
        for uy in range(M):
            assert any(k for _dx, _dy, k in PR.candidates([(uy, 0)], M, N, h, w))
    # the peak rule: a plateau names its first element only; a constant surface has the one peak (0, 0)
    R = np.zeros((5, 7)); R[2, 3] = R[2, 4] = 1.0
    assert PR.peaks(R, 3)[0][0] == (2, 3) and (2, 4) not in PR.peaks(R, 8)[0]
    assert PR.peaks(np.ones((4, 6)), 2)[0] == [(0, 0), (-1, -1)]
    R = np.zeros((4, 6)); R[0, 0] = 2.0; R[3, 5] = 2.0                                    # circular neighbours: (3, 5) touches (0, 0), which precedes it
    assert PR.peaks(R, 2)[0] == [(0, 0), (-1, -1)]
    R = np.zeros((6, 8)); R[1, 1] = 3.0; R[4, 5] = 3.0; R[2, 6] = 5.0
    assert PR.peaks(R, 3)[0] == [(2, 6), (1, 1), (4, 5)]                                  # value descending, then index ascending


# ---- the state machine over the reference ---------------------------------------------------------------------------------------------
def reference_evaluator(tiles, roiRatio=0.2, peaks=2, threshold=0.5, min_pixels=4096, log=None):
    def attempts(items):
        rows = []
        for (k, d, i) in items:
            ra = roi_rect(tiles[k].shape, d, "first", i * roiRatio); rb = roi_rect(tiles[k + 1].shape, d, "second", i * roiRatio)
            A = np.ascontiguousarray(tiles[k][ra[0]:ra[0] + ra[2], ra[1]:ra[1] + ra[3]])
            B = np.ascontiguousarray(tiles[k + 1][rb[0]:rb[0] + rb[2], rb[1]:rb[1] + rb[3]])
            rows.append(PR.resolve(A, B, peaks, threshold, min_pixels)["row"])
            if log is not None:
                log.append(((k, d, i), rows[-1].copy()))
        return np.array(rows, np.int32)
    return attempts


def reference_chain(tiles, log=None):
    shapes = [t.shape for t in tiles]
    p = Engine.grid_params(method="phase", roiRatio=0.2, directIncre=1, window=8)
    return pairs_offsets_eval(reference_evaluator(tiles, log=log), shapes, p, 0, len(tiles) - 1, 1, False, True)


def test_state_machine_registers_a_serpentine_grid():
    tiles, offsets, dirs = PC.grid_tiles()
    assert len(tiles) == 9 and dirs == [1, 1, 2, 3, 3, 2, 1, 1]
    out, d_out, _st = reference_chain(tiles)
    assert out[:, 0].tolist() == [1] * 8
    assert out[:, 1:3].tolist() == offsets                                                # exact full-tile offsets, sign included
    assert out[:, 3].tolist() == dirs and d_out == 1 and out[:, 4].tolist() == [1] * 8


# ---- real pixels ----------------------------------------------------------------------------------------------------------------------------
def dendritic_crops(golden_dir):
    """the 25 committed dendritic crop pairs at the accepted (direction, i) with the raw vote of Stitcher.py:87's gold offset"""
    from test_verify_host import _raw, dendritic_crop_pairs
    meta = json.load(open(os.path.join(golden_dir, "real_path_strips.json")))["neighbourhoods"]
    gold = [_raw(e["gold"], e["direction"], e["i"], nb["shape"]) for nb in meta for e in nb["expected"]]
    crops = dendritic_crop_pairs(golden_dir, "expected")
    assert len(crops) == len(gold) == 25
    return [(t, a, b, g) for (t, _w, a, b, _r, _v), g in zip(crops, gold)]


def test_real_crops_every_accepted_row_is_within_one_pixel(golden_dir):
    """Stitcher's defaults (2 peaks, 0.5, 4096 pixels) on the 25 committed dendritic crops: an accepted row lies within 1 px of the gold
    offset; rejected rows are counted and printed.  Measured: 25 accepted, 0 rejected, winning scores 0.892 .. 0.980."""
    accepted, rejected = 0, []
    for t, a, b, g in dendritic_crops(golden_dir):
        r = PR.resolve(a, b, 2, 0.5, 4096)
        if r["row"][0]:
            accepted += 1
            assert abs(r["row"][1] - g[0]) <= 1 and abs(r["row"][2] - g[1]) <= 1, (t, r["row"], g)
        else:
            rejected.append((t, round(max(r["scores"]), 4), r["row"][1:3].tolist(), g))
    print("accepted %d rejected %d: %s" % (accepted, len(rejected), rejected))
    assert accepted + len(rejected) == 25
    assert (accepted, len(rejected)) == REAL_COUNTS


REAL_COUNTS = (25, 0)


# ---- host plumbing ------------------------------------------------------------------------------------------------------------------------
def test_defaults_and_engines_without_the_resolver():
    from fakes import OracleEngine
    st = isa.Stitcher()
    assert (st.phaseResolve, st.phasePeaks, st.phaseResolveThreshold, st.phaseResolveMinPixels) == ("none", 2, 0.5, 4096)
    assert (st.phaseResolveThreshold, st.phaseResolveMinPixels) == (isa.Method.verifyThreshold, isa.Method.verifyMinPixels)
    st._engine = OracleEngine.__new__(OracleEngine)
    st.phaseResolve = "ncc"
    A, B = PC.cut(64, 64, 3, 2)
    with pytest.raises(NotImplementedError):
        st.calculateOffsetForPhaseCorrleateIncre([A, B])
    reg = GridRegistrar(st.engine, method="phase", phaseResolve="ncc")
    with pytest.raises(NotImplementedError):
        reg._attempts([1, 2], [A.shape, B.shape], [(0, 1, 1)])
    with pytest.raises(NotImplementedError):
        with reg._estimator():
            pass
    with pytest.raises(ValueError):
        GridRegistrar(st.engine, method="phase", phaseResolve="fft")
    assert GridRegistrar(st.engine, method="surf", phaseResolve="ncc").phaseResolve == "none"
    # the batched path is taken with the resolver on whatever phaseSignFix says; off, phaseSignFix keeps the pair-by-pair loop as before
    st.batchRegistration = True
    m = st.calculateOffsetForPhaseCorrleateIncre
    st.phaseSignFix = True
    assert st._batchedMethod(m, 3) == "phase"
    st.phaseResolve = "none"
    assert st._batchedMethod(m, 3) is None
    st.phaseSignFix = False
    assert st._batchedMethod(m, 3) == "phase"


def test_pair_by_pair_loop_takes_the_resolver_row():
    """calculateOffsetForPhaseCorrleateIncre with "ncc": offset = [dx, dy] of the row, accepted on its status, neither the (y, x) swap nor
    phaseSignFix consulted; the axis correction and the direction search as ever"""
    class RefEngine:
        calls = 0

        def phase_resolve(self, a, b, peaks, threshold, min_pixels):
            RefEngine.calls += 1
            r = PR.resolve(a, b, peaks, threshold, min_pixels)
            return r["row"], r["cands"], r["peaks"]
    tiles, offsets, dirs = PC.grid_tiles()
    for fix in (False, True):
        st = isa.Stitcher()
        st.isPrintLog = False
        st._engine = RefEngine()
        st.phaseResolve, st.phaseSignFix, st.direction, st.roiRatio = "ncc", fix, 1, 0.2
        got = [st.calculateOffsetForPhaseCorrleateIncre([tiles[k], tiles[k + 1]]) for k in range(3)]
        assert got == [(True, offsets[k]) for k in range(3)] and st.direction == 2
    assert RefEngine.calls == 2 * (1 + 1 + 2)
