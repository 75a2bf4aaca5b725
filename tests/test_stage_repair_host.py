"""CPU tests of Method.failedPairRepair = "stage": the two specifications (tests/ncc_wide_ref.py, tests/stage_ref.py) hold the properties
they are written for -- the two-level search returns the exhaustive answer, the stage model resolves serpentines and leaves a raster's
fly-back pair alone -- and the product's host code (imagestitch_amd/stage.py, the Method switches) equals them on a spec-backed engine."""
import numpy as np
import pytest

import imagestitch_amd as isa
from imagestitch_amd import stage
from imagestitch_amd.grid import GridRegistrar, serpentine_directions, split_segments
import adjust_cases as AC
import ncc_search_ref as S
import ncc_wide_ref as W
import stage_cases as SC
import stage_ref
import verify_ref

FX = verify_ref.FIXED_ONE


# ---- the wide search ------------------------------------------------------------------------------------------------------------------
def test_the_grid_is_the_one_the_bounds_were_measured_on():
    _tiles, true, classes = SC.grid35()
    assert true[:4] == SC.G35_FIRST_OFFSETS and classes == SC.G35_CLASSES
    assert [stage_ref.offset_class(o[0], o[1], 256, 256) for o in true] == classes


@pytest.mark.parametrize("part", [0, 1])
def test_wide_search_equals_the_exhaustive_search_on_the_3x5_grid(part):
    _tiles, true, _c = SC.grid35()
    disp = SC.displacements(14, 21)
    for k in range(part * 7, part * 7 + 7):
        f, K = SC.CONFIGS[k % 3]
        dx, dy = true[k][0] + disp[k][0], true[k][1] + disp[k][1]
        out8, _seeds = SC.spec_wide(("g35", k), ("g35", k + 1), dx, dy, SC.RADIUS, f, K, SC.MIN_PIXELS)
        ex = SC.spec_exhaustive(("g35", k), ("g35", k + 1), dx, dy, SC.RADIUS, SC.MIN_PIXELS)
        assert tuple(out8[:3]) == ex, (k, f, K, out8, ex)
        assert [dx + out8[0], dy + out8[1]] == true[k] and round(out8[2] / FX, 4) >= SC.TRUE_SCORE_MIN


@pytest.mark.parametrize("name", sorted(AC.GRIDS))
def test_wide_search_equals_the_exhaustive_search_on_the_3x3_grids(name):
    _tiles, true = AC.grid(name)
    disp = SC.displacements(8, 5 + len(name))
    for k in (0, 2, 5, 7):                                    # two column pairs, two turns
        f, K = SC.CONFIGS[k % 3]
        dx, dy = true[k][0] + disp[k][0], true[k][1] + disp[k][1]
        out8, _seeds = SC.spec_wide((name, k), (name, k + 1), dx, dy, SC.RADIUS, f, K, AC.MIN_PIXELS)
        assert tuple(out8[:3]) == SC.spec_exhaustive((name, k), (name, k + 1), dx, dy, SC.RADIUS, AC.MIN_PIXELS), (name, k, f, K)
        assert [dx + out8[0], dy + out8[1]] == true[k]


@pytest.mark.parametrize("f", [2, 4, 8])
def test_reduce_geometry_for_every_residue(f):
    rng = np.random.default_rng(3)
    A = rng.integers(0, 256, (41, 53), dtype=np.uint8); B = rng.integers(0, 256, (41, 53), dtype=np.uint8)
    for dx in range(-f - 1, f + 2):
        for dy in (-2 * f + 1, -1, 0, 1, f, f + 3):
            Ac, Bc, Dx, Dy = W.reduce_pair(A, B, dx, dy, f)
            ox, oy = dx % f, dy % f
            assert 0 <= ox < f and 0 <= oy < f and Dx * f + ox == dx and Dy * f + oy == dy
            assert Ac.shape == Bc.shape == ((41 - ox) // f, (53 - oy) // f)
            u, v = Ac.shape[0] - 1, Ac.shape[1] - 1           # the last block, summed by hand
            assert int(Ac[u, v]) == (int(A[ox + f * u:ox + f * u + f, oy + f * v:oy + f * v + f].astype(np.int64).sum()) + f * f // 2) // (f * f)
            assert int(Bc[0, 0]) == (int(B[:f, :f].astype(np.int64).sum()) + f * f // 2) // (f * f)
    assert W.reduce_pair(np.full((8, 8), 255, np.uint8), np.zeros((8, 8), np.uint8), 0, 0, f)[0].max() == 255


def test_seed_suppression_and_tie_rules():
    s = np.zeros((5, 5), np.int32)
    s[2, 2], s[2, 3], s[0, 0], s[4, 4] = 900, 950, 700, 700
    assert W.seeds_of(s, 4) == [(0, 1, 950), (-2, -2, 700), (2, 2, 700), (0, -1, 0)]      # (0, 0) and (-1, 0) are (0, 1)'s neighbours; equal scores: i * i + j * j, i, j
    assert W.seeds_of(s, 1) == [(0, 1, 950)]
    assert W.seeds_of(np.zeros((5, 5), np.int32), 3) == [(0, 0, 0), (-2, 0, 0), (0, -2, 0)]     # all equal: the smallest i * i + j * j, i, j
    assert W.seeds_of(np.zeros((3, 3), np.int32), 4) == [(0, 0, 0)]                              # the centre suppresses the whole 3 x 3 surface
    t = np.zeros((3, 3), np.int32); t[0, 0] = 5
    assert W.seeds_of(t, 4) == [(-1, -1, 5), (0, 1, 0), (1, -1, 0)]     # (0, 1) comes before the corners and shuts two of them out: three seeds


def test_clamping_at_small_radii_and_on_the_rim():
    assert [W.centre(c, 4, 1) for c in (-1, 0, 1)] == [0, 0, 0]                # R = 1 < f: one fine window of radius 1 around the prediction
    assert [W.centre(c, 4, 3) for c in (-1, 0, 1)] == [0, 0, 0]                # R = 3 < f likewise
    assert [W.centre(c, 4, 6) for c in (-2, -1, 0, 1, 2)] == [-2, -2, 0, 2, 2]  # R = 6: Rc = 2, the fine windows stay inside [-6, 6]
    assert [W.centre(c, 4, 32) for c in (-8, -7, 7, 8)] == [-28, -28, 28, 28]   # a seed on the rim: its window ends at the rim
    assert W.centre(16, 8, 128) == 120 and W.centre(-16, 8, 128) == -120
    tiles, true, _c = SC.grid35()
    for R in (1, 3):
        out8, seeds = SC.spec_wide(("g35", 0), ("g35", 1), true[0][0] + 1, true[0][1] - 1, R, 4, 2, SC.MIN_PIXELS)
        assert out8[:2] == [-1, 1] and out8[7] == 1 and not seeds[1:].any()    # Rc = 1: one seed
        assert out8[:3] == list(S.search(tiles[0], tiles[1], true[0][0] + 1, true[0][1] - 1, R, SC.MIN_PIXELS)[:3])
    with pytest.raises(AssertionError):
        W.check_args(40, 2, 2)
    with pytest.raises(AssertionError):
        W.check_args(32, 3, 2)


# ---- the stage model -------------------------------------------------------------------------------------------------------------------
def test_lower_median_and_opposite_class_fallback():
    assert stage_ref.lower_median([5, 1, 9, 3]) == 3 and stage_ref.lower_median([4]) == 4 and stage_ref.lower_median([2, 8, 5]) == 5
    table = [[1, 190, 0, 1, 1, 9], [1, 188, -5, 1, 1, 9], [1, 186, 3, 1, 1, 9], [1, 192, 2, 1, 1, 9], [1, 5, 198, 2, 1, 9], [0, 0, 0, 0, 0, 0]]
    M, counts = stage_ref.model(table, 256, 256)
    assert M == {1: (188, 0), 2: (5, 198), 3: (-188, 0), 4: (-5, -198)} and counts == {1: 4, 2: 1, 3: 0, 4: 0}
    M, _ = stage_ref.model(table[:4], 256, 256)
    assert M[2] is None and M[4] is None
    Mp, avail, count = stage.stage_model(np.array(table, np.int64)[:5, 1:3], np.array([1, 1, 1, 1, 2]))
    assert Mp[1:].tolist() == [[188, 0], [5, 198], [-188, 0], [-5, -198]] and avail[1:].all() and count.tolist() == [0, 4, 1, 0, 0]
    assert stage_ref.offset_class(100, 100, 256, 256) == 1 and stage_ref.offset_class(-100, 100, 256, 256) == 3     # ties between the axes: the rows'
    assert stage_ref.offset_class(100, 100, 256, 200) == 2 and stage_ref.offset_class(0, 0, 256, 256) == 3
    assert stage.classes_of([[100, 100], [-100, 100], [0, -7], [0, 0]], 256, 256).tolist() == [1, 3, 4, 3]


@pytest.mark.parametrize("rows,cols,one,two", [(3, 5, [4], [0, 14]), (4, 6, [5], [5, 18]), (2, 8, [3], [3, 10])])
def test_period_rule_resolves_serpentines(rows, cols, one, two):
    """T = 2 rows needs 2 rows pairs that agree a period apart: 3 x 5 has 8 such couples, so its blank tiles may cost two of them (a tile
    inside the first or last period costs one per pair, the path's two end tiles one each); the larger grids have couples to spare"""
    d = serpentine_directions(rows, cols)
    for blanks in (one, two):                                 # the pairs before and behind a blank tile are unknown
        known = list(d)
        for t in blanks:
            for k in (t - 1, t):
                if 0 <= k < len(known):
                    known[k] = None
        T = stage_ref.period(known)
        assert T == 2 * rows
        assert stage.path_period([c or 0 for c in known]) == T
        for k in range(len(d)):
            if known[k] is None:
                assert stage_ref.period_class(known, T, k) == d[k]


def test_a_3x3_serpentine_with_its_centre_blank_needs_the_hint():
    d = serpentine_directions(3, 3)                           # 1 1 2 3 3 2 1 1: the centre is tile 4, pairs 3 and 4
    known = list(d); known[3] = known[4] = None
    assert stage_ref.period(known) is None and stage.path_period([c or 0 for c in known]) is None
    _tiles, true = AC.grid("g7")
    keys = [("g7", k) for k in range(9)]
    keys[4] = ("blank200", 5)
    table = SC.truth_table(true, d, [3, 4])
    up = [-stage_ref.lower_median([true[k][0] for k in (0, 1, 6, 7)]), -stage_ref.lower_median([true[k][1] for k in (0, 1, 6, 7)])]
    for hint, kinds in ((None, ["unresolved", "unresolved"]), (d, ["predicted", "predicted"])):
        want, want_report = SC.ref_repair(keys, table, hint=hint)
        got, report = stage.repair_table(SC.SpecWideEngine(), keys, [(160, 200)] * 9, table, hint=hint)
        assert np.array_equal(got, want) and report == want_report
        assert [e["kind"] for e in report["pairs"]] == kinds and report["model"][3] == {"offset": up, "count": 0}
        if hint is not None:                                  # nobody travelled upwards: the model's offset is the negated "down"
            assert got[3].tolist() == got[4].tolist() == [1] + up + [3, 0, 0]


def test_ties_between_classes_go_to_the_smaller_class():
    calls = []

    def wide(A, B, dx, dy, R, f, K, mp):
        calls.append((dx, dy))
        return [1, 1, FX // 2 + 7, 5000, 0, 0, 0, 1], None
    flat = [np.zeros((64, 64), np.uint8)] * 3
    table = [[1, 50, 0, 1, 1, 9], [0, 0, 0, 0, 0, 0]]
    out, rep = stage_ref.repair(flat, table, min_pixels=0, wide=wide, sums=lambda *a: (0, 0, 0, 0, 0, 0))
    assert calls == [(50, 0), (-50, 0)] and out[1].tolist() == [1, 51, 1, 1, 0, 0] and rep["pairs"][0]["class"] == 1


# ---- the product's host code against the specification ------------------------------------------------------------------------------------
def scenarios():
    _tiles, true, classes = SC.grid35()
    return {
        "turn_measured": (SC.g35_keys(), SC.truth_table(true, classes, [8]), None),
        "blank_tile_predicted": (SC.g35_keys({4: ("blank", 5)}), SC.truth_table(true, classes, [3, 4]), None),
        "foreign_tile_unresolved": (SC.g35_keys({7: ("alt", 7)}), SC.truth_table(true, classes, [6, 7]), None),
        "blank_with_hint": (SC.g35_keys({4: ("blank", 5)}), SC.truth_table(true, classes, [3, 4]), serpentine_directions(3, 5)),
        "nothing_failed": (SC.g35_keys(), SC.truth_table(true, classes), None),
    }


@pytest.mark.parametrize("name", ["turn_measured", "blank_tile_predicted", "foreign_tile_unresolved", "blank_with_hint", "nothing_failed"])
def test_repair_table_equals_the_specification(name):
    keys, table, hint = scenarios()[name]
    _tiles, true, _classes = SC.grid35()
    want, want_report = SC.ref_repair(keys, table, hint=hint)
    eng = SC.SpecWideEngine()
    got, report = stage.repair_table(eng, keys, [(256, 256)] * 15, table, hint=hint)
    assert np.array_equal(got, want) and got.dtype == np.int32
    assert report == want_report and eng.calls <= 3
    if name == "turn_measured":
        e = report["pairs"][0]
        assert got[8].tolist() == [1] + true[8] + [2, 0, 0] and e["kind"] == "measured" and round(e["score"], 4) >= SC.TRUE_SCORE_MIN
        assert report["counts"] == {"measured": 1, "predicted": 0, "unresolved": 0}
    if name in ("blank_tile_predicted", "blank_with_hint"):
        assert report["period"] == 6 and got[3].tolist() == got[4].tolist() == [1, -192, -2, 3, 0, 0]
        assert report["counts"] == {"measured": 0, "predicted": 2, "unresolved": 0}
    if name == "foreign_tile_unresolved":
        assert not got[6, 0] and not got[7, 0] and report["counts"]["unresolved"] == 2
        assert [(a, b) for a, b, _o in split_segments(got)] == [(0, 6), (7, 7), (8, 14)]


def test_the_conditions_under_which_the_threshold_separates():
    """the three bounds the issue measured on the specification: asserted here before any device is compared with it"""
    _tiles, true, classes = SC.grid35()
    M, _counts = stage_ref.model(SC.truth_table(true, classes), 256, 256)
    for f, K in SC.CONFIGS:
        for c in (1, 2, 3, 4):
            o8, _s = SC.spec_wide(("g35", 6), ("alt", 7), M[c][0], M[c][1], SC.RADIUS, f, K, SC.MIN_PIXELS)
            assert round(o8[2] / FX, 4) <= SC.UNRELATED_SCORE_MAX, (f, K, c, o8)
            o8, _s = SC.spec_wide(("g35", 3), ("blank", 5), M[c][0], M[c][1], SC.RADIUS, f, K, SC.MIN_PIXELS)
            assert round(o8[2] / FX, 4) <= SC.BLANK_SCORE_MAX, (f, K, c, o8)


def test_a_raster_fly_back_pair_is_never_predicted():
    """a raster path (every column scanned downwards) over the grid's tiles: the fly-back pair fails in every column, so the known classes
    have period 1 and the period rule says "down" -- the tiles are textured, so the blank test stops the prediction"""
    _tiles, true, _classes = SC.grid35()
    order = [0, 1, 2, 5, 4, 3, 6, 7, 8]                       # tiles of columns 0..2, each top to bottom
    pos = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(np.array(true, np.int64), axis=0)])
    keys = [("g35", k) for k in order]
    table = []
    for a, b in zip(order[:-1], order[1:]):
        o = (pos[b] - pos[a]).tolist()
        table.append([1, o[0], o[1], 1, 1, 9] if abs(o[0]) < 256 and abs(o[1]) < 64 else [0, 0, 0, 0, 0, 0])
    assert [r[0] for r in table] == [1, 1, 0, 1, 1, 0, 1, 1]
    want, want_report = SC.ref_repair(keys, table)
    assert want_report["period"] == 1 and [e["kind"] for e in want_report["pairs"]] == ["unresolved", "unresolved"]
    got, report = stage.repair_table(SC.SpecWideEngine(), keys, [(256, 256)] * 9, table)
    assert np.array_equal(got, want) and report == want_report and not got[2, 0] and not got[5, 0]


def test_repair_table_refusals():
    _tiles, true, classes = SC.grid35()
    table = SC.truth_table(true, classes, [8])
    with pytest.raises(ValueError, match="one shape"):
        stage.repair_table(SC.SpecWideEngine(), SC.g35_keys(), [(256, 256)] * 14 + [(256, 200)], table)
    with pytest.raises(ValueError):
        stage.repair_table(SC.SpecWideEngine(), SC.g35_keys()[:5], [(256, 256)] * 5, table)
    with pytest.raises(NotImplementedError):
        stage.repair_table(object(), SC.g35_keys(), [(256, 256)] * 15, table)
    reg = GridRegistrar(SC.SpecWideEngine())
    got, _report = reg.repair(SC.g35_keys(), [(256, 256)] * 15, table, radius=SC.RADIUS, min_pixels=SC.MIN_PIXELS)
    assert got[8].tolist() == [1] + true[8] + [2, 0, 0]


# ---- the switches --------------------------------------------------------------------------------------------------------------------------
def test_method_defaults_and_refusals():
    m = isa.Method()
    assert (m.failedPairRepair, m.repairRadius, m.repairFactor, m.repairPeaks, m.repairThreshold, m.repairMinPixels, m.repairBlankRatio) == \
        ("none", 32, 4, 2, 0.5, 4096, 0.25)
    assert isa.Stitcher().repairReport is None

    class NoFiles(isa.Stitcher):
        def printAndWrite(self, content):
            raise AssertionError("a refusal comes before anything is logged or listed")
    for attr, value in (("failedPairRepair", "model"), ("repairRadius", 0), ("repairRadius", 129), ("repairFactor", 3), ("repairPeaks", 0),
                        ("repairPeaks", 5), ("repairMinPixels", -1)):
        st = NoFiles(); st._engine = SC.SpecWideEngine(); st.failedPairRepair = "stage"
        setattr(st, attr, value)
        for call in (lambda: st.imageSetStitch("/nonexistent", "/nonexistent", 1, st.calculateOffsetForFeatureSearchIncre),
                     lambda: st.imageSetStitchWithMutiple("/nonexistent", "/nonexistent", 1, st.calculateOffsetForFeatureSearchIncre)):
            with pytest.raises(ValueError):
                call()
    st = NoFiles(); st._engine = SC.SpecWideEngine(); st.failedPairRepair, st.repairRadius, st.repairFactor = "stage", 40, 2
    with pytest.raises(ValueError, match="coarse radius"):
        st.imageSetStitch("/nonexistent", "/nonexistent", 1, st.calculateOffsetForFeatureSearchIncre)
    st = NoFiles(); st._engine = object(); st.failedPairRepair = "stage"
    with pytest.raises(NotImplementedError):
        st.imageSetStitchWithMutiple("/nonexistent", "/nonexistent", 1, st.calculateOffsetForFeatureSearchIncre)


# ---- the Stitcher through _registerBatched ------------------------------------------------------------------------------------------------
class LoggedStitcher(isa.Stitcher):
    def __init__(self, engine):
        super().__init__()
        self._engine, self.lines = engine, []
        self.isPrintLog, self.isColorMode, self.featureMethod, self.fuseMethod, self.direction = False, False, "surf", "notFuse", 1

    def printAndWrite(self, content):
        self.lines.append(content)


def test_stitcher_keeps_one_mosaic_through_the_batched_registration(oracle, tmp_path):
    from PIL import Image
    tiles, true, classes = SC.grid35()
    files = []
    for k, t in enumerate(tiles):
        files.append(str(tmp_path / ("t%02d.png" % k)))
        Image.fromarray(t).save(files[-1])

    def engine():
        return SC.RepairOracleEngine(oracle, SC.g35_keys(), true, classes, failed=[8])
    st = LoggedStitcher(engine())
    st.failedPairRepair = "stage"
    (status, end), got = st.flowStitch(list(files), st.calculateOffsetForFeatureSearchIncre)
    assert status and end == 14 and not st.engine.live
    ref = LoggedStitcher(engine())
    want = ref.getStitchByOffset(list(files), [list(o) for o in true])
    assert np.array_equal(np.asarray(got), np.asarray(want))
    e = st.repairReport["pairs"][0]
    assert st.repairReport["counts"] == {"measured": 1, "predicted": 0, "unresolved": 0} and e["pair"] == 8
    line = "  %s and %s can not be registered: repaired from the stage model (measured, score %.3f)" % (files[8], files[9], e["score"])
    at = st.lines.index(line)
    assert st.lines[at - 1] == "stitching %s and %s" % (files[8], files[9])
    assert st.lines[at + 1] == "  The offset of stitching: dx is %d dy is %d" % tuple(true[8])
    assert not any("can not be stitched" in ln for ln in st.lines)
    # "none": the same script gives the pieces and the log lines of today
    off = LoggedStitcher(engine())
    pieces = off.flowStitchWithMutiple(list(files), off.calculateOffsetForFeatureSearchIncre)
    assert len(pieces) == 2 and off.repairReport is None and off.engine.spec.calls == 0 and not off.engine.live
    assert "  %s and %s can not be stitched" % (files[8], files[9]) in off.lines and not any("repaired" in ln for ln in off.lines)
    assert "stitching Break, start from " + files[9] + " again" in off.lines
    halves = LoggedStitcher(engine())
    assert np.array_equal(np.asarray(pieces[0]), np.asarray(halves.getStitchByOffset(list(files[:9]), [list(o) for o in true[:8]])))


def test_stitcher_breaks_at_the_first_pair_that_stays_unresolved(oracle, tmp_path):
    """a foreign tile: its two pairs stay failed, the mosaic ends in front of it exactly as without the switch"""
    from PIL import Image
    _tiles, true, classes = SC.grid35()
    keys = SC.g35_keys({7: ("alt", 7)})
    files = []
    for k, key in enumerate(keys):
        files.append(str(tmp_path / ("t%02d.png" % k)))
        Image.fromarray(SC.tile(key)).save(files[-1])
    out = {}
    for switch in ("none", "stage"):
        st = LoggedStitcher(SC.RepairOracleEngine(oracle, keys, true, classes, failed=[6, 7]))
        st.failedPairRepair = switch
        (status, end), img = st.flowStitch(list(files), st.calculateOffsetForFeatureSearchIncre)
        assert status is False and end == 6 and not st.engine.live
        assert st.lines[-1] == "  %s and %s can not be stitched" % (files[6], files[7])
        out[switch] = np.asarray(img)
    assert np.array_equal(out["none"], out["stage"])
