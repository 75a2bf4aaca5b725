"""CPU tests of the ORB path: the independent numpy reference tests/orb_ref.py equals the CPU oracle (oracle/vfsms_oracle_orb.c) bit for
bit on synthetic, real, adversarial and parameter-variant inputs, and passes the float64 checks of tests/orb_f64.py.  An oracle slip is
caught here without a GPU; tests/test_orb_gpu.py holds the device to the same reference."""
import numpy as np
import pytest

import orb_cases as OC
import orb_f64 as F
import orb_ref as R

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def _oracle_run(oracle, name):
    img = OC.image(name)
    kr, _, _ = OC.reference(name)
    return oracle.orb_detect_describe(img, cap=len(kr) + 16, **OC.CASES[name][1])


def assert_same(name, got, want):
    (kg, dg), (kw, dw) = got, want
    assert len(kg) == len(kw), (name, len(kg), len(kw))
    for f in FIELDS:
        bad = np.nonzero(kg[f] != kw[f])[0]
        assert bad.size == 0, (name, f, int(bad[0]), kg[bad[0]], kw[bad[0]])
    bad = np.nonzero((dg != dw).any(1))[0]
    assert bad.size == 0, (name, "descriptor", int(bad[0]), kg[bad[0]])


@pytest.mark.parametrize("name", sorted(OC.CASES))
def test_reference_equals_oracle(oracle, name):
    kr, dr, _ = OC.reference(name)
    assert_same(name, _oracle_run(oracle, name), (kr, dr))


@pytest.mark.parametrize("name", OC.SMALL_EDGE)
def test_small_edge_threshold_reads_leave_the_level(name):
    """the cases the oracle once got wrong (it read past its level buffers): keypoints whose Harris window or rotated pattern reaches
    beyond the level exist, so the reflect-101 reads are exercised"""
    k, _, st = OC.reference(name)
    p = OC.CASES[name][1]
    sizes = R.level_sizes(*OC.image(name).shape, p["scale_factor"], p["nlevels"])
    h = np.array([sizes[o][0] for o in k["octave"]]); w = np.array([sizes[o][1] for o in k["octave"]])
    d = np.minimum.reduce([st["lx"], st["ly"], w - 1 - st["lx"], h - 1 - st["ly"]])
    reach = 4 if p["patch_size"] == 2 else 18
    assert (d < reach).sum() >= 5, (name, int((d < reach).sum()))


@pytest.mark.parametrize("name", ["tex409x2048", "real387x2584", "wedges", "near0", "near255", "lattice12", "patch31_edge16",
                                  "patch2_edge2", "scale1.5", "scale2", "nlevels1"])
def test_float64_checks_on_the_reference(name):
    k, d, st = OC.reference(name)
    p = OC.CASES[name][1]
    F.check_all(k, d, st, p["scale_factor"], p["patch_size"])


def test_fast_score_is_the_brute_force_definition():
    rng = np.random.default_rng(11)
    for t in (0, 1, 20, 254):
        for img in (rng.integers(0, 256, (24, 29), dtype=np.uint8), OC.smooth(rng.integers(0, 256, (30, 26), dtype=np.uint8)),
                    rng.integers(0, 21, (20, 20), dtype=np.uint8), rng.integers(235, 256, (20, 20), dtype=np.uint8), OC.lattice(20, 20, 6, 3)):
            assert np.array_equal(R.fast_scores(img, t), F.fast_brute(img, t)), t


def test_quotas_and_level_geometry():
    q7 = R.level_quotas(7, 1.2, 8)
    assert q7 == [2, 1, 1, 1, 1, 1, 1, 0]                                   # cvRound of each share: 8 in all, above nfeatures
    q10 = R.level_quotas(10, 1.2, 8)
    assert sum(q10[:-1]) == 10 and q10[-1] == 0
    assert R.level_quotas(1, 1.2, 8) == [0] * 7 + [1]
    q = R.level_quotas(5000, 1.2, 8)
    assert sum(q) == 5000 and q[0] == 1086
    assert R.level_sizes(409, 2048, 1.2, 8)[-1] == (114, 572)
    assert [s[0] for s in R.level_sizes(1, 2048, 1.2, 8)][-1] == 0         # a level of 0 rows: no keypoints at all
    k, d = R.detect_describe(np.full((1, 2048), 9, np.uint8))
    assert len(k) == 0 and d.shape == (0, 32)


def test_adversarial_inputs_hit_their_edges():
    """each adversarial case exercises what it is named for"""
    k, _, st = OC.reference("wedges")
    assert {0.0, 90.0, 180.0, 270.0} <= set(np.unique(k["angle"]).tolist())
    k, _, st = OC.reference("lattice8")
    assert len(k) > 12048 and (k["octave"] == 0).sum() > 6388 and np.all(k["angle"][k["octave"] == 0] == 0)
    assert len(OC.reference("binary_blocks")[0]) == 0 or not (OC.reference("binary_blocks")[0]["octave"] == 0).any()
    assert len(OC.reference("flat")[0]) == 0
    k, _, st = OC.reference("border_lattice")
    assert (st["lx"] == 31).any() and (st["ly"] == 31).any()
    assert len(OC.reference("nfeatures20000")[0]) > 0
    assert len(OC.reference("near0")[0]) > 0 and len(OC.reference("near255")[0]) > 0


def test_random_pattern_is_upstreams_generator(oracle):
    for ps in (2, 15, 30):
        assert np.array_equal(R.random_pattern(ps).reshape(-1), oracle.orb_pattern(ps).reshape(-1)), ps
        assert R.random_pattern(ps).min() == -(ps // 2) and R.random_pattern(ps).max() == ps // 2


def test_hamming_1nn_equals_the_oracle_matcher(oracle):
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (700, 32), dtype=np.uint8)
    t = rng.integers(0, 256, (2600, 32), dtype=np.uint8)
    t[2100:2300] = t[10:210]                        # exact ties across the 2048-train blocks: the lower index wins
    q[:50] = t[10:60]
    for max_dist in (-1, 0, 30, 100):
        p, d = R.hamming_1nn(q, t, max_dist)
        po, do = oracle.bf_hamming_matches(q, t, max_dist)
        assert np.array_equal(p, po) and np.array_equal(d, do), max_dist
    assert np.array_equal(R.hamming_1nn(q, t)[0][:50, 0], np.arange(10, 60))
