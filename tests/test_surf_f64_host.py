"""CPU only: the float64 SURF reference (tests/surf_f64.py) against the CPU oracle on every case of tests/surf_f64_cases.py.  This is where
the bounds are settled -- the measured figures are printed and held to the *_MEASURED constants -- and where the checks are shown to
bite: perturbed copies of the oracle's arrays fail them, and the reference with one planted transcription mistake rejects the oracle."""
import numpy as np
import pytest

import surf_f64 as F
import surf_f64_cases as Cs

_cache = {}


def _run(oracle, name):
    """oracle results of one case, computed once: image, parameters, detect-only list, described list, descriptors, float64 layers"""
    if name not in _cache:
        img, p = Cs.case(name)
        kw = dict(hessian=p["hessian"], n_octaves=p["n_octaves"], n_layers=p["n_layers"])
        kd = oracle.surf_detect(img, **kw)
        k, d = oracle.surf_detect_describe(img, extended=p["extended"], upright=p["upright"], **kw)
        _cache[name] = (img, p, kd, k, d, F.layers(img, p["n_octaves"], p["n_layers"]))
    return _cache[name]


def _figures(oracle, name):
    key = ("figures", name)
    if key not in _cache:
        img, p, kd, k, d, L = _run(oracle, name)
        S = oracle.integral(img)
        fig = dict(layer=F.check_layers(L, [oracle.surf_layer(S, l["size"], l["step"]) for l in L]))
        fig.update(F.check_all(img, p, kd, k, d, L=L))
        print("surf_f64 %-10s %s" % (name, " ".join("%s=%.3g" % kv for kv in fig.items())))
        _cache[key] = fig
    return _cache[key]


def test_case_coverage(oracle):
    img, p, kd, k, d, L = _run(oracle, "blobs")
    assert max(img.shape) <= 420
    o, l = Cs.layer_cell(k)
    for cell in [(a, b) for a in range(4) for b in (1, 2, 3)]:
        assert int(((o == cell[0]) & (l == cell[1])).sum()) >= 3, ("keypoints in (octave, layer)", cell)
    assert np.bincount(F.window_class(k), minlength=4).min() >= 2
    assert F.border_crossings(k, img.shape).sum(1).min() >= 20
    for name in Cs.NAMES:
        img, p, kd, k, d, L = _run(oracle, name)
        assert len(k) > 50, name
        cls = F.window_class(k)
        assert (cls == 3).any() and (name == "thin" or (cls < 3).any()), name                 # k_describe_small, and k_describe
        idx = F.subsample(k, img.shape, p["upright"])
        assert len(idx) <= 150 and len(np.unique(idx)) == len(idx)
        if name in ("blobs", "extended"):                                                      # every border window, every large window
            assert np.all(np.isin(np.nonzero(F.border_crossings(k, img.shape).any(0) | (cls <= 1))[0], idx))
    assert np.all(_run(oracle, "thin")[3]["octave"] == 0)
    for name, octaves in (("noise", {0, 1}), ("strip", {0, 1, 2}), ("crop", {0, 1, 2, 3}), ("blobs", {0, 1, 2, 3})):
        assert set(_run(oracle, name)[3]["octave"]) == octaves, name                            # lds<1>, lds<2>, rows2, coarse
    k = _run(oracle, "generic")[3]
    assert set(k["octave"]) == {0, 1, 2} and set(Cs.layer_cell(k, 4)[1]) == {1, 2, 3, 4}
    assert _run(oracle, "strided")[0].strides == (640, 1)
    assert all(np.array_equal(_run(oracle, "strided")[i], _run(oracle, "crop")[i]) for i in (3, 4))
    assert len(_run(oracle, "hessian400")[3]) < len(_run(oracle, "crop")[3])
    assert _run(oracle, "extended")[4].shape[1] == 128


@pytest.mark.parametrize("name", Cs.NAMES)
def test_oracle_passes_every_check(oracle, name):
    fig = _figures(oracle, name)
    assert fig["n"] > 50 and fig["described"] == fig["n"]


def test_measured_constants_are_the_measured_figures(oracle):
    """each *_MEASURED constant is the worst figure over all cases: no case exceeds it, and one case comes within 2 % of it"""
    figs = [_figures(oracle, name) for name in Cs.NAMES]
    for key, const in (("layer", F.LAYER_MEASURED), ("pos", F.POS_MEASURED), ("ori", F.ORI_MEASURED), ("desc_rounded", F.DESC_Q_MEASURED),
                       ("desc_plain", F.DESC_R_MEASURED)):
        worst = max(f[key] for f in figs)
        assert 0.98 * const <= worst <= const, (key, worst, const)
    assert F.LAYER_BOUND == 4 * F.LAYER_MEASURED and F.POS_BOUND == 4 * F.POS_MEASURED and F.ORI_BOUND == 4 * F.ORI_MEASURED
    assert F.DESC_Q_BOUND == min(4 * F.DESC_Q_MEASURED, F.DESC_CAP) < 2e-2 and F.DESC_R_BOUND == min(4 * F.DESC_R_MEASURED, F.DESC_CAP) < 2e-2
    assert max(f["resp"] for f in figs) <= F.LAYER_MEASURED


def test_perturbed_results_fail(oracle):
    img, p, kd, k, d, L = _run(oracle, "crop")
    F.check_keypoints(img, kd, p, L=L)
    sub = np.arange(40)

    def kp(change, match):
        q = kd.copy()
        q = change(q)
        with pytest.raises(AssertionError, match=match):
            F.check_keypoints(img, q, p, L=L)

    kp(lambda q: np.delete(q, 0), "firm float64 keypoint not reported")
    def moved(q):
        q["x"][7] += 1 << q["octave"][7]
        return q
    kp(moved, "without a float64 keypoint")
    def flipped(q):
        q["class_id"][11] = -q["class_id"][11]
        return q
    kp(flipped, "class_id")
    def swapped(q):
        q[[20, 21]] = q[[21, 20]]
        return q
    assert kd["response"][20] != kd["response"][21]
    kp(swapped, "keypoint order")

    F.check_orientation(img, k[sub])
    q = k[sub].copy()
    q["angle"][3] = (q["angle"][3] + 5.0) % 360.0
    with pytest.raises(AssertionError, match="orientation"):
        F.check_orientation(img, q)

    F.check_descriptors(img, k[sub], d[sub])

    def de(change, match):
        e = d[sub].copy()
        change(e)
        with pytest.raises(AssertionError, match=match):
            F.check_descriptors(img, k[sub], e)

    def exchanged(e):
        e[5] = e[5].reshape(16, 4)[:, [1, 0, 3, 2]].ravel()
    de(exchanged, "descriptor against")
    def cells(e):
        c = e[9].reshape(16, 4).copy()
        c[[5, 6]] = c[[6, 5]]
        e[9] = c.ravel()
    de(cells, "descriptor against")
    def scaled(e):
        e[2] *= np.float32(1.01)
    de(scaled, "norm")
    def plus(e):
        e[4, 10] += np.float32(0.02)
    de(plus, "norm|descriptor against")
    # the same with the norm kept (another component pays for it), on a component that lies on or above the rounded reference: the
    # component bound alone
    win = F.window64(img, float(k["x"][4]), float(k["y"][4]), k["size"][4], float(k["angle"][4]))
    dev = d[4] - F.descriptor64(win, True)
    c = int(np.argmax(dev))
    j = int(np.argmax(np.abs(d[4]) * (np.arange(64) != c)))
    assert dev[c] >= 0

    def plus_unit(e):
        v = e[4].astype(np.float64)
        v[c] += 0.02
        v[j] = np.sign(v[j]) * np.sqrt(1.0 - (v * v).sum() + v[j] * v[j])
        e[4] = v
    de(plus_unit, "descriptor against")


def test_planted_transcription_mistakes_reject_the_oracle(oracle):
    img, p, kd, k, d, L = _run(oracle, "crop")
    S = oracle.integral(img)
    got = [oracle.surf_layer(S, l["size"], l["step"]) for l in L]
    for kw in (dict(corner=np.floor), dict(xy_weight=0.9)):
        bad = F.layers(img, p["n_octaves"], p["n_layers"], **kw)
        with pytest.raises(AssertionError, match="layer det|layer trace"):
            F.check_layers(bad, got)
        with pytest.raises(AssertionError):
            F.check_keypoints(img, kd, p, L=bad)
    sub = np.arange(40)
    for kw in (dict(sigma=2.5), dict(rot_sign=1)):
        with pytest.raises(AssertionError, match="descriptor against"):
            F.check_descriptors(img, k[sub], d[sub], **kw)
    # and the extended layout with its halves exchanged
    img, p, kd, k, d, L = _run(oracle, "extended")
    e = d[:20].copy().reshape(20, 16, 8)[:, :, [2, 3, 0, 1, 6, 7, 4, 5]].reshape(20, 128)
    with pytest.raises(AssertionError, match="sign-split"):
        F.check_descriptors(img, k[:20], e, extended=True)
