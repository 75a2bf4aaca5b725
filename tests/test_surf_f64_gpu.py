"""The device's SURF output through the float64 checks of tests/surf_f64.py, with the bounds the CPU oracle settled (the host test): on
every case of tests/surf_f64_cases.py the device equals the oracle bit for bit -- the existing bar, on new shapes -- and its own arrays
pass the keypoint, orientation and descriptor checks.  The keypoint check runs on every keypoint; the per-keypoint orientation and
descriptor references run on surf_f64.subsample (at most 150, every border window and every large window of the blob cases)."""
import numpy as np
import pytest

import surf_f64 as F
import surf_f64_cases as Cs

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "response", "octave", "class_id")


@pytest.mark.parametrize("name", Cs.NAMES)
def test_device_passes_float64_checks(engine, oracle, name):
    img, p = Cs.case(name)
    sp = engine.surf_params(p["hessian"], p["n_octaves"], p["n_layers"], p["extended"], p["upright"])
    det = engine.surf_detect(img, sp)
    kxy, desc, kps = engine.surf_detect_describe(img, sp, full=True)
    kw = dict(hessian=p["hessian"], n_octaves=p["n_octaves"], n_layers=p["n_layers"])
    odet = oracle.surf_detect(img, **kw)
    ok, od = oracle.surf_detect_describe(img, extended=p["extended"], upright=p["upright"], **kw)
    assert len(det) == len(odet) > 50 and all(np.array_equal(det[f], odet[f]) for f in FIELDS)
    assert len(kps) == len(ok) and all(np.array_equal(kps[f], ok[f]) for f in FIELDS + ("angle",))
    assert np.array_equal(kxy, np.stack([ok["x"], ok["y"]], 1)) and np.array_equal(desc, od)
    fig = F.check_all(img, p, det, kps, desc, sample=150)
    print("surf_f64 device %-10s %s" % (name, " ".join("%s=%.3g" % kv for kv in fig.items())))
    assert 0 < fig["described"] <= 150
