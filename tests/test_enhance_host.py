"""The numpy reference of the enhancement kernels (tests/enhance_ref.py: OpenCV 3.3.1's equalizeHist and CLAHE restated from the upstream
sources) against the C oracle, on the case table the device test uses.  Two independent restatements of the same upstream code: where
they agree byte for byte on every edge of the table, a device difference is the device's."""
import numpy as np
import pytest

import enhance_ref as R


def test_case_table_is_the_one_the_device_test_runs():
    cs = R.cases()
    assert len(cs) == 351 and len(set(cs)) == 351
    regimes = {"grid_larger": 0, "side_one": 0, "one_side_divides": 0, "past_one_block": 0, "clip_floors_to_one": 0}
    for (h, w), _c, op in cs:
        if op is None:
            continue
        clip, t = op
        eh, ew = (h, w) if (h % t == 0 and w % t == 0) else (h + t - h % t, w + t - w % t)
        regimes["grid_larger"] += t > h or t > w
        regimes["side_one"] += h == 1 or w == 1
        regimes["one_side_divides"] += (h % t == 0) != (w % t == 0)
        regimes["past_one_block"] += w > 256
        regimes["clip_floors_to_one"] += clip > 0 and int(clip * (eh // t) * (ew // t) / 256) < 1
    assert all(v > 0 for v in regimes.values()), regimes


def test_reflect101_is_opencv_s_border_rule():
    assert R.reflect101(np.arange(-3, 9), 4).tolist() == [3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert R.reflect101(np.arange(0, 5), 1).tolist() == [0, 0, 0, 0, 0]
    assert R.reflect101(np.arange(0, 7), 2).tolist() == [0, 1, 0, 1, 0, 1, 0]


def test_reference_on_hand_computed_images():
    """small enough to follow with a pencil"""
    img = np.array([[0, 0, 1, 3]], np.uint8)                  # hist 2 1 0 1, i0 = 0, scale 255 / 2: sums 0 1 1 2 -> 0 127.5 -> 128 (even), 255
    assert R.equalize_hist(img).tolist() == [[0, 0, 128, 255]]
    assert R.equalize_hist(np.full((3, 2), 9, np.uint8)).tolist() == [[9, 9]] * 3
    # CLAHE, one tile, no clipping: cumsum(5) = 1, (9) = 3, (200) = 4; lut = cvRound(cumsum * 255 / 4) -> 64 (63.75), 191 (191.25), 255
    assert R.clahe(np.array([[5, 9], [9, 200]], np.uint8), 0, 1).tolist() == [[64, 191], [191, 255]]
    # the same with clip limit max(int(1 * 4 / 256), 1) = 1: bin 9 loses 1, excess 1 -> bin 0 gains it: cumsum(5) = 2, (9) = 3, (200) = 4
    # -> 128 (127.5, to even), 191, 255
    assert R.clahe(np.array([[5, 9], [9, 200]], np.uint8), 1, 1).tolist() == [[128, 191], [191, 255]]


@pytest.mark.parametrize("shape", R.SHAPES, ids=lambda s: "%dx%d" % s)
def test_reference_equals_the_oracle(oracle, shape):
    for content in R.CONTENTS:
        img = R.image(shape, content)
        assert np.array_equal(R.equalize_hist(img), oracle.equalize_hist(img)), (shape, content, "equalizeHist")
        for clip, grid in R.CLAHE_PARAMS:
            assert np.array_equal(R.clahe(img, clip, grid), oracle.clahe(img, float(clip), grid)), (shape, content, clip, grid)
