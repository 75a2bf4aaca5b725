"""tests/jpeg_enc_ref.py -- the specification of the device JPEG encoder -- pinned to the system's libjpeg on the CPU: byte for byte at one
interval (header included), pixel for pixel with restart intervals, byte for byte against JpegBandWriter's files, and its own band and
refusal rules.  No GPU."""
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_cases as cases            # noqa: E402
import jpeg_enc_ref as ref                # noqa: E402

from imagestitch_amd import _lib          # noqa: E402
from imagestitch_amd.io import JpegBandWriter       # noqa: E402

pytestmark = pytest.mark.skipif(_lib.jpeg_encode(np.zeros((8, 8), np.uint8)) is None, reason="no libjpeg.so.8 on this host")

CASES = cases.cases()
IDS = ["%s-%dx%d-%s" % (c, h, w, "gray" if ch == 1 else "bgr") for c, h, w, ch in CASES]


def _pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("quality", cases.QUALITIES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_one_interval_is_libjpeg_byte_for_byte(case, quality):
    img = cases.image(*case)
    assert ref.encode(img, quality, 0) == bytes(_lib.jpeg_encode(img, quality=quality))


@pytest.mark.parametrize("quality", cases.QUALITIES)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_restart_intervals_decode_to_libjpegs_pixels(case, quality):
    img = cases.image(*case)
    theirs = bytes(_lib.jpeg_encode(img, quality=quality))
    planes, pixels = _lib.jpeg_decode(theirs, want_planes=True), _pillow(theirs)
    for R in (1, 3, 8):
        mine = ref.encode(img, quality, R)
        assert np.array_equal(_lib.jpeg_decode(mine, want_planes=True), planes), R
        assert np.array_equal(_pillow(mine), pixels), R


@pytest.mark.parametrize("shape", [(48, 40, 3), (24, 40)], ids=["bgr", "gray"])
def test_one_stripe_per_interval_is_jpegbandwriters_file(tmp_path, shape):
    img = np.random.default_rng(5).integers(0, 256, shape, dtype=np.uint8)
    mcu = 16 if len(shape) == 3 else 8
    path = str(tmp_path / "w.jpg")
    JpegBandWriter(path, stripe_rows=16)(0, img, img.shape)
    with open(path, "rb") as f:
        theirs = f.read()
    R = -(-shape[1] // mcu) * (16 // mcu)
    assert ref.encode(img, 95, R) == theirs


@pytest.mark.parametrize("shape,R,band", [((80, 100, 3), 1, 2), ((80, 100, 3), 7, 1), ((80, 100, 3), 14, 2), ((33, 47), 3, 1), ((33, 47, 3), 0, 3)])
def test_bands_of_mcu_rows_concatenate_to_the_file(shape, R, band):
    img = np.random.default_rng(6).integers(0, 256, shape, dtype=np.uint8)
    ch = 1 if len(shape) == 2 else 3
    mh = -(-shape[0] // (16 if ch == 3 else 8))
    body = b"".join(ref.scan(img, 95, R, True, r0, min(band, mh - r0)) for r0 in range(0, mh, band))
    assert ref.header(shape[0], shape[1], ch, 95, R) + body + b"\xFF\xD9" == ref.encode(img, 95, R)


def test_bands_must_be_whole_intervals():
    img = np.zeros((80, 100, 3), np.uint8)                      # 7 MCUs per row
    with pytest.raises(ValueError):
        ref.scan(img, 95, 2, True, 0, 1)                        # 7 MCUs are not whole intervals of 2
    with pytest.raises(ValueError):
        ref.scan(img, 95, 2, True, 1, 1)
    assert ref.scan(img, 95, 2, True, 2, 3)                     # 14 in front; the range ends at the last row


def test_refusals():
    big = np.zeros((16 * 300, 16 * 300, 3), np.uint8)           # 90000 MCUs
    with pytest.raises(ValueError):
        ref.encode(big, 95, 0)
    with pytest.raises(ValueError):
        ref.header(4800, 4800, 3, 95, 0)
    assert ref.header(4800, 4800, 3, 95, 65535)
    with pytest.raises(ValueError):
        ref.header(64, 64, 3, 95, 65536)
    with pytest.raises(ValueError):
        ref.header(65501, 8, 1, 95, 8)
    with pytest.raises(ValueError):
        ref.header(8, 65501, 1, 95, 8)
    for ch in (2, 4):
        with pytest.raises(ValueError):
            ref.header(8, 8, ch, 95, 0)
        with pytest.raises(ValueError):
            ref.encode(np.zeros((8, 8, ch), np.uint8), 95, 0)
