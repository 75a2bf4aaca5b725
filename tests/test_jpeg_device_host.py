"""The host half of Method.jpegEncoder = "device" -- the header writer of the library, DeviceJpegFile, the driver's refusals -- without a
GPU: payloads come from the specification (tests/jpeg_enc_ref.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_enc_ref as ref                # noqa: E402

import imagestitch_amd as isa             # noqa: E402
from imagestitch_amd import _lib          # noqa: E402
from imagestitch_amd.io import DeviceJpegFile       # noqa: E402


@pytest.mark.parametrize("rows,cols,ch", [(8, 8, 1), (17, 23, 3), (65500, 300, 1), (4800, 4800, 3)])
@pytest.mark.parametrize("quality", [1, 50, 95, 100])
@pytest.mark.parametrize("R", [1, 8, 258, 65535])
def test_library_header_is_the_specifications(rows, cols, ch, quality, R):
    assert _lib.jpeg_header(rows, cols, ch, quality, R) == ref.header(rows, cols, ch, quality, R)


def test_library_header_one_interval_and_refusals():
    assert _lib.jpeg_header(33, 47, 3, 95, 0) == ref.header(33, 47, 3, 95, 0)
    for args in [(4800, 4800, 3, 95, 0), (64, 64, 3, 95, 65536), (65501, 8, 1, 95, 8), (8, 65501, 1, 95, 8), (8, 8, 2, 95, 0), (8, 8, 4, 95, 0),
                 (8, 8, 1, 0, 0), (8, 8, 1, 101, 0), (0, 8, 1, 95, 0)]:
        with pytest.raises(_lib.VfsmsError):
            _lib.jpeg_header(*args)


@pytest.mark.parametrize("shape,R,band", [((80, 100, 3), 7, 1), ((40, 100), 13, 2)])
def test_device_jpeg_file_appends_bands_behind_the_header(tmp_path, shape, R, band):
    img = np.random.default_rng(2).integers(0, 256, shape, dtype=np.uint8)
    mcu = 16 if len(shape) == 3 else 8
    mh = -(-shape[0] // mcu)
    path = str(tmp_path / "sub" / "m.jpg")                      # (the directory does not exist yet)
    f = DeviceJpegFile(path, shape, 95, R)
    for r0 in range(0, mh, band):
        f.append(np.frombuffer(ref.scan(img, 95, R, True, r0, min(band, mh - r0)), np.uint8))
    f.close()
    with open(path, "rb") as fh:
        data = fh.read()
    assert data == ref.encode(img, 95, R) and f.bytes_written == len(data)
    if _lib.jpeg_encode(np.zeros((8, 8), np.uint8)) is not None:
        theirs = bytes(_lib.jpeg_encode(img, quality=95))
        assert np.array_equal(_lib.jpeg_decode(data, want_planes=True), _lib.jpeg_decode(theirs, want_planes=True))


def test_device_jpeg_file_refuses_what_jpeg_cannot_hold(tmp_path):
    for shape in [(70000, 8), (8, 70000, 3), (8, 8, 4)]:
        with pytest.raises(ValueError, match="JPEG holds 1- or 3-channel images of at most 65500 pixels a side"):
            DeviceJpegFile(str(tmp_path / "x.jpg"), shape)
    assert not os.path.exists(str(tmp_path / "x.jpg"))


def test_method_defaults_and_driver_refusals(tmp_path):
    from fakes import OracleEngine

    def FakeEngine():
        return OracleEngine(None)
    assert (isa.Stitcher.jpegEncoder, isa.Stitcher.jpegQuality, isa.Stitcher.jpegRestartMcus) == ("host", 95, 8)
    st = isa.Stitcher(); st._engine = FakeEngine()
    args = (str(tmp_path / "none"), str(tmp_path / "out") + os.sep, 1, st.calculateOffsetForFeatureSearchIncre)
    st.jpegEncoder = "device"
    with pytest.raises(NotImplementedError):                  # an engine without canvas_encode_jpeg_bands
        st.imageSetStitchWithMutiple(*args)
    with pytest.raises(NotImplementedError):
        st.imageSetStitch(*args)
    st.jpegEncoder = "gpu"
    with pytest.raises(ValueError):
        st.imageSetStitchWithMutiple(*args)
    assert not os.path.exists(str(tmp_path / "out"))

    class WithEncoder(OracleEngine):
        def canvas_encode_jpeg_bands(self, *a):
            raise AssertionError("not reached")
    st = isa.Stitcher(); st._engine = WithEncoder(None)
    st.jpegEncoder = "device"
    for bad in (4096 + 16, 64, 0):                             # not a multiple of 16 * 8
        st.mosaicBandRows = bad
        with pytest.raises(ValueError, match="mosaicBandRows"):
            st.imageSetStitchWithMutiple(*args)
    st.mosaicBandRows, st.jpegRestartMcus = 4096, 0
    with pytest.raises(ValueError, match="jpegRestartMcus"):
        st.imageSetStitchWithMutiple(*args)
    st.jpegRestartMcus, st.streamOutput = 8, False               # not streamed: the host encoder writes the file, nothing to refuse
    assert st._deviceJpeg("jpg") is False
    st.streamOutput = True
    assert st._deviceJpeg("jpg") is True and st._deviceJpeg("png") is False
