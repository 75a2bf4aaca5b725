"""The host side of the ingest path against tests/ingest_ref.py: the package's numpy twin of the colour conversion on the whole Y Cb Cr
cube, which 4:2:0 files the raw-plane decode takes (libjpeg upsamples with the triangle filter only beyond two chroma columns), and the
restated triangle filter against the library's own decode on block content that reaches the clamps."""
import numpy as np
import pytest

import ingest_ref as R


def test_fixed_point_constants_are_jdcolor_s():
    assert (R.FIX_1_40200, R.FIX_1_77200, R.FIX_0_34414, R.FIX_0_71414) == (91881, 116130, 22554, 46802)


def test_host_twin_of_the_conversion_equals_the_reference_on_the_whole_cube():
    from imagestitch_amd import stitcher as ST
    cbcr = np.stack(np.meshgrid(np.arange(256), np.arange(256), indexing="ij"), -1).astype(np.uint8)          # (256, 256, 2)
    seen = np.zeros(3, bool)
    for y in range(256):
        ycc = np.concatenate([np.full((256, 256, 1), y, np.uint8), cbcr], -1)
        want = R.ycc_to_bgr(ycc)
        assert np.array_equal(ST._ycc_to_bgr(ycc), want), y
        seen |= np.array([(want == 0).any(), (want == 255).any(), ((want > 0) & (want < 255)).any()])
    assert seen.all()


def _library_or_skip():
    from imagestitch_amd import _lib
    if _lib.jpeg_decode(R.jpeg_bytes(R.corner_blocks(8, 8, 0)), False) is None:
        pytest.skip("no libjpeg.so.8 on this host: the Stitcher decodes with Pillow")
    return _lib


def test_raw_420_decode_leaves_files_of_two_chroma_columns_to_the_full_decode():
    """jdsample.c: h2v2_fancy_upsample needs downsampled_width > 2.  A 4:2:0 file of 3 or 4 columns is upsampled by replication -- its
    decoded chroma is constant over 2 x 2 blocks, which the triangle filter of the same samples is not -- so the raw-plane decode (whose
    consumer, k_ingest_420, is the triangle filter) refuses it; from 5 columns on it takes the file."""
    _lib = _library_or_skip()
    for w in (3, 4, 5):
        for h in (2, 6, 17):
            data = R.jpeg_bytes(R.corner_blocks(h, w, 10 * w + h), quality=100, subsampling=2)
            raw = _lib.jpeg_decode_raw420(data)
            full = _lib.jpeg_decode(data, True)
            assert full is not None and np.array_equal(full, R.decode_ycc(data)), (w, h)
            if w >= 5:
                assert raw is not None and raw[3:] == (h, w), (w, h)
                continue
            assert raw is None, (w, h)
            # the evidence: the library's planes ARE the replicated samples (the samples read back from the block corners)
            for c in (1, 2):
                assert np.array_equal(full[:, :, c], R.replicate_h2v2(full[0::2, 0::2, c], h, w)), (w, h, c)
    # ... and the triangle filter of such samples differs from them (so the device path would have been wrong there)
    data = R.jpeg_bytes(R.corner_blocks(6, 4, 46), quality=100, subsampling=2)
    full = _lib.jpeg_decode(data, True)
    samples = full[0::2, 0::2, 1]
    assert samples.min() != samples.max()
    assert not np.array_equal(R.fancy_h2v2(samples, 6, 4), full[:, :, 1])


@pytest.mark.parametrize("w,h", R.HOST_SIZES, ids=lambda v: str(v))
def test_restated_fancy_upsampler_equals_the_library_on_block_content(w, h):
    _lib = _library_or_skip()
    for q in (100, 60):
        data = R.jpeg_bytes(R.corner_blocks(h, w, 7 * w + h), quality=q, subsampling=2)
        full = _lib.jpeg_decode(data, True)
        raw = _lib.jpeg_decode_raw420(data)
        assert raw is not None and full is not None, (w, h, q)
        Y, Cb, Cr, H, W = raw
        assert (H, W) == (h, w) and Y.shape == ((h + 15) // 16 * 16, (w + 15) // 16 * 16)
        assert np.array_equal(Y[:H, :W], full[:, :, 0]), (w, h, q)
        assert np.array_equal(R.fancy_h2v2(Cb, H, W), full[:, :, 1]) and np.array_equal(R.fancy_h2v2(Cr, H, W), full[:, :, 2]), (w, h, q)
        assert np.array_equal(full, R.decode_ycc(data)), (w, h, q)


def test_jpeg_set_reaches_the_clamps_and_the_corners_of_the_chroma_plane():
    """the condition the device test puts on its reference, checked here without a device: over the whole set at least a quarter of the
    pixels have a channel at 0 or 255 after the conversion, and Cb and Cr each reach <= 8 and >= 247"""
    files = R.jpeg_set()
    assert len(files) == 39
    for h in R.JPEG_HEIGHTS:
        ws = [w for _n, w, hh, _d in files if hh == h]
        assert any(w % 2 for w in ws) and any(w % 2 == 0 for w in ws) and any(w % 4 == 0 for w in ws), (h, ws)
    assert sorted({w for _n, w, _h, _d in files[:36]}) == sorted(R.JPEG_WIDTHS)
    share, lo, hi = R.clamp_statistics([(R.ycc_to_bgr(ycc), ycc) for ycc in (R.decode_ycc(d) for _n, _w, _h, d in files)])
    print("jpeg set: saturated share %.3f, Cb %d..%d, Cr %d..%d" % (share, lo[0], hi[0], lo[1], hi[1]))
    assert share >= 0.25 and (lo <= 8).all() and (hi >= 247).all(), (share, lo, hi)
