"""Plain numpy references for csrc/ingest_kernels.hip, written from libjpeg's formulas (jdcolor.c, jdsample.c) and from nothing in the
package: the fixed-point Y Cb Cr -> B G R conversion in exact int64, the h2v2 "fancy" chroma upsampler, and the JPEG test content that
drives the conversion into its clamps."""
import io

import numpy as np

SCALEBITS = 16
ONE_HALF = 1 << (SCALEBITS - 1)


def _fix(x):
    """jdcolor.c: #define FIX(x) ((JLONG)((x) * (1L << SCALEBITS) + 0.5))"""
    return int(x * (1 << SCALEBITS) + 0.5)


FIX_1_40200, FIX_1_77200, FIX_0_34414, FIX_0_71414 = _fix(1.40200), _fix(1.77200), _fix(0.34414), _fix(0.71414)


def ycc_to_bgr(ycc):
    """u8 (..., 3) Y Cb Cr -> u8 (..., 3) B G R as jdcolor.c's build_ycc_rgb_table / ycc_rgb_convert compute it: the Cr -> R and Cb -> B tables
    are rounded (ONE_HALF) and shifted on their own, the Cb and Cr parts of G share one ONE_HALF and one shift; >> is a floor shift."""
    ycc = np.asarray(ycc)
    y = ycc[..., 0].astype(np.int64)
    cb = ycc[..., 1].astype(np.int64) - 128
    cr = ycc[..., 2].astype(np.int64) - 128
    r = y + ((FIX_1_40200 * cr + ONE_HALF) >> SCALEBITS)
    b = y + ((FIX_1_77200 * cb + ONE_HALF) >> SCALEBITS)
    g = y + ((-FIX_0_34414 * cb + ONE_HALF - FIX_0_71414 * cr) >> SCALEBITS)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def fancy_h2v2(plane, H, W):
    """jdsample.c h2v2_fancy_upsample of a chroma plane coded at half size in both directions, for an H x W image: the triangle filter
    colsum(c) = 3 near + far, out(2c) = (3 colsum(c) + colsum(c - 1) + 8) >> 4, out(2c + 1) = (3 colsum(c) + colsum(c + 1) + 7) >> 4, the
    neighbours clamped to the image's first / last sample row and column.  (libjpeg takes this routine only when the plane has more than two
    sample columns, W >= 5; narrower files are replicated.)"""
    dh, dw = (H + 1) // 2, (W + 1) // 2
    p = plane[:dh, :dw].astype(np.int32)
    up = np.vstack([p[:1], p[:-1]]); dn = np.vstack([p[1:], p[-1:]])
    rows = np.empty((2 * dh, dw), np.int32); rows[0::2] = 3 * p + up; rows[1::2] = 3 * p + dn
    left = np.hstack([rows[:, :1], rows[:, :-1]]); right = np.hstack([rows[:, 1:], rows[:, -1:]])
    out = np.empty((2 * dh, 2 * dw), np.int32)
    out[:, 0::2] = (3 * rows + left + 8) >> 4; out[:, 1::2] = (3 * rows + right + 7) >> 4
    return out[:H, :W].astype(np.uint8)


def replicate_h2v2(plane, H, W):
    """jdsample.c h2v2_upsample: every chroma sample stands for its 2 x 2 pixels (what files of 3 or 4 columns get)"""
    dh, dw = (H + 1) // 2, (W + 1) // 2
    return np.repeat(np.repeat(plane[:dh, :dw], 2, 0), 2, 1)[:H, :W]


# ---- JPEG content that reaches the clamps -----------------------------------------------------------------------------------------------
JPEG_WIDTHS = (4, 5, 6, 7, 8, 15, 16, 17, 31, 32, 33, 1020, 1023, 1024, 1025, 1026, 1027, 1028)
JPEG_HEIGHTS = (2, 3, 15, 16, 17, 33)
HOST_SIZES = ((5, 2), (6, 2), (7, 3), (8, 16), (16, 17), (17, 2), (31, 33), (1028, 18))        # (w, h)


def corner_blocks(h, w, seed):
    """u8 (h, w, 3) R G B: 2 x 2-pixel blocks drawn from the eight corner colours of the RGB cube.  Chroma subsampling averages a block's
    own colour only, so the coded Cb / Cr sit at the corners of their plane, and the quantisation ringing around the block edges sends the
    decoded planes beyond them: the conversion clamps on about half of the pixels."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 8, ((h + 1) // 2, (w + 1) // 2))
    rgb = (np.stack([bits & 1, (bits >> 1) & 1, (bits >> 2) & 1], -1) * 255).astype(np.uint8)
    return np.ascontiguousarray(np.repeat(np.repeat(rgb, 2, 0), 2, 1)[:h, :w])


def jpeg_bytes(rgb, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(rgb).save(bio, "JPEG", **kw)
    return bio.getvalue()


def jpeg_set():
    """[(name, w, h, bytes)]: the 4:2:0 files of the device test.  The 18 widths with the 6 heights cycled twice, the second time shifted
    by three, at quality 100 and 60 in turn: 36 files in which every height meets an odd width, an even width and a multiple of four;
    then h = 1, w = 3 (both take the full decode) and a progressive file whose width is a multiple of four."""
    out = []
    for rnd in range(2):
        for k, w in enumerate(JPEG_WIDTHS):
            h = JPEG_HEIGHTS[(k + 3 * rnd) % len(JPEG_HEIGHTS)]
            q = (100, 60)[(k + rnd) % 2]
            out.append(("w%d_h%d_q%d" % (w, h, q), w, h, jpeg_bytes(corner_blocks(h, w, 1000 * rnd + k), quality=q, subsampling=2)))
    out.append(("w16_h1_q100", 16, 1, jpeg_bytes(corner_blocks(1, 16, 77), quality=100, subsampling=2)))
    out.append(("w3_h5_q60", 3, 5, jpeg_bytes(corner_blocks(5, 3, 78), quality=60, subsampling=2)))
    out.append(("w64_h17_q100_progressive", 64, 17, jpeg_bytes(corner_blocks(17, 64, 79), quality=100, subsampling=2, progressive=True)))
    return out


def decode_ycc(data):
    """Pillow's decode of a JPEG to its upsampled Y Cb Cr planes, u8 (h, w, 3)"""
    from PIL import Image
    im = Image.open(io.BytesIO(data)); im.draft("YCbCr", im.size); im.load()
    assert im.mode == "YCbCr"
    return np.asarray(im)


def clamp_statistics(decodes):
    """[(B G R decode, Y Cb Cr decode)] -> (share of pixels with a channel at 0 or 255, [min Cb, min Cr], [max Cb, max Cr])"""
    sat = tot = 0
    lo, hi = np.full(2, 255), np.zeros(2, int)
    for bgr, ycc in decodes:
        sat += int(((bgr == 0) | (bgr == 255)).any(-1).sum()); tot += bgr.shape[0] * bgr.shape[1]
        c = ycc[:, :, 1:].reshape(-1, 2)
        lo = np.minimum(lo, c.min(0)); hi = np.maximum(hi, c.max(0))
    return sat / tot, lo, hi
