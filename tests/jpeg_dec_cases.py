"""The files of the device JPEG decoder's tests (tests/test_jpeg_dec_host.py, tests/test_jpeg_dec_gpu.py), made once per process."""
import functools
import io

import numpy as np


def texture(h, w, colour=False, seed=7):
    """a smooth wave under noise: AC energy in every band without saturating everywhere"""
    rng = np.random.default_rng([seed, h, w, int(colour)])
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(x / 5.0) * np.cos(y / 7.0) + rng.normal(0, 25, (h, w))
    if colour:
        base = np.stack([base, np.roll(base, 3, 1) * 0.8 + 20, 255 - base], -1) + rng.normal(0, 10, (h, w, 3))
    return np.clip(base, 0, 255).astype(np.uint8)


def bit_noise(h, w, seed=11):
    """every pixel 0 or 255: the decoded samples overshoot both ends of the range"""
    return (np.random.default_rng([seed, h, w]).integers(0, 2, (h, w)) * 255).astype(np.uint8)


def jpeg_bytes(arr, **kw):
    from PIL import Image
    bio = io.BytesIO()
    Image.fromarray(arr).save(bio, "JPEG", **kw)
    return bio.getvalue()


@functools.lru_cache(maxsize=None)
def host_set():
    """((name, h, w, components, bytes), ...): the files the device path takes.  Sizes (h, w) as in the file"""
    c420 = texture(45, 61, True)
    return (
        ("gray_40x24_q95", 40, 24, 1, jpeg_bytes(texture(40, 24), quality=95)),
        ("gray_37x29_q75", 37, 29, 1, jpeg_bytes(texture(37, 29), quality=75)),
        ("bits_33x47_q100", 33, 47, 1, jpeg_bytes(bit_noise(33, 47), quality=100)),
        ("bits_33x47_q10", 33, 47, 1, jpeg_bytes(bit_noise(33, 47), quality=10)),
        ("c420_48x64_q95", 48, 64, 3, jpeg_bytes(texture(48, 64, True), quality=95, subsampling=2)),
        ("c420_45x61_q60", 45, 61, 3, jpeg_bytes(c420, quality=60, subsampling=2)),
        ("c420_45x61_q60_progressive", 45, 61, 3, jpeg_bytes(c420, quality=60, subsampling=2, progressive=True)),
        ("gray_512x640_q95", 512, 640, 1, jpeg_bytes(texture(512, 640), quality=95)),
    )


BIT_NOISE_FILES = ("bits_33x47_q100", "bits_33x47_q10")


@functools.lru_cache(maxsize=None)
def device_extra_set():
    """two more 4:2:0 files for the device: the smallest the path takes (5 columns, 2 rows), and one with a partial iMCU on both axes and
    several workgroups (200 rows x 328 columns: 13 x 21 iMCUs, 1092 luma blocks)"""
    return (
        ("c420_2x5_q90", 2, 5, 3, jpeg_bytes(texture(2, 5, True), quality=90, subsampling=2)),
        ("c420_200x328_q85", 200, 328, 3, jpeg_bytes(texture(200, 328, True), quality=85, subsampling=2)),
    )


def sixteen_bit_tables(data):
    """the same image with its DQT segments rewritten at 16-bit precision (Pq = 1), entries unchanged: what a file with a table entry
    beyond 255 looks like to a parser.  Decodes to the same samples."""
    out, p = bytearray(data[:2]), 2
    while True:
        m, n = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if m == 0xDA:
            return bytes(out) + data[p:]
        if m != 0xDB:
            out += data[p:p + 2 + n]
        else:
            seg, s, body = data[p + 4:p + 2 + n], 0, bytearray()
            while s < len(seg):
                assert seg[s] >> 4 == 0
                body.append(0x10 | (seg[s] & 15))
                for v in seg[s + 1:s + 65]:
                    body += bytes((0, v))
                s += 65
            out += bytes((0xFF, 0xDB, (len(body) + 2) >> 8, (len(body) + 2) & 255)) + body
        p += 2 + n


def refused_set():
    """((name, h, w, bytes), ...): files the device path must hand back"""
    rgb = texture(31, 43, True)
    from PIL import Image
    cmyk = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(cmyk, "JPEG", quality=90)
    good = host_set()[4][4]
    return (
        ("c444", 31, 43, jpeg_bytes(rgb, quality=90, subsampling=0)),
        ("c422", 31, 43, jpeg_bytes(rgb, quality=90, subsampling=1)),
        ("cmyk", 31, 43, cmyk.getvalue()),
        ("c420_4_columns", 9, 4, jpeg_bytes(texture(9, 4, True), quality=90, subsampling=2)),
        ("twelve_bit", 40, 24, twelve_bit(host_set()[0][4])),
        ("truncated", 48, 64, good[:len(good) * 2 // 3]),
    )


def twelve_bit(data):
    """a frame header that announces 12-bit samples (SOF1, precision 12) in front of an 8-bit file's scans: what the path must refuse from
    the header alone, before the library sees the file"""
    p = data.index(b"\xff\xc0")
    return data[:p + 1] + b"\xc1" + data[p + 2:p + 4] + b"\x0c" + data[p + 5:]
