"""The images tests/test_jpeg_enc_ref.py and tests/test_jpeg_device.py share: five sizes (two odd in both axes: edge replication, dummy
blocks, the bias alternation), six contents, gray and colour."""
import numpy as np

SIZES = [(8, 8), (16, 16), (17, 23), (33, 47), (64, 200)]
CONTENTS = ["noise", "zeros", "full", "ramp", "checker", "flatmix"]
QUALITIES = [50, 95, 100]


def image(content, h, w, ch):
    """u8 (h, w) for ch == 1, else (h, w, 3)"""
    shape = (h, w) if ch == 1 else (h, w, 3)
    rng = np.random.default_rng(1000 * h + w + ch)
    if content == "noise":                                   # long codes, stuffed 0xFF bytes, the largest amplitude categories at q 100
        return rng.integers(0, 256, shape, dtype=np.uint8)
    if content == "zeros":                                   # DC only
        return np.zeros(shape, np.uint8)
    if content == "full":
        return np.full(shape, 255, np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    if content == "ramp":
        g = (xx * 255 // max(w - 1, 1)).astype(np.uint8)
        return g if ch == 1 else np.stack([g, 255 - g, (g // 2 + 17).astype(np.uint8)], -1)
    if content == "checker":                                 # 1-px checkerboard: high frequencies behind long zero runs (ZRL)
        g = (((xx + yy) & 1) * 255).astype(np.uint8)
        return g if ch == 1 else np.stack([g, g, 255 - g], -1)
    if content == "flatmix":                                 # noise with every second 8 x 8 block flat: EOB next to full blocks, DC steps of both signs
        a = rng.integers(0, 256, shape, dtype=np.uint8)
        flat = (((yy >> 3) + (xx >> 3)) & 1).astype(bool)
        level = (((yy >> 3) * 37 + (xx >> 3) * 91) & 255).astype(np.uint8)
        if ch == 1:
            a[flat] = level[flat]
        else:
            a[flat] = level[flat][:, None]
        return a
    raise ValueError(content)


def cases():
    return [(c, h, w, ch) for (h, w) in SIZES for c in CONTENTS for ch in (1, 3)]
