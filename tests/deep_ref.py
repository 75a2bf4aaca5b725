"""The specification of the 16-bit path (csrc/deep_kernels.hip, include/vfsms.h: vfsms_deep_*), numpy only.

All integer, the project's own, no reference counterpart: every device result must equal these functions exactly.
  window  one intensity window (lo, hi) for a whole dataset, from two order statistics given in parts per million
  reduce  a 16-bit tile -> its 8-bit registration view through that window, rounded to nearest
  mosaic  a 16-bit canvas GATHERED from the tiles that cover each pixel: the sample of the covering tile of the largest index ("paste"),
          or the mean weighted by the distance to the tile's border ("feather", the linear blend of microscopy stitching tools)
"""
import numpy as np

PPM = 1_000_000


def window(tiles, lo_ppm, hi_ppm):
    """-> (lo, hi): s = all samples of all tiles sorted, lo = s[(N - 1) * lo_ppm // 10^6], hi likewise; hi == lo is opened by one level"""
    lo_ppm, hi_ppm = int(lo_ppm), int(hi_ppm)
    if not 0 <= lo_ppm <= hi_ppm <= PPM:
        raise ValueError("0 <= lo_ppm <= hi_ppm <= 1000000")
    hist = np.zeros(65536, np.int64)
    for t in tiles:
        t = np.asarray(t)
        assert t.dtype == np.uint16
        hist += np.bincount(t.reshape(-1), minlength=65536)
    N = int(hist.sum())
    assert N >= 1
    cum = np.cumsum(hist)
    # s[k] = the smallest value v with #{samples <= v} > k
    lo = int(np.searchsorted(cum, (N - 1) * lo_ppm // PPM, side="right"))
    hi = int(np.searchsorted(cum, (N - 1) * hi_ppm // PPM, side="right"))
    if hi == lo:
        if lo < 65535:
            hi = lo + 1
        else:
            lo = hi - 1
    return lo, hi


def reduce(tile, lo, hi):
    """-> uint8: ((clamp(v, lo, hi) - lo) * 255 + D // 2) // D with D = hi - lo"""
    lo, hi = int(lo), int(hi)
    if not 0 <= lo < hi <= 65535:
        raise ValueError("0 <= lo < hi <= 65535")
    D = hi - lo
    v = np.clip(np.asarray(tile).astype(np.int64), lo, hi) - lo
    return ((v * 255 + D // 2) // D).astype(np.uint8)


def weights(h, w, feather):
    """the feather weight of every sample of an h x w tile: d = min(r + 1, h - r, c + 1, w - c), cut at `feather` when it is positive"""
    r = np.arange(h, dtype=np.int64)[:, None]
    c = np.arange(w, dtype=np.int64)[None, :]
    d = np.minimum(np.minimum(r + 1, h - r), np.minimum(c + 1, w - c))
    return np.minimum(d, feather) if feather > 0 else d


def mosaic(tiles, yx, rows, cols, mode, feather=0):
    """-> uint16 [rows][cols]; tile t's top-left corner at yx[t] = (y, x), wholly inside the canvas.  mode 0 paste, 1 feather"""
    if mode not in (0, 1):
        raise ValueError("mode 0 (paste) or 1 (feather)")
    if not 0 <= int(feather) <= 32767:
        raise ValueError("feather 0..32767")
    out = np.zeros((rows, cols), np.uint16)
    sw = np.zeros((rows, cols), np.uint64)
    sp = np.zeros((rows, cols), np.uint64)
    for t, (y, x) in zip(tiles, yx):
        t = np.asarray(t)
        assert t.dtype == np.uint16 and t.ndim == 2
        h, w = t.shape
        y, x = int(y), int(x)
        if y < 0 or x < 0 or y + h > rows or x + w > cols:
            raise ValueError("a tile lies outside the canvas")
        if mode == 0:
            out[y:y + h, x:x + w] = t
        else:
            wg = weights(h, w, int(feather)).astype(np.uint64)
            sw[y:y + h, x:x + w] += wg
            sp[y:y + h, x:x + w] += wg * t.astype(np.uint64)
    if mode == 1:
        m = sw > 0
        out[m] = ((sp[m] + sw[m] // np.uint64(2)) // sw[m]).astype(np.uint16)
    return out


def deepen(tile8, rng):
    """the 16-bit test tile behind an 8-bit one: 2000 + 12 * tile8 + noise in 0..11 (a 12-bit camera's range)"""
    tile8 = np.asarray(tile8)
    return (2000 + 12 * tile8.astype(np.int64) + rng.integers(0, 12, tile8.shape)).astype(np.uint16)
