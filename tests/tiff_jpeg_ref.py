"""The specification of JPEG-compressed pyramidal TIFF (Method.pyramidCompression = "jpeg"; TIFF compression 7 with shared tables in
JPEGTables), in numpy on top of tests/pyramid_ref.py (the levels) and tests/jpeg_enc_ref.py (the coder).  The device's tile streams
(csrc/jpeg_enc_kernels.hip in tile order) and the bytes PyramidTiffBandWriter stores must equal this file's.

  tile_image(level, ty, tx, T)                              the T x T (x ch) pixels of tile (ty, tx) of a level
  tables(ch, quality) -> bytes                              the JPEGTables datastream: SOI, DQT .., DHT .., EOI
  tile_stream(tile, quality, restart_mcus, bgr=True)        the abbreviated image datastream of one tile: SOI, SOF0, [DRI], SOS, scan, EOI
  file_tiles(img, levels, T, quality, restart_mcus)         per level 0 .. levels the row-major list of tile streams: what a file holds
  rebuilt(tables_bytes, stream)                             a tile stream with the tables' segments put back behind its SOI: a complete file

Samples beyond a level's last row or column replicate that row or column, also in MCUs that lie wholly outside the level (the "none" and
"deflate" writers pad with zeros; for JPEG that would ring into the boundary MCU and cost bits; readers crop either way).  A tile is a
whole T x T image to the coder: its DC predictors start at 0, its RSTn numbering at 0, and no RSTn follows its last interval.
"""
import numpy as np

import jpeg_enc_ref as J
import pyramid_ref as P


def geometry(T, ch, quality, restart_mcus):
    """the refusals, then (MCUs per tile, MCUs per restart interval)"""
    T, ch, R = int(T), int(ch), int(restart_mcus)
    if ch not in (1, 3):
        raise ValueError("tiff jpeg: 1 or 3 channels, got %d" % ch)
    if T <= 0 or T % 16:
        raise ValueError("tiff jpeg: the tile must be a positive multiple of 16, got %d" % T)
    if R < 0 or R > J.MAX_INTERVAL:
        raise ValueError("tiff jpeg: restart_mcus must be 0..%d, got %d" % (J.MAX_INTERVAL, R))
    J.quant_table(J.QT_LUMA, quality)
    mcu = 16 if ch == 3 else 8
    n = (T // mcu) ** 2
    interval = R if R else n
    if n % interval:
        raise ValueError("tiff jpeg: the %d MCUs of a tile are not a whole number of restart intervals of %d MCUs" % (n, interval))
    if interval > J.MAX_INTERVAL:
        raise ValueError("tiff jpeg: a tile of %d MCUs cannot be one restart interval (at most %d)" % (n, J.MAX_INTERVAL))
    return n, interval


def tile_image(level, ty, tx, T):
    level = np.asarray(level)
    R, C = level.shape[:2]
    assert 0 <= ty * T < R and 0 <= tx * T < C
    rows = np.minimum(ty * T + np.arange(T), R - 1)
    cols = np.minimum(tx * T + np.arange(T), C - 1)
    return np.ascontiguousarray(level[rows][:, cols])


def _segments(data):
    """[(marker, bytes of the whole segment)] of the marker segments in front of the scan (or up to EOI)"""
    assert data[:2] == b"\xFF\xD8"
    out, p = [], 2
    while True:
        assert data[p] == 0xFF
        m = data[p + 1]
        if m == 0xD9:
            return out, p
        n = (data[p + 2] << 8) | data[p + 3]
        out.append((m, data[p:p + 2 + n]))
        p += 2 + n
        if m == 0xDA:
            return out, p


def tables(ch, quality):
    segs, _ = _segments(J.header(16, 16, int(ch), quality, 0))
    return b"\xFF\xD8" + b"".join(s for m, s in segs if m in (0xDB, 0xC4)) + b"\xFF\xD9"


def tile_prefix(T, ch, quality, restart_mcus):
    """SOI, SOF0 (T x T), DRI (restart_mcus > 0), SOS: the same for every tile of a file"""
    geometry(T, ch, quality, restart_mcus)
    segs, _ = _segments(J.header(T, T, int(ch), quality, int(restart_mcus)))
    return b"\xFF\xD8" + b"".join(s for m, s in segs if m in (0xC0, 0xDD, 0xDA))


def tile_stream(tile, quality, restart_mcus, bgr=True):
    tile = np.asarray(tile)
    assert tile.dtype == np.uint8 and tile.ndim in (2, 3) and tile.shape[0] == tile.shape[1]
    ch = 1 if tile.ndim == 2 else tile.shape[2]
    T = tile.shape[0]
    return tile_prefix(T, ch, quality, restart_mcus) + J.scan(tile, quality, int(restart_mcus), bgr) + b"\xFF\xD9"


def rebuilt(tables_bytes, stream):
    """the tile stream as a complete interchange file: the segments of `tables_bytes` behind its SOI"""
    assert tables_bytes[:2] == b"\xFF\xD8" and tables_bytes[-2:] == b"\xFF\xD9" and stream[:2] == b"\xFF\xD8"
    return b"\xFF\xD8" + tables_bytes[2:-2] + stream[2:]


def level_tiles(level, T, quality, restart_mcus, bgr=True):
    """the row-major tile streams of one level"""
    level = np.asarray(level)
    geometry(T, 1 if level.ndim == 2 else level.shape[2], quality, restart_mcus)
    R, C = level.shape[:2]
    return [tile_stream(tile_image(level, ty, tx, T), quality, restart_mcus, bgr) for ty in range(-(-R // T)) for tx in range(-(-C // T))]


def file_tiles(img, levels, T, quality, restart_mcus):
    """img: the mosaic as the canvas holds it (gray, or B G R) -> [level 0's tile streams, ..., level `levels`'s]"""
    img = np.asarray(img)
    return [level_tiles(lv, T, quality, restart_mcus, True) for lv in [img] + P.pyramid_levels(img, int(levels))]
