"""The specification of the device's PNG coder (Method.pngEncoder = "device"), in numpy and the standard library on top of
tests/deflate_ref.py (tokens, code lengths, the dynamic block).  The device's bytes (the PNG kernels and the coder's passes of
csrc/deflate_kernels.hip, over csrc/png_core.h and csrc/deflate_core.h) and the file DevicePngFile writes must equal this file's.

  filter_rows(img)                     (R, 1 + C*ch): per row its filter type (minimum sum of absolutes, ties to the lowest), then its bytes
  segment(data)                        the deflate bytes of one segment: ONE dynamic block, not final, then an empty stored block
  encode(img, S)                       the whole file: signature, IHDR, IDAT(78 01), one IDAT a segment of S rows, IDAT(final + Adler), IEND
  device_payload(img, S, row0, nrows)  the IDAT chunks of a band's segments back to back: what the engine returns for the band
  band_adler(img, row0, nrows)         zlib.adler32 of the band's filtered bytes
  adler_combine, crc_combine           the checksums of A || B from those of A and B (zlib's, which Python does not export)
  check_geometry(S, rows, cols, ch)    what the coder refuses

`img` is in the file's channel order (R G B).  The row above a row is always the raw row above it in the whole image (zeros above row 0),
never a band's or a segment's own first row, so any split into bands and segments filters alike.  A segment carries no zlib header and no
Adler-32; every segment ends on a byte boundary (the empty stored block's 00 00 FF FF), so the segments of a file concatenate into one
deflate stream behind 78 01, which the last IDAT closes with an empty final stored block and the Adler-32 of all filtered bytes.
"""
import struct
import zlib

import numpy as np

import deflate_ref as D

SIGNATURE = b"\x89PNG\r\n\x1a\n"
MAX_SEGMENT_ROWS = 4096
ADLER_MOD = 65521
CRC_POLY = 0xEDB88320


def _paeth(a, b, c):
    """int arrays -> the Paeth predictor: the first of a, b, c nearest to a + b - c"""
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def candidates(x, prev, bpp):
    """the five filtered forms of the raw row x (bytes) given the raw row above -> (5, len) u8"""
    x = np.asarray(x, np.int32); b = np.asarray(prev, np.int32)
    a = np.r_[np.zeros(bpp, np.int32), x[:-bpp]] if len(x) > bpp else np.zeros_like(x)
    c = np.r_[np.zeros(bpp, np.int32), b[:-bpp]] if len(x) > bpp else np.zeros_like(x)
    a, c = a[:len(x)], c[:len(x)]
    return np.stack([x, x - a, x - b, x - ((a + b) >> 1), x - _paeth(a, b, c)]).astype(np.uint8)


def cost(v):
    """the sum of |v| as signed bytes; the byte 128 costs 128"""
    v = np.asarray(v, np.int64)
    return int(np.minimum(v, 256 - v).sum())


def filter_rows(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    R, C = img.shape[:2]
    bpp = 1 if img.ndim == 2 else img.shape[2]
    rows = img.reshape(R, C * bpp)
    out = np.empty((R, 1 + C * bpp), np.uint8)
    prev = np.zeros(C * bpp, np.uint8)
    for r in range(R):
        cand = candidates(rows[r], prev, bpp)
        costs = [cost(cand[t]) for t in range(5)]
        t = costs.index(min(costs))                                 # (the first minimum: ties go to the lowest type)
        out[r, 0] = t; out[r, 1:] = cand[t]
        prev = rows[r]
    return out


def segment(data):
    data = bytes(data)
    assert len(data) >= 1
    toks = D.tokens(data)
    lens, _ = D.code_lengths(D.histogram(toks))
    codes = D.canonical_codes(lens)
    w = D._Bits()
    w.put(0, 1); w.put(2, 2); w.put(29, 5); w.put(0, 5); w.put(15, 4)
    for s in D.CLEN_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for k in list(lens) + [1]:
        w.code(k, 4)
    for kind, v in toks:
        if kind == "lit":
            w.code(codes[v], lens[v])
        else:
            s, eb, ev = D.length_symbol(v)
            w.code(codes[s], lens[s]); w.put(ev, eb); w.put(0, 1)
    w.code(codes[D.END], lens[D.END])
    w.put(0, 3)                                                     # an empty stored block, not final
    return w.done() + b"\x00\x00\xff\xff"


def chunk(tag, data):
    return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)


def check_geometry(S, rows, cols, ch):
    if ch not in (1, 3):
        raise ValueError("png: 1 or 3 channels, got %d" % ch)
    if rows < 1 or cols < 1:
        raise ValueError("png: an image has at least one row and one column, got %d x %d" % (rows, cols))
    if not 1 <= S <= MAX_SEGMENT_ROWS:
        raise ValueError("png: segment_rows must be 1..%d, got %d" % (MAX_SEGMENT_ROWS, S))
    if S * (1 + cols * ch) * 15 >= 1 << 32:
        raise ValueError("png: a segment of %d rows of %d bytes is more than the coder's 32-bit bit counts take" % (S, 1 + cols * ch))


def _rgb(img):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    return img, (1 if img.ndim == 2 else img.shape[2])


def device_payload(img, S, row0=0, nrows=None, filtered=None):
    img, ch = _rgb(img)
    R, C = img.shape[:2]
    nrows = R - row0 if nrows is None else nrows
    check_geometry(int(S), R, C, ch)
    assert row0 % S == 0 and 0 <= row0 and nrows > 0 and row0 + nrows <= R and (nrows % S == 0 or row0 + nrows == R)
    f = filter_rows(img) if filtered is None else filtered
    return b"".join(chunk(b"IDAT", segment(f[r:min(r + S, row0 + nrows)].tobytes())) for r in range(row0, row0 + nrows, S))


def band_adler(img, row0=0, nrows=None, filtered=None):
    f = filter_rows(img) if filtered is None else filtered
    nrows = len(f) - row0 if nrows is None else nrows
    return zlib.adler32(f[row0:row0 + nrows].tobytes()) & 0xFFFFFFFF


def head(rows, cols, ch):
    """what stands in front of the segments: signature, IHDR, and the zlib header in an IDAT of its own"""
    return SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", cols, rows, 8, 0 if ch == 1 else 2, 0, 0, 0)) + chunk(b"IDAT", b"\x78\x01")


def tail(adler):
    """what stands behind them: the final empty stored block with the Adler-32 of all filtered bytes, and IEND"""
    return chunk(b"IDAT", b"\x01\x00\x00\xff\xff" + struct.pack(">I", adler)) + chunk(b"IEND", b"")


def encode(img, S=16):
    img, ch = _rgb(img)
    R, C = img.shape[:2]
    f = filter_rows(img)
    return head(R, C, ch) + device_payload(img, S, filtered=f) + tail(band_adler(img, filtered=f))


def adler_combine(a1, a2, len2):
    """the Adler-32 of A || B from those of A and B and B's length"""
    rem = len2 % ADLER_MOD
    s1, s2 = a1 & 0xFFFF, (a1 >> 16) & 0xFFFF
    t1, t2 = a2 & 0xFFFF, (a2 >> 16) & 0xFFFF
    lo = (s1 + t1 + ADLER_MOD - 1) % ADLER_MOD
    hi = (s2 + t2 + rem * s1 + ADLER_MOD * ADLER_MOD - rem) % ADLER_MOD
    return hi << 16 | lo


def _gf_mul(a, b):
    """a * b in GF(2)[x] / P, reflected: bit 31 is x^0"""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = (b >> 1) ^ (CRC_POLY if b & 1 else 0)
    return p


def _xpow8(n):
    """x^(8 n) mod P"""
    r, sq = 0x80000000, 0x00800000
    while n:
        if n & 1:
            r = _gf_mul(r, sq)
        sq = _gf_mul(sq, sq); n >>= 1
    return r


def crc_combine(c1, c2, len2):
    """the CRC-32 of A || B from those of A and B and B's length"""
    return _gf_mul(_xpow8(len2), c1) ^ c2
