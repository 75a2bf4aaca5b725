"""The specification of the device's lossless tile coder (Method.pyramidCompression = "deflate-device": TIFF compression 8 with
Predictor = 2), in numpy and the standard library on top of tests/pyramid_ref.py (the levels).  The device's tile streams
(csrc/deflate_kernels.hip over csrc/deflate_core.h) and the bytes PyramidTiffBandWriter stores must equal this file's.

  predict(tile)                        TIFF predictor 2 over a T x T (x ch) tile: per tile row and channel d[c] = p[c] - p[c-1] mod 256
  tokens(data)                         the literal / match tokens of a byte string: ("lit", byte) and ("match", length), all at distance 1
  histogram(toks)                      the counts of the 286 literal/length symbols, end of block included
  code_lengths(counts)                 -> (lengths, halvings): the Huffman lengths, at most 15 bits
  unlimited_depth(counts)              the deepest code of the same construction without the 15-bit limit
  encode(data)                         the zlib stream of a (predicted) byte string: 78 01, ONE final dynamic block, Adler-32
  tile_image(level, ty, tx, T)         the T x T (x ch) pixels of a tile, ZERO beyond the level's last row and column
  tile_streams(img, T, bgr)            the row-major tile streams of an image (B G R when `bgr`, stored R G B)
  file_tiles(img, levels, T)           per level 0 .. levels the row-major list of tile streams: what a file holds

Samples beyond a level's last row or column are 0, as in the "none" and "deflate" writers, so the decoded pages are identical to theirs,
padding included (the JPEG tiles of tests/tiff_jpeg_ref.py replicate the edge instead: zeros would ring into the boundary MCU there; here
they are the cheapest bytes there are).  The predictor is applied after padding, which is what libtiff undoes.

The coder is deflate restricted to what has no serial state: runs at distance 1 (zlib's Z_RLE strategy) and one dynamic Huffman block per
tile.  The token rule is position-local: a byte at offset o >= 1 of a run of n equal bytes has m, i = divmod(o - 1, 258) and
L = min(258, n - 1 - 258 m); with L >= 3 it is the match L when i == 0 and nothing otherwise, with L < 3 it is a literal.  The block's
header has a fixed shape (HLIT = 29, HDIST = 0, HCLEN = 15, the code-length code being the 4-bit code s for s = 0..15), so no second
Huffman stage exists.
"""
import zlib

import numpy as np

import pyramid_ref as P

N_SYMS = 286
END = 256
MAX_BITS = 15
MAX_MATCH = 258
HEADER_BITS = 3 + 5 + 5 + 4 + 19 * 3 + (N_SYMS + 1) * 4

# RFC 1951, 3.2.5: the length symbols 257 .. 285, their base lengths and extra bits
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
# the 3-bit code-length-code lengths are sent in this order (RFC 1951, 3.2.7)
CLEN_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def length_symbol(L):
    """-> (symbol, extra bit count, extra bits' value) of a match length 3 .. 258"""
    assert 3 <= L <= MAX_MATCH
    k = max(i for i in range(29) if LEN_BASE[i] <= L)
    return 257 + k, LEN_EXTRA[k], L - LEN_BASE[k]


def predict(tile):
    tile = np.asarray(tile)
    assert tile.dtype == np.uint8 and tile.ndim in (2, 3)
    d = tile.copy()
    d[:, 1:] = tile[:, 1:] - tile[:, :-1]
    return d


def tokens(data):
    """the sequential parse: maximal runs, the first byte a literal, the rest matches of min(rest, 258) while rest >= 3, then literals"""
    data = bytes(data)
    out, p, n = [], 0, len(data)
    while p < n:
        q = p
        while q < n and data[q] == data[p]:
            q += 1
        out.append(("lit", data[p]))
        rest = q - p - 1
        while rest >= 3:
            L = min(rest, MAX_MATCH)
            out.append(("match", L))
            rest -= L
        out.extend([("lit", data[p])] * rest)
        p = q
    return out


def tokens_local(data):
    """the same tokens by the position-local rule"""
    data = np.frombuffer(bytes(data), np.uint8)
    n = len(data)
    if n == 0:
        return []
    cut = np.flatnonzero(np.r_[True, data[1:] != data[:-1]])
    start = np.repeat(cut, np.diff(np.r_[cut, n]))
    length = np.repeat(np.diff(np.r_[cut, n]), np.diff(np.r_[cut, n]))
    out = []
    for p in range(n):
        o, rl = p - int(start[p]), int(length[p])
        if o == 0:
            out.append(("lit", int(data[p])))
            continue
        m, i = divmod(o - 1, MAX_MATCH)
        L = min(MAX_MATCH, rl - 1 - MAX_MATCH * m)
        if L < 3:
            out.append(("lit", int(data[p])))
        elif i == 0:
            out.append(("match", L))
    return out


def histogram(toks):
    h = [0] * N_SYMS
    for kind, v in toks:
        h[v if kind == "lit" else length_symbol(v)[0]] += 1
    h[END] = 1
    return h


def _depths(counts):
    """the two-queue construction over the used symbols: leaves by (count, symbol); at equal weight a leaf before an internal node, internal
    nodes in creation order -> {symbol: depth}"""
    leaves = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    if not leaves:
        return {}
    if len(leaves) == 1:
        return {leaves[0][1]: 1}
    n = len(leaves)
    weight = [c for c, _ in leaves]
    parent = [0] * (2 * n - 1)
    li, ii = 0, n                                                   # the next leaf, the next internal node
    for node in range(n, 2 * n - 1):
        w = 0
        for _ in range(2):
            if li < n and (ii >= node or weight[li] <= weight[ii]):
                pick = li; li += 1
            else:
                pick = ii; ii += 1
            parent[pick] = node
            w += weight[pick]
        weight.append(w)
    depth = [0] * (2 * n - 1)
    for node in range(2 * n - 3, -1, -1):
        depth[node] = depth[parent[node]] + 1
    return {leaves[k][1]: depth[k] for k in range(n)}


def unlimited_depth(counts):
    d = _depths(counts)
    return max(d.values()) if d else 0


def code_lengths(counts):
    """-> (the 286 lengths, how often the counts were halved to fit 15 bits)"""
    counts = list(counts)
    assert len(counts) == N_SYMS
    halvings = 0
    while True:
        d = _depths(counts)
        if not d or max(d.values()) <= MAX_BITS:
            break
        counts = [(c + 1) >> 1 if c else 0 for c in counts]
        halvings += 1
    lens = [0] * N_SYMS
    for s, k in d.items():
        lens[s] = k
    return lens, halvings


def canonical_codes(lens):
    """RFC 1951, 3.2.2 -> the codes, to be sent from their most significant bit"""
    bl_count = [0] * (MAX_BITS + 2)
    for k in lens:
        bl_count[k] += 1
    bl_count[0] = 0
    code, next_code = 0, [0] * (MAX_BITS + 2)
    for bits in range(1, MAX_BITS + 1):
        code = (code + bl_count[bits - 1]) << 1
        next_code[bits] = code
    out = [0] * len(lens)
    for s, k in enumerate(lens):
        if k:
            out[s] = next_code[k]; next_code[k] += 1
    return out


class _Bits:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, value, nbits):
        """the low `nbits` of value, least significant bit first (header fields, extra bits)"""
        self.acc |= (value & ((1 << nbits) - 1)) << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 255); self.acc >>= 8; self.n -= 8

    def code(self, code, nbits):
        """a Huffman code, most significant bit first"""
        rev = 0
        for b in range(nbits):
            rev |= ((code >> b) & 1) << (nbits - 1 - b)
        self.put(rev, nbits)

    def done(self):
        if self.n:
            self.out.append(self.acc & 255)
        return bytes(self.out)


def block(toks, lens):
    """the one final dynamic block of the tokens under the lengths `lens`"""
    codes = canonical_codes(lens)
    w = _Bits()
    w.put(1, 1); w.put(2, 2); w.put(29, 5); w.put(0, 5); w.put(15, 4)
    for s in CLEN_ORDER:
        w.put(4 if s < 16 else 0, 3)
    for k in list(lens) + [1]:
        w.code(k, 4)
    # every symbol's code as put() takes it: first bit lowest
    first_low = [(int(format(codes[s], "0%db" % lens[s])[::-1], 2), lens[s]) if lens[s] else None for s in range(N_SYMS)]
    for kind, v in toks:
        if kind == "lit":
            w.put(*first_low[v])
        else:
            s, eb, ev = length_symbol(v)
            w.put(*first_low[s]); w.put(ev, eb); w.put(0, 1)
    w.put(*first_low[END])
    return w.done()


def encode(data):
    data = bytes(data)
    assert len(data) >= 1
    toks = tokens(data)
    lens, _ = code_lengths(histogram(toks))
    return b"\x78\x01" + block(toks, lens) + (zlib.adler32(data) & 0xFFFFFFFF).to_bytes(4, "big")


def tile_image(level, ty, tx, T):
    level = np.asarray(level)
    R, C = level.shape[:2]
    assert 0 <= ty * T < R and 0 <= tx * T < C
    out = np.zeros((T, T) + level.shape[2:], np.uint8)
    part = level[ty * T:(ty + 1) * T, tx * T:(tx + 1) * T]
    out[:part.shape[0], :part.shape[1]] = part
    return out


def check_geometry(T, ch):
    if ch not in (1, 3):
        raise ValueError("deflate tiles: 1 or 3 channels, got %d" % ch)
    if T <= 0 or T % 16:
        raise ValueError("deflate tiles: the tile must be a positive multiple of 16, got %d" % T)


def tile_streams(img, T, bgr=True):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim in (2, 3)
    check_geometry(int(T), 1 if img.ndim == 2 else img.shape[2])
    if img.ndim == 3 and bgr:
        img = img[:, :, ::-1]
    R, C = img.shape[:2]
    return [encode(predict(tile_image(img, ty, tx, T)).tobytes()) for ty in range(-(-R // T)) for tx in range(-(-C // T))]


def file_tiles(img, levels, T):
    """img: the mosaic as the canvas holds it (gray, or B G R) -> [level 0's tile streams, ..., level `levels`'s]"""
    img = np.asarray(img)
    return [tile_streams(lv, T, True) for lv in [img] + P.pyramid_levels(img, int(levels))]
