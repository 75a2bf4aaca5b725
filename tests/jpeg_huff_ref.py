"""The specification of the entropy decoder of Method.jpegDecoder = "device-entropy" (csrc/jpeg_huff_core.h, csrc/jpeg_huff_kernels.hip, the
marker scan vfsms_jpeg_scan in csrc/jpeg_host.cpp), in plain Python and numpy, with no libjpeg: file bytes in, the layout of
vfsms_jpeg_coefficients out.

    file -> parse(): SOI .. SOS: DQT (8- and 16-bit), DHT (counts[16] + values), SOF0 / SOF1 at 8 bits, DRI, ONE SOS holding every component
         -> the entropy-coded data cut at RSTn into segments, FF 00 unstuffed, up to EOI; ceil(MCUs / Ri) segments, or 1 without DRI
         -> per segment the decode step iterated from (p, c, z) = (0, 0, 0) until the segment's blocks are complete
         -> DC differences summed per component per segment (int32 wrap), stored int16; coefficients de-zigzagged onto the block grids

The decode step  (bits, p, c, z) -> (p', c', z', coefficient | None, closed, damage)  is TOTAL: it is defined for every bit pattern and every
state, because the parallel decoder of the device starts its threads at guessed states and must be able to decode rubbish.
    bits past the segment's end read as 1
    z == 0: a DC symbol s (its low 4 bits count) and s more bits -> the difference, z' = 1
    z >= 1: an AC symbol (r, s).  s == 0: r == 15 skips 16 positions, any other r closes the block (EOB).  s > 0: z += r, a coefficient of s
            bits at z, z' = z + 1.  A position beyond 63 (by a run or a skip) closes the block and stores nothing: DAMAGE_INDEX.
    a bit pattern that is no code of the table consumes 16 bits and yields symbol 0: DAMAGE_CODE
    a block closes at z' == 64, at EOB, or by a position beyond 63: c' = (c + 1) mod blocks-per-MCU, z' = 0
The damage bits make a file a damaged one in the TRUE sequential decode only; so does DAMAGE_BITS: the bits of a segment exhausted before its
blocks are complete (a step that starts at or reads beyond the segment's end).  Bits left over are ignored.

sync_rounds() models the parallel scheme of the device in Jacobi rounds (Klein & Wiseman's self-synchronisation, Weissenberger & Schmidt for
JPEG): it documents why the test files of tests/jpeg_huff_cases.py are what they are, and its round counts set VFSMS_JPEG_HUFF_MAX_ROUNDS."""
import functools

import numpy as np

from jpeg_dec_ref import ZIGZAG, block_grid

DAMAGE_CODE, DAMAGE_INDEX, DAMAGE_BITS = 1, 2, 4
_ZZ = [int(v) for v in ZIGZAG]


class Unsupported(Exception):
    """a file this decoder does not take (VFSMS_ERR_UNSUPPORTED)"""


class Damaged(Exception):
    """a file of the kind it takes that cannot be decoded (VFSMS_ERR_BAD_ARG)"""


def _lut(counts, values):
    """16-bit prefix -> (length << 8) | symbol, 0 where the prefix starts no code; None for a table whose codes overflow their length"""
    lut = np.zeros(65536, np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            if code >= (1 << length):
                return None
            lut[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | values[k]
            code += 1
            k += 1
        code <<= 1
    return lut.tolist()


def parse(data):
    """-> dict(h, w, comps = [(hs, vs, quant slot, dc slot, ac slot)], quant = [int64[64] natural order per component],
    dht = {(class, slot): (counts[16], values)}, ri, mcus, blocks_per_mcu, grid = [(block rows, block columns)], segments = [bytes] unstuffed,
    first_mcu = [int]).  Raises Unsupported / Damaged."""
    data = bytes(data)
    if len(data) < 4 or data[:2] != b"\xff\xd8":
        raise Unsupported("no SOI")
    quant, dht, frame, ri, p = {}, {}, None, 0, 2
    while True:
        if p + 4 > len(data):
            raise Damaged("no scan")
        if data[p] != 0xFF:
            raise Damaged("marker expected")
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if 0xD0 <= m <= 0xD7 or m == 0x01:
            p += 2
            continue
        if m in (0xD8, 0xD9):
            raise Damaged("SOI / EOI in front of the scan")
        n = (data[p + 2] << 8) | data[p + 3]
        if n < 2 or p + 2 + n > len(data):
            raise Damaged("segment beyond the file")
        seg = data[p + 4:p + 2 + n]
        if m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                s += 1
                if pq > 1 or tq > 3 or s + (128 if pq else 64) > len(seg):
                    raise Damaged("DQT")
                t = np.zeros(64, np.int64)
                for k in range(64):
                    t[_ZZ[k]] = ((seg[s] << 8) | seg[s + 1]) if pq else seg[s]
                    s += 2 if pq else 1
                quant[tq] = t
        elif m == 0xC4:
            s = 0
            while s < len(seg):
                if s + 17 > len(seg):
                    raise Damaged("DHT")
                tc, th = seg[s] >> 4, seg[s] & 15
                counts = list(seg[s + 1:s + 17])
                nv = sum(counts)
                if tc > 1 or th > 3 or nv > 256 or s + 17 + nv > len(seg):
                    raise Damaged("DHT")
                values = list(seg[s + 17:s + 17 + nv])
                if _lut(counts, values) is None or (tc == 0 and any(v > 15 for v in values)):
                    raise Damaged("DHT: no prefix code")
                dht[(tc, th)] = (counts, values)
                s += 17 + nv
        elif m == 0xDD:
            if n != 4:
                raise Damaged("DRI")
            ri = (seg[0] << 8) | seg[1]
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            if frame is not None:
                raise Unsupported("two frames")
            if m > 0xC1:
                raise Unsupported("not baseline / extended sequential Huffman")
            if n < 8 or n != 8 + 3 * seg[5]:
                raise Damaged("SOF")
            frame = dict(precision=seg[0], h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4],
                         comps=[(seg[6 + 3 * k], seg[7 + 3 * k] >> 4, seg[7 + 3 * k] & 15, seg[8 + 3 * k]) for k in range(seg[5])])
        elif m == 0xDA:
            break
        p += 2 + n
    if frame is None:
        raise Damaged("a scan without a frame")
    if frame["precision"] != 8 or frame["h"] <= 0 or frame["w"] <= 0 or len(frame["comps"]) not in (1, 3):
        raise Unsupported("not 8 bits, 1 or 3 components")
    h, w, nc = frame["h"], frame["w"], len(frame["comps"])
    samp = [(c[1], c[2]) for c in frame["comps"]]
    if nc == 3 and (samp != [(2, 2), (1, 1), (1, 1)] or w < 5 or h < 2):
        raise Unsupported("not 4:2:0")
    if nc == 1 and not (1 <= samp[0][0] <= 2 and 1 <= samp[0][1] <= 2):
        raise Unsupported("sampling factors beyond 2")
    if len(seg) < 1 or seg[0] != nc or len(seg) != 4 + 2 * nc:
        raise Unsupported("several scans")                         # (a scan that does not hold every component)
    comps = []
    for k in range(nc):
        cid, hs, vs, tq = frame["comps"][k]
        if seg[1 + 2 * k] != cid:
            raise Unsupported("scan components out of frame order")
        td, ta = seg[2 + 2 * k] >> 4, seg[2 + 2 * k] & 15
        if tq not in quant or (0, td) not in dht or (1, ta) not in dht:
            raise Unsupported("a table is not defined in front of the scan")
        comps.append((hs, vs, tq, td, ta))
    if tuple(seg[1 + 2 * nc:]) != (0, 63, 0):
        raise Unsupported("not a sequential scan")
    p += 2 + n
    # the entropy-coded data: FF 00 is a data byte FF, FF RSTn ends a segment, FF FF is fill, any other marker ends the scan
    segments, cur, end_marker = [], bytearray(), None
    while p < len(data):
        q = data.find(b"\xff", p)
        if q < 0 or q + 1 >= len(data):
            cur += data[p:]
            p = len(data)
            break
        cur += data[p:q]
        m = data[q + 1]
        if m == 0:
            cur.append(0xFF)
            p = q + 2
        elif m == 0xFF:
            p = q + 1
        elif 0xD0 <= m <= 0xD7:
            if m != 0xD0 + (len(segments) & 7):
                raise Damaged("restart markers out of order")
            segments.append(bytes(cur))
            cur = bytearray()
            p = q + 2
        else:
            end_marker = m
            p = q
            break
    segments.append(bytes(cur))
    if end_marker is None:
        raise Damaged("no EOI")
    if end_marker != 0xD9:
        raise Unsupported("several scans, or tables behind SOS")     # DHT, DQT, SOS, DNL, ... behind the first scan
    grid = block_grid(h, w, [(c[0], c[1], c[2]) for c in comps])
    if nc == 3:
        mcus, bpm = grid[1][0] * grid[1][1], 6
    else:
        mcus, bpm = -(-h // 8) * -(-w // 8), 1
    want = -(-mcus // ri) if ri else 1
    if len(segments) != want:
        raise Damaged("%d segments for %d MCUs at interval %d" % (len(segments), mcus, ri))
    first = [k * ri for k in range(len(segments))]
    return dict(h=h, w=w, comps=comps, quant=[quant[c[2]] for c in comps], dht=dht, ri=ri, mcus=mcus, blocks_per_mcu=bpm, grid=grid,
                segments=segments, first_mcu=first)


class Stream:
    """one segment and the tables of its blocks: what the step function reads"""

    def __init__(self, seg, info):
        self.nbits = 8 * len(seg)
        self.raw = seg + b"\xff" * 8                                 # bits past the end read as 1
        self.bpm = info["blocks_per_mcu"]
        comp_of = (0,) if self.bpm == 1 else (0, 0, 0, 0, 1, 2)
        self.comp_of = comp_of
        luts = {key: _lut(*tab) for key, tab in info["dht"].items()}
        self.dc = [luts[(0, info["comps"][k][3])] for k in comp_of]
        self.ac = [luts[(1, info["comps"][k][4])] for k in comp_of]

    def peek32(self, p):
        if p >= self.nbits:
            return 0xFFFFFFFF
        b = p >> 3
        return (int.from_bytes(self.raw[b:b + 5], "big") >> (8 - (p & 7))) & 0xFFFFFFFF


def step(st, p, c, z):
    """the decode step -> (p', c', z', (z index, value) | None, closed, damage).  Total."""
    v = st.peek32(p)
    e = (st.dc[c] if z == 0 else st.ac[c])[v >> 16]
    damage = 0
    if e:
        length, sym = e >> 8, e & 255
    else:
        length, sym, damage = 16, 0, DAMAGE_CODE
    s = sym & 15
    x = ((v << length) & 0xFFFFFFFF) >> (32 - s) if s else 0
    if s and x < (1 << (s - 1)):
        x -= (1 << s) - 1
    p2 = p + length + s
    coef, closed = None, False
    if z == 0:
        coef, z = (0, x), 1
    else:
        r = sym >> 4
        if s == 0:
            if r == 15:
                z += 16
                if z > 63:
                    damage |= DAMAGE_INDEX
                    closed = True
            else:
                closed = True
        else:
            z += r
            if z > 63:
                damage |= DAMAGE_INDEX
                closed = True
            else:
                coef = (z, x)
                z += 1
                closed = z == 64
    if closed:
        c, z = (c + 1) % st.bpm, 0
    return p2, c, z, coef, closed, damage


def decode_segment(st, nblocks):
    """the true sequential decode: the step iterated from (0, 0, 0) until nblocks are complete -> [(block, z index, value)] with the DC
    DIFFERENCES at index 0, and the damage bits"""
    p = c = z = blk = 0
    out, damage = [], 0
    while blk < nblocks:
        if p >= st.nbits:
            damage |= DAMAGE_BITS
            break
        p, c, z, coef, closed, d = step(st, p, c, z)
        damage |= d
        if damage:
            break                                                   # (what follows damage is not part of any answer)
        if coef is not None:
            out.append((blk, coef[0], coef[1]))
        blk += closed
    if p > st.nbits:
        damage |= DAMAGE_BITS
    return out, damage


def block_place(info, blk):
    """block number in scan order -> (component, block row, block column) on the component's grid"""
    if info["blocks_per_mcu"] == 1:
        bw = -(-info["w"] // 8)
        return 0, blk // bw, blk % bw
    m, c = divmod(blk, 6)
    my, mx = divmod(m, info["grid"][1][1])
    if c < 4:
        return 0, 2 * my + c // 2, 2 * mx + c % 2
    return c - 3, my, mx


def decode(data):
    """file bytes -> (h, w, [(coef int16 (block_rows, block_cols, 64), quant uint16 (64,))]): what _lib.jpeg_coefficients returns"""
    info = parse(data)
    coefs = [np.zeros(g + (64,), np.int16) for g in info["grid"]]
    bpm = info["blocks_per_mcu"]
    for k, seg in enumerate(info["segments"]):
        st = Stream(seg, info)
        m0 = info["first_mcu"][k]
        nm = min(info["ri"], info["mcus"] - m0) if info["ri"] else info["mcus"]
        items, damage = decode_segment(st, nm * bpm)
        if damage:
            raise Damaged("segment %d: damage bits %d" % (k, damage))
        pred = [0, 0, 0]
        for blk, zi, val in items:
            comp, br, bc = block_place(info, m0 * bpm + blk)
            if zi == 0:
                pred[comp] = (pred[comp] + val) & 0xFFFFFFFF           # int32, wrapping
                val = pred[comp]
            coefs[comp][br, bc, _ZZ[zi]] = np.array(val & 0xFFFF, np.uint16).astype(np.int16)
    return info["h"], info["w"], [(coefs[k], info["quant"][k].astype(np.uint16)) for k in range(len(coefs))]


def layout_bytes(decoded):
    """decode()'s answer as the bytes of vfsms_jpeg_coefficients' layout: the tables, then each component's blocks"""
    _, _, comps = decoded
    return b"".join(q.astype("<u2").tobytes() for _, q in comps) + b"".join(c.astype("<i2").tobytes() for c, _ in comps)


# ---- the parallel scheme, as a model ----------------------------------------------------------------------------------------------------------
def _run(st, state, end):
    """decode from `state` until the position reaches `end` -> (exit state, blocks closed)"""
    p, c, z = state
    n = 0
    while p < end:
        p, c, z, _, closed, _ = step(st, p, c, z)
        n += closed
    return (p, c, z), n


@functools.lru_cache(maxsize=None)
def sync_rounds(data, sub_bits):
    """every segment cut into subsequences of sub_bits; subsequence 0 of a segment starts at the true state, every other at the guess
    (its first bit, 0, 0); then Jacobi rounds: a subsequence whose predecessor's exit of the round before differs from its entry takes it and
    decodes again.  -> (rounds in which something changed, subsequences in all, the fixed point equals the sequential decode: bool)"""
    info = parse(data)
    rounds, total, exact = 0, 0, True
    work = []
    for seg in info["segments"]:
        st = Stream(seg, info)
        ns = max(1, -(-st.nbits // sub_bits))
        total += ns
        ends = [min((j + 1) * sub_bits, st.nbits) for j in range(ns)]
        entry = [(j * sub_bits, 0, 0) for j in range(ns)]
        res = [_run(st, entry[j], ends[j]) for j in range(ns)]
        work.append((st, ends, entry, res))
    while True:
        changed = False
        for st, ends, entry, res in work:
            prev = [r[0] for r in res]
            for j in range(1, len(ends)):
                if prev[j - 1] != entry[j]:
                    entry[j] = prev[j - 1]
                    res[j] = _run(st, entry[j], ends[j])
                    changed = True
        if not changed:
            break
        rounds += 1
    for st, ends, entry, res in work:
        state = (0, 0, 0)
        for j in range(len(ends)):
            exact = exact and entry[j] == state
            state, _ = _run(st, state, ends[j])
    return rounds, total, exact
