"""The specification of the device JPEG encoder (imagestitch_amd/csrc/jpeg_enc_kernels.hip): libjpeg's baseline encoder with
jpeg_set_defaults + jpeg_set_quality(q, force_baseline) -- what cv2.imwrite and vfsms_jpeg_encode write -- restated in numpy, plus restart
intervals.  tests/test_jpeg_enc_ref.py pins it to the system's libjpeg byte for byte; the device's bytes must equal this file's.

  encode(img, quality=95, restart_mcus=0, bgr=True) -> bytes    a complete file
  header(rows, cols, ch, quality, restart_mcus) -> bytes        SOI .. SOS header
  scan(img, quality, restart_mcus, bgr, mcu_row0=0, mcu_rows=None) -> bytes   the entropy-coded bytes of a range of MCU rows

What libjpeg does, by source file:
  jccolor.c    Y Cb Cr from R G B through 16-bit fixed-point tables
  jcprepct.c   the bottom edge: the image's last row repeated up to an even row count, and -- after downsampling -- every component's last
               row repeated down to its block grid
  jcsample.c   the right edge repeated to the component's block grid; chroma = 2 x 2 box, bias 1, 2, 1, 2 .. along a row
  jccoefct.c   Y blocks of the 16 x 16 MCU grid that lie wholly beyond the Y block grid (an odd number of 8 x 8 blocks in an axis) are DUMMY
               blocks: no AC, the DC of the block in front of them in the MCU -- not replicated samples
  jfdctint.c   the "islow" forward DCT (CONST_BITS 13, PASS1_BITS 2) on samples - 128; output scaled by 8
  jcdctmgr.c   coefficient / (8 * q), rounded half away from zero
  jchuff.c     Annex K tables, DC prediction per component, 0xFF stuffing, the last byte of an interval padded with 1-bits
One rule on restart intervals for every caller: an interval holds at most 65535 MCUs; restart_mcus = 0 is "the image is one interval".
"""
import numpy as np

MAX_SIDE = 65500
MAX_INTERVAL = 65535

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

QT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                    18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

# Annex K: (codes per length 1..16, symbols)
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], list(bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7"
    "c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")))
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], list(bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748494a"
    "535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6"
    "c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")))


def quant_table(base, quality):
    """jpeg_quality_scaling + jpeg_add_quant_table(force_baseline): natural order, 1..255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("jpeg: quality must be 1..100, got %r" % (quality,))
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip((np.asarray(base, np.int64) * scale + 50) // 100, 1, 255)


def huff_codes(table):
    """(bits, vals) -> (code[256], length[256]); length 0 = no such symbol (jchuff.c: jpeg_make_c_derived_tbl)"""
    bits, vals = table
    code_of, len_of = np.zeros(256, np.int64), np.zeros(256, np.int64)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            code_of[vals[k]], len_of[vals[k]] = code, length
            code, k = code + 1, k + 1
        code <<= 1
    return code_of, len_of


def _geometry(rows, cols, ch, restart_mcus):
    """the refusals, then (MCU side, MCUs per row, MCU rows, interval in MCUs)"""
    rows, cols, ch, R = int(rows), int(cols), int(ch), int(restart_mcus)
    if ch not in (1, 3):
        raise ValueError("jpeg: 1 or 3 channels, got %d" % ch)
    if rows < 1 or cols < 1 or rows > MAX_SIDE or cols > MAX_SIDE:
        raise ValueError("jpeg: 1..%d pixels a side, got %d x %d" % (MAX_SIDE, rows, cols))
    if R < 0 or R > MAX_INTERVAL:
        raise ValueError("jpeg: restart_mcus must be 0..%d, got %d" % (MAX_INTERVAL, R))
    mcu = 16 if ch == 3 else 8
    mw, mh = -(-cols // mcu), -(-rows // mcu)
    if R == 0 and mw * mh > MAX_INTERVAL:
        raise ValueError("jpeg: an image of %d MCUs cannot be one restart interval (at most %d)" % (mw * mh, MAX_INTERVAL))
    return mcu, mw, mh, (R if R else mw * mh)


def _seg(marker, payload):
    n = len(payload) + 2
    return bytes([0xFF, marker, n >> 8, n & 255]) + bytes(payload)


def header(rows, cols, ch, quality, restart_mcus):
    """SOI, JFIF APP0, DQT per table, SOF0, DHT per table, DRI (restart_mcus > 0), SOS header: libjpeg's layout byte for byte"""
    _geometry(rows, cols, ch, restart_mcus)
    rows, cols, ch, R = int(rows), int(cols), int(ch), int(restart_mcus)
    out = b"\xFF\xD8" + _seg(0xE0, b"JFIF\0\x01\x01\0\0\x01\0\x01\0\0")
    for k, base in enumerate((QT_LUMA, QT_CHROMA)[:1 if ch == 1 else 2]):
        out += _seg(0xDB, bytes([k]) + bytes(quant_table(base, quality)[ZIGZAG].astype(np.uint8)))
    comps = [(1, 0x11, 0)] if ch == 1 else [(1, 0x22, 0), (2, 0x11, 1), (3, 0x11, 1)]
    out += _seg(0xC0, bytes([8, rows >> 8, rows & 255, cols >> 8, cols & 255, ch]) + b"".join(bytes(c) for c in comps))
    for k, (dc, ac) in enumerate(((DC_LUMA, AC_LUMA), (DC_CHROMA, AC_CHROMA))[:1 if ch == 1 else 2]):
        out += _seg(0xC4, bytes([k]) + bytes(dc[0]) + bytes(dc[1])) + _seg(0xC4, bytes([0x10 | k]) + bytes(ac[0]) + bytes(ac[1]))
    if R:
        out += _seg(0xDD, bytes([R >> 8, R & 255]))
    return out + _seg(0xDA, bytes([ch]) + b"".join(bytes([c[0], c[2] * 0x11]) for c in comps) + b"\0\x3F\0")


# ---- samples ----------------------------------------------------------------------------------------------------------------------------
def _fix(x):
    return int(x * 65536 + 0.5)


def ycc(img, bgr):
    """jccolor.c rgb_ycc_convert -> three int64 planes"""
    a = np.asarray(img).astype(np.int64)
    r, g, b = (a[..., 2], a[..., 1], a[..., 0]) if bgr else (a[..., 0], a[..., 1], a[..., 2])
    half, off = 1 << 15, 128 << 16
    y = (_fix(0.29900) * r + _fix(0.58700) * g + _fix(0.11400) * b + half) >> 16
    cb = (-_fix(0.16874) * r - _fix(0.33126) * g + _fix(0.50000) * b + off + half - 1) >> 16
    cr = (_fix(0.50000) * r - _fix(0.41869) * g - _fix(0.08131) * b + off + half - 1) >> 16
    return y, cb, cr


def _grow(p, rows, cols):
    """edge replication to rows x cols"""
    return np.pad(p, ((0, rows - p.shape[0]), (0, cols - p.shape[1])), mode="edge")


def h2v2(p):
    """jcsample.c h2v2_downsample on a plane of even sides"""
    s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


# ---- transform --------------------------------------------------------------------------------------------------------------------------
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """one pass of jfdctint.c over the LAST axis of d (.., 8)"""
    CB, PB = 13, 2
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., k] for k in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    out = [None] * 8
    if first:
        out[0], out[4] = (t10 + t11) << PB, (t10 - t11) << PB
    else:
        out[0], out[4] = _descale(t10 + t11, PB), _descale(t10 - t11, PB)
    sh = CB - PB if first else CB + PB
    z1 = (t12 + t13) * 4433
    out[2], out[6] = _descale(z1 + t13 * 6270, sh), _descale(z1 - t12 * 15137, sh)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    out[7], out[5], out[3], out[1] = _descale(t4 + z1 + z3, sh), _descale(t5 + z2 + z4, sh), _descale(t6 + z2 + z3, sh), _descale(t7 + z1 + z4, sh)
    return np.stack(out, -1)


def fdct_quant(plane, qt):
    """a plane of whole 8 x 8 blocks -> quantised coefficients (block rows, block cols, 64) in zigzag order"""
    bh, bw = plane.shape[0] // 8, plane.shape[1] // 8
    blk = plane.reshape(bh, 8, bw, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    w = _fdct_pass(blk, True)                                             # rows
    w = _fdct_pass(w.swapaxes(-1, -2), False).swapaxes(-1, -2)            # columns
    w = w.reshape(bh, bw, 64)
    q8 = np.asarray(qt, np.int64) * 8
    mag = (np.abs(w) + (q8 >> 1)) // q8
    return np.where(w < 0, -mag, mag)[..., ZIGZAG]


def mcu_coefficients(img, quality, bgr=True):
    """-> (coefficients (MCU rows, MCUs per row, blocks per MCU, 64) in zigzag order, component of every block of an MCU)"""
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("jpeg: a u8 (h, w) or (h, w, 3) image")
    ch = 1 if img.ndim == 2 else img.shape[2]
    mcu, mw, mh, _ = _geometry(img.shape[0], img.shape[1], ch, 1)
    h, w = img.shape[:2]
    ql, qc = quant_table(QT_LUMA, quality), quant_table(QT_CHROMA, quality)
    if ch == 1:
        return fdct_quant(_grow(img.astype(np.int64), 8 * mh, 8 * mw), ql)[:, :, None, :], [0]
    y, cb, cr = ycc(img, bgr)
    bh, bw = -(-h // 8), -(-w // 8)                                        # the Y block grid: it may end one block short of the MCU grid
    cy = np.zeros((2 * mh, 2 * mw, 64), np.int64)
    cy[:bh, :bw] = fdct_quant(_grow(y, 8 * bh, 8 * bw), ql)
    cy = cy.reshape(mh, 2, mw, 2, 64).transpose(0, 2, 1, 3, 4).reshape(mh, mw, 4, 64).copy()      # MCU order: (0,0) (0,1) (1,0) (1,1) as (row, col)
    if bw < 2 * mw:                                                        # jccoefct.c: dummy blocks at the right edge take the DC in front of them
        cy[:, -1, 1, 0] = cy[:, -1, 0, 0]
        cy[:, -1, 3, 0] = cy[:, -1, 2, 0]
    if bh < 2 * mh:                                                        # .. and a dummy block row the DC of the block in front of the row
        cy[-1, :, 2, :] = 0
        cy[-1, :, 3, :] = 0
        cy[-1, :, 2, 0] = cy[-1, :, 1, 0]
        cy[-1, :, 3, 0] = cy[-1, :, 1, 0]
    h2 = h + (h & 1)
    chroma = [fdct_quant(_grow(h2v2(_grow(p, h2, 16 * mw)), 8 * mh, 8 * mw), qc) for p in (cb, cr)]
    return np.concatenate([cy, chroma[0][:, :, None, :], chroma[1][:, :, None, :]], 2), [0, 0, 0, 0, 1, 2]


# ---- entropy coding ---------------------------------------------------------------------------------------------------------------------
def _bitlen(a):
    n = np.zeros(a.shape, np.int64)
    a = a.copy()
    while True:
        m = a > 0
        if not m.any():
            return n
        n += m
        a >>= 1


def _pack(vals, lens):
    """tokens (value, bit length), MSB first -> bytes; the total is a whole number of bytes"""
    out = []
    cum = np.cumsum(lens)
    assert len(cum) == 0 or cum[-1] % 8 == 0
    step, a = 1 << 22, 0
    while a < len(lens):                                                   # (in pieces, to bound the memory of the per-bit arrays)
        base = cum[a - 1] if a else 0
        b = int(np.searchsorted(cum, base + step, side="left")) + 1
        b = min(b, len(lens))
        while b < len(lens) and cum[b - 1] % 8:
            b += 1
        v, n = vals[a:b], lens[a:b]
        start = np.cumsum(n) - n
        rep = np.repeat(np.arange(len(n)), n)
        idx = np.arange(int(n.sum())) - start[rep]
        out.append(np.packbits(((v[rep] >> (n[rep] - 1 - idx)) & 1).astype(np.uint8)))
        a = b
    return np.concatenate(out) if out else np.zeros(0, np.uint8)


def entropy_code(coef, comp_of_block, interval, first_mcu=0, last=True):
    """coef (MCUs, blocks per MCU, 64): jchuff.c over consecutive MCUs, the first being MCU `first_mcu` of the image (a multiple of
    `interval`) -> bytes, RSTn behind every interval but -- with `last` -- the final one"""
    nm, nb, _ = coef.shape
    assert first_mcu % interval == 0
    comp = np.asarray(comp_of_block)
    dc_tabs = [huff_codes(DC_LUMA), huff_codes(DC_CHROMA)]
    ac_tabs = [huff_codes(AC_LUMA), huff_codes(AC_CHROMA)]
    tab_of_block = (comp > 0).astype(np.int64)
    c = coef.reshape(nm * nb, 64).astype(np.int64)
    N = nm * nb
    mcu_of = np.repeat(np.arange(nm), nb)
    tab = np.tile(tab_of_block, nm)
    # DC differences: per component, predictor 0 at the start of an interval
    diff = np.zeros(N, np.int64)
    cid = np.tile(comp, nm)
    for k in sorted(set(comp_of_block)):
        sel = np.nonzero(cid == k)[0]
        dc = c[sel, 0]
        prev = np.concatenate([[0], dc[:-1]])
        first_of_interval = (mcu_of[sel] % interval == 0) & (np.concatenate([[-1], mcu_of[sel][:-1]]) != mcu_of[sel])
        prev[first_of_interval] = 0
        diff[sel] = dc - prev
    keys, vals, lens = [], [], []

    def magnitude_bits(v):
        s = _bitlen(np.abs(v))
        return s, np.where(v < 0, v - 1, v) & ((1 << s) - 1)

    s, extra = magnitude_bits(diff)
    dcode = np.where(tab == 0, dc_tabs[0][0][s], dc_tabs[1][0][s]); dlen = np.where(tab == 0, dc_tabs[0][1][s], dc_tabs[1][1][s])
    keys.append(np.arange(N) * 256); vals.append((dcode << s) | extra); lens.append(dlen + s)
    bi, ki = np.nonzero(c[:, 1:])
    ki = ki + 1
    prevk = np.zeros(len(ki), np.int64)
    same = np.zeros(len(ki), bool)
    same[1:] = bi[1:] == bi[:-1]
    prevk[1:] = np.where(same[1:], ki[:-1], 0)
    run = ki - prevk - 1
    s, extra = magnitude_bits(c[bi, ki])
    t = tab[bi]
    sym = ((run & 15) << 4) | s
    acode = np.where(t == 0, ac_tabs[0][0][sym], ac_tabs[1][0][sym]); alen = np.where(t == 0, ac_tabs[0][1][sym], ac_tabs[1][1][sym])
    assert (alen > 0).all()
    keys.append(bi * 256 + ki * 2 + 1); vals.append((acode << s) | extra); lens.append(alen + s)
    nz = run >> 4                                                          # ZRL codes in front of the coefficient
    for n in (1, 2, 3):
        m = nz == n
        zc = np.where(t[m] == 0, ac_tabs[0][0][0xF0], ac_tabs[1][0][0xF0]); zl = np.where(t[m] == 0, ac_tabs[0][1][0xF0], ac_tabs[1][1][0xF0])
        v = np.zeros(int(m.sum()), np.int64)
        for _ in range(n):
            v = (v << zl) | zc
        keys.append(bi[m] * 256 + ki[m] * 2); vals.append(v); lens.append(zl * n)
    lastk = np.zeros(N, np.int64)
    np.maximum.at(lastk, bi, ki)
    eb = np.nonzero(lastk < 63)[0]                                         # end of block
    keys.append(eb * 256 + 200); vals.append(np.where(tab[eb] == 0, ac_tabs[0][0][0], ac_tabs[1][0][0])); lens.append(np.where(tab[eb] == 0, ac_tabs[0][1][0], ac_tabs[1][1][0]))
    keys, vals, lens = np.concatenate(keys), np.concatenate(vals), np.concatenate(lens)
    order = np.argsort(keys, kind="stable")
    keys, vals, lens = keys[order], vals[order], lens[order]
    # the intervals: padding with 1-bits to a whole byte
    n_int = -(-nm // interval)
    end_block = np.minimum((np.arange(n_int) + 1) * interval, nm) * nb     # first block behind the interval
    tok_end = np.searchsorted(keys, end_block * 256, side="left")
    cum = np.concatenate([[0], np.cumsum(lens)])
    bits_in = cum[tok_end] - cum[np.concatenate([[0], tok_end[:-1]])]
    pad = (-bits_in) % 8
    vals = np.insert(vals, tok_end, (1 << pad) - 1); lens = np.insert(lens, tok_end, pad)
    raw = _pack(vals, lens)
    nbytes = (bits_in + pad) // 8
    ends = np.cumsum(nbytes)                                               # interval ends in `raw`
    ff = raw == 0xFF
    pos = np.arange(len(raw)) + np.concatenate([[0], np.cumsum(ff)[:-1]]) if len(raw) else np.zeros(0, np.int64)
    stuffed = np.zeros(len(raw) + int(ff.sum()), np.uint8)
    stuffed[pos] = raw
    cumff = np.concatenate([[0], np.cumsum(ff)])
    ends_s = ends + cumff[ends]
    n_mark = n_int - 1 if last else n_int
    idx = first_mcu // interval + np.arange(n_mark)
    marks = np.stack([np.full(n_mark, 0xFF), 0xD0 + (idx & 7)], 1).astype(np.uint8).reshape(-1)
    return np.insert(stuffed, np.repeat(ends_s[:n_mark], 2), marks).tobytes()


def scan(img, quality, restart_mcus, bgr, mcu_row0=0, mcu_rows=None):
    """the entropy-coded bytes of MCU rows [mcu_row0, mcu_row0 + mcu_rows) of `img` (to the last row by default), every interval but the
    IMAGE's last followed by its RSTn.  The MCUs in front of the range must be whole intervals, and so must the range's own unless it
    ends at the last row: then the ranges of an image, one behind the other, are its scan."""
    img = np.asarray(img)
    ch = 1 if img.ndim == 2 else img.shape[2]
    mcu, mw, mh, interval = _geometry(img.shape[0], img.shape[1], ch, restart_mcus)
    r0 = int(mcu_row0)
    n = mh - r0 if mcu_rows is None else int(mcu_rows)
    if r0 < 0 or n < 1 or r0 + n > mh:
        raise ValueError("jpeg: MCU rows [%d, %d) of %d" % (r0, r0 + n, mh))
    last = r0 + n == mh
    if (r0 * mw) % interval or (not last and (n * mw) % interval):
        raise ValueError("jpeg: MCU rows [%d, %d) of %d MCUs each are not whole restart intervals of %d MCUs" % (r0, r0 + n, mw, interval))
    coef, comps = mcu_coefficients(img[r0 * mcu:(r0 + n) * mcu], quality, bgr)          # (every step before the entropy coder is local to an MCU row)
    return entropy_code(coef.reshape(n * mw, len(comps), 64), comps, interval, r0 * mw, last)


def encode(img, quality=95, restart_mcus=0, bgr=True):
    img = np.asarray(img)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError("jpeg: a u8 (h, w) or (h, w, 3) image")
    ch = 1 if img.ndim == 2 else img.shape[2]
    return header(img.shape[0], img.shape[1], ch, quality, restart_mcus) + scan(img, quality, restart_mcus, bgr) + b"\xFF\xD9"
