"""The specification of the device half of the JPEG decoder (Method.jpegDecoder = "device"; csrc/jpeg_dec_kernels.hip, the host half in
csrc/jpeg_host.cpp), in numpy and int64: what lies between the entropy decode and the sample planes in libjpeg's default decoder.

    file -> marker walk: SOF (size, sampling factors, table slots), DQT (tables, zig-zag -> natural order)
         -> per component a grid of 8 x 8 blocks of quantised coefficients (the entropy decode: NOT restated here, it stays in libjpeg)
         -> dequantise: coefficient * table entry
         -> jidctint.c, jpeg_idct_islow (JDCT_ISLOW, CONST_BITS = 13, PASS1_BITS = 2): the 1-D transform down every COLUMN of the block,
            every output descaled by 11 bits; then the same transform along every ROW of that result, descaled by 18 bits.
            descale(x, n) = (x + (1 << (n - 1))) >> n, arithmetic shift.  The roundings make the order of the passes part of the result.
         -> + 128, clamp to 0 .. 255, crop the grid to the component's size

libjpeg's zero-AC shortcuts (a column whose AC terms are all zero is DC << PASS1_BITS) are the same values: with x1..x7 = 0 every odd-part
term vanishes and descale((x0 << 13), 11) = x0 << 2 exactly.

Two conditions bound the inputs this specification speaks for; `idct_blocks` asserts them.  libjpeg-turbo's C transform computes in `long`
(64 bits here) and stores the column pass in an int workspace, its SIMD transforms compute in 32 bits and keep the column pass in 16: they
agree -- with each other and with an int32 device kernel -- exactly while
    (a) every intermediate of both passes fits int32, and
    (b) every output of the column pass fits int16.
Coefficients from files are far inside (bit noise at quality 10 and 100: intermediates <= 4.3e8, column outputs <= 5548)."""
import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])

FIX_0_298631336, FIX_0_390180644, FIX_0_541196100, FIX_0_765366865 = 2446, 3196, 4433, 6270
FIX_0_899976223, FIX_1_175875602, FIX_1_501321110, FIX_1_847759065 = 7373, 9633, 12299, 15137
FIX_1_961570560, FIX_2_053119869, FIX_2_562915447, FIX_3_072711026 = 16069, 16819, 20995, 25172
CONST_BITS, PASS1_BITS = 13, 2
INT32_MAX, INT16_MAX = 2 ** 31 - 1, 2 ** 15 - 1


def parse_frame(data):
    """SOI .. the first SOS -> dict(h, w, precision, progressive, comps = [(hs, vs, table slot)], tables = {slot: int64[64] natural order},
    table_bits = {slot: 8 | 16})"""
    assert data[:2] == b"\xff\xd8"
    out = dict(tables={}, table_bits={}, comps=None)
    p = 2
    while p + 4 <= len(data):
        assert data[p] == 0xFF, "marker expected"
        m = data[p + 1]
        if m == 0xFF:
            p += 1
            continue
        if 0xD0 <= m <= 0xD9 or m == 0x01:
            p += 2
            continue
        n = (data[p + 2] << 8) | data[p + 3]
        seg = data[p + 4:p + 2 + n]
        if m == 0xDA:
            break
        if m == 0xDB:
            s = 0
            while s < len(seg):
                pq, tq = seg[s] >> 4, seg[s] & 15
                s += 1
                t = np.zeros(64, np.int64)
                for k in range(64):
                    if pq:
                        t[ZIGZAG[k]] = (seg[s] << 8) | seg[s + 1]
                        s += 2
                    else:
                        t[ZIGZAG[k]] = seg[s]
                        s += 1
                out["tables"][tq] = t
                out["table_bits"][tq] = 16 if pq else 8
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            out.update(precision=seg[0], h=(seg[1] << 8) | seg[2], w=(seg[3] << 8) | seg[4], progressive=m == 0xC2, sof=m,
                       comps=[(seg[6 + 3 * k + 1] >> 4, seg[6 + 3 * k + 1] & 15, seg[6 + 3 * k + 2]) for k in range(seg[5])])
        p += 2 + n
    assert out["comps"] is not None, "no frame header"
    return out


def block_grid(h, w, comps):
    """[(block rows, block columns)] per component: ceil(h * vs / (vmax * 8)) rounded up to a multiple of vs by ceil(w * hs / (hmax * 8))
    rounded up to a multiple of hs -- whole iMCUs"""
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    grid = []
    for hs, vs, _ in comps:
        br, bc = -(-h * vs // (vmax * 8)), -(-w * hs // (hmax * 8))
        grid.append((-(-br // vs) * vs, -(-bc // hs) * hs))
    return grid


def component_size(h, w, comps):
    """[(rows, cols)] of each component's samples: ceil(h * vs / vmax), ceil(w * hs / hmax)"""
    hmax, vmax = max(c[0] for c in comps), max(c[1] for c in comps)
    return [(-(-h * vs // vmax), -(-w * hs // hmax)) for hs, vs, _ in comps]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _pass(x, shift, peak):
    """jpeg_idct_islow's 1-D transform along the last axis of int64 x[..., 8]; peak[0] collects the largest |intermediate|"""
    def see(*vals):
        for v in vals:
            peak[0] = max(peak[0], int(np.abs(v).max()) if v.size else 0)
        return vals[0] if len(vals) == 1 else vals
    z2, z3 = x[..., 2], x[..., 6]
    z1 = see((z2 + z3) * FIX_0_541196100)
    tmp2 = see(z1 + z3 * (-FIX_1_847759065))
    tmp3 = see(z1 + z2 * FIX_0_765366865)
    z2, z3 = x[..., 0], x[..., 4]
    tmp0 = see((z2 + z3) << CONST_BITS)
    tmp1 = see((z2 - z3) << CONST_BITS)
    tmp10, tmp13, tmp11, tmp12 = see(tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2)
    tmp0, tmp1, tmp2, tmp3 = x[..., 7], x[..., 5], x[..., 3], x[..., 1]
    z1, z2, z3, z4 = tmp0 + tmp3, tmp1 + tmp2, tmp0 + tmp2, tmp1 + tmp3
    z5 = see((z3 + z4) * FIX_1_175875602)
    tmp0, tmp1, tmp2, tmp3 = see(tmp0 * FIX_0_298631336, tmp1 * FIX_2_053119869, tmp2 * FIX_3_072711026, tmp3 * FIX_1_501321110)
    z1, z2 = see(z1 * (-FIX_0_899976223), z2 * (-FIX_2_562915447))
    z3 = see(see(z3 * (-FIX_1_961570560)) + z5)
    z4 = see(see(z4 * (-FIX_0_390180644)) + z5)
    tmp0 = see(see(tmp0 + z1) + z3)
    tmp1 = see(see(tmp1 + z2) + z4)
    tmp2 = see(see(tmp2 + z2) + z3)
    tmp3 = see(see(tmp3 + z1) + z4)
    half = 1 << (shift - 1)
    outs = [tmp10 + tmp3, tmp11 + tmp2, tmp12 + tmp1, tmp13 + tmp0, tmp13 - tmp0, tmp12 - tmp1, tmp11 - tmp2, tmp10 - tmp3]
    see(*[o + half for o in outs])
    return np.stack([_descale(o, shift) for o in outs], -1)


def idct_blocks(coef, quant, report=None):
    """coef int[..., 64] (natural order), quant int[64] -> the UNCLAMPED samples int64[..., 8, 8] (level shift included).  Asserts the two
    conditions of this specification; report (a dict) receives the largest intermediate and the largest column-pass output."""
    blk = (np.asarray(coef, np.int64) * np.asarray(quant, np.int64)).reshape(np.shape(coef)[:-1] + (8, 8))       # [row][column]
    peak = [int(np.abs(blk).max()) if blk.size else 0]
    ws = np.swapaxes(_pass(np.swapaxes(blk, -1, -2), CONST_BITS - PASS1_BITS, peak), -1, -2)                      # down the columns
    ws_peak = int(np.abs(ws).max()) if ws.size else 0
    px = _pass(ws, CONST_BITS + PASS1_BITS + 3, peak)                                                           # along the rows
    if report is not None:
        report["intermediate"] = max(report.get("intermediate", 0), peak[0])
        report["column_pass"] = max(report.get("column_pass", 0), ws_peak)
    assert peak[0] <= INT32_MAX, "condition (a): an intermediate of %d does not fit int32" % peak[0]
    assert ws_peak <= INT16_MAX, "condition (b): a column-pass output of %d does not fit int16" % ws_peak
    return px + 128


def idct_plane(coef, quant, rows=None, cols=None, report=None, unclamped=False):
    """coef int[block_rows, block_cols, 64] -> the u8 plane (block_rows * 8, block_cols * 8), cropped to rows x cols when given"""
    coef = np.asarray(coef)
    br, bc = coef.shape[:2]
    px = idct_blocks(coef, quant, report)
    if not unclamped:
        px = np.clip(px, 0, 255).astype(np.uint8)
    plane = px.transpose(0, 2, 1, 3).reshape(br * 8, bc * 8)
    return plane[:rows, :cols]


def decode_planes(coefs, tables, h, w, comps, report=None, unclamped=False):
    """per component (coefs[k] on block_grid's grid, tables[k] its table) -> its sample plane, cropped to component_size"""
    grid, sizes = block_grid(h, w, comps), component_size(h, w, comps)
    planes = []
    for k in range(len(comps)):
        assert tuple(np.shape(coefs[k])) == grid[k] + (64,), (np.shape(coefs[k]), grid[k])
        planes.append(idct_plane(coefs[k], tables[k], sizes[k][0], sizes[k][1], report, unclamped))
    return planes


# ---- inputs for the operator test: the forward DCT in floating point, only to make plausible coefficients (no part of the specification) ----
def forward_dct_quantised(blocks, quant):
    """u8 / int blocks[..., 8, 8] -> round(DCT(block - 128) / quant) as int16[..., 64]"""
    k = np.arange(8)
    c = np.where(k == 0, np.sqrt(1 / 8), np.sqrt(2 / 8))[:, None] * np.cos((2 * k[None, :] + 1) * k[:, None] * np.pi / 16)
    f = c @ (np.asarray(blocks, np.float64) - 128) @ c.T
    q = np.rint(f.reshape(f.shape[:-2] + (64,)) / np.asarray(quant, np.float64))
    return np.clip(q, -32768, 32767).astype(np.int16)


Q50_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
