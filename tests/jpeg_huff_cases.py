"""The files of the device entropy decoder's tests (tests/test_jpeg_huff_host.py, tests/test_jpeg_huff_gpu.py), made once per process.  Each
is the smallest shape at which something named can go wrong; tests/jpeg_huff_ref.py: sync_rounds says what the parallel scheme makes of them."""
import functools

import numpy as np

import jpeg_dec_cases as D
import jpeg_huff_ref as H

HEADLINE = "gray_512x640_q95"           # about 1830 subsequences of 1024 bits: several workgroups, repair rounds
DENSE = ("dense_64x96_q100_opt", "dense_64x96_q1tables")


@functools.lru_cache(maxsize=None)
def taken_set():
    """((name, h, w, components, bytes), ...): the files the entropy decoder takes"""
    baseline = tuple(c for c in D.host_set() + D.device_extra_set() if "progressive" not in c[0])
    c420 = D.texture(45, 61, True)
    noise = D.bit_noise(64, 96)
    kw = dict(quality=60, subsampling=2)
    return baseline + (
        ("flat_8x8", 8, 8, 1, D.jpeg_bytes(np.full((8, 8), 97, np.uint8), quality=90)),                      # one block
        # DC-only blocks of about 6 bits: well over a hundred blocks in one subsequence, the block-count prefix
        ("flat_64x96", 64, 96, 1, D.jpeg_bytes(np.full((64, 96), 97, np.uint8), quality=90)),
        # dense blocks without end-of-block: the decoders almost never fall in step; optimised tables with long codes; plenty of FF 00
        (DENSE[0], 64, 96, 1, D.jpeg_bytes(noise, quality=100, optimize=True)),
        # the same pixels under a table of ones: a block is longer than a subsequence of 1024 bits
        (DENSE[1], 64, 96, 1, D.jpeg_bytes(noise, qtables=[[1] * 64])),
        # 12 MCUs.  12 segments, each shorter than a subsequence, 11 markers: the RST0-7 cycle wraps
        ("c420_45x61_rst1", 45, 61, 3, D.jpeg_bytes(c420, restart_marker_blocks=1, **kw)),
        ("c420_45x61_rst5", 45, 61, 3, D.jpeg_bytes(c420, restart_marker_blocks=5, **kw)),                   # an interval that does not divide 12
        ("c420_45x61_rstrow", 45, 61, 3, D.jpeg_bytes(c420, restart_marker_rows=1, **kw)),
        ("c420_45x61_opt", 45, 61, 3, D.jpeg_bytes(c420, optimize=True, **kw)),
        ("c420_45x61_plain", 45, 61, 3, D.jpeg_bytes(c420, **kw)),
    )


def texture_set():
    """the taken files the default round bound must take: everything but the two dense files"""
    return tuple(c for c in taken_set() if c[0] not in DENSE)


def two_scans(data):
    """a 4:2:0 baseline file cut into two scans: the scan header rewritten to hold the luma alone, a second scan header for the chroma
    behind the data.  What is decodable does not matter: the file must be refused from its first scan header"""
    p = data.index(b"\xff\xda")
    n = (data[p + 2] << 8) | data[p + 3]
    assert data[p + 4] == 3 and n == 12
    first = b"\xff\xda\x00\x08\x01" + data[p + 5:p + 7] + data[p + 11:p + 14]
    second = b"\xff\xda\x00\x0a\x02" + data[p + 7:p + 11] + data[p + 11:p + 14]
    body = data[p + 2 + n:-2]
    return data[:p] + first + body + second + body + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def refused_set():
    """((name, h, w, bytes), ...): files the entropy decoder must hand back: the refused set of the dct tests, the progressive file, two scans"""
    prog = [c for c in D.host_set() if "progressive" in c[0]][0]
    plain = [c for c in taken_set() if c[0] == "c420_45x61_plain"][0]
    return tuple(D.refused_set()) + ((prog[0], prog[1], prog[2], prog[4]), ("two_scans", 45, 61, two_scans(plain[4])))


def restuff(data, stream):
    """the file `data` with its entropy-coded bytes replaced by `stream` (unstuffed, no restart markers), stuffed again"""
    p = data.index(b"\xff\xda")
    n = (data[p + 2] << 8) | data[p + 3]
    return data[:p + 2 + n] + bytes(stream).replace(b"\xff", b"\xff\x00") + b"\xff\xd9"


@functools.lru_cache(maxsize=None)
def damaged_set():
    """((name, h, w, bytes), ...): damaged files -- each must be refused, never decoded: one truncated at 2 / 3, one with its last restart
    segment removed, and the headline file with 32 bytes of its stream XORed at seeded positions with seeded values, the first seed whose
    corruption the reference reports as damaged"""
    plain = [c for c in taken_set() if c[0] == "c420_45x61_plain"][0][4]
    rst = [c for c in taken_set() if c[0] == "c420_45x61_rst5"][0][4]
    last = rst.rindex(b"\xff\xd1")                                 # 12 MCUs at interval 5: three segments, RST0 and RST1 between them
    assert last > rst.index(b"\xff\xda")
    head = [c for c in taken_set() if c[0] == HEADLINE][0][4]
    stream = H.parse(head)["segments"][0]
    xored = None
    for seed in range(8):
        rng = np.random.default_rng([31, seed])
        s = bytearray(stream)
        for pos, val in zip(rng.integers(0, len(s), 32), rng.integers(1, 256, 32)):
            s[int(pos)] ^= int(val)
        cand = restuff(head, s)
        try:
            H.decode(cand)
        except H.Damaged:
            xored = cand
            break
    assert xored is not None
    return (("truncated", 45, 61, plain[:len(plain) * 2 // 3]), ("last_segment_removed", 45, 61, rst[:last] + b"\xff\xd9"),
            ("xor_512x640", 512, 640, xored))
