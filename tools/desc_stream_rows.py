"""Window rows that describe_one stages for windows larger than the LDS buffer (win > 123), counted on the host as 8-row strips x 8 over
win: the super-band form (before the stream) against the strip stream (csrc/surf_kernels.hip).  Restates the row runs of
ctx_prepare_area_tab (computeResizeAreaTab: output row dy reads window rows [j0, j0 + n)) and both loops; no GPU needed.

    python tools/desc_stream_rows.py            # a few window sizes, then weighted by the keypoints of a production 409 x 2048 strip
"""
import math
import os
import sys

import numpy as np

DSZ, WBUF, MAX_WIN = 21, 15360, 739
ACC_OFF = WBUF - 441 * 4


def runs(win):
    """(j0, n) of the 21 output rows of window `win`, as ctx_prepare_area_tab builds them"""
    scale = win / DSZ
    isc = int(round(scale))
    if abs(scale - isc) < sys.float_info.epsilon:
        return [(dy * isc, isc) for dy in range(DSZ)]
    out = []
    for dy in range(DSZ):
        f1 = dy * scale
        f2 = f1 + scale
        s1, s2 = math.ceil(f1), math.floor(f2)
        s2 = min(s2, win - 1)
        s1 = min(s1, s2)
        left, right = s1 - f1 > 1e-3, f2 - s2 > 1e-3
        out.append((s1 - 1 if left else s1, (1 if left else 0) + (s2 - s1) + (1 if right else 0)))
    return out


def strips(n):
    return (n + 7) // 8


def superband_rows(win):
    """staged strip rows of the super-band form: super-bands of whole output rows, and bands taller than the buffer in chunks"""
    R = runs(win)
    crows = max(WBUF // win, 1)
    rows, dy = 0, 0
    while dy < DSZ:
        lo, n = R[dy]
        if n <= crows:
            stop = dy + 1
            while stop < DSZ and R[stop][0] + R[stop][1] - lo <= crows:
                stop += 1
            rows += 8 * strips(R[stop - 1][0] + R[stop - 1][1] - lo)
            dy = stop
        else:
            rows += sum(8 * strips(min(crows, n - c)) for c in range(0, n, crows))
            dy += 1
    return rows


def stream_rows(win):
    """staged strip rows of the stream: chunks of whole strips in front of the column sums, every window row once"""
    crows = (ACC_OFF // win) & ~7
    return sum(8 * strips(min(crows, win - c)) for c in range(0, win, crows))


def main():
    for win in (124, 150, 200, 300, 400, 500, 666, 739):
        print("win %3d: super-band %.3f x win, stream %.3f x win" % (win, superband_rows(win) / win, stream_rows(win) / win))
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from oracle import oracle as O
    from imagestitch_amd.synthetic import SyntheticGrid
    O.build()
    k, _ = O.surf_detect_describe(np.ascontiguousarray(SyntheticGrid(10, 9, 2048).tile(0)[-409:, :]))
    wins = np.minimum((21 * (k["size"] * np.float32(1.2) / np.float32(9.0))).astype(np.int64), MAX_WIN)
    wins = wins[wins > 123]
    need = float((wins.astype(np.float64) ** 2).sum())
    sb = float(sum(superband_rows(int(w)) * int(w) for w in wins))
    st = float(sum(stream_rows(int(w)) * int(w) for w in wins))
    print("production 409 x 2048 strip, %d windows > 123 px: samples staged / needed: super-band %.3f, stream %.3f (-%.1f %%)"
          % (len(wins), sb / need, st / need, 100 * (1 - st / sb)))


if __name__ == "__main__":
    main()
