"""The specification of the path registrar's candidate state machine (imagestitch_amd/csrc/grid.hip: Chain::run, Chain::evaluate and the
blind entry point) as a plain Python chain: which (pair, direction, i) attempts go into the next fused
batch, and the selection of results in the reference's candidate order (Stitcher.py:319-351).  tests/test_grid_registrar.py holds
the library's machine to it decision for decision: the same rows, the same attempts in the same order, the same batch count.

It is expressed over `attempts(items)`: items = [(pair, direction, i), ...] -> evaluator rows [status, raw dx, raw dy, votes, nA, nB, ...]
(the layout of vfsms_attempt_eval), and it never imports the library or the package."""
import numpy as np

RESULT_INTS = 6   # status, dx, dy, direction, i, votes


def _rotate(direction, incre):
    direction += incre
    if direction == 5:
        direction = 1
    if direction == 0:
        direction = 4
    return direction


class ChainRef:
    def __init__(self, attempts, shapes, roiRatio=0.2, directIncre=1, window=16):
        self.attempts, self.shapes, self.roiRatio, self.directIncre, self.window = attempts, shapes, roiRatio, directIncre, max(1, int(window))
        self.stats = dict(attempts=0, batches=0)

    # -- candidate order of Stitcher.py:319-351 --------------------------------------------------------------
    def maxI(self):
        return int(np.floor(0.5 / self.roiRatio) + 1) + 1

    def rings(self, d0):
        """[[(direction, i), ...] per i]: each i restarts at d0 and rotates until it is back at d0."""
        out = []
        for i in range(1, self.maxI()):
            ring, d = [], d0
            while True:
                ring.append((d, i))
                d = _rotate(d, self.directIncre)
                if d == d0:
                    break
            out.append(ring)
        return out

    def _attempts(self, items):
        """one fused batch -> [(status, raw_dx, raw_dy, votes)]: an image without keypoints never matches"""
        self.stats["attempts"] += len(items)
        self.stats["batches"] += 1
        return [(bool(r[0]) and r[4] > 0 and r[5] > 0, int(r[1]), int(r[2]), int(r[3])) for r in self.attempts(list(items))]

    def _correct(self, raw, d, i, shapeA, shapeB):
        """Stitcher.py:352-360: ROI-relative vote -> full-tile offset."""
        dx, dy = raw
        if d == 1:
            dx = dx + shapeA[0] - int(i * self.roiRatio * shapeA[0])
        elif d == 2:
            dy = dy + shapeA[1] - int(i * self.roiRatio * shapeA[1])
        elif d == 3:
            dx = dx - (shapeB[0] - int(i * self.roiRatio * shapeB[0]))
        elif d == 4:
            dy = dy - (shapeB[1] - int(i * self.roiRatio * shapeB[1]))
        return dx, dy

    def chain(self, first, last, d_in, memo=None, cache=None, midpath=False, stop_on_fail=False, hint=None):
        """-> (int32[last-first, 6], d_out).

        An attempt is a pure function of (pair, direction, i), so WHICH attempts are evaluated together is free;
        the result is always selected in the reference's candidate order.  What is batched is chosen by a small
        predictor fed with the history of this chain: the length of the run of pairs that kept the direction
        (shooting paths are serpentines: long run, turn, long run, ...) bounds the speculation window, a predicted
        turn gets its whole first candidate ring in one batch, and the ring position that resolved the last turn
        from the same incoming direction bounds the first resolve batch.
        memo: {(k, d): (row, d_next)} and cache: {(k, d, i): attempt} may be shared between chains."""
        memo = {} if memo is None else memo
        cache = {} if cache is None else cache
        out = np.zeros((last - first, RESULT_INTS), np.int32)

        def evaluate(items):
            todo = [it for it in dict.fromkeys(items) if it not in cache and it[0] < last]
            if todo:
                for it, r in zip(todo, self._attempts(todo)):
                    cache[it] = r

        runs, run_len, slow, ring_hint = [], 0, 1, {}
        trans2 = {}                                   # (direction before, direction) -> direction the next turn led to
        prev_d = 0
        if hint is not None and len(hint) and first > 0:
            # a chain that starts inside the path: prime the predictor with the history the predicted directions imply for the pairs
            # before `first` (imagestitch_amd/csrc/grid.hip does the same); bookkeeping only
            hd = int(hint[0])
            for kk in range(min(first, len(hint))):
                nd = int(hint[kk])
                if not (1 <= hd <= 4 and 1 <= nd <= 4):
                    break
                if nd == hd:
                    run_len += 1
                    slow = min(2 * slow, self.window)
                else:
                    runs.append(run_len)
                    run_len, slow = 1, 1
                    trans2[(prev_d, hd)] = nd
                    ring0 = [c[0] for c in self.rings(hd)[0]]
                    if nd in ring0:
                        ring_hint[hd] = ring0.index(nd)
                    prev_d = hd
                hd = nd
            if hd != d_in:                            # entered differently than predicted: no basis
                runs, run_len, slow, ring_hint, trans2, prev_d = [], 0, 1, {}, {}, 0
        d = d_in
        k = first

        def plan(k0, d0, p0):
            """Predicted continuation of the path as one batch (up to `window` attempts): the rest of the current run, the
            candidate ring of the predicted turn up to the direction it led to last time, the following run(s), ..."""
            items, R, rl, cd, cp, kk = [], list(runs), run_len, d0, p0, k0
            while kk < last and len(items) < self.window:
                pred = R[-2] if len(R) >= 2 else None
                if pred is None:
                    break
                remaining = pred - rl
                if remaining < 0:
                    break                                  # this run already outlived the prediction: no basis for a turn, slow start instead
                if remaining >= 1:
                    n = min(remaining, self.window - len(items), last - kk)
                    items += [(kk + t, cd, 1) for t in range(n)]
                    kk += n; rl += n
                    if n < remaining:
                        break
                    continue
                ring = self.rings(cd)[0]
                nd = trans2.get((cp, cd))
                if nd is None or all(c[0] != nd for c in ring):
                    items += [(kk,) + c for c in ring[:ring_hint.get(cd, len(ring) - 1) + 1]]
                    break
                upto = [c[0] for c in ring].index(nd)
                items += [(kk,) + c for c in ring[:upto + 1]]
                R.append(rl); rl = 1
                cp, cd = cd, nd
                kk += 1
            return items

        def plan_hint(k0, d0):
            """The predicted directions as the plan itself: the run at the current direction up to the predicted change, the candidate ring
            of that pair up to the predicted new direction, the next run, ... -- what the history-driven plan arrives at after two
            serpentine periods, available from the first pair on."""
            items, cd, kk = [], d0, k0
            while kk < last and kk < len(hint) and len(items) < self.window:
                hd = int(hint[kk])
                if not 1 <= hd <= 4:
                    break
                ring = self.rings(cd)[0]
                ds = [c[0] for c in ring]
                if hd == cd or hd not in ds:
                    items.append((kk, cd, 1))
                else:
                    items += [(kk,) + c for c in ring[:ds.index(hd) + 1]]
                    cd = hd
                kk += 1
            return items

        while k < last:
            if (k, d) in memo:
                row, d_next = memo[(k, d)]
            else:
                rings = self.rings(d)
                if (k, d, 1) not in cache:
                    items = plan_hint(k, d) if hint is not None and len(hint) else []
                    if not items:
                        items = plan(k, d, prev_d)
                    if not items:                              # no history yet: slow start
                        items = [(kk, d, 1) for kk in range(k, min(k + slow, last)) if (kk, d) not in memo]
                    evaluate(items)
                    if (k, d, 1) not in cache:
                        evaluate([(k, d, 1)])
                found = None
                for ri, ring in enumerate(rings):
                    pos = 0
                    while pos < len(ring) and found is None:
                        if (k,) + ring[pos] not in cache:
                            h = ring_hint.get(d, len(ring) - 1) if ri == 0 else len(ring) - 1
                            stop = max(pos, min(h, len(ring) - 1))
                            evaluate([(k,) + c for c in ring[pos:stop + 1]])
                        st, a, b, v = cache[(k,) + ring[pos]]
                        if st:
                            found = ring[pos] + (a, b, v)
                            if ri == 0:
                                ring_hint[d] = pos
                        pos += 1
                    if found is not None:
                        break
                if found is not None:
                    dd, ii, a, b, v = found
                    dx, dy = self._correct((a, b), dd, ii, self.shapes[k], self.shapes[k + 1])
                    row = np.array([1, dx, dy, dd, ii, v], np.int32)
                    d_next = dd                       # self.direction = localDirection
                else:
                    row = np.array([0, 0, 0, d, 0, 0], np.int32)
                    d_next = d                        # a failed pair leaves self.direction untouched
                memo[(k, d)] = (row, d_next)
            # predictor bookkeeping
            if row[0] and d_next == d:
                run_len += 1
                # a chain that starts in the middle of a path sees a truncated run and a turn soon after: until it has seen two
                # runs, an overshoot past that turn is all waste, so it speculates at most 4 pairs ahead
                slow = min(2 * slow, 4 if (midpath and len(runs) < 2) else self.window)
            elif row[0]:
                runs.append(run_len)
                run_len, slow = 1, 1
                trans2[(prev_d, d)] = d_next
                prev_d = d
            out[k - first] = row
            d = d_next
            k += 1
            if stop_on_fail and not row[0]:
                break                             # flowStitch discards everything behind the first break (Stitcher.py:74-76)
        return out, d

    # -- a chunk entered with an unknown direction (rank > 0 of the pair-sharded form) ------------------------------------------------
    def blind_payload(self, lo, hi, per):
        """-> int32[4 * per * 6 + 4]: the chunk [lo, hi) for each of the four possible incoming directions, then the direction each chain
        ends in -- the payload GridRegistrar.shard_payload gathers."""
        table = np.zeros((4, per, RESULT_INTS), np.int32)
        d_out = np.zeros(4, np.int32)
        memo, cache = {}, {}
        dirs = [1, 2, 3, 4]
        if hi > lo:
            # the incoming direction is unknown here: every chain needs its own first candidate of the first pair, so all four
            # are evaluated as one batch instead of being discovered one chain after the other
            for it, r in zip([(lo, d, 1) for d in dirs], self._attempts([(lo, d, 1) for d in dirs])):
                cache[it] = r
        for d_in in dirs:
            if hi > lo:
                res, dn = self.chain(lo, hi, d_in, memo, cache, midpath=True)
                table[d_in - 1, :hi - lo] = res
            else:
                dn = d_in
            d_out[d_in - 1] = dn
        return np.concatenate([table.reshape(-1), d_out])
