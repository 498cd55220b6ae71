"""Plain Python restatement of temporal-coherence learning on the batch-mean rule, written from
include/g2048_ntmeantc.h alone, in Python integers, over tests/ntuple_ref.py's Net (policy, V, idx,
delta, the table's sparse dict and its wrap into int32).  The floor division is ntmean_ref's, the
rate and the step's shift are nttc_ref's.

    mt = MeanTC(net, base_ea=None)        net: an ntuple_ref.Net;  mt.E / mt.A: sparse dicts
                                          {(t, idx): int}, missing = base_ea(t, idx) or (0, 0)
    mt.step(boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)
    mt.last_hits                          {(t, idx): (D, C)} of the last step (the library's acc
                                          between its second and third launch)
    mt.last_m                             {(t, idx): m} of the last step, m = 0 included

Anchors, computed by hand (asserted by tests/test_ntmeantc.py)
-------------------------------------------------------------
Spec ((0,),), lut[i] = 1024 * i, A = [1, 1, 0, ...], C = the checkerboard (no legal move), P2 =
[2, 0, ...], P3 = [3, 0, ...]: ntmean_ref's boards.  idx(P2, g) = 2 for g = 0 and 4, else 0.

1.  ntmean_ref's three-board anchor from a zero ea.  Boards [A, C, C], prev [P2, P3, P3], lr =
    1 / 2: delta = [2048, -3072, -3072].  Every rate is 65536, so step = m.  Entry 2: (4096, 2), m =
    2048, lut[2] = 4096, ea[2] = (2048, 2048).  Entry 3: (-12288, 4), m = -3072, lut[3] = 0, ea[3] =
    (-3072, 3072).  Entry 0: (-24576, 18), m = -1366, lut[0] = -1366, ea[0] = (-1366, 1366).

2.  The same boards, prev and has_prev = [1, 1, 1] a second time, on the table and the ea that
    anchor 1 left.  After one update every entry has |E| = A, so the rates of this call are still
    65536; the rate below 2^16 is the one entry 0 holds AFTER it.  lut = [-1366, 1024, 4096, 0,
    ...].  Board A: q[down] = 2 * (1024 + 3 * -1366) = -6148, q[left] = q[right] = 4096 + 2 *
    (4096 + 3 * -1366) = 4092, action 2; V(P2) = -4, err = 4096, delta = 2048.  Board C: target
    0, V(P3) = 2 * (0 + 3 * -1366) = -8196, err = 8196, delta = 4098.
      Entry 2: (4096, 2), m = 2048, lut[2] = 6144, ea[2] = (4096, 4096).
      Entry 3: (16392, 4), m = 4098, lut[3] = 4098, ea[3] = (-3072 + 4098, 3072 + 4098) =
      (1026, 7170).
      Entry 0: D = 6 * 2048 + 12 * 4098 = 61464, C = 18: 3414.67, m = 3414, lut[0] = 2048, ea[0] =
      (2048, 4780).
    Now rate(2048, 4780) = floor(2048 * 65536 / 4780) = floor(134217728 / 4780) = 28079
    (4780 * 28079 = 134217620) and rate(1026, 7170) = floor(67239936 / 7170) = 9377.
    A third time: lut = [2048, 1024, 6144, 4098, ...].  Board A: q[left] = 4096 + 2 * (6144 +
    3 * 2048) = 28672, V(P2) = 24576, delta = 2048.  Board C: V(P3) = 2 * (4098 + 6144) = 20484,
    err = -20484, delta = -10242.
      Entry 2: m = 2048 at 65536: lut[2] = 8192, ea[2] = (6144, 6144).
      Entry 3: m = -10242 at 9377: step = (-96039234) >> 16 = -1466, lut[3] = 2632, ea[3] =
      (-9216, 17412).
      Entry 0: D = 6 * 2048 - 12 * 10242 = -110616, C = 18: -6145.33, m = -6146, at 28079: step =
      (-172573534) >> 16 = -2634, lut[0] = -586, ea[0] = (-4098, 10926).

3.  An entry whose errors have cancelled.  ntuple_ref's TD anchor (board A, prev P2, lr = 1 / 2:
    delta 2048, entry 2 has (4096, 2) and entry 0 has (12288, 6), m = 2048 on both) with ea[0]
    preset to (0, 7): rate(0, 7) = 0, step = 0, lut[0] stays 0 -- and ea[0] still becomes
    (2048, 2055).  Entry 2 is fresh: lut[2] = 4096, ea[2] = (2048, 2048).

4.  The two floors compose.  Spec ((0, 1),), lut[33] = lut[5] = 1, else 0; X1 = [1, 2, 0, ...] and
    X2 = X1 with cell 11 = 6 and cell 15 = 5.  The eight symmetries read the cell pairs (0, 1),
    (12, 13), (3, 2), (15, 14), (0, 4), (3, 7), (12, 8), (15, 11): idx(X1, .) = 33, 0, 0, 0, 1, 0, 0,
    0 and idx(X2, .) = 33, 0, 0, 5, 1, 0, 0, 101.  V(X1) = 1, V(X2) = 2.  Boards [C, C], prev
    [X1, X2], lr = 1: delta = [-1, -2].  Entry 33: (D, C) = (-3, 2), m = floor(-3 / 2) = -2; with
    ea[33] preset to (1, 2) its rate is 32768 and step = (-2 * 32768) >> 16 = -1: lut[33] = 0,
    ea[33] = (-1, 4).  (-3 * 32768 >> 16 = -2, then halved, would give -1 too; -3 / 2 * 1 / 2
    rounded once would give -1 or 0.)  Entry 1: (-3, 2), m = -2, fresh: lut[1] = -2.  Entry 0:
    D = 6 * -1 + 4 * -2 = -14, C = 10, m = -2.

5.  An A of more than 16 bits.  Anchor 3 with ea[0] preset to (-3 * 2^38, 2^40 + 12345): A has 41
    bits, s = 25, rate = 49152 (nttc_ref's anchor, 3 / 4); m = 2048, step = (2048 * 49152) >> 16 =
    1536, lut[0] = 1536, ea[0] = (-3 * 2^38 + 2048, 2^40 + 12345 + 2048).
"""
from __future__ import annotations

import ntmean_ref as MR
import nttc_ref as TR
import ntuple_ref as NR


class MeanTC:
    def __init__(self, net: NR.Net, base_ea=None):
        """base_ea: None (zeros) or a callable (t, idx) -> (E, A) for entries not yet written."""
        self.net = net
        self.base_ea = base_ea if base_ea is not None else (lambda t, i: (0, 0))
        self.E, self.A = {}, {}
        self.last_hits, self.last_m = {}, {}

    def get_ea(self, t: int, i: int):
        if (t, i) in self.A:
            return self.E[(t, i)], self.A[(t, i)]
        return self.base_ea(t, i)

    def step(self, boards, prev, has_prev, lr_num: int, lr_shift: int):
        """One step over all boards; prev (list of lists) and has_prev (list) are updated in
        place.  Every read of the table and of (E, A) sees them as they were before the call."""
        net, n = self.net, len(boards)
        actions, errs, deltas, afters, legal = [0] * n, [0] * n, [0] * n, [None] * n, [False] * n
        pol, val = {}, {}  # every read sees the table before the call: equal boards, one evaluation
        for i in range(n):
            b, p = tuple(int(x) for x in boards[i]), tuple(int(x) for x in prev[i])
            if b not in pol:
                pol[b] = net.policy(list(b))
            if has_prev[i] and p not in val:
                val[p] = net.V(list(p))
            q, actions[i], afters[i] = pol[b]
            live = [x for x in q if x is not None]
            legal[i] = bool(live)
            target = max(live) if live else 0
            errs[i] = target - val[p] if has_prev[i] else 0
            deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
        hits = {}
        for i in range(n):
            if has_prev[i] and deltas[i] != 0:
                for key in net.indices(prev[i]):  # all 8 T pairs, coinciding ones each a hit
                    D, C = hits.get(key, (0, 0))
                    hits[key] = (D + deltas[i], C + 1)
        moves = {}
        for key, (D, C) in hits.items():
            m = MR.floor_div(D, C)
            moves[key] = m
            if m == 0:
                continue  # left as it is, ea included
            e0, a0 = self.get_ea(*key)
            step = TR.step_of(m, TR.rate(e0, a0))
            net.touched[key] = NR.wrap32(net.get(*key) + step)
            self.E[key], self.A[key] = e0 + m, a0 + abs(m)
        self.last_hits, self.last_m = hits, moves
        for i in range(n):
            if legal[i]:
                prev[i] = list(afters[i])
                has_prev[i] = 1
            else:
                has_prev[i] = 0
        return actions, errs, deltas
