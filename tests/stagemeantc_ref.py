"""Plain Python restatement of temporal-coherence learning on the batch-mean rule for the
multi-stage n-tuple network, written from include/g2048_stagemeantc.h alone, in Python integers,
over tests/ntstage_ref.py's StagedNet (stage, raw / val with the fall-through, V, policy, the
stages' sparse dicts) and tests/ntuple_ref.py (delta, the wrap into int32).  The floor division is
ntmean_ref's, the rate and the step's shift are nttc_ref's.

    mt = StagedMeanTC(net, base_ea=None)  net: an ntstage_ref.StagedNet;  mt.E / mt.A: sparse dicts
                                          {(s, t, idx): int}, missing = base_ea(s, t, idx) or (0, 0)
    mt.step(boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)
                                          net.stages[s] gets the promoted and the moved entries,
                                          net.promoted what this step promoted
    mt.last_hits                          {(s, t, idx): (D, C)} of the last step (the library's acc
                                          between its second and third launch)
    mt.last_m                             {(s, t, idx): m} of the last step, m = 0 included

Anchors, computed by hand by composing stagemean_ref's and ntmeantc_ref's (asserted by
tests/test_stagemeantc.py).  The common setup is the spec ((0,),), whose index is the clamped
exponent of one corner, read by two symmetries per corner: a board [x, 0, ...] reads index x twice
and index 0 six times.  Stage 0 is lut0[i] = 1024 * i, the upper stages are UNSET, ea is zero
unless noted.  A = [1, 1, 0, ...]; CB is the checkerboard (no legal move, target 0); Q2 = [2, 0,
...], Q3 = [3, 0, ...].
------------------------------------------------------------------------------------------------
1.  The stage split, three times.  bounds (3,): Q2 is of stage 0 and Q3 of stage 1.  Boards [A, CB,
    CB], prev [Q2, Q3, Q3], has_prev [1, 1, 1], lr = 1 / 2; prev and has_prev are reset before each
    call.
    Call 1 is stagemean_ref's split anchor: delta = [2048, -3072, -3072], hits (0, 0, 2): (4096, 2),
    (0, 0, 0): (12288, 6), (1, 0, 3): (-12288, 4), (1, 0, 0): (-36864, 12); (1, 0, 3) is promoted to
    3072 and (1, 0, 0) to 0.  Every rate is 2^16: lut0[2] = 4096, lut0[0] = 2048, lut1[3] = 0,
    lut1[0] = -3072; ea = (2048, 2048) at both stage-0 entries, (-3072, 3072) at both stage-1
    entries.
    Call 2.  A's left afterstate [2, 0, ...] is of stage 0: q = 4096 + 2 * 4096 + 6 * 2048 = 24576;
    V(Q2) = 2 * 4096 + 6 * 2048 = 20480, err 4096, delta 2048.  CB: V(Q3) = 2 * 0 + 6 * -3072 =
    -18432, err 18432, delta 9216.  Nothing is promoted and |E| = A everywhere, so every rate is
    still 2^16: lut0[2] = 6144, lut0[0] = 4096, lut1[3] = 9216, lut1[0] = 6144; the stage-0 ea is
    (4096, 4096), the stage-1 ea (-3072 + 9216, 3072 + 9216) = (6144, 12288): rate 32768.
    Call 3.  A: q = 4096 + 2 * 6144 + 6 * 4096 = 40960, V(Q2) = 36864, delta 2048.  CB: V(Q3) = 2 *
    9216 + 6 * 6144 = 55296, delta -27648.  Stage 1 moves by (-27648 * 32768) >> 16 = -13824,
    stage 0's index 0 by the full 2048: lut0[2] = 8192, lut0[0] = 6144, lut1[3] = -4608, lut1[0] =
    -7680; ea = (6144, 6144) at stage 0 and (-21504, 39936) at stage 1: rate floor(21504 * 65536 /
    39936) = 35288.  Index 0 runs at two rates in two stages.

2.  A cancelled entry in one stage only.  Call 1 of anchor 1 with ea[(1, 0, 0)] preset to (0, 7):
    (1, 0, 0) is promoted to 0 and stays 0 at rate 0, and its ea becomes (-3072, 3079); (0, 0, 0)
    still moves to 2048.  The other entries are as in call 1.

3.  m = 0.  bounds (2,), so Q2 and Q3 are both of stage 1.  Boards [A, A, CB], prev [Q2, Q2, Q3],
    lr = 1 / 2^12, ea[(1, 0, 0)] preset to (5, 9).  A: left gives [2, 0, ...], q = 4096 + 4096 =
    8192, V(Q2) = 4096, err 4096, delta 1.  CB: err -6144, delta floor(-6144 / 4096) = -2.  Hits
    (1, 0, 2): (4, 4), (1, 0, 0): (12 - 12, 18) = (0, 18), (1, 0, 3): (-4, 2); m = 1, 0, -2.  All
    three entries are promoted, to 2048 / 0 / 3072: lut1[2] = 2049, lut1[0] = 0, lut1[3] = 3070; ea
    = (1, 1) at (1, 0, 2), (-2, 2) at (1, 0, 3), and (1, 0, 0) is still (5, 9).  has_prev ends as
    [1, 1, 0].

4.  Two stages promoted and moved in one call.  stagemean_ref's first anchor (bounds (2, 3), boards
    [CB, A], prev [P1, P2]): the table is as there, ea = (-1024, 1024) at (1, 0, 1) and (1, 0, 0),
    (3072, 3072) at (2, 0, 1) and (2, 0, 0).

5.  ntmeantc_ref's anchors 4 and 5 (the two floors composing at rate 2^15; an A of 41 bits) on a
    two-stage net whose bound (12,) puts every board in stage 0: the same numbers, at (0, t, i).
"""
from __future__ import annotations

import ntmean_ref as MR
import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR


class StagedMeanTC:
    def __init__(self, net: SR.StagedNet, base_ea=None):
        """base_ea: None (zeros) or a callable (s, t, idx) -> (E, A) for entries not yet written."""
        self.net = net
        self.base_ea = base_ea if base_ea is not None else (lambda s, t, i: (0, 0))
        self.E, self.A = {}, {}
        self.last_hits, self.last_m = {}, {}

    def get_ea(self, s: int, t: int, i: int):
        if (s, t, i) in self.A:
            return self.E[(s, t, i)], self.A[(s, t, i)]
        return self.base_ea(s, t, i)

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
        promoted, hits = {}, {}
        for i in range(n):
            if not has_prev[i]:
                continue
            s = net.stage(prev[i])
            for t, idx in net.indices(prev[i]):  # all 8 T pairs, coinciding ones each a hit
                key = (s, t, idx)
                if net.raw(s, t, idx) is None:
                    promoted[key] = net.val(s, t, idx)  # the pre-call table's; the weight only
                if deltas[i] != 0:
                    D, C = hits.get(key, (0, 0))
                    hits[key] = (D + deltas[i], C + 1)
        for (s, t, idx), v in promoted.items():
            net.stages[s][(t, idx)] = v
        moves = {}
        for key, (D, C) in hits.items():
            m = MR.floor_div(D, C)
            moves[key] = m
            if m == 0:
                continue  # keeps its value after promotion, ea untouched
            s, t, idx = key
            e0, a0 = self.get_ea(s, t, idx)
            step = TR.step_of(m, TR.rate(e0, a0))
            net.stages[s][(t, idx)] = NR.wrap32(net.raw(s, t, idx) + step)
            self.E[key], self.A[key] = e0 + m, a0 + abs(m)
        net.promoted = promoted
        self.last_hits, self.last_m = hits, moves
        for i in range(n):
            if legal[i]:
                prev[i] = list(afters[i])
                has_prev[i] = 1
            else:
                has_prev[i] = 0
        return actions, errs, deltas
