"""Plain Python restatement of the multi-stage n-tuple network of include/g2048_ntstage.h,
written from the definition alone, in Python integers, on top of tests/ntuple_ref.py (symmetries,
indices, delta) and tests/expectimax_ref.py (the slide).  UNSET is absence.

    net = StagedNet(tuples, bounds, base=None)
                          base: None (every entry UNSET), an int array [S, T, 16^m] in which
                          INT32_MIN stands for UNSET, or a callable (s, t, idx) -> int or None
    net.stage(board); net.raw(s, t, i) -> int or None; net.val(s, t, i)
    net.V(board); net.policy(board) -> (q[4] with None for illegal, action, after)
    net.td_step(boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)

Entries the TD step has written (promoted or added into) live in the sparse dicts
`net.stages[s]` {(t, idx): value}; `net.promoted` {(s, t, idx): value} records what the last
td_step promoted.  `net.set_entries()` lists every (s, t, idx) of the dicts.

Anchors, computed by hand (asserted by tests/test_ntstage.py).  All use the spec ((0,),), whose
index is the clamped exponent of one corner: V(b) = 2 * (val[b0] + val[b3] + val[b12] + val[b15]),
each corner being read by two symmetries.  Stage 0 is lut0[i] = 1024 * i unless stated otherwise.
------------------------------------------------------------------------------------------------
Stage.  bounds (5, 8): a board whose largest exponent is 4 has stage 0, 5 or 7 stage 1, 8 or 17
stage 2.  With no bounds every board has stage 0.

A merge crosses a bound inside policy.  bounds (2,), lut1[2] = 5000 and the rest of stage 1 UNSET.
Board A = [1, 1, 0, ...] has stage 0; up is illegal.
  down   after = two 2-tiles (exponent 1) in cells 12, 13: stage 0, q = 0 + 2 * 1024 = 2048
  left   after = [2, 0, ...]: M = 2 reaches the bound, stage 1.  The corner reads lut1[2] = 5000
         twice, the six other reads find lut1[0] UNSET and fall to lut0[0] = 0:
         q = (4 << 10) + 10000 = 14096            (one table would give 4096 + 4096 = 8192)
  right  the same, 14096: the tie goes to the smaller move, action 2, after = [2, 0, ...].

Three-stage fall-through.  bounds (2, 3); board [3, 0, ...] has stage 2.
  stages 1 and 2 UNSET:                      V = 2 * 3072 + 6 * 0 = 6144
  lut1[3] = 7 set, stage 2 UNSET:            V = 2 * 7 = 14
  also lut2[0] = 5 set (lut2[3] still not):  V = 2 * 7 + 6 * 5 = 44

The same entry promoted at two stages in one call.  bounds (2, 3), stages 1 and 2 UNSET, lr = 1/2.
  board 0 = the checkerboard (no legal move), prev = P1 = [1, 0, 0, 0, 0, 2, 0, ...]   stage 1
  board 1 = A,                                prev = P2 = [1, 0, 0, 0, 0, 3, 0, ...]   stage 2
The tuple does not see cell 5, so P1 and P2 both read index 1 twice and index 0 six times, and
V(P1) = V(P2) = 2048 through the fall-through.
  board 0: target 0, err = -2048, delta = -1024, action 0
  board 1: left gives [2, 0, ...] of stage 1, all of it UNSET before the call: q = 4096 + 4096 =
           8192 (down: 2048), action 2, err = 8192 - 2048 = 6144, delta = 3072
  promoted: (1, 0, 1) and (2, 0, 1) to 1024, (1, 0, 0) and (2, 0, 0) to 0
  after:   lut1[1] = 1024 - 2 * 1024 = -1024     lut1[0] = -6 * 1024 = -6144
           lut2[1] = 1024 + 2 * 3072 = 7168      lut2[0] = 6 * 3072 = 18432
  The stage-2 entries start from val(0, .), not from the stage-1 entries' new values, and board
  1's afterstate read lut1[0] as it was before the call.  Stage 0 is untouched.  Board 0 drops
  has_prev and keeps prev; board 1's prev becomes [2, 0, ...].

Promotion with delta == 0.  bounds (2,), stage 1 UNSET, prev = P1 with has_prev, lr_num = 0 on
board A: err = 6144 but delta = 0.  promoted = {(1, 0, 1): 1024, (1, 0, 0): 0}; these are now set
entries of stage 1 with the values they resolved to, nothing is added and no V changes.  The same
board without has_prev promotes nothing.

A terminal board on a fresh table.  bounds (2,), every entry UNSET, the checkerboard with prev =
[1, 0, ...] and has_prev: target 0, V(prev) = 0, err = delta = 0, action 0.  Stage 0 gets
(0, 0, 1) and (0, 0, 0) promoted to 0 -- the only way a stage-0 entry is ever promoted -- and
has_prev drops to 0 with prev as it was.
"""
from __future__ import annotations

import expectimax_ref as E
import ntuple_ref as NR

F = NR.F
UNSET = -(1 << 31)
MAX_STAGES, MAX_BOUND = 8, 27


class StagedNet:
    def __init__(self, tuples, bounds, base=None):
        self.tuples = tuple(tuple(t) for t in tuples)
        self.bounds = tuple(int(b) for b in bounds)
        if len(self.bounds) > MAX_STAGES - 1:
            raise ValueError("at most 8 stages")
        if any(not 1 <= b <= MAX_BOUND for b in self.bounds):
            raise ValueError("bounds are exponents in 1..27")
        if any(b <= a for a, b in zip(self.bounds, self.bounds[1:])):
            raise ValueError("bounds must be strictly increasing")
        self.S = len(self.bounds) + 1
        self.cells = NR.expand(self.tuples)
        if base is None:
            self.base = lambda s, t, i: None
        elif callable(base):
            self.base = base
        else:
            self.base = lambda s, t, i: None if int(base[s][t][i]) == UNSET else int(base[s][t][i])
        self.stages = [{} for _ in range(self.S)]
        self.promoted = {}

    def stage(self, board) -> int:
        m = max(int(x) for x in board)
        return sum(1 for b in self.bounds if m >= b)

    def raw(self, s: int, t: int, i: int):
        """lut[s][t][i], None for UNSET."""
        got = self.stages[s].get((t, i))
        return self.base(s, t, i) if got is None else got

    def val(self, s: int, t: int, i: int) -> int:
        while s >= 0:
            got = self.raw(s, t, i)
            if got is not None:
                return got
            s -= 1
        return 0

    def indices(self, board):
        """[(t, idx)] over all 8 T pairs (g, t), coinciding ones repeated."""
        return [(t, NR.index(board, cells)) for per_g in self.cells
                for t, cells in enumerate(per_g)]

    def V(self, board) -> int:
        s = self.stage(board)
        return sum(self.val(s, t, i) for t, i in self.indices(board))

    def policy(self, board):
        """(q, action, after): q[a] None for an illegal move; each afterstate at its own stage."""
        b = [int(x) for x in board]
        q, afters = [None] * 4, [None] * 4
        for a in range(4):
            after, gain = E.move(b, a)
            if after != b:
                q[a] = (gain << F) + self.V(after)
                afters[a] = after
        action, best = 0, None
        for a in range(4):
            if q[a] is not None and (best is None or q[a] > best):
                action, best = a, q[a]
        return q, action, (afters[action] if best is not None else b)

    def td_step(self, boards, prev, has_prev, lr_num: int, lr_shift: int):
        """One TD step over all boards; prev (list of lists) and has_prev (list) are updated in
        place.  Every read of the table sees it as it was before the call."""
        n = len(boards)
        actions, errs, deltas, afters, legal = [0] * n, [0] * n, [0] * n, [None] * n, [False] * n
        for i in range(n):
            q, actions[i], afters[i] = self.policy(boards[i])
            live = [x for x in q if x is not None]
            legal[i] = bool(live)
            target = max(live) if live else 0
            errs[i] = target - self.V(prev[i]) if has_prev[i] else 0
            deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
        promoted, adds = {}, {}
        for i in range(n):
            if not has_prev[i]:
                continue
            s = self.stage(prev[i])
            for t, idx in self.indices(prev[i]):
                if self.raw(s, t, idx) is None:
                    promoted[(s, t, idx)] = self.val(s, t, idx)  # the pre-call table's
                if deltas[i] != 0:
                    adds[(s, t, idx)] = adds.get((s, t, idx), 0) + deltas[i]
        for (s, t, idx), v in promoted.items():
            self.stages[s][(t, idx)] = v
        for (s, t, idx), d in adds.items():
            self.stages[s][(t, idx)] = NR.wrap32(self.raw(s, t, idx) + d)
        self.promoted = promoted
        for i in range(n):
            if legal[i]:
                prev[i] = list(afters[i])
                has_prev[i] = 1
            else:
                has_prev[i] = 0
        return actions, errs, deltas

    def set_entries(self):
        """Every (s, t, idx) the TD steps have written."""
        return [(s, t, i) for s in range(self.S) for (t, i) in self.stages[s]]
