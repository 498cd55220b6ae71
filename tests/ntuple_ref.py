"""Plain Python restatement of the n-tuple network of include/g2048_ntuple.h, written from the
definition alone, in Python integers; table additions are reduced mod 2^32 into int32.  The slide
(move, gain, legality) is tests/expectimax_ref.py's.

    net = Net(tuples, base=None)     base: None (a zero table), an int array [T, 16^m], or a
                                     callable (t, idx) -> int (entries fetched on demand)
    net.V(board); net.policy(board) -> (q[4] with None for illegal, action, after)
    net.td_step(boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)

Entries the TD step has written live in the sparse dict `net.touched` {(t, idx): value}.

Anchors, computed by hand (asserted by tests/test_ntuple.py)
-----------------------------------------------------------
Symmetry g = 4 tr + 2 fc + fr.  The cell that g reads for cell 0: g = 0..7 -> 0, 12, 3, 15, 0, 3,
12, 15.  The tuple (0, 1, 2, 3) becomes (12, 13, 14, 15) under g = 1, (3, 2, 1, 0) under g = 2,
(0, 4, 8, 12) under g = 4 and (15, 11, 7, 3) under g = 7.

Index.  Board A = [1, 1, 0, ...], tuple (0, 1, 2, 3), g = 0: 1 + (1 << 4) = 17.  A board that
starts 17, 16, 15, 3: the first three clamp to 15, so 15 + 15 * 16 + 15 * 256 + 3 * 4096 = 16383.

Value.  Spec ((0,),) with lut[i] = i: V(b) = 2 * (min(b0, 15) + min(b3, 15) + min(b12, 15) +
min(b15, 15)), each corner being read by two symmetries.  D = [11, 10, 9, 8, 4, 5, 6, 7, 3, 2, 1,
1, 0, 0, 0, 0] gives 2 * (11 + 8) = 38; with a 17 in cell 0 it gives 2 * (15 + 8) = 46.

Policy.  A zero table on A: up is illegal, down gains 0, left and right merge the two 2s into a 4:
q = [None, 0, 4 << 10, 4 << 10], the tie goes to the smaller move, action 2, after = [2, 0, ...].
The checkerboard has no legal move: action 0 and after = the board.

TD step.  Spec ((0,),), lut[i] = 1024 * i, board A, prev = [2, 0, ...], has_prev = 1, lr = 1 / 2:
  q[down]  = 0 + V(two 2s in cells 12, 13)    = 1024 * 2 * 1          = 2048
  q[left]  = (4 << 10) + V(a 4 in cell 0)     = 4096 + 1024 * 2 * 2   = 8192
  q[right] = (4 << 10) + V(a 4 in cell 3)     = 8192, so action 2 and target 8192
  V(prev) = 1024 * 2 * 2 = 4096, err = 4096, delta = 4096 >> 1 = 2048
  idx(prev, g) = 2 for g = 0 and 4, else 0: lut[2] = 2048 + 2 * 2048 = 6144, lut[0] = 6 * 2048 =
  12288; prev becomes [2, 0, ...] and has_prev stays 1.
The shift floors: err = -3 at lr = 1 / 2 gives delta = -2.
"""
from __future__ import annotations

import expectimax_ref as E

F = 10
INT64_MIN = -(1 << 63)
TUPLES_4x6 = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))
TUPLES_2x4 = ((0, 1, 2, 3), (0, 1, 4, 5))


def wrap32(x: int) -> int:
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def source_cell(cell: int, g: int) -> int:
    """The cell of b that g(b)[cell] reads."""
    tr, fc, fr = g >> 2, (g >> 1) & 1, g & 1
    r, c = cell >> 2, cell & 3
    r = 3 - r if fr else r
    c = 3 - c if fc else c
    return 4 * c + r if tr else 4 * r + c


def transform(board, g: int):
    """g(b) as a list of 16 exponents."""
    return [int(board[source_cell(cell, g)]) for cell in range(16)]


def expand(tuples):
    """[g][t][k]: the cell of b that symmetry g reads for position k of tuple t."""
    return [[[source_cell(c, g) for c in cells] for cells in tuples] for g in range(8)]


def index(board, cells) -> int:
    return sum(min(int(board[c]), 15) << (4 * k) for k, c in enumerate(cells))


def delta_of(err: int, lr_num: int, lr_shift: int) -> int:
    return wrap32((err * lr_num) >> lr_shift)  # Python's >> floors


class Net:
    def __init__(self, tuples, base=None):
        self.tuples = tuple(tuple(t) for t in tuples)
        self.cells = expand(self.tuples)
        if base is None:
            self.base = lambda t, i: 0
        elif callable(base):
            self.base = base
        else:
            self.base = lambda t, i: int(base[t][i])
        self.touched = {}

    def get(self, t: int, i: int) -> int:
        got = self.touched.get((t, i))
        return self.base(t, i) if got is None else got

    def indices(self, board):
        """[(t, idx)] over all 8 T pairs (g, t), coinciding ones repeated."""
        return [(t, index(board, cells)) for per_g in self.cells for t, cells in enumerate(per_g)]

    def V(self, board) -> int:
        return sum(self.get(t, i) for t, i in self.indices(board))

    def policy(self, board):
        """(q, action, after): q[a] None for an illegal move."""
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
            deltas[i] = delta_of(errs[i], lr_num, lr_shift)
        adds = {}
        for i in range(n):
            if has_prev[i] and deltas[i] != 0:
                for key in self.indices(prev[i]):
                    adds[key] = adds.get(key, 0) + deltas[i]
        for (t, idx), d in adds.items():
            self.touched[(t, idx)] = wrap32(self.get(t, idx) + d)
        for i in range(n):
            if legal[i]:
                prev[i] = list(afters[i])
                has_prev[i] = 1
            else:
                has_prev[i] = 0
        return actions, errs, deltas
