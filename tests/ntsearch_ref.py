"""Plain Python restatement of the expectimax over the n-tuple network of
include/g2048_ntsearch.h, written from the definition alone, in Python integers.  The network is
tests/ntuple_ref.py's Net, the slide (move, gain, legality) tests/expectimax_ref.py's.

    s = Search(net, p4=0.5)          net: ntuple_ref.Net; values are memoised per board
    values, action = s.root(board, depth)         values[a] None for an illegal move
    actions, values = s.root_batch(boards, depth) the library's output format (INT64_MIN)

Anchors, checked by hand (asserted by tests/test_ntsearch.py)
-------------------------------------------------------------
Board A = [1, 1, 0, ...]: up is illegal; down keeps the two 2s (gain 0), left and right merge
them into a 4 (gain 4, 4 << 10 = 4096).  Values in move order up/down/left/right.

Zero table, TUPLES_2x4, p(4) = 0.5.  Depth 1 is the gain: [-, 0, 4096, 4096].  Depth 2, left:
after = a 4 in cell 0 and 15 empty cells.  With a zero table Vmax(child, 1) is the child's best
gain << 10: a spawned 2 merges with nothing (0); a spawned 4 merges with the 4 of cell 0 iff it
lies in row 0 or column 0 (6 cells, the cells between being empty): 8 << 10 = 8192.  So
left = 4096 + floor(6 * 1 * 8192 / (2 * 15)) = 4096 + 1638 = 5734; right is its mirror image.
Down: after = 2s in cells 12 and 13; every child can merge them (4096), and no child does better
(a spawned 2 next to them still merges only one pair, a spawned 4 merges with nothing), so
down = 0 + floor(15 * 2 * 4096 / 30) = 4096.  Depth 3: [-, 9006, 9152, 9152].

Spec ((0,),), lut[i] = 1024 * i: V(b) = 2048 * (min(b0, 15) + min(b3, 15) + min(b12, 15) +
min(b15, 15)), each corner being read by two symmetries.  Depth 1 (tests/ntuple_ref.py's TD
anchor): [-, 2048, 8192, 8192].  Depth 2 at p(4) = 0.5 [-, 9069, 11400, 11400], at 0.1
[-, 8835, 9598, 9598]; depth 3 [-, 15526, 15865, 15865] and [-, 11652, 11975, 11975].

The same spec with lut[i] = -1000 * i - 7 (negative chance sums, so the floor matters):
V(b) = -2000 * (corner sum) - 56.  Depth 1: down = -2000 * 1 - 56 = -2056, left = 4096 - 4000 - 56
= 40: [-, -2056, 40, 40]; depth 2 [-, -256, 1478, 1478]; depth 3 [-, 4161, 4654, 4654].

The action is 2 in every case above (the tie between left and right goes to the smaller move).

Board N = [1,2,1,2, 2,1,2,1, 1,2,1,2, 2,1,2,0], first table: only down and right are legal and
most children are terminal (Vmax = 0): [-, 10240, -, 10240], [-, 33792, -, 33792],
[-, 53205, -, 53205] at depths 1, 2, 3; action 1.
"""
from __future__ import annotations

import numpy as np

import expectimax_ref as E
import ntuple_ref as N

F = N.F
INT64_MIN = N.INT64_MIN
MAX_DEPTH = 3


class Search:
    def __init__(self, net: N.Net, p4=0.5):
        if p4 not in (0.5, 0.1):
            raise ValueError("p4 must be 0.5 or 0.1")
        self.net = net
        self.W, self.w4 = (2, 1) if p4 == 0.5 else (10, 1)
        self._moves, self._V, self._vmax, self._vafter = {}, {}, {}, {}

    def moves(self, key):
        """[(a, after, gain)] of the legal moves of a board (bytes)."""
        got = self._moves.get(key)
        if got is None:
            got = []
            for a in range(4):
                after, gain = E.move(key, a)
                if bytes(after) != key:
                    got.append((a, bytes(after), gain))
            self._moves[key] = got
        return got

    def V(self, key):
        got = self._V.get(key)
        if got is None:
            got = self._V[key] = self.net.V(key)
        return got

    def vmax(self, key, d):
        got = self._vmax.get((key, d))
        if got is None:
            moves = self.moves(key)
            got = max(((gain << F) + self.vafter(after, d - 1) for _, after, gain in moves),
                      default=0)  # no legal move: the TD target of a terminal board
            self._vmax[(key, d)] = got
        return got

    def vafter(self, key, d):
        if d == 0:
            return self.V(key)
        got = self._vafter.get((key, d))
        if got is None:
            empties = [c for c in range(16) if key[c] == 0]
            total = 0
            for c in empties:
                two = key[:c] + b"\x01" + key[c + 1:]
                four = key[:c] + b"\x02" + key[c + 1:]
                total += (self.W - self.w4) * self.vmax(two, d) + self.w4 * self.vmax(four, d)
            got = total // (self.W * len(empties))  # Python's // floors toward -infinity
            self._vafter[(key, d)] = got
        return got

    def root(self, board, depth):
        if not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
        values = [None] * 4
        for a, after, gain in self.moves(E._key(board)):
            values[a] = (gain << F) + self.vafter(after, depth - 1)
        action, best = 0, None
        for a in range(4):
            if values[a] is not None and (best is None or values[a] > best):
                action, best = a, values[a]
        return values, action

    def leaf_boards(self, board, depth):
        """The afterstates whose V the search of `board` reads, with repetitions: the tree's
        leaves as the kernel walks them (no memo)."""
        out = []

        def after_node(key, d):
            if d == 0:
                out.append(key)
                return
            for c in range(16):
                if key[c] == 0:
                    for e in (b"\x01", b"\x02"):
                        for _, after, _g in self.moves(key[:c] + e + key[c + 1:]):
                            after_node(after, d - 1)

        for _, after, _g in self.moves(E._key(board)):
            after_node(after, depth - 1)
        return out

    def root_batch(self, boards, depth):
        """(actions u8[n], values i64[n, 4]) in the library's output format."""
        boards = np.asarray(boards, np.uint8).reshape(-1, 16)
        acts = np.zeros(len(boards), np.uint8)
        vals = np.full((len(boards), 4), INT64_MIN, np.int64)
        for i, b in enumerate(boards):
            v, acts[i] = self.root(b, depth)
            for k in range(4):
                if v[k] is not None:
                    vals[i, k] = v[k]
        return acts, vals


def root(net, board, depth, p4=0.5):
    return Search(net, p4).root(board, depth)


def root_batch(net, boards, depth, p4=0.5):
    return Search(net, p4).root_batch(boards, depth)
