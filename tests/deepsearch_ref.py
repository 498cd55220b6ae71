"""Plain Python restatement of the wide expectimax of include/g2048_deepsearch.h, written from that
header alone, in Python integers: the slots of the expanded levels with their sentinels, the
sub-search of the frontier and the backups, level by level.

It has no tree arithmetic of its own below the frontier.  The sub-search values are
`search.vmax(slot, sub)` of tests/ntsearch_ref.py's Search (over ntuple_ref.Net for the flat entry
point, over ntstage_ref.StagedNet -- stagesearch_ref.staged_search -- for the staged one), and the
plain recursion this is compared with is that Search's `vafter` under the root formula (`plain`;
`Search.root` itself refuses depth 4).

    d = Deep(search)                              search: an ntsearch_ref.Search
    values, action = d.root(board, depth, top)    the level-wise algorithm; None = illegal
    values, action = d.plain(board, depth)        the recursion, any depth
    d.levels(board, top)                          [level 1 slots, level 2 slots]; None = sentinel
    actions, values = d.root_batch(boards, depth, top)   the library's format (INT64_MIN)
    workspace_bytes(n, top); legal_tops(depth); slot(q, a, tile, cell)

Anchors (asserted by tests/test_deepsearch.py, from the device by tests/test_deepsearch_gpu.py)
---------------------------------------------------------------------------------------------
Spec ((0,),) with lut[i] = 1024 i (ntsearch_ref's anchor table), p(4) = 0.5.  Values in move order
up/down/left/right, - = illegal.
  Board A = [1, 1, 0, ...]: depth 4 and 5 are in the tests as literals beside ntsearch_ref's
    depths 1..3 ([-, 2048, 8192, 8192], [-, 9069, 11400, 11400], [-, 15526, 15865, 15865]).
  Board ONE = [1, 0, ...] (one tile, 15 empty cells): up and left are illegal.
"""
from __future__ import annotations

import numpy as np

import expectimax_ref as E
import ntsearch_ref as S

F = S.F
INT64_MIN = S.INT64_MIN
MAX_DEPTH, MAX_TOP, MAX_SUB = 5, 2, 3
MAX_EXPONENT = 22
FAN = 128        # slots of level j + 1 per slot of level j
SLOT_BYTES = 24  # a 16-byte board and an 8-byte Vmax


def slot(q: int, a: int, tile: int, cell: int) -> int:
    return q * FAN + a * 32 + tile * 16 + cell


def legal_tops(depth: int) -> tuple:
    if not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
    return tuple(t for t in range(MAX_TOP + 1) if 1 <= depth - t <= MAX_SUB)


def workspace_bytes(n: int, top: int) -> int:
    if n < 1 or top not in (0, 1, 2):
        raise ValueError("n >= 1 and top in 0..2")
    return n * SLOT_BYTES * (0, FAN, FAN + FAN * FAN)[top]


class Deep:
    def __init__(self, search: S.Search):
        self.s = search

    def expand(self, nodes):
        """The 128 slots of every node: the spawned boards (bytes), None for a sentinel."""
        out = [None] * (FAN * len(nodes))
        for q, b in enumerate(nodes):
            if b is None:
                continue  # every slot below a sentinel is a sentinel
            for a, after, _gain in self.s.moves(b):
                for c in range(16):
                    if after[c] == 0:
                        for tile in (0, 1):
                            out[slot(q, a, tile, c)] = after[:c] + bytes([tile + 1]) + after[c + 1:]
        return out

    def levels(self, board, top):
        levels, nodes = [], [E._key(board)]
        for _ in range(top):
            nodes = self.expand(nodes)
            levels.append(nodes)
        return levels

    def backup(self, nodes, child_vmax):
        """Per node the four values (None for an illegal move); None for a sentinel node."""
        W, w4 = self.s.W, self.s.w4
        out = []
        for q, b in enumerate(nodes):
            if b is None:
                out.append(None)
                continue
            values = [None] * 4
            for a, after, gain in self.s.moves(b):
                cells = [c for c in range(16) if after[c] == 0]
                total = sum((W - w4) * child_vmax[slot(q, a, 0, c)]
                            + w4 * child_vmax[slot(q, a, 1, c)] for c in cells)
                values[a] = (gain << F) + total // (W * len(cells))  # // floors
            out.append(values)
        return out

    @staticmethod
    def vmax_of(values):
        """Vmax of a max node from its four values: the largest legal one, 0 with none."""
        return max((v for v in values if v is not None), default=0)

    @staticmethod
    def choose(values):
        action, best = 0, None
        for a in range(4):
            if values[a] is not None and (best is None or values[a] > best):
                action, best = a, values[a]
        return values, action

    def plain(self, board, depth):
        """The recursion of the definition at any depth."""
        values = [None] * 4
        for a, after, gain in self.s.moves(E._key(board)):
            values[a] = (gain << F) + self.s.vafter(after, depth - 1)
        return self.choose(values)

    def root(self, board, depth, top):
        if top not in legal_tops(depth):
            raise ValueError(f"top = {top} is no split of depth {depth}")
        if top == 0:
            return self.plain(board, depth)
        sub = depth - top
        levels = [[E._key(board)]] + self.levels(board, top)
        # the sub-search: only slots that are no sentinel are valued
        vmax = [None if b is None else self.s.vmax(b, sub) for b in levels[top]]
        for j in range(top - 1, 0, -1):
            vmax = [None if v is None else self.vmax_of(v) for v in self.backup(levels[j], vmax)]
        return self.choose(self.backup(levels[0], vmax)[0])

    def root_batch(self, boards, depth, top):
        boards = np.asarray(boards, np.uint8).reshape(-1, 16)
        acts = np.zeros(len(boards), np.uint8)
        vals = np.full((len(boards), 4), INT64_MIN, np.int64)
        for i, b in enumerate(boards):
            v, acts[i] = self.root(b, depth, top)
            for k in range(4):
                if v[k] is not None:
                    vals[i, k] = v[k]
        return acts, vals
