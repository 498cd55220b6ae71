"""Plain restatement of the on-device player of include/g2048_ntplay.h, in Python integers.

It needs no arithmetic of its own for a move: the policy is tests/ntsearch_ref.py's Search (over
tests/ntuple_ref.py's Net, or over tests/ntstage_ref.py's StagedNet through
tests/stagesearch_ref.py), and the step is the oracle's action-given env step (oracle/oracle2048.c,
the checker of g2048_env_step).  What is this file's own is the latch (fin, result), the
translation between the oracle's moves counter and the library's start row, and the closed form
for a terminal board under NO_AUTORESET, which the header allows the library to take.

    p = Play(search, n, seed, flags, board_offset)   one single-board oracle env per board, so a
                                                     board can leave the loop on its own
    p.set_board(i, board, score, moves)              hand-made states
    p.set_clock(t)
    p.steps(K, depth, closed=True)                   K moves; closed=False steps every move
    p.state()                                        board, meta [2, n] (score, start), ep, clock,
                                                     fin, result as the library leaves them

The closed form.  A terminal board under NO_AUTORESET stays as it is, and every later step ends
its episode again: ep.episodes += 1, ep.moves = (t + 1) - start.  R such steps from clock t are
    result = (episodes + 1, score, (t + 1) - start, max)    if fin == 0, and fin = 1
    ep     = (episodes + R, score, (t + R) - start, max)
all mod 2^32, and the clock is R larger.
"""
from __future__ import annotations

import numpy as np

import ntsearch_ref as S
from oracle import oracle as O

M32 = 0xFFFFFFFF
MAX_DEPTH = 3
MAX_STEPS = 1 << 20


def terminal_tail(ep, score, moves, mx, R):
    """(ep, first) after R steps of a terminal board that is never re-dealt: `moves` is the
    board's count before them; `first` is the ep row of the first of them (what the latch takes)."""
    first = ((ep[0] + 1) & M32, score, (moves + 1) & M32, mx)
    return ((ep[0] + R) & M32, score, (moves + R) & M32, mx), first


class Play:
    def __init__(self, search: S.Search, n: int, seed: int = 0x2048, flags: int = 0,
                 board_offset: int = 0):
        self.search, self.n, self.flags = search, int(n), int(flags)
        self.envs = [O.OracleEnv(1, seed, flags, board_offset + i) for i in range(self.n)]
        self.fin = np.zeros(self.n, np.uint8)
        self.result = np.zeros((self.n, 4), np.uint32)

    def set_board(self, i, board, score=0, moves=0):
        e = self.envs[i]
        e.board[0] = np.asarray(board, np.uint8)
        e.meta[0] = (score, moves)

    def set_clock(self, t):
        for e in self.envs:
            e.clock[0] = t

    def steps(self, K: int, depth: int = 1, closed: bool = True):
        if not 1 <= K <= MAX_STEPS:
            raise ValueError(f"k_steps must be in [1, {MAX_STEPS}]")
        if not 1 <= depth <= MAX_DEPTH:
            raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
        frozen = bool(self.flags & O.NO_AUTORESET)
        for i, e in enumerate(self.envs):
            k = 0
            while k < K:
                b = e.board[0]
                if closed and frozen and O.legal_mask(b) == 0:
                    R = K - k
                    ep, first = terminal_tail([int(x) for x in e.ep[0]], int(e.meta[0, 0]),
                                              int(e.meta[0, 1]), int(b.max()), R)
                    if not self.fin[i]:
                        self.result[i], self.fin[i] = first, 1
                    e.ep[0] = ep
                    e.meta[0, 1] = ep[2]
                    e.clock[0] += np.uint64(R)
                    break
                act = self.search.root(b, depth)[1]
                out = e.step(O.MODE_ACTIONS, actions=[act])
                if out["done"][0] and not self.fin[i]:
                    self.result[i], self.fin[i] = e.ep[0], 1
                k += 1

    def state(self) -> dict:
        board = np.stack([e.board[0] for e in self.envs])
        clocks = [int(e.clock[0]) for e in self.envs]
        score = [int(e.meta[0, 0]) for e in self.envs]
        start = [(t - int(e.meta[0, 1])) & M32 for t, e in zip(clocks, self.envs)]
        return dict(board=board, meta=np.array([score, start], np.uint32),
                    ep=np.stack([e.ep[0] for e in self.envs]),
                    clock=np.array(clocks[::64], np.uint64), fin=self.fin.copy(),
                    result=self.result.copy())
