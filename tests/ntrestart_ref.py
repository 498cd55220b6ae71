"""Plain Python restatement of the per-board restart pool of include/g2048_ntrestart.h, written
from the definition alone, in Python integers with dicts.

    state = fresh(n, stagger=False)   {"snap": [ {e: (board, score, moves)} per board ],
                                       "valid": [int], "top": [int], "turn": [int]}
    state, board, meta, restored = apply(levels, state, board, meta, clock, done)

`apply` is a pure function: it copies what it changes and returns the new state, the new boards
(a list of 16-lists), the new meta ([scores, starts], as the env's u32 meta[2][n]) and
restored_out.  `clock` is the env's u64 word per 64 boards, `done` what the env's step wrote.
`dense(state)` gives the four state buffers as numpy arrays with the device layout (a slot is 32
bytes: board, u32 score, u32 moves, 8 zero bytes; unset slots are zero).

Anchors, computed by hand (asserted by tests/test_ntrestart.py)
-------------------------------------------------------------
One board, fresh state (top = 0, turn = 0, nothing valid).  B2 = [1, 2, 0, ...] (M = 2),
B2x = [2, 2, 1, 0, ...] (M = 2), B3 = [3, 1, 0, ...] (M = 3), B4 = [4, 0, ...] (M = 4).

Capture.  done = 0, board B2, score 4, start 10, clock 13: M = 2 > top = 0, so slot 2 =
(B2, 4, 13 - 10 = 3), valid = 0b100, top = 2.  A fresh board can start at 2: slot 1 stays unset.
A move raises M by at most one, so no level above the first is skipped.

No re-capture.  Next, done = 0, board B2x, score 8, clock 14: M = 2 is not above top = 2, so
nothing changes: slot 2 still holds B2 with score 4 and 3 moves.

Climb.  Next, done = 0, board B3, score 12, clock 15: slot 3 = (B3, 12, 5), valid = 0b1100,
top = 3.

Restore across a wrap of start.  levels = (0, 3), turn = 1, done = 1, the env has dealt
F = [1, 0, 0, 1, 0, ...] with score 0 and start = now, at clock 2^32 + 2 (now = 2):
e = levels[1 % 2] = 3 is valid, so board = B3, score = 12, start = (2 - 5) mod 2^32 = 4294967293,
moves = (now - start) mod 2^32 = 5, top = 3, restored = 3, turn = 2.  Slot 3 is kept.

Fallback.  The same call with levels = (0, 7): slot 7 is unset, so F, score 0 and start 2 stay,
top = M(F) = 1, restored = 0 and turn is still advanced to 2.  With turn = 0 (e = 0) the same.

L = 1, levels = (0,): a done board changes nothing but top (= M of the fresh board) and turn.

Restore, then climb.  After the restore above (top = 3, start = 4294967293), done = 0, board B4,
score 28, clock 2^32 + 4: M = 4 > 3, so slot 4 = (B4, 28, (4 - 4294967293) mod 2^32 = 7) whatever
it held before, valid gains bit 4, top = 4.

Out of the domain.  A board with a 16 on it is never captured and leaves top alone.
"""
from __future__ import annotations

import numpy as np

LEVELS = 16
MAX_ROTATION = 8
SLOT_BYTES = 32
U32 = 0xFFFFFFFF


def check_levels(levels) -> tuple:
    levels = tuple(int(e) for e in levels)
    if not 1 <= len(levels) <= MAX_ROTATION:
        raise ValueError(f"a rotation holds 1..{MAX_ROTATION} levels")
    if any(not 0 <= e < LEVELS for e in levels):
        raise ValueError(f"levels must be in 0..{LEVELS - 1}")
    return levels


def fresh(n: int, stagger: bool = False) -> dict:
    return {"snap": [{} for _ in range(n)], "valid": [0] * n, "top": [0] * n,
            "turn": [i if stagger else 0 for i in range(n)]}


def apply(levels, state, board, meta, clock, done):
    levels = check_levels(levels)
    n = len(board)
    snap = [dict(s) for s in state["snap"]]
    valid, top, turn = list(state["valid"]), list(state["top"]), list(state["turn"])
    board = [[int(x) for x in b] for b in board]
    score, start = [int(x) & U32 for x in meta[0]], [int(x) & U32 for x in meta[1]]
    restored = [0] * n
    for i in range(n):
        m = max(board[i])
        now = int(clock[i >> 6]) & U32
        if not done[i]:
            if top[i] < m < LEVELS:
                snap[i][m] = (tuple(board[i]), score[i], (now - start[i]) & U32)
                valid[i] |= 1 << m
                top[i] = m
            continue
        e = levels[turn[i] % len(levels)]
        turn[i] = (turn[i] + 1) & U32
        if e != 0 and (valid[i] >> e) & 1:
            b, s, moves = snap[i][e]
            board[i], score[i] = list(b), s
            start[i] = (start[i] - moves) & U32
            top[i] = restored[i] = e
        else:
            top[i] = m
    new = {"snap": snap, "valid": valid, "top": top, "turn": turn}
    return new, board, [score, start], restored


def dense(state) -> dict:
    """The state as numpy arrays with the device layout."""
    n = len(state["valid"])
    snap = np.zeros((n, LEVELS, SLOT_BYTES), np.uint8)
    for i, slots in enumerate(state["snap"]):
        for e, (b, s, moves) in slots.items():
            snap[i, e, :16] = b
            snap[i, e, 16:24] = np.array([s, moves], "<u4").view(np.uint8)
    return {"snap": snap, "valid": np.array(state["valid"], np.uint16),
            "top": np.array(state["top"], np.uint8), "turn": np.array(state["turn"], np.uint32)}


def sparse(arrays) -> dict:
    """dense()'s inverse, for a state whose set slots are exactly its valid bits."""
    snap = np.asarray(arrays["snap"], np.uint8)
    valid = [int(v) & 0xFFFF for v in np.asarray(arrays["valid"]).view(np.uint16)]
    out = []
    for i, v in enumerate(valid):
        slots = {}
        for e in range(LEVELS):
            if (v >> e) & 1:
                s, moves = (int(x) for x in snap[i, e, 16:24].copy().view("<u4"))
                slots[e] = (tuple(int(x) for x in snap[i, e, :16]), s, moves)
        out.append(slots)
    return {"snap": out, "valid": valid,
            "top": [int(x) for x in np.asarray(arrays["top"])],
            "turn": [int(x) & U32 for x in np.asarray(arrays["turn"]).view(np.uint32)]}
