"""Plain Python restatement of the expectimax search of include/g2048_search.h, written from the
definition alone, in Python integers, so nothing can overflow -- the slide is its own too (the CPU
oracle's merge gain is a uint32); tests/test_search.py checks it against oracle.oracle.move.

    values, action = expectimax(board, depth, weights=DEFAULT, p4=0.5)

`board` is 16 log2 exponents, row-major; `values` holds None for an illegal move (the library
writes INT64_MIN there).
"""
from __future__ import annotations

from collections import namedtuple
from functools import lru_cache

import numpy as np

Weights = namedtuple("Weights", "gain empty smooth mono corner lost")
DEFAULT = Weights(256, 2048, 256, 1024, 512, 1000000)
INT64_MIN = -(1 << 63)

ROWS = [[4 * r + c for c in range(4)] for r in range(4)]
COLS = [[4 * r + c for r in range(4)] for c in range(4)]
LINES = ROWS + COLS
CORNERS = (0, 3, 12, 15)


# the cells of each move's four lines, in the direction the tiles travel (front first)
MOVE_LINES = ([[4 * k + j for k in range(4)] for j in range(4)],        # up
              [[4 * (3 - k) + j for k in range(4)] for j in range(4)],  # down
              [[4 * j + k for k in range(4)] for j in range(4)],        # left
              [[4 * j + 3 - k for k in range(4)] for j in range(4)])    # right


def _key(board):
    return bytes(int(x) for x in board)


@lru_cache(maxsize=None)
def slide_line(cells):
    """Four exponents (a tuple), front first -> (slid line, gain): tiles travel to the front, equal
    neighbours merge once, front first; the gain is the value of every tile a merge creates."""
    tiles = [x for x in cells if x]
    out, gain, k = [], 0, 0
    while k < len(tiles):
        if k + 1 < len(tiles) and tiles[k] == tiles[k + 1]:
            out.append(tiles[k] + 1)
            gain += 1 << (tiles[k] + 1)
            k += 2
        else:
            out.append(tiles[k])
            k += 1
    return out + [0] * (4 - len(out)), gain


def move(board, a):
    """(after(b, a), gain(b, a)); the move is legal iff after != b."""
    e = [int(x) for x in board]
    out, gain = list(e), 0
    for line in MOVE_LINES[a]:
        slid, g = slide_line(tuple(e[c] for c in line))
        gain += g
        for c, x in zip(line, slid):
            out[c] = x
    return out, gain


@lru_cache(maxsize=None)
def line_terms(cells):
    """(sum |d|, min(inc, dec)) over the three adjacent pairs of one line (a tuple)."""
    sm = inc = dec = 0
    for k in range(3):
        d = cells[k + 1] - cells[k]
        sm += abs(d)
        inc += max(d, 0)
        dec += max(-d, 0)
    return sm, min(inc, dec)


PAIRS = [(line[k], line[k + 1]) for line in LINES for k in range(3)]


def has_move(board):
    """legal(b) != 0: a tile can travel into an empty cell, or two equal neighbours can merge."""
    if not any(board):
        return False
    return 0 in board or any(board[x] == board[y] for x, y in PAIRS)


def terms(board):
    """(E, Sm, Mo, C) of the leaf heuristic."""
    e = [int(x) for x in board]
    E = sum(1 for x in e if x == 0)
    Sm = 0
    Mo = 0
    for line in LINES:
        sm, mo = line_terms(tuple(e[c] for c in line))
        Sm += sm
        Mo += mo
    top = max(e)
    C = top if any(e[c] == top for c in CORNERS) else 0
    return E, Sm, Mo, C


def H(board, w=DEFAULT):
    E, Sm, Mo, C = terms(board)
    return w.empty * E - w.smooth * Sm - w.mono * Mo + w.corner * C


class Search:
    def __init__(self, weights=DEFAULT, p4=0.5):
        if p4 not in (0.5, 0.1):
            raise ValueError("p4 must be 0.5 or 0.1")
        self.w = Weights(*weights)
        self.W, self.w4 = (2, 1) if p4 == 0.5 else (10, 1)
        self._moves = {}
        self._vmax = {}

    def moves(self, key):
        """[(a, after, gain)] of the legal moves of a board."""
        got = self._moves.get(key)
        if got is None:
            got = []
            for a in range(4):
                after, gain = move(key, a)
                if _key(after) != key:
                    got.append((a, _key(after), gain))
            self._moves[key] = got
        return got

    def vmax(self, key, d):
        got = self._vmax.get((key, d))
        if got is not None:
            return got
        if not has_move(key):
            v = -self.w.lost
        elif d == 0:
            v = H(key, self.w)
        else:
            v = max(self.w.gain * gain + self.vchance(after, d - 1)
                    for _, after, gain in self.moves(key))
        self._vmax[(key, d)] = v
        return v

    def vchance(self, key, d):
        empties = [c for c in range(16) if key[c] == 0]
        total = 0
        for c in empties:
            two = key[:c] + b"\x01" + key[c + 1:]
            four = key[:c] + b"\x02" + key[c + 1:]
            total += (self.W - self.w4) * self.vmax(two, d) + self.w4 * self.vmax(four, d)
        return total // (self.W * len(empties))  # Python's // floors toward -infinity

    def root(self, board, depth):
        if not 1 <= depth <= 4:
            raise ValueError("depth must be in [1, 4]")
        values = [None] * 4
        for a, after, gain in self.moves(_key(board)):
            values[a] = self.w.gain * gain + self.vchance(after, depth - 1)
        action = 0
        best = None
        for a in range(4):
            if values[a] is not None and (best is None or values[a] > best):
                action, best = a, values[a]
        return values, action


def expectimax(board, depth, weights=DEFAULT, p4=0.5):
    return Search(weights, p4).root(board, depth)


def expectimax_batch(boards, depth, weights=DEFAULT, p4=0.5):
    """(actions u8[n], values i64[n, 4]) in the library's output format."""
    boards = np.asarray(boards, np.uint8).reshape(-1, 16)
    s = Search(weights, p4)
    acts = np.zeros(len(boards), np.uint8)
    vals = np.full((len(boards), 4), INT64_MIN, np.int64)
    for i, b in enumerate(boards):
        v, a = s.root(b, depth)
        acts[i] = a
        for k in range(4):
            if v[k] is not None:
                vals[i, k] = v[k]
    return acts, vals
