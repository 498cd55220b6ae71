"""Plain Python restatement of truncated TD(lambda) learning for the n-tuple network, written from
include/g2048_ntlambda.h alone, in Python integers, over tests/ntuple_ref.py's Net (policy, V,
idx, delta, the table's sparse dict and its wrap into int32).  The ring layout of the header is
kept: hist[plane][board] is a list of 16 exponents, head[board] and depth[board] are ints.

    shifted(delta, k, s)                  delta_k = sgn(delta) * (|delta| >> (k s))
    lam = Lam(net, n, horizon, lam_shift) lam.hist / lam.head / lam.depth: the fresh (zero) state
    lam.back(i, k)                        the afterstate k steps back of board i
    lam.step(boards, lr_num, lr_shift) -> (actions, err, delta)

Anchors, computed by hand (asserted by tests/test_ntlambda.py)
-------------------------------------------------------------
Rounding toward zero.  shifted(-7, 1, 1) = -(7 >> 1) = -3 (a floor would give -4);
shifted(7, 1, 1) = 3; shifted(-7, 2, 1) = -1; shifted(-7, 3, 1) = 0; shifted(-7, 0, s) = -7;
shifted(-2^31, 1, 31) = -1 (the magnitude 2^31 does not fit int32).

A worked step with a two-deep history.  Spec ((0,),), lut[i] = 1024 * i, H = 2, s = 1, board A =
[1, 1, 0, ...] as in ntuple_ref's TD anchor (action 2, target 8192).  head = 1, depth = 2, plane
1 row 0 = P0 = [4, 0, ...] (0 steps back), plane 0 row 0 = P1 = [2, 0, ...] (1 step back).
  V(P0) = 1024 * 2 * 4 = 8192 (cell 0 is read by g = 0 and g = 4), err = 8192 - 8192 = 0: nothing.
  With lut[4] = 4099 instead: V(P0) = 8198 + 6 lut[0] = 8198, err = -6, lr = 7 / 2^2:
  delta = (-42) >> 2 = -11 (the floor of -10.5).  delta_0 = -11, delta_1 = -(11 >> 1) = -5.
  idx(P0, g) = 4 for g = 0 and 4, else 0: lut[4] = 4099 - 22 = 4077, lut[0] = 6 * -11 = -66.
  idx(P1, g) = 2 for g = 0 and 4, else 0: lut[2] = 2048 - 10 = 2038, lut[0] = -66 + 6 * -5 = -96.
  The board has a legal move: head = (1 + 1) mod 2 = 0, plane 0 row 0 = after(A, 2) = [2, 0,
  ...], depth stays 2.
"""
from __future__ import annotations

import ntuple_ref as NR

MAX_HORIZON = 8


def shifted(delta: int, k: int, s: int) -> int:
    m = abs(delta) >> (k * s)
    return -m if delta < 0 else m


class Lam:
    def __init__(self, net: NR.Net, n: int, horizon: int, lam_shift: int):
        if not 1 <= horizon <= MAX_HORIZON or not 1 <= lam_shift <= 31 \
                or (horizon - 1) * lam_shift > 31:
            raise ValueError(f"(horizon, lam_shift) = ({horizon}, {lam_shift}) is outside the "
                             f"domain")
        self.net, self.n, self.H, self.s = net, n, horizon, lam_shift
        self.hist = [[[0] * 16 for _ in range(n)] for _ in range(horizon)]
        self.head = [0] * n
        self.depth = [0] * n

    def back(self, i: int, k: int):
        assert 0 <= k < self.depth[i]
        return self.hist[(self.head[i] - k) % self.H][i]

    def step(self, boards, lr_num: int, lr_shift: int):
        """One step over all boards; hist, head and depth are updated in place.  Every read of
        the table and of the state sees them as they were before the call."""
        net, n = self.net, len(boards)
        assert n == self.n
        actions, errs, deltas, afters, legal = [0] * n, [0] * n, [0] * n, [None] * n, [False] * n
        for i in range(n):
            q, actions[i], afters[i] = net.policy(boards[i])
            live = [x for x in q if x is not None]
            legal[i] = bool(live)
            target = max(live) if live else 0
            errs[i] = target - net.V(self.hist[self.head[i]][i]) if self.depth[i] else 0
            deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
        adds = {}
        for i in range(n):
            for k in range(self.depth[i]):
                dk = shifted(deltas[i], k, self.s)
                if dk != 0:
                    for key in net.indices(self.back(i, k)):  # all 8 T pairs, each applied
                        adds[key] = adds.get(key, 0) + dk
        for key, d in adds.items():
            net.touched[key] = NR.wrap32(net.get(*key) + d)
        for i in range(n):
            if legal[i]:
                self.head[i] = (self.head[i] + 1) % self.H
                self.hist[self.head[i]][i] = list(afters[i])
                self.depth[i] = min(self.depth[i] + 1, self.H)
            else:
                self.depth[i] = 0
        return actions, errs, deltas
