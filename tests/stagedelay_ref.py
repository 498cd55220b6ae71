"""Plain Python restatement of delayed TD(lambda) on the staged batch-mean temporal-coherence rule,
written from include/g2048_stagedelay.h alone, in Python integers, over
tests/stagemeantc_ref.py's StagedMeanTC (the sparse (E, A) with its base) and through it
tests/ntstage_ref.py's StagedNet (stage, raw / val with the fall-through, V, policy) and
tests/ntuple_ref.py (delta, the wrap into int32).  The floor division is ntmean_ref's, the rate
and the step's shift are nttc_ref's.

    d = Delayed(net, n, H, s, base_ea=None)   net: an ntstage_ref.StagedNet;  d.E / d.A / d.get_ea
                                              as StagedMeanTC's
    d.hist[p][i], d.head[i], d.depth[i], d.g[p][i]     the ring, plain lists, all zero when fresh
    d.step(boards, lr_num, lr_shift) -> (actions, err, delta)     delta[k][i], H planes
    d.last_hits   {(s, t, idx): (D, C)} of the last step;  d.last_m  {(s, t, idx): m}, 0 included
    collect(g, err, k, s)                     G_k of the header

An entry that is UNSET when a hit moves it raises: consequence 4 says that cannot happen on a ring
this rule built.

Anchors, computed by hand (asserted by tests/test_stagedelay.py, and on the device by
tests/test_stagedelay_gpu.py).  The corner spec ((0,),) reads the clamped exponent of one corner
under two symmetries per corner: a board [x, 0, ...] reads index x twice and index 0 six times,
V = 2 lut[x] + 6 lut[0].  lut0[i] = 1024 i, upper stages UNSET, ea zero, lr = 1 / 2 unless noted.
A = [1, 1, 0, ...] moves left to Q2 = [2, 0, ...] with q = 4096 + V(Q2) (action 2); CB is the
checkerboard (no legal move, target 0); Q3 = [3, 0, ...].
------------------------------------------------------------------------------------------------
R.  Rounding toward zero.  collect(0, -1, k, 1) = -1, 0, 0 and collect(0, -3, k, 1) = -3, -1, 0
    for k = 0, 1, 2 (an arithmetic shift of err itself would give -1, -1, -1 and -3, -2, -1).
    End to end on the spec ((0, 1),) with S = 1, lut[33] = 1 and every other entry 0, lr = 1, H =
    3, s = 1: X1 = [1, 2, 0, ...] reads 33 once, 1 once and 0 six times, V(X1) = 1.  A ring of
    depth 3 whose latest afterstate is X1, g zero, on CB: err = -1, delta = [-1, 0, 0].  With
    lut[1] = 2 besides, V(X1) = 3, err = -3, delta = [-3, -1, 0].

W.  A window that fills, applies its oldest slot and wraps head; then terminal calls at depth H
    and at depth 0.  S = 1, H = 2, s = 1, one board, boards A, A, A, CB, CB.
    Call 1: depth 0, err 0, action 2; head = 1, hist[1] = Q2, depth 1.
    Call 2: err = 8192 - V(Q2) = 8192 - 4096 = 4096; depth 1 < H, nothing applied; g[1] = 4096;
            head = 0, hist[0] = Q2, g[0] = 0, depth 2.
    Call 3: err 4096 again.  k = 0 (plane 0) keeps G = 4096.  k = 1 (plane 1): G = 4096 + 2048 =
            6144, applied, delta_1 = 3072.  Q2 hits (0, 0, 2): (6144, 2) and (0, 0, 0): (18432, 6),
            m = 3072 both: lut[2] = 5120, lut[0] = 3072, ea (3072, 3072).  head wraps to 1,
            hist[1] = Q2, g = [4096, 0], depth 2.  delta = [[0], [3072]].
    Call 4: CB.  V(Q2) = 2 * 5120 + 6 * 3072 = 28672, err = -28672.  k = 0 (plane 1): G = -28672,
            delta_0 = -14336.  k = 1 (plane 0): G = 4096 - 14336 = -10240, delta_1 = -5120.  Both
            afterstates are Q2: (0, 0, 2): (-38912, 4), (0, 0, 0): (-116736, 12), m = -9728 both, at
            rate 2^16: lut[2] = -4608, lut[0] = -6656, ea (-6656, 12800).  depth = 0; head = 1 and
            g = [4096, 0] stay.
    Call 5: CB at depth 0: err 0, delta all 0, nothing moves, depth stays 0.

T1. A terminal call at depth 1.  S = 1, H = 2: A, then CB: err = -4096, delta = [[-2048], [0]],
    lut[2] = 0, lut[0] = -2048.

C2. Two afterstates of one terminal board share an entry.  Spec ((0, 1),), S = 1, lut[33] = 1,
    lut[1] = 2, the rest 0, lr = 1, H = 2, s = 1.  X2 = X1 with cell 11 = 6 and cell 15 = 5 reads
    33, 1, 5 and 101 once each and 0 four times.  Ring: k = 0 is X1, k = 1 is X2 with g = -4.  CB:
    err = -V(X1) = -3; G_0 = -3, G_1 = -4 - 1 = -5; delta = [-3, -5].  (0, 0, 33): (-8, 2) and
    (0, 0, 1): (-8, 2), m = -4: the mean of two different delta_k; (0, 0, 0): (-18 - 20, 10), m =
    floor(-3.8) = -4; (0, 0, 5) and (0, 0, 101): (-5, 1).  lut[33] = -3, lut[1] = -2, lut[0] = -4,
    lut[5] = lut[101] = -5; ea = (m, |m|).

S2. Two boards of different stages address one (t, i).  bounds (3,): Q2 is of stage 0, Q3 of stage
    1.  H = 2, rings of depth 1 holding Q2 and Q3, both boards CB: err = [-4096, -6144], delta_0 =
    [-2048, -3072]; (1, 0, 3) is promoted to 3072 and (1, 0, 0) to 0; lut0[2] = 0, lut0[0] = -2048,
    lut1[3] = 0, lut1[0] = -3072; ea (0, 0, 0) = (-2048, 2048), (1, 0, 0) = (-3072, 3072).

P.  Promoted while prev, moved H - 1 calls later.  bounds (2,): Q2 is of stage 1.  H = 2, boards
    A, A, A.  Call 2 promotes (1, 0, 2) to 2048 and (1, 0, 0) to 0 (err 4096, nothing applied);
    call 3 promotes nothing and moves them by delta_1 = 3072: lut1[2] = 5120, lut1[0] = 3072;
    stage 0 is untouched.

Z.  A G that cancels.  S = 1, H = 2, ring of depth 2 with head 0: k = 0 (plane 0) is Q2, k = 1
    (plane 1) is Q3 with g = -2048; ea[(0, 0, 3)] = (5, 9).  Board A: err = 4096, G_1 = -2048 +
    2048 = 0, delta_1 = 0: no hit, the table and ea stay; head = 1, hist[1] = Q2, g = [4096, 0].
"""
from __future__ import annotations

import ntmean_ref as MR
import nttc_ref as TR
import ntuple_ref as NR
import stagemeantc_ref as SMT

MAX_HORIZON, MAX_LAM_SHIFT = 8, 31


def collect(g: int, err: int, k: int, s: int) -> int:
    """G_k = g_k + sgn(err) (|err| >> (k s)): the magnitude is shifted, so it rounds toward 0."""
    mag = abs(err) >> (k * s)
    return g + (-mag if err < 0 else mag)


class Delayed(SMT.StagedMeanTC):
    def __init__(self, net, n: int, H: int, s: int, base_ea=None):
        if not (1 <= H <= MAX_HORIZON and 1 <= s <= MAX_LAM_SHIFT and (H - 1) * s <= 31):
            raise ValueError(f"(H, s) = ({H}, {s}) is outside the domain")
        super().__init__(net, base_ea)
        self.n, self.H, self.s = n, H, s
        self.hist = [[[0] * 16 for _ in range(n)] for _ in range(H)]
        self.head, self.depth = [0] * n, [0] * n
        self.g = [[0] * n for _ in range(H)]

    def plane(self, i: int, k: int) -> int:
        return (self.head[i] - k) % self.H

    def back(self, i: int, k: int):
        """The afterstate k steps back of board i (k < depth)."""
        return self.hist[self.plane(i, k)][i]

    def step(self, boards, lr_num: int, lr_shift: int):
        """One step over all boards.  Every read of the table, of (E, A) and of the ring sees them
        as they were before the call: the ring is only written in the commit at the end."""
        net, n, H = self.net, self.n, self.H
        assert len(boards) == n
        actions, errs, afters, legal = [0] * n, [0] * n, [None] * n, [False] * n
        delta = [[0] * n for _ in range(H)]
        G = [[None] * n for _ in range(H)]  # G[k][i] for k < depth
        pol, val = {}, {}
        for i in range(n):
            b = tuple(int(x) for x in boards[i])
            if b not in pol:
                pol[b] = net.policy(list(b))
            q, actions[i], afters[i] = pol[b]
            live = [x for x in q if x is not None]
            legal[i] = bool(live)
            target = max(live) if live else 0
            if self.depth[i] > 0:
                p = tuple(self.back(i, 0))
                if p not in val:
                    val[p] = net.V(list(p))
                errs[i] = target - val[p]
            for k in range(self.depth[i]):
                G[k][i] = collect(self.g[self.plane(i, k)][i], errs[i], k, self.s)
                applied = True if not legal[i] else (self.depth[i] == H and k == H - 1)
                if applied:
                    delta[k][i] = NR.delta_of(G[k][i], lr_num, lr_shift)
        promoted, hits = {}, {}
        for i in range(n):
            if self.depth[i] == 0:
                continue
            prev = self.back(i, 0)
            s = net.stage(prev)
            for t, idx in net.indices(prev):
                if net.raw(s, t, idx) is None:
                    promoted[(s, t, idx)] = net.val(s, t, idx)  # the pre-call table's
            for k in range(self.depth[i]):
                if delta[k][i] == 0:
                    continue
                h = self.back(i, k)
                s = net.stage(h)
                for t, idx in net.indices(h):  # all 8 T pairs, coinciding ones each a hit
                    D, C = hits.get((s, t, idx), (0, 0))
                    hits[(s, t, idx)] = (D + delta[k][i], C + 1)
        for (s, t, idx), v in promoted.items():
            net.stages[s][(t, idx)] = v
        moves = {}
        for key, (D, C) in hits.items():
            s, t, idx = key
            if net.raw(s, t, idx) is None:
                raise AssertionError(f"a hit on the UNSET entry {key}")
            m = MR.floor_div(D, C)
            moves[key] = m
            if m == 0:
                continue
            e0, a0 = self.get_ea(s, t, idx)
            step = TR.step_of(m, TR.rate(e0, a0))
            net.stages[s][(t, idx)] = NR.wrap32(net.raw(s, t, idx) + step)
            self.E[key], self.A[key] = e0 + m, a0 + abs(m)
        net.promoted = promoted
        self.last_hits, self.last_m = hits, moves
        for i in range(n):
            if not legal[i]:
                self.depth[i] = 0
                continue
            for k in range(self.depth[i]):  # the kept slots; the one at H - 1 is overwritten below
                self.g[self.plane(i, k)][i] = G[k][i]
            self.head[i] = (self.head[i] + 1) % H
            self.hist[self.head[i]][i] = list(afters[i])
            self.g[self.head[i]][i] = 0
            self.depth[i] = min(self.depth[i] + 1, H)
        return actions, errs, delta
