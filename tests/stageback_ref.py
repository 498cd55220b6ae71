"""Plain Python restatement of backward episode learning on the staged batch-mean
temporal-coherence rule, written from include/g2048_stageback.h alone, in Python integers, over
tests/stagemeantc_ref.py's StagedMeanTC (the sparse (E, A) with its base) and through it
tests/ntstage_ref.py's StagedNet (stage, raw / val with the fall-through, V, policy) and
tests/ntuple_ref.py (delta, the wrap into int32).  The floor division is ntmean_ref's, the rate
and the step's shift are nttc_ref's, the move and its gain expectimax_ref's.

    d = Backward(net, n, L, base_ea=None)     net: an ntstage_ref.StagedNet;  d.E / d.A / d.get_ea
                                              as StagedMeanTC's
    d.traj[i][buf][slot], d.gain[i][buf][slot], d.cur[i], d.rec[i], d.rep_n[i], d.rep_k[i]
                                              the state, plain lists, all zero when fresh; a gain
                                              is the unsigned number (up to 2^31)
    d.step(boards, lr_num, lr_shift) -> (actions, err, delta, x, replays)
                                              x[i] is None where board i does not replay
    d.last_hits   {(s, t, idx): (D, C)} of the last step;  d.last_m  {(s, t, idx): m}, 0 included

An entry that is UNSET when a hit moves it raises: consequence 4 says that cannot happen.

Anchors, computed by hand (asserted by tests/test_stageback.py, and on the device by
tests/test_stageback_gpu.py).  The corner spec ((0,),) reads the clamped exponent of one corner
under two symmetries per corner: a board [x, 0, ...] reads index x twice and index 0 six times,
V = 2 lut[x] + 6 lut[0].  lut0[i] = 1024 i, upper stages UNSET, ea zero, lr = 1 / 2 unless noted.
A = [1, 1, 0, ...] moves left to Q2 = [2, 0, ...] with gain 4 (action 2); CB is the checkerboard
(no legal move); Q3 = [3, 0, ...].  V(Q2) = 4096 and V(Q3) = 6144 on the fresh table.
------------------------------------------------------------------------------------------------
1.  L = 4, one board, boards A, A, CB, A, A, A.
    Calls 1, 2: record Q2 (gain 4) in slots 0 and 1 of buffer 0; rec = 1, 2.  Nothing replays.
    Call 3: CB, action 0, the episode closes: cur = 1, rep_n = 2, rep_k = 0, rec = 0; the table
            is untouched.
    Call 4: replays j = 1, x = Q2, the last one: target 0, err = -4096, delta = -2048.  Hits
            (0, 0, 2): (-4096, 2) and (0, 0, 0): (-12288, 6), m = -2048 both: lut[2] = 0, lut[0] =
            -2048, ea (-2048, 2048) both.  rep_k = 1; A records into buffer 1: rec = 1.
    Call 5: replays j = 0, x = Q2, y = Q2 with gain 4: V(Q2) = 2 * 0 + 6 * -2048 = -12288, target
            = 4096 - 12288, err = 4096, delta = 2048; m = 2048 both, rate(-2048, 2048) = 2^16:
            lut[2] = 2048, lut[0] = 0, ea (0, 4096) both.  rep_k = 2, rec = 2.
    Call 6: rep_k = 2 = min(rep_n, L): idle, nothing moves.  rec = 3.

2.  L = 2, boards A, A, A, CB, A, A, A: the episode of 3 keeps its last 2.  Slot 0 is overwritten
    by the third afterstate.  rep_n = 3.  Call 5 replays j = 2 (slot 0), call 6 j = 1 (slot 1)
    against slot 0, with the table values of calls 4 and 5 above.  Call 7 idles at rep_k = 2.

3.  An episode that ends while a replay is active.  L = 4, boards A, A, A, CB, A, CB, A, A.
    Call 4 closes an episode of 3.  Call 5 replays j = 2 (as call 4 of anchor 1) and records.
    Call 6: CB.  The replay's transition is still made, j = 1: err 4096, delta 2048, lut[2] =
    2048, lut[0] = 0 (as call 5 of anchor 1), and then the episode of one afterstate closes: cur
    = 0, rep_n = 1, rep_k = 0, rec = 0.  j = 0 of the older episode is dropped.  Call 7 replays
    the new episode's only afterstate: x = Q2, target 0, V = 4096, err = -4096, delta -2048, m =
    -2048 at rate(0, 4096) = 0: nothing moves in lut, ea = (-2048, 6144).  Call 8 idles.

4.  A terminal board at rec == 0.  Fresh state, CB: action 0, no replay, nothing changes at all.
    After an episode closed (A, CB), a second CB replays j = 0 and leaves cur, rep_n and rec.

5.  Two boards of different stages replaying onto one (t, i).  bounds (3,): Q2 is of stage 0, Q3 of
    stage 1.  Replay buffers holding the one-afterstate episodes Q2 and Q3, both boards CB: err =
    [-4096, -6144], delta = [-2048, -3072]; (1, 0, 3) is promoted to 3072 and (1, 0, 0) to 0;
    lut0[2] = 0, lut0[0] = -2048, lut1[3] = 0, lut1[0] = -3072; ea (0, 0, 0) = (-2048, 2048),
    (1, 0, 0) = (-3072, 3072).

6.  An x whose stage-1 entries are UNSET, promoted and then moved in the same call.  bounds (2,):
    Q2 is of stage 1.  Boards A, CB, CB: call 3 replays x = Q2: (1, 0, 2) is promoted to 2048 and
    (1, 0, 0) to 0, then both move by -2048: lut1[2] = 0, lut1[0] = -2048; stage 0 is untouched.

7.  Two replaying boards sharing an entry with deltas that cancel.  S = 1, lr = 1.  Board 0
    replays the last afterstate Q2 of its episode: err = -4096.  Board 1 replays x = Q2 with the
    successor Q3 at gain 2: target = 2048 + 6144, err = 4096.  (0, 0, 2): (0, 4), (0, 0, 0):
    (0, 12): m = 0 both, the table stays and ea, preset to (5, 9) at (0, 0, 2), is untouched.
"""
from __future__ import annotations

import expectimax_ref as E
import ntmean_ref as MR
import nttc_ref as TR
import ntuple_ref as NR
import stagemeantc_ref as SMT

F = NR.F
MAX_HORIZON, MAX_SLOTS = 1 << 20, 1 << 31
U32 = (1 << 32) - 1


class Backward(SMT.StagedMeanTC):
    def __init__(self, net, n: int, L: int, base_ea=None):
        if not (1 <= L <= MAX_HORIZON and n >= 1 and n * L <= MAX_SLOTS):
            raise ValueError(f"(n, L) = ({n}, {L}) is outside the domain")
        super().__init__(net, base_ea)
        self.n, self.L = n, L
        self.traj = [[[[0] * 16 for _ in range(L)] for _ in range(2)] for _ in range(n)]
        self.gain = [[[0] * L for _ in range(2)] for _ in range(n)]
        self.cur, self.rec = [0] * n, [0] * n
        self.rep_n, self.rep_k = [0] * n, [0] * n

    def replays(self, i: int) -> bool:
        return self.rep_k[i] < min(self.rep_n[i], self.L)

    def step(self, boards, lr_num: int, lr_shift: int):
        """One call over all boards.  Every read of the table, of (E, A) and of the state sees
        them as they were before the call: the state is only written in the commit at the end."""
        net, n, L = self.net, self.n, self.L
        assert len(boards) == n
        actions, errs, deltas = [0] * n, [0] * n, [0] * n
        xs, rep = [None] * n, [False] * n
        afters, gains, legal = [None] * n, [0] * n, [False] * n
        pol, val = {}, {}

        def V(b):
            b = tuple(b)
            if b not in val:
                val[b] = net.V(list(b))
            return val[b]

        for i in range(n):
            b = tuple(int(v) for v in boards[i])
            if b not in pol:  # equal boards, one evaluation: (action, after, legal, gain)
                q, act, after = net.policy(list(b))
                ok = any(v is not None for v in q)
                pol[b] = (act, after, ok, E.move(list(b), act)[1] if ok else 0)
            actions[i], afters[i], legal[i], gains[i] = pol[b]
            rep[i] = self.replays(i)
            if not rep[i]:
                continue
            buf = (self.cur[i] & 1) ^ 1
            j = self.rep_n[i] - 1 - self.rep_k[i]
            xs[i] = list(self.traj[i][buf][j % L])
            if self.rep_k[i] == 0:
                target = 0
            else:
                sy = (j + 1) % L
                target = (self.gain[i][buf][sy] << F) + V(self.traj[i][buf][sy])
            errs[i] = target - V(xs[i])
            deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
        promoted, hits, keys = {}, {}, {}
        for i in range(n):
            if not rep[i]:
                continue
            x = tuple(xs[i])
            if x not in keys:  # equal afterstates, one evaluation
                keys[x] = (net.stage(xs[i]), net.indices(xs[i]))
            s, pairs = keys[x]
            for t, idx in pairs:  # all 8 T pairs, coinciding ones each a hit
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
            s, t, idx = key
            if net.raw(s, t, idx) is None:
                raise AssertionError(f"a hit on the UNSET entry {key}")
            m = MR.floor_div(D, C)
            moves[key] = m
            if m == 0:
                continue  # keeps its value after promotion, ea untouched
            e0, a0 = self.get_ea(s, t, idx)
            step = TR.step_of(m, TR.rate(e0, a0))
            net.stages[s][(t, idx)] = NR.wrap32(net.raw(s, t, idx) + step)
            self.E[key], self.A[key] = e0 + m, a0 + abs(m)
        net.promoted = promoted
        self.last_hits, self.last_m = hits, moves
        for i in range(n):
            if rep[i]:
                self.rep_k[i] += 1
            if legal[i]:
                buf, slot = self.cur[i] & 1, self.rec[i] % L
                self.traj[i][buf][slot] = list(afters[i])
                self.gain[i][buf][slot] = gains[i]
                self.rec[i] = (self.rec[i] + 1) & U32
            elif self.rec[i] > 0:
                self.cur[i] ^= 1
                self.rep_n[i], self.rep_k[i], self.rec[i] = self.rec[i], 0, 0
        return actions, errs, deltas, xs, rep
