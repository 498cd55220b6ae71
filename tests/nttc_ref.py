"""Plain Python restatement of temporal-coherence learning for the n-tuple network, written from
include/g2048_nttc.h alone, in Python integers, over tests/ntuple_ref.py's Net (policy, V, idx,
delta, the table's sparse dict and its wrap into int32).

    rate(E, A)                            the entry's rate, a fraction with 16 bits
    tc = TC(net)                          net: an ntuple_ref.Net;  tc.E / tc.A: sparse dicts
                                          {(t, idx): int}, missing = base_ea(t, idx) or (0, 0)
    tc.step(boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)

Anchors, computed by hand (asserted by tests/test_nttc.py)
---------------------------------------------------------
The rate.  rate(0, 0) = 65536 (a fresh entry moves at full speed); rate(A, A) = rate(-A, A) =
65536 for every A > 0; rate(1, 3) = floor(65536 / 3) = 21845; rate(0, 7) = 0.
  A = 2^16 - 1 = 65535 has 16 bits, s = 0:  rate(32768, 65535) = floor(2^31 / 65535) = 32768
                                            (65535 * 32768 = 2^31 - 32768).
  A = 2^16 has 17 bits, s = 1:              rate(32769, 65536) = ((32769 >> 1) << 16) / 32768
                                            = 16384 * 2 = 32768: the shift drops E's low bit (the
                                            unshifted quotient would be 32769).
  A = 2^16 + 1, s = 1, A >> 1 = 32768:      rate(3, 65537) = ((3 >> 1) << 16) / 32768 = 2, and
                                            rate(65537, 65537) = (32768 << 16) / 32768 = 65536.
  A = 2^40 + 12345 has 41 bits, s = 25:     A >> 25 = 32768; E = -3 * 2^38 gives |E| >> 25 =
                                            3 * 2^13 = 24576 and rate = 24576 * 2 = 49152 (3 / 4).
The step floors: delta = -3 at rate 21845 gives (-65535) >> 16 = -1; delta = 3 gives 0.

A worked step on ntuple_ref's TD anchor.  Spec ((0,),), lut[i] = 1024 * i, board A = [1, 1, 0,
...], prev = [2, 0, ...], has_prev = 1, lr = 1 / 2: action 2, err 4096, delta 2048; idx(prev, g)
= 2 for g = 0 and 4, else 0 (six pairs).
  Fresh ea: every rate is 65536, step = delta, so lut[2] = 2048 + 2 * 2048 = 6144 and lut[0] =
  6 * 2048 = 12288, exactly TD(0); E[2] = A[2] = 2 * 2048 = 4096, E[0] = A[0] = 6 * 2048 = 12288.
  With ea[2] = (1, 3) and ea[0] = (-5, 10): rate 21845 at entry 2, step = (2048 * 21845) >> 16 =
  44738560 >> 16 = 682, lut[2] = 2048 + 2 * 682 = 3412; rate (5 << 16) / 10 = 32768 at entry 0,
  step = 1024, lut[0] = 6 * 1024 = 6144; ea[2] = (1 + 4096, 3 + 4096) = (4097, 4099), ea[0] =
  (-5 + 12288, 10 + 12288) = (12283, 12298).
"""
from __future__ import annotations

import ntuple_ref as NR

RATE_BITS = 16
ONE = 1 << RATE_BITS
MAX_A = (1 << 62) - 1


def rate(E: int, A: int) -> int:
    if not (0 <= A <= MAX_A and abs(E) <= A):
        raise ValueError(f"(E, A) = ({E}, {A}) is outside the domain")
    if A == 0:
        return ONE
    s = max(0, A.bit_length() - RATE_BITS)
    return ((abs(E) >> s) << RATE_BITS) // (A >> s)


def shift_of(A: int) -> int:
    """The s of rate(., A)."""
    return max(0, A.bit_length() - RATE_BITS)


def step_of(delta: int, r: int) -> int:
    return (delta * r) >> RATE_BITS  # Python's >> floors


class TC:
    def __init__(self, net: NR.Net, base_ea=None):
        """base_ea: None (zeros) or a callable (t, idx) -> (E, A) for entries not yet written."""
        self.net = net
        self.base_ea = base_ea if base_ea is not None else (lambda t, i: (0, 0))
        self.E, self.A = {}, {}

    def get_ea(self, t: int, i: int):
        if (t, i) in self.A:
            return self.E[(t, i)], self.A[(t, i)]
        return self.base_ea(t, i)

    def step(self, boards, prev, has_prev, lr_num: int, lr_shift: int):
        """One TC step over all boards; prev (list of lists) and has_prev (list) are updated in
        place.  Every read of the table and of (E, A) sees them as they were before the call."""
        net, n = self.net, len(boards)
        actions, errs, deltas, afters, legal = [0] * n, [0] * n, [0] * n, [None] * n, [False] * n
        for i in range(n):
            q, actions[i], afters[i] = net.policy(boards[i])
            live = [x for x in q if x is not None]
            legal[i] = bool(live)
            target = max(live) if live else 0
            errs[i] = target - net.V(prev[i]) if has_prev[i] else 0
            deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
        steps, dE, dA = {}, {}, {}
        for i in range(n):
            if has_prev[i] and deltas[i] != 0:
                for key in net.indices(prev[i]):  # all 8 T pairs, coinciding ones each applied
                    r = rate(*self.get_ea(*key))
                    steps[key] = steps.get(key, 0) + step_of(deltas[i], r)
                    dE[key] = dE.get(key, 0) + deltas[i]
                    dA[key] = dA.get(key, 0) + abs(deltas[i])
        for key in dA:
            e0, a0 = self.get_ea(*key)
            net.touched[key] = NR.wrap32(net.get(*key) + steps[key])
            self.E[key], self.A[key] = e0 + dE[key], a0 + dA[key]
        for i in range(n):
            if legal[i]:
                prev[i] = list(afters[i])
                has_prev[i] = 1
            else:
                has_prev[i] = 0
        return actions, errs, deltas
