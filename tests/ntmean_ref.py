"""Plain Python restatement of batch-mean TD learning for the n-tuple network, written from
include/g2048_ntmean.h alone, in Python integers, over tests/ntuple_ref.py's Net (policy, V, idx,
delta, the table's sparse dict and its wrap into int32).

    floor_div(D, C)                       floor(D / C), C >= 1
    step(net, boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)
                                          net: an ntuple_ref.Net; net.touched gets the moved entries
    last_hits                             {(t, idx): (D, C)} of the last step (the library's acc
                                          between its second and third launch)

Anchors, computed by hand (asserted by tests/test_ntmean.py)
-----------------------------------------------------------
The quotient floors like the shifts: floor_div(-3, 2) = -2, floor_div(3, 2) = 1, floor_div(-4, 2)
= -2, floor_div(-1, 18) = -1, floor_div(0, 5) = 0.

The TD anchor of ntuple_ref.  Spec ((0,),), lut[i] = 1024 * i, board A = [1, 1, 0, ...], prev =
[2, 0, ...], has_prev = 1, lr = 1 / 2: action 2, err 4096, delta 2048; idx(prev, g) = 2 for g = 0
and 4, else 0 (six pairs).  Entry 2 has (D, C) = (4096, 2) and entry 0 has (12288, 6): both move by
2048, lut[2] = 2048 + 2048 = 4096 and lut[0] = 0 + 2048 = 2048 (TD(0) leaves 6144 and 12288).  The
same batch with the board given three times: (12288, 6) and (36864, 18), the same two numbers.

Two boards of different delta on one entry.  C = the checkerboard [1, 2, 1, 2, 2, 1, 2, 1, ...]
has no legal move: target 0.  With prev = [3, 0, ...]: V(prev) = 2 * 3072 + 6 * 0 = 6144, err =
-6144, delta = -3072; idx(prev, g) = 3 for g = 0 and 4, else 0.
  Boards [A, C, C], prev [[2, 0, ...], [3, 0, ...], [3, 0, ...]], lr = 1 / 2: delta = [2048,
  -3072, -3072].  Entry 2: (4096, 2) -> +2048, lut[2] = 4096.  Entry 3: (4 * -3072, 4) = (-12288,
  4) -> -3072, lut[3] = 3072 - 3072 = 0.  Entry 0: D = 6 * 2048 - 12 * 3072 = -24576, C = 18:
  -24576 / 18 = -1365.33..., floor -1366, lut[0] = -1366 (TD(0) leaves -24576).  has_prev becomes
  [1, 0, 0]; prev[1] and prev[2] stay.
  Boards [A, A, C]: entry 0 has D = 12 * 2048 - 6 * 3072 = 6144, C = 18: 341.33..., floor 341,
  lut[0] = 341; entry 2: (8192, 4) -> 2048, lut[2] = 4096; entry 3: (-6144, 2) -> -3072, lut[3] = 0.
"""
from __future__ import annotations

import ntuple_ref as NR


def floor_div(D: int, C: int) -> int:
    if C < 1:
        raise ValueError(f"C = {C} is not a hit count")
    return D // C  # Python's // floors


last_hits: dict = {}


def step(net: NR.Net, boards, prev, has_prev, lr_num: int, lr_shift: int):
    """One batch-mean step over all boards; prev (list of lists) and has_prev (list) are updated
    in place.  Every read of the table sees it as it was before the call."""
    global last_hits
    n = len(boards)
    actions, errs, deltas, afters, legal = [0] * n, [0] * n, [0] * n, [None] * n, [False] * n
    for i in range(n):
        q, actions[i], afters[i] = net.policy(boards[i])
        live = [x for x in q if x is not None]
        legal[i] = bool(live)
        target = max(live) if live else 0
        errs[i] = target - net.V(prev[i]) if has_prev[i] else 0
        deltas[i] = NR.delta_of(errs[i], lr_num, lr_shift)
    hits = {}
    for i in range(n):
        if has_prev[i] and deltas[i] != 0:
            for key in net.indices(prev[i]):  # all 8 T pairs, coinciding ones each a hit
                D, C = hits.get(key, (0, 0))
                hits[key] = (D + deltas[i], C + 1)
    for key, (D, C) in hits.items():
        net.touched[key] = NR.wrap32(net.get(*key) + floor_div(D, C))
    last_hits = hits
    for i in range(n):
        if legal[i]:
            prev[i] = list(afters[i])
            has_prev[i] = 1
        else:
            has_prev[i] = 0
    return actions, errs, deltas
