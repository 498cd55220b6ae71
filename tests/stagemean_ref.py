"""Plain Python restatement of batch-mean TD learning for the multi-stage n-tuple network, written
from include/g2048_stagemean.h alone, in Python integers, over tests/ntstage_ref.py's StagedNet
(stage, raw / val with the fall-through, V, policy, the stages' sparse dicts) and
tests/ntuple_ref.py (delta, the wrap into int32).

    floor_div(D, C)                       floor(D / C), C >= 1
    step(net, boards, prev, has_prev, lr_num, lr_shift) -> (actions, err, delta)
                                          net: an ntstage_ref.StagedNet; net.stages[s] gets the
                                          promoted and the moved entries, net.promoted what this
                                          step promoted
    last_hits                             {(s, t, idx): (D, C)} of the last step (the library's acc
                                          between its second and third launch)

Anchors, computed by hand (asserted by tests/test_stagemean.py).  All use the spec ((0,),), whose
index is the clamped exponent of one corner, read by two symmetries per corner: a board [x, 0, ...]
reads index x twice and index 0 six times.  Stage 0 is lut0[i] = 1024 * i, the upper stages are
UNSET, lr = 1 / 2.  A = [1, 1, 0, ...]; CB is the checkerboard (no legal move, target 0).
------------------------------------------------------------------------------------------------
Two stages promoted and moved in one call.  bounds (2, 3), boards [CB, A], prev [P1, P2] of
ntstage_ref's two-stage anchor (P1 of stage 1, P2 of stage 2, both reading index 1 twice and index
0 six times): delta = [-1024, 3072] as there, and (1, 0, 1), (2, 0, 1) are promoted to 1024,
(1, 0, 0), (2, 0, 0) to 0.  Every entry is hit by one board only, so the mean is that board's
delta: hits (1, 0, 1): (-2048, 2), (1, 0, 0): (-6144, 6), (2, 0, 1): (6144, 2), (2, 0, 0):
(18432, 6), and
  lut1[1] = 1024 - 1024 = 0      lut1[0] = 0 - 1024 = -1024
  lut2[1] = 1024 + 3072 = 4096   lut2[0] = 0 + 3072 = 3072
(the sum rule leaves -1024 / -6144 / 7168 / 18432).  Stage 0 is untouched.

Two deltas on one staged entry.  bounds (2,), so [2, 0, ...] and [3, 0, ...] are both of stage 1,
all of it UNSET before the call, every read falling through to lut0.
  A: left gives [2, 0, ...], q = 4096 + 2 * 2048 = 8192 (down: 2048), action 2; with prev =
     [2, 0, ...]: V = 4096, err = 4096, delta = 2048.
  CB with prev = [3, 0, ...]: V = 2 * 3072 = 6144, err = -6144, delta = -3072.
  Boards [A, CB, CB], prev [[2, 0, ...], [3, 0, ...], [3, 0, ...]]: delta = [2048, -3072, -3072].
    (1, 0, 2): (2 * 2048, 2) = (4096, 2), promoted to 2048, + 2048 = 4096
    (1, 0, 3): (4 * -3072, 4) = (-12288, 4), promoted to 3072, - 3072 = 0
    (1, 0, 0): D = 6 * 2048 - 12 * 3072 = -24576, C = 18: -1365.33..., floor -1366, promoted to
               0: lut1[0] = -1366
    has_prev becomes [1, 0, 0]; prev[1] and prev[2] stay.
  Boards [A, A, CB], prev [[2, 0, ...], [2, 0, ...], [3, 0, ...]]:
    (1, 0, 0): D = 12 * 2048 - 6 * 3072 = 6144, C = 18: 341.33..., floor 341: lut1[0] = 341
    (1, 0, 2): (8192, 4) -> 2048 + 2048 = 4096;  (1, 0, 3): (-6144, 2) -> 3072 - 3072 = 0.

The stage split.  The same [A, CB, CB] batch with bounds (3,): [2, 0, ...] is of stage 0 and
[3, 0, ...] of stage 1, so index 0 is hit at both stages and the two (D, C) stay apart.  A's left
afterstate [2, 0, ...] is of stage 0: q = 4096 + 4096 = 8192, delta 2048 as before; CB: -3072.
    (0, 0, 2): (4096, 2) -> lut0[2] = 2048 + 2048 = 4096
    (0, 0, 0): (6 * 2048, 6) = (12288, 6) -> lut0[0] = 0 + 2048 = 2048
    (1, 0, 3): (-12288, 4), promoted to 3072 -> lut1[3] = 0
    (1, 0, 0): (12 * -3072, 12) = (-36864, 12), promoted to 0 -> lut1[0] = -3072
  One table gives index 0 the one quotient -1366.  Only (1, 0, 3) and (1, 0, 0) are promoted: the
  stage-0 entries are set.

lr_num = 0 with has_prev: delta = 0 on every board, the entries of prev are promoted to the values
they resolve to, last_hits is empty and no V changes.
"""
from __future__ import annotations

import ntstage_ref as SR
import ntuple_ref as NR


def floor_div(D: int, C: int) -> int:
    if C < 1:
        raise ValueError(f"C = {C} is not a hit count")
    return D // C  # Python's // floors


last_hits: dict = {}


def step(net: SR.StagedNet, boards, prev, has_prev, lr_num: int, lr_shift: int):
    """One staged batch-mean step over all boards; prev (list of lists) and has_prev (list) are
    updated in place.  Every read of the table sees it as it was before the call."""
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
    promoted, hits = {}, {}
    for i in range(n):
        if not has_prev[i]:
            continue
        s = net.stage(prev[i])
        for t, idx in net.indices(prev[i]):  # all 8 T pairs, coinciding ones each a hit
            key = (s, t, idx)
            if net.raw(s, t, idx) is None:
                promoted[key] = net.val(s, t, idx)  # the pre-call table's
            if deltas[i] != 0:
                D, C = hits.get(key, (0, 0))
                hits[key] = (D + deltas[i], C + 1)
    for (s, t, idx), v in promoted.items():
        net.stages[s][(t, idx)] = v
    for (s, t, idx), (D, C) in hits.items():
        net.stages[s][(t, idx)] = NR.wrap32(net.raw(s, t, idx) + floor_div(D, C))
    net.promoted = promoted
    last_hits = hits
    for i in range(n):
        if legal[i]:
            prev[i] = list(afters[i])
            has_prev[i] = 1
        else:
            has_prev[i] = 0
    return actions, errs, deltas
