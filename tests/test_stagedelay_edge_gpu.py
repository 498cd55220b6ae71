"""libg2048_stagedelay.so at the edges of the domain include/g2048_stagedelay.h declares, in the
manner of tests/domain_edge.py: every case is built from seeds, runs through the reference inside
domain_edge.InDomain (which fails the test when the *reference* leaves the domain) and is compared
bit for bit -- G * lr_num next to 2^59, delta_k of INT32_MIN and INT32_MAX, lr_num = 0, and a head
and a depth that are out of range in memory."""
import numpy as np
import pytest
import torch

import domain_edge as DE
import ntuple_ref as NR
import stagedelay_ref as R
from g2048 import stagedelay as _library
from test_ntstage_gpu import dev, make_net
from test_stagedelay_gpu import (CHECKER, LR, M, Pair, batch,  # noqa: F401  (M is the fixture)
                                 random_ring)

_library.load()
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN, INT32_MAX = DE.INT32_MIN, DE.INT32_MAX
ALL_27 = [27] * 16  # every move merges sixteen 27s into eight 28s: a gain of exactly 2^31


def guarded_step(pair, boards, lr):
    with DE.InDomain(pair.ref.net, pair.ref):
        return pair.step(boards, *lr)


def zero_pair(M, n, H, s):
    """The 2 x 4 set, one stage, every entry 0."""
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (), device=DEV)
    net.lut.zero_()
    return Pair(M, net, n, H, s)


def test_every_delta_of_the_edge_list_in_both_slots_of_a_terminal_board(M):
    """lr = 1 / 1 and H = 2, s = 1 on terminal boards whose two afterstates have pairwise distinct
    hits, so m = delta_k and every entry receives exactly one delta.  The entries under an
    afterstate hold 2^30 with the sign opposite to its delta, so the sum stays inside int32 and
    off INT32_MIN; err = -V(prev) is -+2^34 and g_k is chosen so that G_k, and with it delta_k,
    is each of INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX -- in slot 0 and, rotated by one,
    in slot 1."""
    deltas = list(DE.DELTAS)
    n, H, s = len(deltas), 2, 1
    prevs = DE.distinct_prev(NR.TUPLES_2x4, 2 * n, 700, highs=(0,))
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (), device=DEV)
    want = [[deltas[i] for i in range(n)], [deltas[(i + 1) % n] for i in range(n)]]
    lut = np.zeros(tuple(net.lut.shape), np.int32)
    for i in range(n):
        for k in range(2):
            v = (1 << 30) if want[k][i] < 0 else -(1 << 30) if want[k][i] > 0 else 0
            for t, idx in NR.Net(NR.TUPLES_2x4).indices(prevs[2 * i + k]):
                lut[0, t, idx] = v
    net.lut.copy_(dev(lut, np.int32))
    pair = Pair(M, net, n, H, s)
    hist = np.stack([prevs[0::2], prevs[1::2]])  # plane 0: k = 0 (head 0), plane 1: k = 1
    g = np.zeros((H, n), np.int64)
    for i in range(n):
        err = -pair.ref.net.V([int(x) for x in prevs[2 * i]])
        assert abs(err) in (0, 1 << 34)
        for k in range(2):
            g[k, i] = want[k][i] - R.collect(0, err, k, s)
    pair.set_ring(hist, np.zeros(n, np.uint8), np.full(n, 2, np.uint8), g)
    c = guarded_step(pair, np.array([CHECKER] * n, np.uint8), (1, 0))
    assert c.delta == want
    assert INT32_MIN in c.ms.values() and INT32_MAX in c.ms.values()
    assert all(cnt == 1 for _d, cnt in c.hits.values())
    got = pair.net.lut.cpu().numpy()
    assert int(got.min()) == (1 << 30) + INT32_MIN and int(got.max()) == -(1 << 30) + INT32_MAX


@pytest.mark.parametrize("sign", [1, -1])
def test_g_times_lr_num_next_to_2_to_the_59(M, sign):
    """lr = 2^16 / 2^31 on a zero table.  Terminal rows: err = 0 and G_k = g_k = +-(2^43 - 1) in
    every slot of a full window of H = 3.  Non-terminal rows (the board of sixteen 27s, err =
    2^41 exactly): the slot that leaves holds G = g + (2^41 >> 2 s), again +-(2^43 - 1) or next to
    it, and the kept slots store sums of 42 bits.  The product G * lr_num is a 59-bit number and
    delta = G >> 15 a 28-bit one."""
    n, H, s = 9, 3, 1
    top = (1 << 43) - 1
    pair = zero_pair(M, n, H, s)
    rng = np.random.default_rng(710)
    hist = np.stack([DE.low_boards(rng, n, hi=14) for _ in range(H)])
    g = np.zeros((H, n), np.int64)
    boards = np.array([CHECKER if i % 2 == 0 else ALL_27 for i in range(n)], np.uint8)
    head = (np.arange(n) % H).astype(np.uint8)
    for i in range(n):
        for k in range(H):
            p = (int(head[i]) - k) % H
            if i % 2 == 0:
                g[p, i] = sign * (top - k)
            else:  # err = 2^41: G_k = g_k + (2^41 >> k)
                g[p, i] = sign * top - (1 << 41 >> k) if sign > 0 else -top
    pair.set_ring(hist, head, np.full(n, H, np.uint8), g)
    c = guarded_step(pair, boards, (1 << 16, 31))
    assert c.errs == [0 if i % 2 == 0 else 1 << 41 for i in range(n)]
    for i in range(n):
        if i % 2 == 0:
            assert [c.delta[k][i] for k in range(H)] == [(sign * (top - k)) >> 15 for k in range(H)]
        else:
            G = sign * top if sign > 0 else -top + (1 << 39)
            assert [c.delta[k][i] for k in range(H)] == [0, 0, G >> 15]
    assert max(abs(x) for p in pair.ref.g for x in p) >= 1 << 41
    assert max(abs(d) for p in c.delta for d in p) == ((top >> 15) if sign > 0 else (top >> 15) + 1)


def test_lr_num_0_promotes_moves_nothing_and_still_turns_the_ring(M):
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 720)
    lut0 = net.lut.clone()
    n, H = 129, 3
    pair = Pair(M, net, n, H, 1)
    rng = np.random.default_rng(721)
    promoted, heads = 0, set()
    for t in range(H + 2):
        c = guarded_step(pair, batch(rng, n, t), (0, 5))
        assert any(c.errs) or t == 0
        assert not any(any(p) for p in c.delta) and not c.hits
        promoted += len(c.promoted)
        heads |= set(pair.ref.head)
    assert promoted > 100 and not bool(pair.st.ea.any())
    changed = net.lut != lut0
    assert int(changed.sum()) == promoted and bool((lut0[changed] == DE.UNSET).all())
    assert max(pair.ref.depth) == H and heads == set(range(H))
    assert bool(pair.st.g.any())  # the errors are still collected


def test_a_head_and_a_depth_out_of_range_in_memory_are_clamped(M):
    """head = 200 reads as H - 1 and depth = 255 as H, as g2048_ntlambda.hip clamps them: the
    reference runs on the clamped ring.  hist and g are the middle of larger buffers whose guard
    planes on either side must come back untouched."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 730, upper=1.0)
    n, H = 129, 3
    pair = Pair(M, net, n, H, 1)
    st = pair.st
    guard_h = torch.full((H + 2, n, 16), 0xAB, dtype=torch.uint8, device=DEV)
    guard_g = torch.full((H + 2, n), -(0x5A5A << 40), dtype=torch.int64, device=DEV)
    st.hist, st.g = guard_h[1:H + 1], guard_g[1:H + 1]
    assert st.hist.is_contiguous() and st.hist.data_ptr() % 16 == 0 and st.g.data_ptr() % 8 == 0
    rng = np.random.default_rng(731)
    hist, head, depth, g = random_ring(rng, n, H)
    pair.set_ring(hist, head, depth, g)
    bad_head, bad_depth = head.copy(), depth.copy()
    # rows that have a legal move in the first call (the terminal ones are i % 5 == 2), so that
    # its commit rewrites head; depth is rewritten by every commit
    bad_head[::5], bad_depth[1::5] = 200, 255
    bad_head[10], bad_depth[10] = H, H + 1
    st.head.copy_(dev(bad_head))
    st.depth.copy_(dev(bad_depth))
    pair.ref.head = [min(int(x), H - 1) for x in bad_head]
    pair.ref.depth = [min(int(x), H) for x in bad_depth]
    for t in range(2):
        c = guarded_step(pair, batch(rng, n, t), LR)
        assert any(c.hits)
        for guard, fill in ((guard_h, 0xAB), (guard_g, -(0x5A5A << 40))):
            assert bool((guard[0] == fill).all()) and bool((guard[-1] == fill).all())
    assert int(st.head.max()) < H and int(st.depth.max()) <= H
