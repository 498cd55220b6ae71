"""libg2048_stageback.so at the edges of the domain include/g2048_stageback.h declares, in the
manner of tests/domain_edge.py: every case is built from seeds, runs through the reference inside
domain_edge.InDomain (which fails the test when the *reference* leaves the domain) and is compared
bit for bit -- deltas of INT32_MIN and INT32_MAX, lr_num = 0, tables at the edges of int32,
counters above 2^31 and next to 2^32, and a cur and a rep_k that are out of range in memory."""
import numpy as np
import pytest
import torch

import domain_edge as DE
import ntuple_ref as NR
from g2048 import stageback as _library
from test_ntstage_gpu import dev, make_net
from test_stageback_gpu import (CHECKER, LR, M, NOT_WRITTEN, Pair,  # noqa: F401  (M: the fixture)
                                live_pool, outputs, script, scripted_batch, u32)

_library.load()
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT32_MIN, INT32_MAX = DE.INT32_MIN, DE.INT32_MAX


def guarded_step(pair, boards, lr, out=None):
    with DE.InDomain(pair.ref.net, pair.ref):
        return pair.step(boards, *lr, out=out)


def set_counters(pair, **values):
    """u32 values (numpy, [n]) into the named counters of both sides."""
    for name, v in values.items():
        v = np.asarray(v).astype(np.uint32)
        getattr(pair.st, name).copy_(dev(v.view(np.int32), np.int32))
        setattr(pair.ref, name, [int(x) for x in v])


def fill_buffers(pair, rng, hi=9):
    """Every slot of both buffers of every board holds a low board and a gain, on both sides."""
    n, L = pair.n, pair.L
    traj = np.stack([DE.low_boards(rng, 2 * L, hi=hi) for _ in range(n)]).reshape(n, 2, L, 16)
    gain = 4 * rng.integers(0, 1 << 8, (n, 2, L)).astype(np.uint32)
    pair.traj[:], pair.gain[:] = traj, gain
    pair.st.traj.copy_(dev(traj))
    pair.st.gain.copy_(dev(gain.view(np.int32), np.int32))
    pair.ref.traj = [[[[int(v) for v in row] for row in buf] for buf in per] for per in traj]
    pair.ref.gain = [[[int(v) for v in buf] for buf in per] for per in gain]


def test_every_delta_of_the_edge_list(M):
    """lr = 1 / 4 on boards that replay the last afterstate of their episode (target 0), whose
    hits are pairwise distinct, so m = delta and every entry receives exactly one delta.  The
    entries under an afterstate share -err evenly with the sign opposite to delta's, so every sum
    stays inside int32 and off INT32_MIN: delta is each of INT32_MIN, INT32_MIN + 1, -1, 0, 1,
    INT32_MAX."""
    rows = DE.solved_rows(NR.TUPLES_2x4, lr=(1, 2), seed=900)
    n = len(rows)
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (), device=DEV)
    lut = np.zeros(tuple(net.lut.shape), np.int32)
    for row in rows:
        for (t, idx), v in row.entries.items():
            lut[0, t, idx] = v
    net.lut.copy_(dev(lut, np.int32))
    pair = Pair(M, net, n, 2)
    for i, row in enumerate(rows):
        pair.set_replay(i, [row.prev])
    boards = live_pool(np.random.default_rng(901), n)
    c = guarded_step(pair, boards, (1, 2))
    assert c.deltas == list(DE.DELTAS) and c.errs == [row.err for row in rows]
    assert INT32_MIN in c.ms.values() and INT32_MAX in c.ms.values()
    assert all(cnt == 1 for _d, cnt in c.hits.values())
    assert pair.ref.rep_k == [1] * n and pair.ref.rec == [1] * n


def test_lr_num_0_promotes_moves_nothing_and_still_records_and_replays(M):
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 910)
    lut0 = net.lut.clone()
    n, L = 129, 3
    pair = Pair(M, net, n, L)
    rng = np.random.default_rng(911)
    pool, terminal = live_pool(rng), script(rng, n, L, 12)
    promoted = replays = 0
    for t in range(12):
        c = guarded_step(pair, scripted_batch(pool, terminal, t), (0, 5))
        assert not any(c.deltas) and not c.hits
        promoted += len(c.promoted)
        replays += sum(c.rep)
    assert promoted > 50 and replays > 3 * n and not bool(pair.st.ea.any())
    assert any(e for e in c.errs)
    changed = net.lut != lut0
    assert int(changed.sum()) == promoted and bool((lut0[changed] == DE.UNSET).all())
    assert max(pair.ref.rep_n) == 2 * L + 1 and max(pair.ref.rep_k) == L and any(pair.ref.rec)
    pair.close()


@pytest.mark.parametrize("edge,lr", [(True, (0, 0)), (False, (1, 31))])
def test_tables_at_the_edges_of_int32(M, edge, lr):
    """Bounds above the index clamp, stage 0 within 2^27 of the ends of int32, the stages above
    half UNSET.  edge: the other half is INT32_MIN + 1, the smallest value an entry may hold, read
    next to UNSETs in one burst, at lr_num = 0 (only promotions write).  Otherwise wide values at
    lr = 2^-31: an error of 40 bits is a delta of 9, inside the headroom.  Episodes of boards up to
    exponent 27 and gains up to 2^31, three calls, so targets with and without a successor."""
    bounds = DE.STAGE_BOUNDS[0]
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, bounds, device=DEV)
    net.lut.copy_(dev(DE.wide_staged(tuple(net.lut.shape), 920, edge=edge), np.int32))
    n, L = 65, 3
    pair = Pair(M, net, n, L)
    rng = np.random.default_rng(921)
    eps = DE.high_boards(rng, n * L, DE.CAP_LEARN)[rng.permutation(n * L)].reshape(n, L, 16)
    for i in range(n):
        # board 0: the largest gain there is, 2^31, which the plane holds as a 32-bit pattern
        pair.set_replay(i, eps[i], gains=4 * rng.integers(0, 1 << 26, L) if i else [1 << 31] * L)
    seen = set()
    for t in range(L):
        boards = DE.high_boards(rng, n, DE.CAP_LEARN)
        c = guarded_step(pair, boards, lr)
        assert all(c.rep) and max(abs(e) for e in c.errs) > 1 << 33
        assert bool(c.hits) == (lr[0] != 0)
        seen |= {k[0] for k in c.promoted}
    assert seen == {1, 2}


def test_counters_above_2_to_the_31_and_next_to_2_to_the_32(M):
    """L = 3.  rec = 2^32 - 2 (the largest the domain has) and other values above 2^31: the slot
    is rec mod 3 of the unsigned value.  rep_n above 2^31 with rep_k in 0..2: j = rep_n - 1 -
    rep_k is a 32-bit unsigned number whose residue mod 3 picks x and, one further, y.  rep_k
    above 2^31 idles.  An episode that closes hands such a rec to rep_n."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 930, upper=1.0)
    n, L = 129, 3
    pair = Pair(M, net, n, L)
    rng = np.random.default_rng(931)
    fill_buffers(pair, rng)
    big = np.array([(1 << 32) - 2, (1 << 32) - 3, (1 << 31) + 1, 1 << 31, (1 << 31) - 1, 7],
                   np.int64)
    i = np.arange(n)
    rec = big[i % 6]
    rep_n = big[(i // 2) % 6] + (big[(i // 2) % 6] < (1 << 32) - 2)  # up to 2^32 - 1
    rep_k = np.where(i % 5 == 4, big[i % 3], i % 3)
    set_counters(pair, rec=rec, rep_n=rep_n, rep_k=rep_k)
    pool = live_pool(rng)
    terminal = np.zeros((2, n), bool)
    # a rec of 2^32 - 1 is outside the domain of the next call unless that call closes the episode
    terminal[0, 3::7] = terminal[1, 1::4] = terminal[1, ::6] = True
    for t in range(2):
        before = list(pair.ref.rec)
        c = guarded_step(pair, scripted_batch(pool, terminal, t), LR)
        assert any(c.rep) and not all(c.rep) and any(c.hits)
        assert all(pair.ref.rep_n[j] == before[j] for j in c.closed) and c.closed
    assert max(pair.ref.rec) == (1 << 32) - 1 == max(pair.ref.rep_n)
    pair.close()


def test_a_cur_and_a_rep_k_out_of_range_in_memory_stay_inside_the_boards_planes(M):
    """cur = 0xFF counts as 1 (and closes to 0xFE); rep_k > rep_n idles.  traj, gain, x_out and
    every counter are the middle of larger buffers whose guard rows on either side must come back
    untouched."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 940, upper=1.0)
    n, L, pad = 129, 3, 16
    pair = Pair(M, net, n, L)
    st = pair.st
    guards = {"traj": torch.full((n + 2, 2, L, 16), 0xAB, dtype=torch.uint8, device=DEV),
              "gain": torch.full((n + 2, 2, L), 0x5A5A5A5, dtype=torch.int32, device=DEV),
              "x": torch.full((n + 2, 16), 0xCD, dtype=torch.uint8, device=DEV)}
    st.traj, st.gain = guards["traj"][1:n + 1], guards["gain"][1:n + 1]
    for name in ("cur", "rec", "rep_n", "rep_k"):
        own = getattr(st, name)
        fill = 0xEE if own.dtype == torch.uint8 else -0x1234567
        guards[name] = torch.full((n + 2 * pad,), fill, dtype=own.dtype, device=DEV)
        setattr(st, name, guards[name][pad:pad + n])
        getattr(st, name).zero_()
    assert st.traj.is_contiguous() and st.traj.data_ptr() % 16 == 0
    rng = np.random.default_rng(941)
    fill_buffers(pair, rng)
    i = np.arange(n)
    rep_n = 1 + i % 5
    rep_k = np.where(i % 4 == 1, rep_n + 1 + i % 7, i % 2)  # a quarter of them past rep_n
    set_counters(pair, rec=i % 4, rep_n=rep_n, rep_k=rep_k)
    cur = np.where(i % 3 == 0, 0xFF, i % 2).astype(np.uint8)
    st.cur.copy_(dev(cur))
    pair.ref.cur = [int(c) for c in cur]
    pool = live_pool(rng)
    terminal = np.zeros((3, n), bool)
    terminal[0, 2::5] = terminal[1, ::4] = terminal[2, 1::3] = True
    fills = {"traj": 0xAB, "gain": 0x5A5A5A5, "x": 0xCD, "cur": 0xEE, "rec": -0x1234567,
             "rep_n": -0x1234567, "rep_k": -0x1234567}
    for t in range(3):
        out = list(outputs(n))
        guards["x"][1:n + 1] = NOT_WRITTEN
        out[2] = guards["x"][1:n + 1]
        c = guarded_step(pair, scripted_batch(pool, terminal, t), LR, out=tuple(out))
        assert any(c.rep) and not all(c.rep) and c.closed
        for name, g in guards.items():
            lo = pad if g.dim() == 1 else 1
            assert bool((g[:lo] == fills[name]).all()) and bool((g[-lo:] == fills[name]).all()), name
    assert 0xFE in pair.ref.cur and 0xFF in pair.ref.cur
    assert any(k > r for k, r in zip(pair.ref.rep_k, pair.ref.rep_n))
    pair.close()
