"""Batch-mean TD learning on the multi-stage network on the GPU (csrc/g2048_stagemean.hip ->
libg2048_stagemean.so) against the plain Python restatement tests/stagemean_ref.py: the table with
its UNSET pattern, prev, has_prev, action, err and delta bit for bit and acc all zero after every
call -- at the frames' edges, for every T and S, on the hand anchors, on crafted batches -- the
rule's four equalities against the other libraries, the 4 x 6 set, the trainer, a captured step,
and that self-play learns."""
import numpy as np
import pytest
import torch

import ntstage_ref as SR
import ntuple_ref as NR
import stagemean_ref as R
from oracle import oracle as O
from test_ntstage_gpu import EDGES, SparseBase, T8M3, dev, lists, make_net, stage_boards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSET = SR.UNSET
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
A = [1, 1] + [0] * 14
T8M2 = tuple((t, (t + 5) % 16) for t in range(8))
T8M4 = tuple((t, t + 1, t + 4, t + 5) for t in range(8))
SPECS = {"corner": ((0,),), "edges": EDGES, "2x4": NR.TUPLES_2x4, "T8m2": T8M2}
# 1, 2: a dead half-wave and a full wave of the policy frame; 7, 9: around a wave of the gather /
# apply frame (8 boards); 127, 128, 129: around their block; 1031: nine blocks, a ragged tail
SIZES = (1, 2, 7, 9, 127, 128, 129, 1031)
LR = (3, 6)  # deltas of about 2^20 on a table of +-2^20: nothing leaves int32


class Modules:
    def __init__(self, ntuple, ntstage, ntmean, stagemean):
        self.NT, self.NS, self.MEAN, self.SM = ntuple, ntstage, ntmean, stagemean


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmean, ntstage, ntuple, stagemean
    for mod in (ntuple, ntstage, ntmean, stagemean):
        mod.load()
    return Modules(ntuple, ntstage, ntmean, stagemean)


def outputs(n):
    return (torch.full((n,), 9, dtype=torch.uint8, device=DEV),
            torch.full((n,), 77, dtype=torch.int32, device=DEV),
            torch.full((n,), 77, dtype=torch.int64, device=DEV))


class Pair:
    """A staged network and its batch-mean workspace on the GPU next to the reference over a
    host copy of the table."""

    def __init__(self, M, net):
        self.net = net
        self.mean = M.SM.StagedMeanState(net)
        self.base = net.lut.cpu().numpy().copy()
        self.ref = SR.StagedNet(net.spec.tuples, net.bounds, base=self.base)

    def want_table(self):
        want = self.base.copy()
        for s, entries in enumerate(self.ref.stages):
            for (t, i), v in entries.items():
                want[s, t, i] = v
        return want

    def step(self, boards, prev, has_prev, lr_num, lr_shift):
        """One mean_step on both sides from the same state (prev, has_prev: lists, updated in
        place); everything is compared, the UNSET pattern first.  Returns (actions, errs, deltas,
        the reference's hits)."""
        n = len(boards)
        dprev, dhas, out = dev(prev), dev(has_prev), outputs(n)
        self.mean.mean_step(dev(boards), dprev, dhas, lr_num, lr_shift, *out)
        acts, errs, deltas = R.step(self.ref, lists(boards), prev, has_prev, lr_num, lr_shift)
        got, want = self.net.lut.cpu().numpy(), self.want_table()
        assert np.array_equal(got == UNSET, want == UNSET)
        assert np.array_equal(got, want)
        assert out[0].cpu().tolist() == acts
        assert out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == deltas
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        assert not bool(self.mean.acc.any())
        return acts, errs, deltas, dict(R.last_hits)


def run_steps(M, net, rng, n, steps=3, caps=(4, 7, 11)):
    """`steps` mean_steps on fresh random boards of all stages.  The first call starts from
    random previous afterstates with a quarter of the rows without one; prev then carries over,
    so a board and its previous afterstate are unrelated (any error, either sign).  A terminal
    board sits in every batch."""
    pair = Pair(M, net)
    prev = lists(stage_boards(rng, n, caps))
    has_prev = [int(i % 4 != 1) for i in range(n)]
    seen, signs, hits_all = set(), set(), {}
    for t in range(steps):
        boards = stage_boards(rng, n, caps)
        if n > 2:
            boards[(t + 1) % n] = CHECKER
        seen |= {pair.ref.stage(p) for p, h in zip(prev, has_prev) if h}
        _a, _e, deltas, hits = pair.step(boards, prev, has_prev, *LR)
        signs |= {d > 0 for d in deltas if d}
        hits_all.update(hits)
    return pair, seen, signs, hits_all


# ------------------------------------------------------------------ sizes, T and S
@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("spec", list(SPECS))
def test_mean_step_at_wave_and_block_edges(M, spec, n, fresh):
    """Every size class on four specs with the bounds (5, 8), on a fresh (all-UNSET) table and
    on one with random stage 0 and a random half of the upper stages set."""
    net = make_net(M.NS, SPECS[spec], (5, 8), None if fresh else 301)
    pair, seen, signs, hits = run_steps(M, net, np.random.default_rng(310 + n), n)
    if n >= 127:
        assert seen == {0, 1, 2} and signs == {True, False}
        assert any(c > 8 for _d, c in hits.values())   # an entry more than one board hits
        assert any(d % c for d, c in hits.values())    # a quotient that floors
        assert {k[0] for k in hits} == {0, 1, 2}
    assert net.set_counts() == [int((row != UNSET).sum()) for row in pair.want_table()]


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(M, T):
    """Every instantiation of the three kernels: the first T tuples of an 8 x 3 set."""
    net = make_net(M.NS, T8M3[:T], (5, 8), 320 + T)
    pair, seen, _signs, hits = run_steps(M, net, np.random.default_rng(330 + T), 129)
    assert seen == {0, 1, 2} and {k[1] for k in hits} == set(range(T))


@pytest.mark.parametrize("S", range(1, 9))
def test_every_stage_count(M, S):
    """S = 1..8 with bounds at 2, 4, 5, 6, 7, 8, 10; a quarter of the upper stages' entries
    set, so fall-throughs of every depth occur."""
    bounds = (2, 4, 5, 6, 7, 8, 10)[:S - 1]
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 340 + S, upper=0.25)
    pair, seen, _signs, hits = run_steps(M, net, np.random.default_rng(350 + S), 129,
                                         caps=(1, 3, 4, 5, 6, 7, 9, 11))
    assert seen == set(range(S)) == {k[0] for k in hits}


# ------------------------------------------------------------------ the anchors, on the device
def corner_pair(M, bounds):
    net = M.NS.StagedNTupleNetwork(((0,),), bounds, device=DEV)
    net.lut[0, 0].copy_(1024 * torch.arange(16, dtype=torch.int32, device=DEV))
    return Pair(M, net)


def entries(pair):
    got = pair.net.lut.cpu().numpy()
    return {(int(s), int(t), int(i)): int(got[s, t, i]) for s, t, i in np.argwhere(got != UNSET)
            if s > 0 or got[s, t, i] != 1024 * i}


def test_anchor_two_stages_promoted_and_moved_in_one_call(M):
    pair = corner_pair(M, (2, 3))
    P1, P2 = [1, 0, 0, 0, 0, 2] + [0] * 10, [1, 0, 0, 0, 0, 3] + [0] * 10
    acts, _e, deltas, hits = pair.step(np.array([CHECKER, A], np.uint8), [P1, P2], [1, 1], 1, 1)
    assert (acts, deltas) == ([0, 2], [-1024, 3072])
    assert entries(pair) == {(1, 0, 1): 0, (1, 0, 0): -1024, (2, 0, 1): 4096, (2, 0, 0): 3072}


def test_anchors_two_deltas_on_one_staged_entry(M):
    Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
    pair = corner_pair(M, (2,))
    has_prev = [1, 1, 1]
    _a, _e, deltas, hits = pair.step(np.array([A, CHECKER, CHECKER], np.uint8),
                                     [list(Q2), list(Q3), list(Q3)], has_prev, 1, 1)
    assert deltas == [2048, -3072, -3072] and has_prev == [1, 0, 0]
    assert hits == {(1, 0, 2): (4096, 2), (1, 0, 3): (-12288, 4), (1, 0, 0): (-24576, 18)}
    assert entries(pair) == {(1, 0, 2): 4096, (1, 0, 3): 0, (1, 0, 0): -1366}
    pair = corner_pair(M, (2,))
    pair.step(np.array([A, A, CHECKER], np.uint8), [list(Q2), list(Q2), list(Q3)], [1, 1, 1], 1, 1)
    assert entries(pair) == {(1, 0, 0): 341, (1, 0, 2): 4096, (1, 0, 3): 0}


def test_anchor_a_hot_index_is_split_by_stage(M):
    Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
    pair = corner_pair(M, (3,))
    _a, _e, _d, hits = pair.step(np.array([A, CHECKER, CHECKER], np.uint8),
                                 [list(Q2), list(Q3), list(Q3)], [1, 1, 1], 1, 1)
    assert hits[(0, 0, 0)] == (12288, 6) and hits[(1, 0, 0)] == (-36864, 12)
    assert pair.ref.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert entries(pair) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): -3072}


def test_anchor_lr_num_0_promotes_and_moves_nothing(M):
    pair = corner_pair(M, (2,))
    P1 = [1, 0, 0, 0, 0, 2] + [0] * 10
    _a, errs, deltas, hits = pair.step(np.array([A, A], np.uint8), [P1, [3] + [0] * 15], [1, 0],
                                       0, 1)
    assert errs == [6144, 0] and deltas == [0, 0] and not hits
    assert entries(pair) == {(1, 0, 1): 1024, (1, 0, 0): 0}


# ------------------------------------------------------------------ crafted batches
def test_129_copies_of_one_board(M):
    """One staged entry set hit by every board: C = 8 * 129 and above on the coinciding pairs,
    many promotions of one entry, one block of 128 boards and one more."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 360)
    net.lut[1:].fill_(UNSET)
    pair = Pair(M, net)
    b = [6, 3, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0, 1, 0, 0, 2]
    p = [7, 1, 0, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 2]
    n = 129
    prev, has_prev = [list(p) for _ in range(n)], [1] * n
    _a, _e, deltas, hits = pair.step(np.array([b] * n, np.uint8), prev, has_prev, 1, 4)
    assert len(set(deltas)) == 1 and deltas[0] != 0
    assert all(c % n == 0 and d == c * deltas[0] for d, c in hits.values())
    assert len(pair.ref.promoted) == len(hits) and {k[0] for k in hits} == {1}
    # all 8 symmetries of a one-valued board coincide: one entry per tuple, C = 8 * 129
    same = [5] * 16
    _a, _e, deltas, hits = pair.step(np.array([b] * n, np.uint8), [list(same) for _ in range(n)],
                                     [1] * n, 1, 4)
    assert deltas[0] != 0 and sorted(c for _d, c in hits.values()) == [8 * n, 8 * n]


def test_an_entry_promoted_by_a_zero_delta_board_and_hit_by_another(M):
    """Corner spec, bounds (2,), stage 1 UNSET.  Board B = a single 4-tile in cell 1 moves left
    to [2, 0, ...]: q = 4096 = V(prev = [2, 0, ...]), err = delta = 0, so it only promotes
    (1, 0, 2) and (1, 0, 0); board A with the same prev hits both with delta 2048.  B sits in
    another block of the policy launch than A."""
    pair = corner_pair(M, (2,))
    B = [0, 2] + [0] * 14
    n = 130
    boards = np.array([B] * (n - 1) + [A], np.uint8)
    prev, has_prev = [[2] + [0] * 15 for _ in range(n)], [1] * n
    _a, errs, deltas, hits = pair.step(boards, prev, has_prev, 1, 1)
    assert deltas == [0] * (n - 1) + [2048] and errs[-1] == 4096
    assert hits == {(1, 0, 2): (4096, 2), (1, 0, 0): (12288, 6)}
    assert pair.ref.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0}
    assert entries(pair) == {(1, 0, 2): 4096, (1, 0, 0): 2048}


OVERFLOW_SEED = 371


def test_more_entries_than_either_lds_table_holds(M):
    """T = 8, m = 4, two stages, 128 random full boards: one block whose distinct staged entries
    exceed the gather's 4096 slots and crowd the apply's 8192, so hits that find no slot after
    four probes go straight to memory beside merged ones, in both launches."""
    net = make_net(M.NS, T8M4, (10,), 370, upper=0.3)
    pair = Pair(M, net)
    rng = np.random.default_rng(OVERFLOW_SEED)
    n = 128
    prev0 = rng.integers(1, 12, (n, 16)).astype(np.uint8)
    boards = rng.integers(0, 12, (n, 16)).astype(np.uint8)
    _a, _e, deltas, hits = pair.step(boards, lists(prev0), [1] * n, 7, 5)
    assert len(hits) > 4096 and {k[0] for k in hits} == {0, 1} and pair.ref.promoted
    assert any(c > 1 for _d, c in hits.values())


# ------------------------------------------------------------------ the four equalities
def random_plain(M, tuples, seed):
    net = M.NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


def test_s1_without_unset_is_the_single_table_library(M):
    plain = random_plain(M, NR.TUPLES_2x4, 380)
    staged = M.NS.StagedNTupleNetwork.from_network(plain, ())
    ms, sm = M.MEAN.MeanState(plain), M.SM.StagedMeanState(staged)
    rng = np.random.default_rng(381)
    n = 1031
    prev0, has0 = stage_boards(rng, n), (np.arange(n) % 5 != 0).astype(np.uint8)
    pa, pb, ha, hb = dev(prev0), dev(prev0), dev(has0), dev(has0)
    for t in range(3):
        boards = stage_boards(rng, n)
        boards[t] = CHECKER
        oa, ob = outputs(n), outputs(n)
        ms.mean_step(dev(boards), pa, ha, *LR, *oa)
        sm.mean_step(dev(boards), pb, hb, *LR, *ob)
        for x, y in zip(oa + (pa, ha), ob + (pb, hb)):
            assert torch.equal(x, y), t
        assert torch.equal(staged.lut[0], plain.lut), t
        assert not bool(sm.acc.any())
    assert int(oa[1].abs().sum()) > 0


def distinct_staged_batch(tuples, bounds, n, seed):
    """n previous afterstates whose 8 T n staged hits are pairwise distinct, of every stage."""
    rng = np.random.default_rng(seed)
    ref, seen, keep = SR.StagedNet(tuples, bounds), set(), []
    for _try in range(100000):
        hi = (bounds[0], bounds[1], 12)[len(keep) % 3]
        p = rng.integers(1, hi, 16).astype(np.uint8)
        keys = [(ref.stage(p), *k) for k in ref.indices([int(x) for x in p])]
        if len(set(keys)) == len(keys) and seen.isdisjoint(keys):
            seen.update(keys)
            keep.append(p)
            if len(keep) == n:
                break
    assert len(keep) == n and {ref.stage(p) for p in keep} == {0, 1, 2}
    return np.stack(keep)


def test_a_batch_of_pairwise_distinct_staged_hits_is_the_staged_td_step(M):
    n, bounds = 129, (9, 11)
    rng = np.random.default_rng(390)
    boards, prev0 = dev(stage_boards(rng, n)), distinct_staged_batch(NR.TUPLES_2x4, bounds, n, 391)
    has0 = np.ones(n, np.uint8)
    td = make_net(M.NS, NR.TUPLES_2x4, bounds, 392)
    lut0 = td.lut.clone()
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs(n)
    td.td_step(boards, td_prev, td_has, *LR, *td_out)
    assert not torch.equal(td.lut, lut0)
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 392)
    sm = M.SM.StagedMeanState(net)
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    sm.mean_step(boards, prev, has_prev, *LR, *out)
    assert torch.equal(net.lut, td.lut)
    for a, b in zip(out + (prev, has_prev), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    assert not bool(sm.acc.any())


def test_a_batch_given_three_times_leaves_the_table_of_the_batch_given_once(M):
    n = 129
    rng = np.random.default_rng(400)
    boards, prev0 = stage_boards(rng, n), stage_boards(rng, n)
    has0 = (np.arange(n) % 5 != 0).astype(np.uint8)
    luts = []
    for k in (1, 3):
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 401)
        sm = M.SM.StagedMeanState(net)
        sm.mean_step(dev(np.tile(boards, (k, 1))), dev(np.tile(prev0, (k, 1))),
                     dev(np.tile(has0, k)), *LR, *outputs(k * n))
        luts.append(net.lut.clone())
        assert not bool(sm.acc.any())
    assert torch.equal(luts[0], luts[1])
    assert not torch.equal(luts[0], make_net(M.NS, NR.TUPLES_2x4, (5, 8), 401).lut)
    td = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 401)  # the sum rule does not have the property
    td.td_step(dev(np.tile(boards, (3, 1))), dev(np.tile(prev0, (3, 1))), dev(np.tile(has0, 3)),
               *LR, *outputs(3 * n))
    assert not torch.equal(td.lut, luts[0])


def test_lr_num_0_is_the_staged_td_step_at_lr_num_0(M):
    n = 129
    rng = np.random.default_rng(410)
    boards, prev0 = dev(stage_boards(rng, n)), stage_boards(rng, n)
    has0 = (np.arange(n) % 4 != 1).astype(np.uint8)
    td = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411)
    lut0 = td.lut.clone()
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs(n)
    td.td_step(boards, td_prev, td_has, 0, 6, *td_out)
    assert not torch.equal(td.lut, lut0)  # promotions
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411)
    sm = M.SM.StagedMeanState(net)
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    sm.mean_step(boards, prev, has_prev, 0, 6, *out)
    assert torch.equal(net.lut, td.lut) and not bool(out[1].any())
    for a, b in zip(out + (prev, has_prev), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    assert not bool(sm.acc.any())


# ------------------------------------------------------------------ the 4 x 6 set
def test_4x6_two_stages_touched_entries_and_set_counts(M):
    """The 4 x 6 table with bounds (11,) (512 MiB, 2 GiB of acc), 128 boards, 2 steps: the touched
    entries (gathered, not a dense copy), the set counts and acc.any()."""
    rng = np.random.default_rng(420)
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_4x6, (11,), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(421)
    net.lut[0].copy_(torch.randint(-(1 << 20), 1 << 20, net.lut[0].shape, generator=g, device=DEV,
                                   dtype=torch.int32))
    sm = M.SM.StagedMeanState(net)
    assert sm.acc.numel() * 8 == 2 << 30
    base = SparseBase(net.lut[0])
    ref = SR.StagedNet(net.spec.tuples, net.bounds, base=base)
    stage0 = net.lut.shape[1] * net.lut.shape[2]
    n = 128
    prev, has_prev = lists(stage_boards(rng, n, caps=(5, 9, 11))), [1] * n
    for _t in range(2):
        boards = stage_boards(rng, n, caps=(5, 9, 11))
        keys = []
        for b in lists(boards) + prev:
            keys += ref.indices(b)
            for a in range(4):
                keys += ref.indices(NR.E.move(b, a)[0])
        base.prefetch(keys)
        dprev, dhas, out = dev(prev), dev(has_prev), outputs(n)
        sm.mean_step(dev(boards), dprev, dhas, 5, 9, *out)
        acts, errs, deltas = R.step(ref, lists(boards), prev, has_prev, 5, 9)
        assert out[0].cpu().tolist() == acts and out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == deltas
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        ent = sorted(ref.set_entries())
        idx = [torch.tensor([k[j] for k in ent], dtype=torch.long, device=DEV) for j in range(3)]
        assert net.lut[idx[0], idx[1], idx[2]].cpu().tolist() == [ref.stages[s][(t, i)]
                                                                  for s, t, i in ent]
        assert net.set_counts() == [stage0, len(ref.stages[1])]
        assert not bool(sm.acc.any())
    assert len(ref.stages[0]) > 500 and len(ref.stages[1]) > 500


# ------------------------------------------------------------------ trainer, graph
def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 430)
        tr = M.SM.StagedMeanTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.mean.acc.any())
        return net.lut, tr.env.board, tr.prev, tr.delta

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], make_net(M.NS, NR.TUPLES_2x4, (3, 5), 430).lut)


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """StagedMeanTrainer at 64 boards on the 2x4 set with bounds (7,), at its default rate, next
    to the reference driving an OracleEnv: actions, err, delta, prev, has_prev and the whole
    table after each of 50 steps, acc all zero.  A low bound besides, so stage 1 is reached."""
    for bounds, n, seed in (((7,), 64, 47), ((3,), 64, 48)):
        net = make_net(M.NS, NR.TUPLES_2x4, bounds, 440)
        net.lut[1:].fill_(UNSET)
        base = net.lut.cpu().numpy().copy()
        tr = M.SM.StagedMeanTrainer(net, n, seed=seed)
        assert (tr.lr_num, tr.lr_shift) == (1, 6)
        ref = SR.StagedNet(NR.TUPLES_2x4, bounds, base=base)
        oracle = O.OracleEnv(n, seed)
        ref_prev, ref_has = [[0] * 16 for _ in range(n)], [0] * n
        for t in range(50):
            boards = oracle.board.copy()
            assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
            tr.step(1)
            acts, errs, deltas = R.step(ref, lists(boards), ref_prev, ref_has, 1, 6)
            oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
            assert tr.actions.cpu().tolist() == acts, t
            assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == deltas, t
            assert tr.prev.cpu().tolist() == ref_prev and tr.has_prev.cpu().tolist() == ref_has, t
            want = base.copy()
            for s, ents in enumerate(ref.stages):
                for (k, i), v in ents.items():
                    want[s, k, i] = v
            assert np.array_equal(net.lut.cpu().numpy(), want), t
            assert not bool(tr.mean.acc.any()), t
        if bounds == (3,):
            assert len(ref.stages[1]) > 100
        tr.env.check_errors()


def test_captured_mean_step_and_env_step_replays(M):
    """mean_step + env.step captured once and replayed 3 times equals 3 eager steps: table (with
    the promotions of each step), boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    start = stage_boards(np.random.default_rng(450), 192)

    def make():
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 451)
        tr = M.SM.StagedMeanTrainer(net, 192, seed=45)
        tr.env.board.copy_(dev(start))
        tr.step(2)  # a state with afterstates on every board
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "prev", "has_prev", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {"lut": net.lut.cpu().clone(), "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(3):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    lut0 = net.lut.clone()
    st0 = {k: getattr(tr, k).clone() for k in ("prev", "has_prev")}
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert torch.equal(net.lut, lut0) and not bool(tr.mean.acc.any())
    assert all(torch.equal(getattr(tr, k), v) for k, v in st0.items())
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = state(net, tr)
        for name, t in want[k].items():
            assert torch.equal(got[name], t), (k, name)
        assert not bool(tr.mean.acc.any())
    tr.env.check_errors()


def test_restart_keyword_works_as_in_the_other_trainers(M):
    import g2048

    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (4,), device=DEV)
    pool = g2048.RestartPool(64, (3, 0, 4), device=DEV, stagger=True)
    tr = M.SM.StagedMeanTrainer(net, 64, seed=49, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and all(net.set_counts()) and not bool(tr.mean.acc.any())
    with pytest.raises(ValueError):
        M.SM.StagedMeanTrainer(net, 32, restart=pool)
    with pytest.raises(TypeError):
        M.SM.StagedMeanTrainer(M.NT.NTupleNetwork(NR.TUPLES_2x4, device=DEV), 64)
    tr.env.check_errors()


# ------------------------------------------------------------------ it learns
def test_staged_self_play_learns_under_batch_mean(M):
    """The recipe of test_ntmean_gpu.py::test_self_play_learns_under_batch_mean on the staged
    network of test_ntstage_gpu.py::test_staged_self_play_learns: TUPLES_2x4, bounds (7,), 256
    boards, p(4) = 0.5, the default rate 2^-6, seed 61, 4000 steps.  The mean merge score of the
    last 200 finished episodes is at least twice the random player's mean on the same seed (880,
    the project's bar), stage 1 has set entries and no set entry exceeds 2^28 in magnitude.  The
    figures are printed.  Measured on an MI355X: 4955 over the last 200 of 4450 episodes, 2945 and
    15 011 set entries in stages 0 and 1, largest |entry| 510 433."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (7,), device=DEV)
    tr = M.SM.StagedMeanTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MEAN.default_mean_lr_shift(net.spec) == 6
    scores = []
    for _ in range(4):
        tr.step(1000)
        scores += tr.episodes()["score"].tolist()
    tr.env.check_errors()
    rnd = BatchedPlayer(256, device=DEV, seed=seed).play("random")
    learned, random_mean = float(np.mean(scores[-200:])), float(rnd.merge_score.mean())
    is_set = net.lut != UNSET
    largest = int(torch.where(is_set, net.lut, torch.zeros_like(net.lut)).to(torch.int64)
                  .abs().max())
    print(f"staged batch-mean 2x4, bounds (7,), after 4000 steps: {learned:.0f} over the last 200 "
          f"of {len(scores)} episodes, set entries {net.set_counts()}, largest |entry| {largest}; "
          f"random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert net.set_counts()[1] > 0
    assert largest <= 1 << 28
    assert not bool(tr.mean.acc.any())
