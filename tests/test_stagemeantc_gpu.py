"""Temporal-coherence learning on the batch-mean rule for the multi-stage network on the GPU
(csrc/g2048_stagemeantc.hip -> libg2048_stagemeantc.so) against the plain Python restatement
tests/stagemeantc_ref.py: the table with its UNSET pattern, ea, prev, has_prev, action, err and
delta bit for bit and acc all zero after every call.  State carries across calls, so every case
makes three consecutive calls, from a zero ea and from a seeded one that holds every branch of the
rate in every stage -- at the frames' edges, for every T and S, on the hand anchors, on crafted
batches -- then the header's consequences next to the other libraries, the 4 x 6 set, the trainer,
a captured step, the restart pool, a resumed run, from_state, and that self-play learns."""
import numpy as np
import pytest
import torch

import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR
import stagemeantc_ref as R
from g2048 import stagemeantc as _library
from oracle import oracle as O
from test_ntstage_gpu import SparseBase, T8M3, dev, lists, make_net, stage_boards
from test_stagemean_gpu import (LR, SIZES, SPECS, T8M4, distinct_staged_batch, outputs,
                                random_plain)

_library.load()  # without the library the file fails here, before any case
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSET = SR.UNSET
ONE = 1 << 16
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
A = [1, 1] + [0] * 14
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15


class Modules:
    def __init__(self, ntuple, ntstage, stagemean, ntmeantc, stagemeantc):
        self.NT, self.NS, self.SM, self.MTC, self.SMTC = (ntuple, ntstage, stagemean, ntmeantc,
                                                          stagemeantc)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmeantc, ntstage, ntuple, stagemean, stagemeantc
    for mod in (ntuple, ntstage, stagemean, ntmeantc, stagemeantc):
        mod.load()
    return Modules(ntuple, ntstage, stagemean, ntmeantc, stagemeantc)


def seeded_ea(shape, seed):
    """int64 [S, T, N, 2] on the host: (E, A) with |E| <= A.  The kind of an entry follows
    (i + 3 t) mod 8 in the order 0 1 3 2 6 4 5 7 -- the low indices, which every stage's boards
    hit most, hold a zero rate and the slow rates -- the same in every stage, so every stage holds
    the whole mix:
      0  A < 2^16, E = 0 (rate 0)          4  A of 41-50 bits, E = +A (rate 2^16)
      1  A < 2^16, 0 < |E| < A             5  A of 41-50 bits, E = -A (rate 2^16)
      2  A = 0 (rate 2^16)                 6  A of 41-50 bits, 0 < |E| < A
      3  A within 2 of 2^16, 0 < |E| < A   7  A within 2 of 2^16, E = 0 (rate 0)"""
    S, T, N = shape
    rng = np.random.default_rng(seed)
    order = np.array([0, 1, 3, 2, 6, 4, 5, 7])
    kind = np.broadcast_to(order[(np.arange(N)[None, :] + 3 * np.arange(T)[:, None]) % 8], shape)
    small = rng.integers(256, 1 << 16, shape)
    near = (1 << 16) + rng.integers(-2, 3, shape)
    big = rng.integers(1 << 40, 1 << 50, shape)
    part = rng.integers(1, 8, shape)          # |E| = part eighths of A
    sign = rng.choice(np.array([-1, 1]), shape)
    a = np.select([kind <= 1, kind == 2, (kind == 3) | (kind == 7)], [small, 0, near], big)
    e = np.select([(kind == 0) | (kind == 2) | (kind == 7), kind == 4, kind == 5],
                  [0, a, -a], sign * (a // 8 * part))
    assert (np.abs(e) <= a).all() and (a >= 0).all()
    return np.ascontiguousarray(np.stack((e, a), axis=-1).astype(np.int64))


class Call:
    """What one call did, from the reference: outputs, hits, m, and the rate every moved entry was
    scaled by."""

    def __init__(self, acts, errs, deltas, mt, rates):
        self.acts, self.errs, self.deltas = acts, errs, deltas
        self.hits, self.ms, self.rates = dict(mt.last_hits), dict(mt.last_m), rates
        self.promoted = dict(mt.net.promoted)


class Pair:
    """A staged network, its workspace and its accumulators on the GPU next to the reference over
    host copies of the table and of the ea it starts from (ea0: None = zeros)."""

    def __init__(self, M, net, ea0=None):
        self.net = net
        self.state = M.SMTC.StagedMeanTCState(net)
        self.base = net.lut.cpu().numpy().copy()
        base_ea = None
        if ea0 is not None:
            self.state.ea.copy_(torch.from_numpy(ea0))
            base_ea = lambda s, t, i: (int(ea0[s, t, i, 0]), int(ea0[s, t, i, 1]))  # noqa: E731
        self.ea0 = np.zeros((*self.base.shape, 2), np.int64) if ea0 is None else ea0
        self.ref = R.StagedMeanTC(SR.StagedNet(net.spec.tuples, net.bounds, base=self.base),
                                  base_ea=base_ea)

    def want_table(self):
        want = self.base.copy()
        for s, entries in enumerate(self.ref.net.stages):
            for (t, i), v in entries.items():
                want[s, t, i] = v
        return want

    def want_ea(self):
        want = self.ea0.copy()
        for (s, t, i), a in self.ref.A.items():
            want[s, t, i] = (self.ref.E[(s, t, i)], a)
        return want

    def step(self, boards, prev, has_prev, lr_num, lr_shift):
        """One meantc_step on both sides from the same state (prev, has_prev: lists, updated in
        place); everything is compared, the UNSET pattern first."""
        n = len(boards)
        dprev, dhas, out = dev(prev), dev(has_prev), outputs(n)
        self.state.meantc_step(dev(boards), dprev, dhas, lr_num, lr_shift, *out)
        mt = self.ref
        before = (dict(mt.E), dict(mt.A))
        acts, errs, deltas = mt.step(lists(boards), prev, has_prev, lr_num, lr_shift)
        rates = {k: TR.rate(before[0][k], before[1][k]) if k in before[1]
                 else TR.rate(*mt.base_ea(*k)) for k, m in mt.last_m.items() if m}
        got, want = self.net.lut.cpu().numpy(), self.want_table()
        assert np.array_equal(got == UNSET, want == UNSET)
        assert np.array_equal(got, want)
        assert np.array_equal(self.state.ea.cpu().numpy(), self.want_ea())
        assert out[0].cpu().tolist() == acts
        assert out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == deltas
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        assert not bool(self.state.acc.any())
        return Call(acts, errs, deltas, mt, rates)


def run_steps(M, net, rng, n, ea0=None, steps=3, caps=(4, 7, 11)):
    """`steps` meantc_steps on fresh random boards of all stages.  The first call starts from
    random previous afterstates with a quarter of the rows without one; prev then carries over,
    so a board and its previous afterstate are unrelated (any error, either sign).  A terminal
    board sits in every batch.  Returns the pair, the stages prev spanned and the calls."""
    pair = Pair(M, net, ea0)
    prev = lists(stage_boards(rng, n, caps))
    has_prev = [int(i % 4 != 1) for i in range(n)]
    seen, calls = set(), []
    for t in range(steps):
        boards = stage_boards(rng, n, caps)
        if n > 2:
            boards[(t + 1) % n] = CHECKER
        seen |= {pair.ref.net.stage(p) for p, h in zip(prev, has_prev) if h}
        calls.append(pair.step(boards, prev, has_prev, *LR))
    return pair, seen, calls


def not_vacuous(n, fresh, seeded, seen, calls, stages=(0, 1, 2)):
    """The conditions that keep a frame-edge case from passing vacuously, from the reference."""
    hits = {k: v for c in calls for k, v in c.hits.items()}
    if n >= 127:
        assert seen == set(stages)
        assert {k[0] for k in hits} == set(stages)
        assert {d > 0 for c in calls for d in c.deltas if d} == {True, False}
        assert any(c > 8 for _d, c in hits.values())   # an entry more than one board hits
        assert any(d % c for c_ in calls for d, c in c_.hits.values())  # a quotient that floors
        if fresh:
            assert any(c.promoted for c in calls)
    if seeded and n >= 9:
        for s in stages:
            rates = [r for c in calls for k, r in c.rates.items() if k[0] == s]
            assert any(0 < r < ONE for r in rates), s  # a moved entry at a slow rate
            assert 0 in rates, s                       # and one whose errors had cancelled


# ------------------------------------------------------------------ sizes, T and S
@pytest.mark.parametrize("seeded", [False, True])
@pytest.mark.parametrize("fresh", [True, False])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("spec", list(SPECS))
def test_meantc_step_at_wave_and_block_edges(M, spec, n, fresh, seeded):
    """Every size class on four specs with the bounds (5, 8), on a fresh (all-UNSET) table and
    on one with random stage 0 and a random half of the upper stages set, from a zero and from a
    seeded ea, three calls each."""
    net = make_net(M.NS, SPECS[spec], (5, 8), None if fresh else 301)
    ea0 = seeded_ea(tuple(net.lut.shape), 302) if seeded else None
    pair, seen, calls = run_steps(M, net, np.random.default_rng(310 + n), n, ea0)
    not_vacuous(n, fresh, seeded, seen, calls)
    assert net.set_counts() == [int((row != UNSET).sum()) for row in pair.want_table()]


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(M, T):
    """Every instantiation of the three kernels: the first T tuples of an 8 x 3 set."""
    net = make_net(M.NS, T8M3[:T], (5, 8), 320 + T)
    ea0 = seeded_ea(tuple(net.lut.shape), 325 + T)
    pair, seen, calls = run_steps(M, net, np.random.default_rng(330 + T), 129, ea0)
    assert seen == {0, 1, 2}
    assert {k[1] for c in calls for k in c.hits} == set(range(T))
    assert any(0 < r < ONE for c in calls for r in c.rates.values())


@pytest.mark.parametrize("S", range(1, 9))
def test_every_stage_count(M, S):
    """S = 1..8 with bounds at 2, 4, 5, 6, 7, 8, 10; a quarter of the upper stages' entries
    set, so fall-throughs of every depth occur; a seeded ea in every stage."""
    bounds = (2, 4, 5, 6, 7, 8, 10)[:S - 1]
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 340 + S, upper=0.25)
    ea0 = seeded_ea(tuple(net.lut.shape), 345 + S)
    pair, seen, calls = run_steps(M, net, np.random.default_rng(350 + S), 129, ea0,
                                  caps=(1, 3, 4, 5, 6, 7, 9, 11))
    moved = {k[0] for c in calls for k, m in c.ms.items() if m}
    assert seen == set(range(S)) == {k[0] for c in calls for k in c.hits} == moved
    assert {k[0] for k in pair.ref.A} == set(range(S))


# ------------------------------------------------------------------ the anchors, on the device
def corner_pair(M, bounds, preset=None, tuples=((0,),), lut0=None):
    net = M.NS.StagedNTupleNetwork(tuples, bounds, device=DEV)
    n = net.lut.shape[2]
    row = 1024 * np.arange(n) if lut0 is None else np.asarray(lut0)
    net.lut[0, 0].copy_(dev(row, np.int32))
    ea0 = None
    if preset:
        ea0 = np.zeros((*net.lut.shape, 2), np.int64)
        for k, v in preset.items():
            ea0[k] = v
    pair = Pair(M, net, ea0)
    pair.lut0 = row
    return pair


def entries(pair):
    got = pair.net.lut.cpu().numpy()
    return {(int(s), int(t), int(i)): int(got[s, t, i]) for s, t, i in np.argwhere(got != UNSET)
            if s > 0 or got[s, t, i] != pair.lut0[i]}


def ea_entries(pair):
    got = pair.state.ea.cpu().numpy()
    return {(int(s), int(t), int(i)): (int(got[s, t, i, 0]), int(got[s, t, i, 1]))
            for s, t, i in np.argwhere(got.any(axis=-1))}


def test_anchor_1_the_stage_split_three_times(M):
    pair = corner_pair(M, (3,))
    boards = np.array([A, CHECKER, CHECKER], np.uint8)

    def call():
        return pair.step(boards, [list(Q2), list(Q3), list(Q3)], [1, 1, 1], 1, 1)

    c = call()
    assert c.deltas == [2048, -3072, -3072] and c.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert entries(pair) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    assert ea_entries(pair) == {(0, 0, 2): (2048, 2048), (0, 0, 0): (2048, 2048),
                                (1, 0, 3): (-3072, 3072), (1, 0, 0): (-3072, 3072)}
    c = call()
    assert c.deltas == [2048, 9216, 9216] and not c.promoted
    assert set(c.rates.values()) == {ONE}
    assert entries(pair) == {(0, 0, 2): 6144, (0, 0, 0): 4096, (1, 0, 3): 9216, (1, 0, 0): 6144}
    assert ea_entries(pair) == {(0, 0, 2): (4096, 4096), (0, 0, 0): (4096, 4096),
                                (1, 0, 3): (6144, 12288), (1, 0, 0): (6144, 12288)}
    c = call()
    assert c.deltas == [2048, -27648, -27648]
    assert c.rates == {(0, 0, 2): ONE, (0, 0, 0): ONE, (1, 0, 3): 32768, (1, 0, 0): 32768}
    assert entries(pair) == {(0, 0, 2): 8192, (0, 0, 0): 6144, (1, 0, 3): -4608,
                             (1, 0, 0): -7680}
    assert ea_entries(pair) == {(0, 0, 2): (6144, 6144), (0, 0, 0): (6144, 6144),
                                (1, 0, 3): (-21504, 39936), (1, 0, 0): (-21504, 39936)}
    assert pair.state.rate(-21504, 39936) == 35288 and pair.state.rate(6144, 6144) == ONE


def test_anchor_2_a_cancelled_entry_in_one_stage_only(M):
    pair = corner_pair(M, (3,), preset={(1, 0, 0): (0, 7)})
    c = pair.step(np.array([A, CHECKER, CHECKER], np.uint8), [list(Q2), list(Q3), list(Q3)],
                  [1, 1, 1], 1, 1)
    assert c.rates[(1, 0, 0)] == 0 and c.rates[(0, 0, 0)] == ONE
    assert entries(pair) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): 0}
    assert ea_entries(pair) == {(0, 0, 2): (2048, 2048), (0, 0, 0): (2048, 2048),
                                (1, 0, 3): (-3072, 3072), (1, 0, 0): (-3072, 3079)}


def test_anchor_3_m_equal_to_zero(M):
    pair = corner_pair(M, (2,), preset={(1, 0, 0): (5, 9)})
    has_prev = [1, 1, 1]
    c = pair.step(np.array([A, A, CHECKER], np.uint8), [list(Q2), list(Q2), list(Q3)], has_prev,
                  1, 12)
    assert c.deltas == [1, 1, -2] and has_prev == [1, 1, 0]
    assert c.hits == {(1, 0, 2): (4, 4), (1, 0, 0): (0, 18), (1, 0, 3): (-4, 2)}
    assert c.ms == {(1, 0, 2): 1, (1, 0, 0): 0, (1, 0, 3): -2}
    assert c.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0, (1, 0, 3): 3072}
    assert entries(pair) == {(1, 0, 2): 2049, (1, 0, 0): 0, (1, 0, 3): 3070}
    assert ea_entries(pair) == {(1, 0, 2): (1, 1), (1, 0, 3): (-2, 2), (1, 0, 0): (5, 9)}


def test_anchor_4_two_stages_promoted_and_moved_in_one_call(M):
    pair = corner_pair(M, (2, 3))
    P1, P2 = [1, 0, 0, 0, 0, 2] + [0] * 10, [1, 0, 0, 0, 0, 3] + [0] * 10
    c = pair.step(np.array([CHECKER, A], np.uint8), [P1, P2], [1, 1], 1, 1)
    assert (c.acts, c.deltas) == ([0, 2], [-1024, 3072])
    assert entries(pair) == {(1, 0, 1): 0, (1, 0, 0): -1024, (2, 0, 1): 4096, (2, 0, 0): 3072}
    assert ea_entries(pair) == {(1, 0, 1): (-1024, 1024), (1, 0, 0): (-1024, 1024),
                                (2, 0, 1): (3072, 3072), (2, 0, 0): (3072, 3072)}


def test_anchor_5_the_two_floors_and_a_41_bit_a_at_stage_0_of_a_two_stage_net(M):
    lut0 = [0] * 256
    lut0[33] = lut0[5] = 1
    pair = corner_pair(M, (12,), preset={(0, 0, 33): (1, 2)}, tuples=((0, 1),), lut0=lut0)
    X1 = [1, 2] + [0] * 14
    X2 = list(X1)
    X2[11], X2[15] = 6, 5
    c = pair.step(np.array([CHECKER, CHECKER], np.uint8), [X1, X2], [1, 1], 1, 0)
    assert c.deltas == [-1, -2] and c.hits[(0, 0, 33)] == (-3, 2) and c.ms[(0, 0, 33)] == -2
    assert c.rates[(0, 0, 33)] == 1 << 15
    got = entries(pair)
    assert got[(0, 0, 33)] == 0 and got[(0, 0, 1)] == -2 and got[(0, 0, 0)] == -2
    assert ea_entries(pair)[(0, 0, 33)] == (-1, 4) and not any(k[0] for k in got)
    big = (-3 << 38, (1 << 40) + 12345)
    pair = corner_pair(M, (12,), preset={(0, 0, 0): big})
    c = pair.step(np.array([A], np.uint8), [list(Q2)], [1], 1, 1)
    assert c.rates[(0, 0, 0)] == 49152
    assert entries(pair) == {(0, 0, 2): 4096, (0, 0, 0): 1536}
    assert ea_entries(pair) == {(0, 0, 2): (2048, 2048), (0, 0, 0): (big[0] + 2048, big[1] + 2048)}


# ------------------------------------------------------------------ crafted batches
def test_129_copies_of_one_board(M):
    """One staged entry set hit by every board: C = 8 * 129 and above on the coinciding pairs,
    many promotions of one entry, one block of 128 boards and one more; three calls, so the
    later ones run at the rates the first left."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 360)
    net.lut[1:].fill_(UNSET)
    pair = Pair(M, net, seeded_ea(tuple(net.lut.shape), 361))
    b = [6, 3, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0, 1, 0, 0, 2]
    p = [7, 1, 0, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 2]
    n = 129
    for k in range(2):
        c = pair.step(np.array([b] * n, np.uint8), [list(p) for _ in range(n)], [1] * n, 1, 4)
        assert len(set(c.deltas)) == 1 and c.deltas[0] != 0
        assert all(cnt % n == 0 and d == cnt * c.deltas[0] for d, cnt in c.hits.values())
        assert all(m == c.deltas[0] for m in c.ms.values()) and {k_[0] for k_ in c.hits} == {1}
        assert (len(c.promoted) == len(c.hits)) if k == 0 else not c.promoted
    # all 8 symmetries of a one-valued board coincide: one entry per tuple, C = 8 * 129
    same = [5] * 16
    c = pair.step(np.array([b] * n, np.uint8), [list(same) for _ in range(n)], [1] * n, 1, 4)
    assert c.deltas[0] != 0 and sorted(cnt for _d, cnt in c.hits.values()) == [8 * n, 8 * n]


def test_an_entry_promoted_by_a_zero_delta_board_and_hit_by_another(M):
    """Corner spec, bounds (2,), stage 1 UNSET.  Board B = a single 4-tile in cell 1 moves left
    to [2, 0, ...]: q = 4096 = V(prev = [2, 0, ...]), err = delta = 0, so it only promotes
    (1, 0, 2) and (1, 0, 0); board A with the same prev hits both with delta 2048.  B sits in
    another block of the policy launch than A.  (1, 0, 0) holds a half rate."""
    pair = corner_pair(M, (2,), preset={(1, 0, 0): (-3, 6)})
    B = [0, 2] + [0] * 14
    n = 130
    boards = np.array([B] * (n - 1) + [A], np.uint8)
    c = pair.step(boards, [list(Q2) for _ in range(n)], [1] * n, 1, 1)
    assert c.deltas == [0] * (n - 1) + [2048] and c.errs[-1] == 4096
    assert c.hits == {(1, 0, 2): (4096, 2), (1, 0, 0): (12288, 6)}
    assert c.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0}
    assert entries(pair) == {(1, 0, 2): 4096, (1, 0, 0): 1024}
    assert ea_entries(pair) == {(1, 0, 2): (2048, 2048), (1, 0, 0): (2045, 2054)}


def test_more_entries_than_either_lds_table_holds(M):
    """T = 8, m = 4, two stages, 128 random full boards: one block whose distinct staged entries
    exceed the gather's 4096 slots and crowd the apply's 8192, so hits that find no slot after
    four probes go straight to memory beside merged ones, in both launches.  The second call hits
    the same entries again: the owners of the direct path read back the (E, A) they stored."""
    net = make_net(M.NS, T8M4, (10,), 370, upper=0.3)
    pair = Pair(M, net)
    rng = np.random.default_rng(371)
    n = 128
    prev0 = rng.integers(1, 12, (n, 16)).astype(np.uint8)
    calls = []
    for _k in range(2):
        boards = rng.integers(0, 12, (n, 16)).astype(np.uint8)
        calls.append(pair.step(boards, lists(prev0), [1] * n, 7, 5))
    for c in calls:
        assert len(c.hits) > 4096 and {k[0] for k in c.hits} == {0, 1}
        assert any(cnt > 1 for _d, cnt in c.hits.values())
    assert calls[0].promoted and not calls[1].promoted
    first = {k for k, m in calls[0].ms.items() if m}
    # (from a zero ea an entry moved once holds |E| = A: the second call's rates are still 2^16,
    # what it reads back is the (m, |m|) it adds to)
    assert sum(1 for k, m in calls[1].ms.items() if m and k in first) > 4096


# ------------------------------------------------------------------ the header's consequences
def test_consequence_1_a_zero_ea_is_the_staged_batch_mean_step(M):
    n = 1031
    rng = np.random.default_rng(380)
    boards, prev0 = dev(stage_boards(rng, n)), stage_boards(rng, n)
    has0 = (np.arange(n) % 5 != 0).astype(np.uint8)
    nets = [make_net(M.NS, NR.TUPLES_2x4, (5, 8), 381) for _ in range(3)]
    sm, st = M.SM.StagedMeanState(nets[0]), M.SMTC.StagedMeanTCState(nets[1])
    outs = []
    for step in (sm.mean_step, st.meantc_step):
        prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
        step(boards, prev, has_prev, *LR, *out)
        outs.append(out + (prev, has_prev))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    assert torch.equal(nets[1].lut, nets[0].lut)
    # the promoted table, by the staged TD step at lr_num = 0: m is what the call added to it
    nets[2].td_step(boards, dev(prev0), dev(has0), 0, 6, *outputs(n))
    promoted = nets[2].lut
    assert torch.equal(promoted == UNSET, nets[1].lut == UNSET)
    m = torch.where(promoted == UNSET, 0, nets[1].lut.to(torch.int64) - promoted.to(torch.int64))
    assert int(m.count_nonzero()) > 1000 and int((m != 0).any(dim=2).any(dim=1).sum()) == 3
    assert torch.equal(st.ea, torch.stack((m, m.abs()), dim=-1))
    assert not bool(st.acc.any())


def test_consequence_2_s1_without_unset_is_the_single_table_library(M):
    plain = random_plain(M, NR.TUPLES_2x4, 390)
    staged = M.NS.StagedNTupleNetwork.from_network(plain, ())
    one, st = M.MTC.MeanTCState(plain), M.SMTC.StagedMeanTCState(staged)
    ea0 = torch.from_numpy(seeded_ea(tuple(staged.lut.shape), 391)).to(DEV)
    one.ea.copy_(ea0[0])
    st.ea.copy_(ea0)
    rng = np.random.default_rng(392)
    n = 1031
    prev0, has0 = stage_boards(rng, n), (np.arange(n) % 5 != 0).astype(np.uint8)
    pa, pb, ha, hb = dev(prev0), dev(prev0), dev(has0), dev(has0)
    for t in range(3):
        boards = stage_boards(rng, n)
        boards[t] = CHECKER
        oa, ob = outputs(n), outputs(n)
        one.meantc_step(dev(boards), pa, ha, *LR, *oa)
        st.meantc_step(dev(boards), pb, hb, *LR, *ob)
        for x, y in zip(oa + (pa, ha), ob + (pb, hb)):
            assert torch.equal(x, y), t
        assert torch.equal(staged.lut[0], plain.lut), t
        assert torch.equal(st.ea[0], one.ea), t
        assert not bool(st.acc.any())
    assert int(oa[1].abs().sum()) > 0 and not torch.equal(st.ea, ea0)


def test_consequence_3_pairwise_distinct_staged_hits_are_the_staged_td_step(M):
    n, bounds = 129, (9, 11)
    rng = np.random.default_rng(400)
    boards, prev0 = dev(stage_boards(rng, n)), distinct_staged_batch(NR.TUPLES_2x4, bounds, n, 401)
    has0 = np.ones(n, np.uint8)
    td = make_net(M.NS, NR.TUPLES_2x4, bounds, 402)
    lut0 = td.lut.clone()
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs(n)
    td.td_step(boards, td_prev, td_has, *LR, *td_out)
    assert not torch.equal(td.lut, lut0)
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 402)
    st = M.SMTC.StagedMeanTCState(net)
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    st.meantc_step(boards, prev, has_prev, *LR, *out)
    assert torch.equal(net.lut, td.lut)
    for a, b in zip(out + (prev, has_prev), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    assert not bool(st.acc.any()) and bool(st.ea.any())


def test_consequences_4_and_5_repetition_and_a_zero_rate(M):
    n = 129
    rng = np.random.default_rng(410)
    boards, prev0 = stage_boards(rng, n), stage_boards(rng, n)
    has0 = (np.arange(n) % 5 != 0).astype(np.uint8)
    shape = tuple(make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411).lut.shape)
    ea0 = torch.from_numpy(seeded_ea(shape, 412)).to(DEV)
    got = []
    for k in (1, 3):
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411)
        st = M.SMTC.StagedMeanTCState(net)
        st.ea.copy_(ea0)
        st.meantc_step(dev(np.tile(boards, (k, 1))), dev(np.tile(prev0, (k, 1))),
                       dev(np.tile(has0, k)), *LR, *outputs(k * n))
        got.append((net.lut.clone(), st.ea.clone()))
        assert not bool(st.acc.any())
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert not torch.equal(got[0][0], make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411).lut)
    assert not torch.equal(got[0][1], ea0)
    # lr_num = 0: the staged TD step at lr_num = 0 (it promotes), ea as it was
    td = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411)
    lut0 = td.lut.clone()
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs(n)
    td.td_step(dev(boards), td_prev, td_has, 0, 6, *td_out)
    assert not torch.equal(td.lut, lut0)  # promotions
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 411)
    st = M.SMTC.StagedMeanTCState(net)
    st.ea.copy_(ea0)
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    st.meantc_step(dev(boards), prev, has_prev, 0, 6, *out)
    assert torch.equal(net.lut, td.lut) and torch.equal(st.ea, ea0)
    assert not bool(out[1].any()) and bool(out[2].any())
    for a, b in zip(out + (prev, has_prev), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    assert not bool(st.acc.any())


# ------------------------------------------------------------------ the 4 x 6 set
def test_4x6_two_stages_touched_entries_set_counts_and_ea(M):
    """The 4 x 6 table with bounds (11,) (512 MiB, 2 GiB of acc, 2 GiB of ea), 129 boards, three
    calls: the touched staged entries of lut and ea (gathered, not a dense copy), the set counts,
    the number of entries with a non-zero A, and acc.any().  Staged indices reach past 2^24, and
    2 e + 1 past 2^25, in words of 8 bytes: the size_t arithmetic."""
    rng = np.random.default_rng(420)
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_4x6, (11,), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(421)
    net.lut[0].copy_(torch.randint(-(1 << 20), 1 << 20, net.lut[0].shape, generator=g, device=DEV,
                                   dtype=torch.int32))
    st = M.SMTC.StagedMeanTCState(net)
    assert st.acc.numel() * 8 == 2 << 30 == st.ea.numel() * 8
    base = SparseBase(net.lut[0])
    mt = R.StagedMeanTC(SR.StagedNet(net.spec.tuples, net.bounds, base=base))
    ref = mt.net
    stage0 = net.lut.shape[1] * net.lut.shape[2]
    n = 129
    prev, has_prev = lists(stage_boards(rng, n, caps=(5, 9, 11))), [1] * n
    for _t in range(3):
        boards = stage_boards(rng, n, caps=(5, 9, 11))
        keys = []
        for b in lists(boards) + prev:
            keys += ref.indices(b)
            for a in range(4):
                keys += ref.indices(NR.E.move(b, a)[0])
        base.prefetch(keys)
        dprev, dhas, out = dev(prev), dev(has_prev), outputs(n)
        st.meantc_step(dev(boards), dprev, dhas, 5, 9, *out)
        acts, errs, deltas = mt.step(lists(boards), prev, has_prev, 5, 9)
        assert out[0].cpu().tolist() == acts and out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == deltas
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        ent = sorted(ref.set_entries())
        idx = [torch.tensor([k[j] for k in ent], dtype=torch.long, device=DEV) for j in range(3)]
        assert net.lut[idx[0], idx[1], idx[2]].cpu().tolist() == [ref.stages[s][(t, i)]
                                                                  for s, t, i in ent]
        assert st.ea[idx[0], idx[1], idx[2]].cpu().tolist() == [list(mt.get_ea(*k)) for k in ent]
        assert net.set_counts() == [stage0, len(ref.stages[1])]
        assert int(st.ea[..., 1].count_nonzero()) == sum(1 for a in mt.A.values() if a)
        assert not bool(st.acc.any())
    assert len(ref.stages[0]) > 500 and len(ref.stages[1]) > 500
    assert {k[0] for k in mt.A} == {0, 1}


# ------------------------------------------------------------------ trainer, graph
def test_e_stays_within_a_over_200_trainer_steps(M):
    net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 430)
    tr = M.SMTC.StagedMeanTCTrainer(net, 1024, seed=43)
    tr.step(200)
    torch.cuda.synchronize()
    ea = tr.state.ea
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all()) and bool((ea[..., 1] >= 0).all())
    # errors of both signs met on some entries: a rate below 1 is in use; every stage has moved
    assert bool((ea[..., 0].abs() < ea[..., 1]).any())
    assert bool((ea[..., 1] > 0).any(dim=2).any(dim=1).all())
    assert int(ea[..., 1].max()) <= 200 << 31  # at most 2^31 per call
    assert not bool(tr.state.acc.any())
    tr.env.check_errors()


def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 430)
        tr = M.SMTC.StagedMeanTCTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.state.acc.any())
        return net.lut, tr.state.ea, tr.env.board, tr.prev, tr.delta

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], make_net(M.NS, NR.TUPLES_2x4, (3, 5), 430).lut)
    assert bool(a[1].any())


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """StagedMeanTCTrainer at 64 boards on the 2x4 set with bounds (7,), at its default rate,
    next to the reference driving an OracleEnv: actions, err, delta, prev, has_prev, the whole
    table and the whole ea after each of 50 steps, acc all zero.  A low bound besides, so stage 1
    is reached."""
    for bounds, n, seed in (((7,), 64, 47), ((3,), 64, 48)):
        net = make_net(M.NS, NR.TUPLES_2x4, bounds, 440)
        net.lut[1:].fill_(UNSET)
        base = net.lut.cpu().numpy().copy()
        tr = M.SMTC.StagedMeanTCTrainer(net, n, seed=seed)
        assert (tr.lr_num, tr.lr_shift) == (1, 4)
        mt = R.StagedMeanTC(SR.StagedNet(NR.TUPLES_2x4, bounds, base=base))
        oracle = O.OracleEnv(n, seed)
        ref_prev, ref_has = [[0] * 16 for _ in range(n)], [0] * n
        slowed = 0
        for t in range(50):
            boards = oracle.board.copy()
            assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
            tr.step(1)
            before = (dict(mt.E), dict(mt.A))
            acts, errs, deltas = mt.step(lists(boards), ref_prev, ref_has, 1, 4)
            slowed += any(0 < TR.rate(before[0][k], before[1][k]) < ONE
                          for k, m in mt.last_m.items() if m and k in before[1])
            oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
            assert tr.actions.cpu().tolist() == acts, t
            assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == deltas, t
            assert tr.prev.cpu().tolist() == ref_prev and tr.has_prev.cpu().tolist() == ref_has, t
            want = base.copy()
            for s, ents in enumerate(mt.net.stages):
                for (k, i), v in ents.items():
                    want[s, k, i] = v
            assert np.array_equal(net.lut.cpu().numpy(), want), t
            want_ea = np.zeros((*base.shape, 2), np.int64)
            for (s, k, i), a in mt.A.items():
                want_ea[s, k, i] = (mt.E[(s, k, i)], a)
            assert np.array_equal(tr.state.ea.cpu().numpy(), want_ea), t
            assert not bool(tr.state.acc.any()), t
        assert slowed >= 10  # moved entries at a rate below 1, in at least ten of the steps
        if bounds == (3,):
            assert len(mt.net.stages[1]) > 100 and any(k[0] == 1 for k in mt.A)
        tr.env.check_errors()


def test_captured_meantc_step_and_env_step_replays(M):
    """meantc_step + env.step captured once and replayed 3 times equals 3 eager steps: table
    (with the promotions of each step), ea, boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    start = stage_boards(np.random.default_rng(450), 192)

    def make():
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 451)
        tr = M.SMTC.StagedMeanTCTrainer(net, 192, seed=45)
        tr.env.board.copy_(dev(start))
        tr.step(2)  # a state with afterstates on every board
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "prev", "has_prev", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {"lut": net.lut.cpu().clone(), "ea": tr.state.ea.cpu().clone(),
                 "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(3):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    lut0, ea0 = net.lut.clone(), tr.state.ea.clone()
    st0 = {k: getattr(tr, k).clone() for k in ("prev", "has_prev")}
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert torch.equal(net.lut, lut0) and torch.equal(tr.state.ea, ea0)
    assert not bool(tr.state.acc.any())
    assert all(torch.equal(getattr(tr, k), v) for k, v in st0.items())
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = state(net, tr)
        for name, t in want[k].items():
            assert torch.equal(got[name], t), (k, name)
        assert not bool(tr.state.acc.any())
    tr.env.check_errors()


def test_restart_keyword_works_as_in_the_other_trainers(M):
    import g2048

    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (4,), device=DEV)
    pool = g2048.RestartPool(64, (3, 0, 4), device=DEV, stagger=True)
    tr = M.SMTC.StagedMeanTCTrainer(net, 64, seed=49, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and all(net.set_counts()) and not bool(tr.state.acc.any())
    assert bool(tr.state.ea[0].any()) and bool(tr.state.ea[1].any())
    with pytest.raises(ValueError):
        M.SMTC.StagedMeanTCTrainer(net, 32, restart=pool)
    with pytest.raises(TypeError):
        M.SMTC.StagedMeanTCTrainer(M.NT.NTupleNetwork(NR.TUPLES_2x4, device=DEV), 64)
    with pytest.raises(ValueError):  # another network's state
        M.SMTC.StagedMeanTCTrainer(M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (4,), device=DEV), 64,
                                   state=tr.state)
    tr.env.check_errors()


def test_a_run_resumes_bit_for_bit_from_a_saved_ea(M, tmp_path):
    """30 steps, save ea, 20 more; a second run of 30 steps takes the file's ea in a new state
    and ends where the first did.  With a zeroed ea it does not."""
    def start():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 460)
        tr = M.SMTC.StagedMeanTCTrainer(net, 256, seed=46)
        tr.step(30)
        torch.cuda.synchronize()
        return net, tr

    net, tr = start()
    tr.state.save(tmp_path / "ea.pt")
    tr.step(20)
    torch.cuda.synchronize()
    want = (net.lut.clone(), tr.state.ea.clone(), tr.env.board.clone())

    net, tr = start()
    loaded = M.SMTC.StagedMeanTCState.load(tmp_path / "ea.pt", net)
    assert loaded is not tr.state and torch.equal(loaded.ea, tr.state.ea)
    assert loaded.ea.device == net.lut.device and not bool(loaded.acc.any())
    tr.state = loaded
    tr.step(20)
    torch.cuda.synchronize()
    for x, y in zip(want, (net.lut, tr.state.ea, tr.env.board)):
        assert torch.equal(x, y)

    net, tr = start()
    tr.state.ea.zero_()
    tr.step(20)
    torch.cuda.synchronize()
    assert not torch.equal(net.lut, want[0])


def test_from_state_continues_a_single_table_run_staged(M):
    """30 single-table steps, then the same batch on the single table and on from_network /
    from_state with a bound no board reaches: stage 0 moves as the single table does, lut and ea
    alike, and stage 1 stays UNSET with a zero ea."""
    plain = random_plain(M, NR.TUPLES_2x4, 470)
    tr = M.MTC.MeanTCTrainer(plain, 256, seed=50)
    tr.step(30)
    torch.cuda.synchronize()
    staged = M.NS.StagedNTupleNetwork.from_network(plain, (14,))
    st = M.SMTC.StagedMeanTCState.from_state(tr.state, staged)
    assert torch.equal(st.ea[0], tr.state.ea) and not bool(st.ea[1].any()) and bool(st.ea.any())
    assert st.ea.data_ptr() != tr.state.ea.data_ptr()
    n = 256
    boards = tr.env.board.clone()
    pa, ha, pb, hb = tr.prev.clone(), tr.has_prev.clone(), tr.prev.clone(), tr.has_prev.clone()
    oa, ob = outputs(n), outputs(n)
    tr.state.meantc_step(boards, pa, ha, 1, 4, *oa)
    st.meantc_step(boards, pb, hb, 1, 4, *ob)
    for x, y in zip(oa + (pa, ha), ob + (pb, hb)):
        assert torch.equal(x, y)
    assert bool(oa[1].any())
    assert torch.equal(staged.lut[0], plain.lut) and torch.equal(st.ea[0], tr.state.ea)
    assert bool((staged.lut[1] == UNSET).all()) and not bool(st.ea[1].any())


# ------------------------------------------------------------------ it learns
def test_staged_self_play_learns_under_batch_mean_tc(M):
    """The recipe of test_stagemean_gpu.py::test_staged_self_play_learns_under_batch_mean with
    this step: TUPLES_2x4, bounds (7,), 256 boards, p(4) = 0.5, the default rate 2^-4 (8 T lr =
    1), seed 61, 4000 steps.  The mean merge score of the last 200 finished episodes is at least
    twice the random player's mean on the same seed (880, the project's bar), stage 1 has set
    entries, no set entry exceeds 2^28 in magnitude and |E| <= A everywhere.  The figures are
    printed.  Measured on an MI355X: 7512 over the last 200 of 3067 episodes, 2908 and 19 625 set
    entries in stages 0 and 1 (2908 and 19 621 of them with A > 0), largest |entry| 735 217
    (DESIGN 4.20)."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (7,), device=DEV)
    tr = M.SMTC.StagedMeanTCTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MTC.default_meantc_lr_shift(net.spec) == 4
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
    ea = tr.state.ea
    print(f"staged batch-mean TC 2x4, bounds (7,), after 4000 steps: {learned:.0f} over the last "
          f"200 of {len(scores)} episodes, set entries {net.set_counts()}, largest |entry| "
          f"{largest}, entries with A > 0 per stage "
          f"{ea[..., 1].count_nonzero(dim=(1, 2)).tolist()}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert net.set_counts()[1] > 0
    assert largest <= 1 << 28
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all())
    assert not bool(tr.state.acc.any())
