"""The multi-stage n-tuple kernels (csrc/g2048_ntstage.hip -> libg2048_ntstage.so) against the
plain Python restatement tests/ntstage_ref.py: values, policy and TD steps bit for bit -- the whole
table with its UNSET pattern, prev, has_prev, actions, err and delta after every step -- and
against libg2048_ntuple.so at S = 1, a captured step, reproducibility, and that self-play
learns."""
import numpy as np
import pytest
import torch

import ntstage_ref as R
import ntuple_ref as NR
from boards import mask_boards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
EDGES = ((0, 1, 2, 3), (0, 3, 12, 15))  # no symmetry of these reads a centre cell (5, 6, 9, 10)
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
UNSET = R.UNSET


@pytest.fixture(scope="module")
def NS():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntstage, ntuple
    ntuple.load()
    ntstage.load()
    return ntstage


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def stage_boards(rng, n, caps=(4, 7, 11)):
    """Random exponents 0..11 at 60 % fill, each board capped at one of `caps`, so that with the
    bounds (5, 8) every stage occurs in a batch (an uncapped board of 16 cells nearly always
    holds an 8)."""
    b = rng.integers(1, 12, (n, 16)) * (rng.random((n, 16)) < 0.6)
    return np.minimum(b, rng.choice(caps, (n, 1))).astype(np.uint8)


def make_net(NS, tuples, bounds, seed=None, upper=0.5):
    """A staged network: fresh (seed None), or random int32 in +-2^20 in stage 0 and in a random
    `upper` share of the higher stages' entries."""
    net = NS.StagedNTupleNetwork(tuples, bounds, device=DEV)
    if seed is not None:
        g = torch.Generator(device=DEV).manual_seed(seed)
        rnd = torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                            dtype=torch.int32)
        keep = torch.rand(net.lut.shape, generator=g, device=DEV) < upper
        keep[0] = True
        net.lut.copy_(torch.where(keep, rnd, torch.full_like(rnd, UNSET)))
    return net


class Pair:
    """A staged network on the GPU next to the reference over a host copy of its table."""

    def __init__(self, net):
        self.net = net
        self.base = net.lut.cpu().numpy().copy()
        self.ref = R.StagedNet(net.spec.tuples, net.bounds, base=self.base)

    def want_table(self):
        want = self.base.copy()
        for s, entries in enumerate(self.ref.stages):
            for (t, i), v in entries.items():
                want[s, t, i] = v
        return want

    def check_values_and_act(self, boards):
        got = self.net.values(dev(boards)).cpu().tolist()
        assert got == [self.ref.V(b) for b in boards]
        acts, q, after = self.net.act(dev(boards), after=True)
        for i, b in enumerate(boards):
            qs, a, aft = self.ref.policy(b)
            assert [NR.INT64_MIN if x is None else x for x in qs] == q[i].cpu().tolist(), i
            assert int(acts[i]) == a and after[i].cpu().tolist() == aft, i

    def step(self, boards, prev, has_prev, lr_num, lr_shift, err_out=True):
        """One td_step on both sides from the same state (prev, has_prev: lists, updated in
        place); everything is compared.  Returns (actions, errs, deltas)."""
        n = len(boards)
        dprev, dhas = dev(prev), dev(has_prev)
        out_a = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        out_d = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        out_e = torch.full((n,), 77, dtype=torch.int64, device=DEV) if err_out else None
        self.net.td_step(dev(boards), dprev, dhas, lr_num, lr_shift, out_a, out_d, out_e)
        acts, errs, deltas = self.ref.td_step(boards, prev, has_prev, lr_num, lr_shift)
        assert out_a.cpu().tolist() == acts
        assert out_d.cpu().tolist() == deltas
        if err_out:
            assert out_e.cpu().tolist() == errs
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        got, want = self.net.lut.cpu().numpy(), self.want_table()
        assert np.array_equal(got == UNSET, want == UNSET)
        assert np.array_equal(got, want)
        return acts, errs, deltas


def lists(a):
    return [[int(x) for x in row] for row in a]


def run_steps(NS, net, rng, n, steps=3, lr=(3, 6), terminal=False):
    """`steps` td_steps on fresh random boards of all stages (prev carries over, so a board's
    previous afterstate and its board are unrelated: any error, either sign)."""
    pair = Pair(net)
    prev, has_prev = [[0] * 16 for _ in range(n)], [0] * n
    seen = set()
    for t in range(steps):
        boards = stage_boards(rng, n)
        if terminal and n > 2:
            boards[(t + 1) % n] = CHECKER
        if t == 0:
            pair.check_values_and_act(boards)
        pair.step(boards, prev, has_prev, *lr)
        seen |= {pair.ref.stage(p) for p, h in zip(prev, has_prev) if h}
    return pair, seen


# ------------------------------------------------------------------ sizes, T and S
@pytest.mark.parametrize("n", [1, 7, 9, 129])
@pytest.mark.parametrize("fresh", [True, False])
def test_values_act_td_step_at_wave_group_and_block_edges(NS, n, fresh):
    """n = 1, 7, 9, 129: a dead half-wave, a partly filled wave of the 8-board kernels, one
    board past it, and one board past the update's 128-board block.  On a fresh (all-UNSET)
    table and on one with random stage 0 and a random half of the upper stages set."""
    net = make_net(NS, NR.TUPLES_2x4, (5, 8), None if fresh else 101)
    pair, seen = run_steps(NS, net, np.random.default_rng(200 + n), n, terminal=True)
    if n == 129:
        assert seen == {0, 1, 2}
    counts = net.set_counts()
    assert counts == [int((row != UNSET).sum()) for row in pair.want_table()]
    if fresh:
        assert sum(counts) == sum(len(s) for s in pair.ref.stages) > 0
    else:
        assert counts[0] == 2 * 65536 and pair.ref.promoted


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(NS, T):
    """Every instantiation of the three kernels: the first T tuples of an 8 x 3 set (4096 entries
    per tuple, so boards collide), 131 boards, 3 steps."""
    net = make_net(NS, T8M3[:T], (5, 8), 110 + T)
    pair, seen = run_steps(NS, net, np.random.default_rng(210 + T), 131)
    assert seen == {0, 1, 2} and pair.ref.promoted
    assert {k[0] for s in pair.ref.stages for k in s} == set(range(T))


@pytest.mark.parametrize("S", range(1, 9))
def test_every_stage_count(NS, S):
    """S = 1..8 with bounds at 2, 4, 5, 6, 7, 8, 10; a quarter of the upper stages' entries set,
    so fall-throughs of every depth occur."""
    bounds = (2, 4, 5, 6, 7, 8, 10)[:S - 1]
    net = make_net(NS, NR.TUPLES_2x4, bounds, 120 + S, upper=0.25)
    pair = Pair(net)
    rng = np.random.default_rng(220 + S)
    n, caps = 67, (1, 3, 4, 5, 6, 7, 9, 11)
    prev, has_prev = lists(stage_boards(rng, n, caps)), [1] * n
    assert {pair.ref.stage(p) for p in prev} == set(range(S))
    for t in range(3):
        boards = stage_boards(rng, n, caps)
        if t == 0:
            assert {pair.ref.stage(b) for b in boards} == set(range(S))
            pair.check_values_and_act(boards)
        pair.step(boards, prev, has_prev, 3, 6)


# ------------------------------------------------------------------ crafted cases
def test_afterstates_in_different_stages_and_a_merge_that_crosses_a_bound(NS):
    """A move raises the largest tile by at most one exponent, so a board's four afterstates lie
    in at most two stages.  Boards whose merging move crosses a bound while their other moves do
    not, at both bounds, next to boards that cross nothing; the crossing stage's entries hold
    values of their own, so the stage decides the move."""
    boards = np.array([
        [4, 4, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # left / right -> a 5: stage 0 -> 1
        [7, 0, 0, 0, 7, 0, 0, 0, 0, 2, 0, 0, 0, 0, 0, 0],   # up / down -> an 8: stage 1 -> 2
        [4, 0, 0, 0, 4, 3, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # up / down cross, left / right do not
        [7, 7, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # left / right cross 8 (and make a 5)
        [3, 3, 0, 0, 2, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # nothing crosses: stage 0
        [8, 8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1],   # stage 2 already
        [5, 4, 4, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0],   # a merge below the largest tile
    ], np.uint8)
    for seed in (131, 132):
        net = make_net(NS, NR.TUPLES_2x4, (5, 8), seed)
        pair = Pair(net)
        stages = []
        for b in boards:
            moved = [NR.E.move(lists([b])[0], a)[0] for a in range(4)]
            stages.append({pair.ref.stage(m) for m in moved if m != lists([b])[0]})
        assert [len(s) for s in stages] == [2, 2, 2, 2, 1, 1, 1]
        assert stages[0] == stages[2] == {0, 1} and stages[1] == stages[3] == {1, 2}
        pair.check_values_and_act(boards)
        prev, has_prev = lists(boards[::-1]), [1] * len(boards)
        pair.step(boards, prev, has_prev, 1, 2)
        pair.step(boards, prev, has_prev, 1, 2)  # prev now holds afterstates that crossed


def test_three_stage_fall_through(NS):
    """Entries that are UNSET at stages 2 and 1 (the value comes from stage 0), and entries UNSET
    at stage 2 only (from stage 1), for boards of stage 2, in values, act and td_step."""
    rng = np.random.default_rng(140)
    boards = stage_boards(rng, 33, caps=(8, 9, 11))
    boards[:, 0] = 8  # every board is of stage 2
    for kind in ("both", "top"):
        net = make_net(NS, NR.TUPLES_2x4, (5, 8), 141)
        if kind == "both":
            net.lut[1:].fill_(UNSET)
        else:
            net.lut[2].fill_(UNSET)
            net.lut[1].copy_(torch.where(net.lut[1] == UNSET, net.lut[0] + 12345, net.lut[1]))
        pair = Pair(net)
        assert {pair.ref.stage(b) for b in boards} == {2}
        pair.check_values_and_act(boards)
        plain = NR.Net(NR.TUPLES_2x4, base=pair.base[0 if kind == "both" else 1])
        assert [pair.ref.V(b) for b in boards] == [plain.V(b) for b in boards]
        prev, has_prev = lists(boards[::-1]), [1] * 33
        pair.step(boards, prev, has_prev, 3, 6)
        assert set(pair.ref.promoted.values()) - {0} and {k[0] for k in pair.ref.promoted} == {2}
        assert not pair.ref.stages[0] and not pair.ref.stages[1]


def test_one_entry_promoted_at_two_stages_in_one_call(NS):
    """Boards of stage 1 and of stage 2 whose cells under the tuples are identical (the stage
    comes from a centre cell the tuples never read), both entries UNSET, different deltas: each
    ends at val(0, .) plus its own deltas."""
    rng = np.random.default_rng(150)
    net = make_net(NS, EDGES, (5, 8), 151)
    net.lut[1:].fill_(UNSET)
    pair = Pair(net)
    n = 16
    rim = stage_boards(rng, n // 2, caps=(4,))
    rim[:, [5, 6, 9, 10]] = 0
    prev = np.concatenate([rim, rim])
    prev[:n // 2, 5] = 6   # stage 1
    prev[n // 2:, 5] = 9   # stage 2
    assert [pair.ref.stage(p) for p in prev] == [1] * (n // 2) + [2] * (n // 2)
    for i in range(n // 2):
        assert pair.ref.indices(prev[i]) == pair.ref.indices(prev[i + n // 2])
    boards = stage_boards(rng, n)
    boards[3] = CHECKER
    prev, has_prev = lists(prev), [1] * n
    keys = [pair.ref.indices(p) for p in prev]
    _acts, _errs, deltas = pair.step(boards, prev, has_prev, 1, 3)
    assert all(deltas[i] != deltas[i + n // 2] and deltas[i] for i in range(n // 2))
    assert not pair.ref.stages[0] and set(pair.ref.stages[1]) == set(pair.ref.stages[2])
    differ = 0
    for k in pair.ref.stages[1]:
        d1 = sum(deltas[i] * keys[i].count(k) for i in range(n // 2))
        d2 = sum(deltas[i] * keys[i].count(k) for i in range(n // 2, n))
        t, idx = k
        assert pair.ref.stages[1][k] == NR.wrap32(int(pair.base[0, t, idx]) + d1)
        assert pair.ref.stages[2][k] == NR.wrap32(int(pair.base[0, t, idx]) + d2)
        differ += d1 != d2
    assert differ > 8


def test_129_copies_of_one_board(NS):
    """Many promotions of one entry meet many adds into it: one block of 128 and one more."""
    net = make_net(NS, NR.TUPLES_2x4, (5, 8), 160)
    net.lut[1:].fill_(UNSET)
    pair = Pair(net)
    b = [6, 3, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0, 1, 0, 0, 2]
    p = [7, 1, 0, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 2]
    n = 129
    prev, has_prev = [list(p) for _ in range(n)], [1] * n
    _a, _e, deltas = pair.step([b] * n, prev, has_prev, 1, 4)
    assert len(set(deltas)) == 1 and deltas[0] != 0
    assert len(pair.ref.promoted) == len(set(pair.ref.indices(p))) and not pair.ref.stages[0]
    first = set(pair.ref.promoted)
    pair.step([b] * n, prev, has_prev, 1, 4)  # prev is now after(b, action), 129 times
    assert pair.ref.promoted and not first & set(pair.ref.promoted)


def test_more_entries_than_the_merge_table_holds(NS):
    """T = 8 on unrelated boards (exponents 0..15, bounds 14 and 15 so that all stages occur): a
    block of the update (128 boards) adds into up to 8192 different entries, as many as its LDS
    table has slots, so adds that find no slot and go straight to memory occur beside merged
    ones, many of them into entries the policy launch promoted in the same call."""
    net = make_net(NS, T8M3, (14, 15), 170, upper=0.3)
    pair = Pair(net)
    rng = np.random.default_rng(171)
    n = 257
    boards = np.concatenate([rng.integers(0, 16, (n - 16, 16)) * (rng.random((n - 16, 16)) < 0.8),
                             np.array(mask_boards(), np.uint8)[:16]]).astype(np.uint8)
    prev0 = rng.integers(0, 16, (n, 16)).astype(np.uint8)  # largest tile < 14, 14, 15: all stages
    assert min([pair.ref.stage(p) for p in prev0].count(s) for s in range(3)) > 10
    has0 = (rng.random(n) < 0.9).astype(np.uint8)
    prev, has_prev = lists(prev0), [int(h) for h in has0]
    _a, _e, deltas = pair.step(boards, prev, has_prev, 7, 5)
    keys = {(pair.ref.stage(prev0[i]), *k) for i in range(n) if has0[i] and deltas[i]
            for k in pair.ref.indices(prev0[i])}
    assert len(keys) > 8192 and len(pair.ref.promoted) > 1000 and 0 in has_prev
    # err_out is optional
    net2 = make_net(NS, T8M3, (14, 15), 170, upper=0.3)
    Pair(net2).step(boards, lists(prev0), [int(h) for h in has0], 7, 5, err_out=False)
    assert torch.equal(net2.lut, net.lut)


class SparseBase:
    """The reference's base over a table too large to copy to the host: stage 0 is gathered from
    a device copy by index, the upper stages were UNSET."""

    def __init__(self, lut0):
        self.lut0, self.cache = lut0.clone(), {}

    def prefetch(self, keys):
        miss = sorted(set(keys) - self.cache.keys())
        if miss:
            t = torch.tensor([k[0] for k in miss], dtype=torch.long, device=DEV)
            i = torch.tensor([k[1] for k in miss], dtype=torch.long, device=DEV)
            self.cache.update(zip(miss, self.lut0[t, i].cpu().tolist()))

    def __call__(self, s, t, i):
        if s > 0:
            return None
        if (t, i) not in self.cache:
            self.prefetch([(t, i)])
        return self.cache[(t, i)]


def big_net(NS, seed):
    """The 4 x 6 set with S = 2 (512 MiB): stage 0 random, stage 1 UNSET."""
    net = NS.StagedNTupleNetwork(NR.TUPLES_4x6, (6,), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut[0].copy_(torch.randint(-(1 << 20), 1 << 20, net.lut[0].shape, generator=g, device=DEV,
                                   dtype=torch.int32))
    return net


def sparse_steps(net, batches, prev, has_prev, lr):
    """td_steps on the big table against the reference; the touched entries (gathered, not a
    dense copy) and the set counts are compared after every step."""
    base = SparseBase(net.lut[0])
    ref = R.StagedNet(net.spec.tuples, net.bounds, base=base)
    stage0 = net.lut.shape[1] * net.lut.shape[2]
    for boards in batches:
        keys = []
        for b in lists(boards) + prev:
            keys += ref.indices(b)
            for a in range(4):
                keys += ref.indices(NR.E.move(b, a)[0])
        base.prefetch(keys)
        n = len(boards)
        dprev, dhas = dev(prev), dev(has_prev)
        out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
        out_d = torch.zeros(n, dtype=torch.int32, device=DEV)
        out_e = torch.zeros(n, dtype=torch.int64, device=DEV)
        net.td_step(dev(boards), dprev, dhas, *lr, out_a, out_d, out_e)
        acts, errs, deltas = ref.td_step(boards, prev, has_prev, *lr)
        assert out_a.cpu().tolist() == acts and out_e.cpu().tolist() == errs
        assert out_d.cpu().tolist() == deltas
        assert dprev.cpu().tolist() == prev and dhas.cpu().tolist() == has_prev
        entries = sorted(ref.set_entries())
        idx = [torch.tensor([k[j] for k in entries], dtype=torch.long, device=DEV)
               for j in range(3)]
        assert net.lut[idx[0], idx[1], idx[2]].cpu().tolist() == [ref.stages[s][(t, i)]
                                                                  for s, t, i in entries]
        assert net.set_counts() == [stage0, len(ref.stages[1])]
    return ref


def test_4x6_two_stages_touched_entries_and_set_counts(NS):
    """The 4 x 6 table with S = 2 (512 MiB), 129 boards, 3 steps."""
    rng = np.random.default_rng(180)
    net = big_net(NS, 181)
    batches = [stage_boards(rng, 129, caps=(4, 5, 7, 11)) for _ in range(3)]
    ref = sparse_steps(net, batches, [[0] * 16 for _ in range(129)], [0] * 129, (5, 9))
    assert len(ref.stages[0]) > 500 and len(ref.stages[1]) > 500


def test_4x6_128_distinct_boards_in_one_block(NS):
    """128 distinct boards on the 4 x 6 set fill one block of the update with 4096 (g, t) adds,
    nearly all into different entries: half the merge table's slots, where probes already run
    out (4 slots, linear) and adds go straight to memory beside merged ones.  (The merge table
    has 8192 slots; more distinct entries than that need T = 8, the test above.)"""
    rng = np.random.default_rng(182)
    net = big_net(NS, 183)
    prev0 = stage_boards(rng, 128, caps=(5, 7, 11))
    assert len({tuple(p) for p in lists(prev0)}) == 128
    ref = sparse_steps(net, [stage_boards(rng, 128)], lists(prev0), [1] * 128, (5, 9))
    assert len(ref.stages[0]) + len(ref.stages[1]) > 3500


def test_zero_delta_promotes_and_adds_nothing(NS):
    """delta == 0 with has_prev (lr_num = 0; and a rate that floors a small error to 0): the
    entries are promoted to the value they resolve to and no value changes."""
    rng = np.random.default_rng(190)
    net = make_net(NS, NR.TUPLES_2x4, (5, 8), 191)
    net.lut[1:].fill_(UNSET)
    pair = Pair(net)
    boards, prev0 = stage_boards(rng, 40), stage_boards(rng, 40)
    probe = np.concatenate([boards, prev0])
    before = net.values(dev(probe)).cpu().tolist()
    prev, has_prev = lists(prev0), [1] * 20 + [0] * 20
    _a, errs, deltas = pair.step(boards, prev, has_prev, 0, 0)
    assert deltas == [0] * 40 and any(errs[:20]) and not any(errs[20:])
    promoted = pair.ref.promoted
    assert promoted and all(v == int(pair.base[0, t, i]) for (s, t, i), v in promoted.items())
    assert {k[0] for k in promoted} == {1, 2}
    assert set(promoted) == {(pair.ref.stage(p), *k) for p in lists(prev0)[:20]
                             if pair.ref.stage(p) for k in pair.ref.indices(p)}
    assert net.values(dev(probe)).cpu().tolist() == before
    assert np.array_equal(net.lut[0].cpu().numpy(), pair.base[0])


def test_terminal_boards_next_to_live_ones_in_one_wave(NS):
    """Boards without a legal move between live ones, of every stage, with and without a
    previous afterstate: target 0, action 0, has_prev dropped, prev kept -- and their prev
    entries promoted and moved like any other."""
    rng = np.random.default_rng(195)
    net = make_net(NS, NR.TUPLES_2x4, (5, 8), 196)
    pair = Pair(net)
    n = 32
    boards = stage_boards(rng, n)
    for k, i in enumerate(range(1, n, 3)):  # checkerboards of several heights: stages 0, 1, 2
        boards[i] = np.array(CHECKER) + 3 * (k % 3)
    prev0 = stage_boards(rng, n)
    prev, has_prev = lists(prev0), [int(i % 4 != 0) for i in range(n)]
    had = list(has_prev)
    acts, errs, _d = pair.step(boards, prev, has_prev, 3, 4)
    terminal = [all(q is None for q in pair.ref.policy(b)[0]) for b in boards]
    assert sum(terminal) >= 10 and not all(terminal)
    assert {pair.ref.stage(b) for b, dead in zip(boards, terminal) if dead} == {0, 1, 2}
    for i in range(n):
        if terminal[i]:
            assert acts[i] == 0 and has_prev[i] == 0 and prev[i] == lists(prev0)[i]
        else:
            assert has_prev[i] == 1
    assert any(terminal[i] and had[i] and errs[i] != 0 for i in range(n))
    pair.step(stage_boards(rng, n), prev, has_prev, 3, 4)


# ------------------------------------------------------------------ against the plain network
def test_s1_is_the_plain_library(NS):
    """S = 1 on a table without UNSET against libg2048_ntuple.so's own values, act and td_step:
    1031 boards, 3 steps of self-play from one seed."""
    from g2048 import ntuple

    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(197)
    plain.lut.copy_(torch.randint(-(1 << 20), 1 << 20, plain.lut.shape, generator=g, device=DEV,
                                  dtype=torch.int32))
    staged = NS.StagedNTupleNetwork.from_network(plain, ())
    assert staged.lut.shape == (1, 2, 65536)
    ta = ntuple.NTupleTrainer(plain, 1031, seed=71, lr_num=3, lr_shift=9)
    tb = ntuple.NTupleTrainer(staged, 1031, seed=71, lr_num=3, lr_shift=9)
    for t in range(3):
        assert torch.equal(ta.env.board, tb.env.board)
        assert torch.equal(plain.values(ta.env.board), staged.values(tb.env.board))
        for x, y in zip(plain.act(ta.env.board, after=True), staged.act(tb.env.board, after=True)):
            assert torch.equal(x, y)
        ta.step(1)
        tb.step(1)
        for name in ("actions", "delta", "err", "prev", "has_prev"):
            assert torch.equal(getattr(ta, name), getattr(tb, name)), (t, name)
        assert torch.equal(staged.lut[0], plain.lut), t
    assert int(ta.delta.abs().sum()) > 0


def test_from_network_and_resolved_value_boards_as_the_plain_network_does(NS):
    from g2048 import ntuple

    rng = np.random.default_rng(198)
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(199)
    plain.lut.copy_(torch.randint(-(1 << 20), 1 << 20, plain.lut.shape, generator=g, device=DEV,
                                  dtype=torch.int32))
    boards = dev(stage_boards(rng, 300))
    staged = NS.StagedNTupleNetwork.from_network(plain, (5, 8))
    assert set(staged.stage_of(boards).tolist()) == {0, 1, 2}
    assert torch.equal(staged.values(boards), plain.values(boards))
    for x, y in zip(staged.act(boards, after=True), plain.act(boards, after=True)):
        assert torch.equal(x, y)
    # resolved(s) values the boards of stage s as the staged network does
    net = make_net(NS, NR.TUPLES_2x4, (5, 8), 201)
    stage, want = net.stage_of(boards), net.values(boards)
    assert stage.device == boards.device
    ref = R.StagedNet(NR.TUPLES_2x4, (5, 8))
    assert stage.tolist() == [ref.stage(b) for b in boards.cpu().tolist()]
    for s in range(3):
        got = net.resolved(s).values(boards)
        mine = stage == s
        assert int(mine.sum()) > 20 and torch.equal(got[mine], want[mine])
        if s < 2:
            assert not torch.equal(got[stage == 2], want[stage == 2])


# ------------------------------------------------------------------ trainer, player, graph
def trainer(NS, n, seed, bounds=(3, 5), table=202, **kw):
    from g2048 import ntuple

    net = make_net(NS, NR.TUPLES_2x4, bounds, table)
    return net, ntuple.NTupleTrainer(net, n, seed=seed, **kw)


def test_two_identical_runs_of_200_trainer_steps_give_equal_tables(NS):
    def run():
        net, tr = trainer(NS, 256, 72, table=None)
        tr.step(200)
        torch.cuda.synchronize()
        return net.lut, tr.env.board, tr.prev, tr.has_prev

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    counts = [int(x) for x in (a[0] != UNSET).sum(dim=(1, 2)).tolist()]
    assert all(c > 0 for c in counts), counts


def test_captured_td_step_and_env_step_replays(NS):
    """td_step + env.step captured once and replayed 3 times equals 3 eager steps: table (with
    the promotions of each step), boards and outputs."""
    from g2048.dist import graph_capture

    start = stage_boards(np.random.default_rng(203), 192)

    def make():
        net, tr = trainer(NS, 192, 73, bounds=(5, 8), lr_num=1, lr_shift=7)
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
    assert not torch.equal(want[0]["lut"] == UNSET, want[2]["lut"] == UNSET)

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    lut0, st0 = net.lut.clone(), {k: getattr(tr, k).clone() for k in ("prev", "has_prev")}
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert torch.equal(net.lut, lut0) and all(torch.equal(getattr(tr, k), v) for k, v in st0.items())
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = state(net, tr)
        for name, t in want[k].items():
            assert torch.equal(got[name], t), (k, name)
    tr.env.check_errors()


def test_trainer_and_player_run_and_the_search_refuses(NS):
    """NTupleTrainer(staged) and BatchedPlayer.play("ntuple") take a staged network as they are;
    the expectimax search, TC and lambda refuse it."""
    import g2048
    from g2048.player import BatchedPlayer

    net, tr = trainer(NS, 64, 74, table=None)
    tr.step(60)
    tr.env.check_errors()
    assert sum(net.set_counts()) > 0
    res = BatchedPlayer(32, device=DEV, seed=75, ntuple=net, record_games=2).play("ntuple")
    assert (res.moves > 14).all() and not res.stuck.any()
    # every move of a recorded game is the staged policy's
    ref = R.StagedNet(net.spec.tuples, net.bounds, base=net.lut.cpu().numpy())
    for h in res.histories[:1]:
        for tiles, letter, *_ in h[:40]:
            b = np.where(tiles > 0, np.log2(np.maximum(tiles, 1)), 0).astype(np.uint8).reshape(16)
            assert "udlr"[ref.policy(b)[1]] == letter
    with pytest.raises(TypeError):
        BatchedPlayer(8, device=DEV, seed=76, ntuple=net).play("ntuple_search")
    with pytest.raises(TypeError):
        net.search(tr.env.board)
    with pytest.raises(TypeError):
        g2048.TCTrainer(net, 64)
    with pytest.raises(TypeError):
        g2048.TDLambdaTrainer(net, 64)


# ------------------------------------------------------------------ it learns
def test_staged_self_play_learns(NS):
    """NTupleTrainer on StagedNTupleNetwork(TUPLES_2x4, bounds=(7,)), 256 boards, lr 1 / 2^10,
    seed 61, 4000 steps: the mean merge score of the last 200 finished episodes is at least 1760
    (twice play("random")'s 880, the bar of the single-table test), stage 1 has set entries and
    no set entry exceeds 2^28.  A numpy prototype of the rule reached 4361 with 16 792 set
    entries in stage 1 and a largest entry of 2.9e5 on its own random stream.  Measured on an
    MI355X: 3010 / 3365 / 3842 / 4491 after 1000 / 2000 / 3000 / 4000 steps, 4331 and 16 527 set
    entries in stages 0 and 1, largest |entry| 293 378."""
    from g2048 import ntuple

    net = NS.StagedNTupleNetwork(ntuple.TUPLES_2x4, (7,), device=DEV)
    tr = ntuple.NTupleTrainer(net, 256, seed=61, p4=0.5, lr_num=1, lr_shift=10, log_slots=64)
    scores = []
    for chunk in range(4):
        tr.step(1000)
        scores += tr.episodes()["score"].tolist()
        print(f"steps {1000 * (chunk + 1)}: {len(scores)} episodes, mean merge score of the last "
              f"200: {np.mean(scores[-200:]):.0f}, set entries per stage {net.set_counts()}")
    tr.env.check_errors()
    learned = float(np.mean(scores[-200:]))
    is_set = net.lut != UNSET
    largest = int(torch.where(is_set, net.lut, torch.zeros_like(net.lut)).to(torch.int64)
                  .abs().max())
    print(f"staged 2x4, bounds (7,), after 4000 steps: {learned:.0f} over the last 200 of "
          f"{len(scores)} episodes, set entries {net.set_counts()}, largest |entry| {largest}")
    assert len(scores) >= 200
    assert learned >= 1760
    assert net.set_counts()[1] > 0
    assert largest <= 1 << 28
