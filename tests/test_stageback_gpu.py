"""Backward episode learning on the staged batch-mean TC rule on the GPU
(csrc/g2048_stageback.hip -> libg2048_stageback.so) against the plain Python restatement
tests/stageback_ref.py: the table with its UNSET pattern, ea, the trajectory (traj, gain, cur, rec,
rep_n, rep_k), action, err, delta, x_out and replay_out bit for bit, and acc all zero, after every
call -- at the frames' edges for every horizon, for every T and S, on the hand anchors, on crafted
batches, the 4 x 6 set, next to libg2048_stagemeantc.so and StagedNTupleNetwork.act, the trainer,
a captured step, the restart pool, a resumed run, and that self-play learns."""
import numpy as np
import pytest
import torch

import ntstage_ref as SR
import ntuple_ref as NR
import stageback_ref as R
from g2048 import stageback as _library
from oracle import oracle as O
from test_ntstage_gpu import SparseBase, T8M3, dev, lists, make_net, stage_boards
from test_stagemean_gpu import T8M4
from test_stagemeantc_gpu import seeded_ea

_library.load()  # without the library the file fails here, before any case
pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSET = SR.UNSET
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
A = [1, 1] + [0] * 14
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
LR = (3, 6)  # deltas of about 2^20 on a table of +-2^20: nothing leaves int32
# 1: a dead half-wave of the policy frame; 2: one wave of it; 7, 8, 9: around a wave of the gather
# / apply frame (8 boards); 127, 128, 129: around their block; 1031: nine blocks
SIZES = (1, 2, 7, 8, 9, 127, 128, 129, 1031)
HORIZONS = (1, 2, 3, 64)
NOT_WRITTEN = 0xAB  # what x_out holds before a call: a row of a board that idles keeps it


class Modules:
    def __init__(self, ntuple, ntstage, ntmeantc, stagemeantc, stageback):
        self.NT, self.NS, self.MTC, self.SMTC, self.SB = (ntuple, ntstage, ntmeantc, stagemeantc,
                                                          stageback)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmeantc, ntstage, ntuple, stageback, stagemeantc
    for mod in (ntuple, ntstage, ntmeantc, stagemeantc, stageback):
        mod.load()
    return Modules(ntuple, ntstage, ntmeantc, stagemeantc, stageback)


def outputs(n):
    """actions, delta, x, replays, err: none of them holds what a call would write."""
    return (torch.full((n,), 9, dtype=torch.uint8, device=DEV),
            torch.full((n,), 77, dtype=torch.int32, device=DEV),
            torch.full((n, 16), NOT_WRITTEN, dtype=torch.uint8, device=DEV),
            torch.full((n,), 9, dtype=torch.uint8, device=DEV),
            torch.full((n,), 77, dtype=torch.int64, device=DEV))


def u32(t):
    """A counter tensor (int32 on the device) as the header's u32."""
    return t.cpu().numpy().view(np.uint32)


COUNTERS = ("cur", "rec", "rep_n", "rep_k")


def check_planes(st, ref, traj, gain, where=None):
    """The device's trajectory against host arrays of it and the reference's counters."""
    assert np.array_equal(st.traj.cpu().numpy(), traj), where
    assert np.array_equal(st.gain.cpu().numpy().view(np.uint32), gain), where  # unsigned: 2^31
    assert st.cur.cpu().tolist() == ref.cur, where
    for name in COUNTERS[1:]:
        assert u32(getattr(st, name)).tolist() == getattr(ref, name), (where, name)


class Call:
    """What one call did, from the reference."""

    def __init__(self, acts, errs, deltas, xs, rep, ref, closed):
        self.acts, self.errs, self.deltas, self.xs, self.rep = acts, errs, deltas, xs, rep
        self.hits, self.ms = dict(ref.last_hits), dict(ref.last_m)
        self.promoted = dict(ref.net.promoted)
        self.closed = closed  # boards whose episode closed in this call


class Pair:
    """A staged network and the rule's state on the GPU next to the reference over host copies of
    the table and of the ea it starts from (ea0: None = zeros).  `traj` and `gain` are host arrays
    of the reference's planes, kept up to date slot by slot so that a call's comparison does not
    convert the whole nested list; close() compares them with the lists themselves."""

    def __init__(self, M, net, n, L, ea0=None):
        self.net, self.n, self.L = net, n, L
        self.st = M.SB.BackwardState(net, n, L)
        self.base = net.lut.cpu().numpy().copy()
        base_ea = None
        if ea0 is not None:
            self.st.ea.copy_(torch.from_numpy(ea0))
            base_ea = lambda s_, t, i: (int(ea0[s_, t, i, 0]), int(ea0[s_, t, i, 1]))  # noqa: E731
        self.ea0 = np.zeros((*self.base.shape, 2), np.int64) if ea0 is None else ea0
        self.ref = R.Backward(SR.StagedNet(net.spec.tuples, net.bounds, base=self.base), n, L,
                              base_ea=base_ea)
        self.traj = np.zeros((n, 2, L, 16), np.uint8)
        self.gain = np.zeros((n, 2, L), np.uint32)

    def set_replay(self, i, episode, gains=None, rep_k=0, cur=0):
        """Board i's replay buffer on both sides: a closed episode of len(episode) <= L
        afterstates, rep_k of them already updated."""
        st, ref = self.st, self.ref
        buf = (cur & 1) ^ 1
        for k, b in enumerate(episode):
            g = 0 if gains is None else int(gains[k])
            ref.traj[i][buf][k], ref.gain[i][buf][k] = [int(v) for v in b], g
            self.traj[i, buf, k], self.gain[i, buf, k] = b, g
        ref.cur[i], ref.rep_n[i], ref.rep_k[i] = cur, len(episode), rep_k
        st.traj.copy_(dev(self.traj))
        st.gain.copy_(dev(self.gain.view(np.int32), np.int32))
        st.cur.copy_(dev(np.array(ref.cur, np.uint8)))
        st.rep_n.copy_(dev(np.array(ref.rep_n, np.uint32).view(np.int32), np.int32))
        st.rep_k.copy_(dev(np.array(ref.rep_k, np.uint32).view(np.int32), np.int32))

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

    def check_state(self):
        got, want = self.net.lut.cpu().numpy(), self.want_table()
        assert np.array_equal(got == UNSET, want == UNSET)
        assert np.array_equal(got, want)
        assert np.array_equal(self.st.ea.cpu().numpy(), self.want_ea())
        check_planes(self.st, self.ref, self.traj, self.gain)
        assert not bool(self.st.acc.any())

    def step(self, boards, lr_num, lr_shift, out=None):
        """One call on both sides from the same state; everything is compared.  `out`: the
        caller's outputs(n), for a test that looks at the memory around them."""
        ref, L = self.ref, self.L
        out = outputs(self.n) if out is None else out
        cur, rec = list(ref.cur), list(ref.rec)
        self.st.step(dev(boards), lr_num, lr_shift, *out)
        acts, errs, deltas, xs, rep = ref.step(lists(boards), lr_num, lr_shift)
        closed = []
        for i in range(self.n):  # the slot the reference recorded into, into the host arrays
            if ref.rec[i] == rec[i] + 1:
                buf, slot = cur[i] & 1, rec[i] % L
                self.traj[i, buf, slot] = ref.traj[i][buf][slot]
                self.gain[i, buf, slot] = ref.gain[i][buf][slot]
            elif rec[i]:
                closed.append(i)
        assert out[0].cpu().tolist() == acts
        assert out[1].cpu().tolist() == deltas
        assert out[4].cpu().tolist() == errs
        assert out[3].cpu().tolist() == [int(r) for r in rep]
        # row i of x_out is written iff board i replays
        assert out[2].cpu().tolist() == [[NOT_WRITTEN] * 16 if x is None else x for x in xs]
        self.check_state()
        return Call(acts, errs, deltas, xs, rep, ref, closed)

    def close(self):
        """The host arrays are the reference's planes."""
        assert self.traj.tolist() == self.ref.traj and self.gain.tolist() == self.ref.gain


# ------------------------------------------------------------------ scripted episodes
def live_pool(rng, k=24):
    """k boards of all three stages with an empty corner, so every one has a legal move."""
    pool = stage_boards(rng, k, caps=(3, 6, 11))  # afterstates below 5, below 8 and above
    pool[:, 0] = 0
    pool[:, 1] = np.maximum(pool[:, 1], 1)
    return pool


def script(rng, n, L, calls):
    """[calls][n] of booleans: board i is terminal in that call.  Its episodes have the lengths
    L + 1, 2 L + 1, L or L - 1 (the first one by i mod 4, so that a batch of any size replays; the
    later ones drawn).  A length 0 is a terminal board at rec == 0."""
    lengths = (L + 1, 2 * L + 1, L, L - 1)
    terminal = np.zeros((calls, n), bool)
    for i in range(n):
        t = 0
        while t < calls:
            t += lengths[i % 4] if t == 0 else int(rng.choice(lengths))
            if t < calls:
                terminal[t, i] = True
            t += 1
    return terminal


def scripted_batch(pool, terminal, t):
    """Live boards that change from call to call and from board to board (so that neighbouring
    slots of a trajectory hold different afterstates), the checkerboard where the script ends an
    episode."""
    n = terminal.shape[1]
    boards = pool[(7 * np.arange(n) + 3 * t) % len(pool)].copy()
    boards[terminal[t]] = CHECKER
    return boards


def run_script(pair, rng, calls, lr=LR):
    pool = live_pool(rng)
    terminal = script(rng, pair.n, pair.L, calls)
    out = []
    for t in range(calls):
        active = [pair.ref.replays(i) for i in range(pair.n)]
        c = pair.step(scripted_batch(pool, terminal, t), *lr)
        c.closed_in_replay = [i for i in c.closed if active[i]]
        out.append(c)
    pair.close()
    return out


# ------------------------------------------------------------------ sizes, L, T and S
@pytest.mark.parametrize("L", HORIZONS)
@pytest.mark.parametrize("n", SIZES)
def test_step_at_wave_and_block_edges_for_every_horizon(M, n, L):
    """Every size class and horizon on the 2 x 4 set with the bounds (5, 8), a half-UNSET table
    and a seeded ea, from the fresh state through 3 L + 3 calls: long enough for an episode of
    2 L + 1 afterstates to be recorded (the ring wraps) and replayed."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 701)
    pair = Pair(M, net, n, L, seeded_ea(tuple(net.lut.shape), 702))
    rng = np.random.default_rng(710 + 16 * n + L)
    calls = run_script(pair, rng, 3 * L + 3)
    assert any(any(c.rep) for c in calls) and any(c.hits for c in calls)
    if n >= 127:
        assert max(pair.ref.rep_n) == 2 * L + 1  # an episode that kept its last L only
        assert L == 1 or any(c.closed_in_replay for c in calls)  # L - 1 after >= L
        assert any(c.promoted for c in calls)
        if L > 1:  # at L = 1 every target is 0, and a greedy afterstate's value is rarely below it
            assert {d > 0 for c in calls for d in c.deltas if d} == {True, False}
        assert any(cnt > 8 for c in calls for _d, cnt in c.hits.values())
        assert {k[0] for c in calls for k in c.hits} == {0, 1, 2}
        assert not all(pair.ref.replays(i) for i in range(n))  # and some boards idle


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(M, T):
    """Every instantiation of the three kernels: the first T tuples of an 8 x 3 set, L = 3."""
    net = make_net(M.NS, T8M3[:T], (5, 8), 730 + T)
    pair = Pair(M, net, 129, 3, seeded_ea(tuple(net.lut.shape), 735 + T))
    calls = run_script(pair, np.random.default_rng(740 + T), 10)
    assert {k[1] for c in calls for k in c.hits} == set(range(T))
    assert {k[0] for c in calls for k in c.hits} == {0, 1, 2}


@pytest.mark.parametrize("S", [1, 2, 3])
def test_every_stage_count(M, S):
    bounds = (5, 8)[:S - 1]
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 750 + S, upper=0.25)
    pair = Pair(M, net, 129, 2, seeded_ea(tuple(net.lut.shape), 755 + S))
    calls = run_script(pair, np.random.default_rng(760 + S), 8)
    assert {k[0] for c in calls for k in c.hits} == set(range(S)) == {k[0] for k in pair.ref.A}


# ------------------------------------------------------------------ the anchors, on the device
def corner_pair(M, bounds, n, L, preset=None):
    net = M.NS.StagedNTupleNetwork(((0,),), bounds, device=DEV)
    row = 1024 * np.arange(net.lut.shape[2])
    net.lut[0, 0].copy_(dev(row, np.int32))
    ea0 = None
    if preset:
        ea0 = np.zeros((*net.lut.shape, 2), np.int64)
        for k, v in preset.items():
            ea0[k] = v
    pair = Pair(M, net, n, L, ea0)
    pair.lut0 = row
    return pair


def entries(pair):
    got = pair.net.lut.cpu().numpy()
    return {(int(s), int(t), int(i)): int(got[s, t, i]) for s, t, i in np.argwhere(got != UNSET)
            if s > 0 or got[s, t, i] != pair.lut0[i]}


def ea_entries(pair):
    got = pair.st.ea.cpu().numpy()
    return {(int(s), int(t), int(i)): (int(got[s, t, i, 0]), int(got[s, t, i, 1]))
            for s, t, i in np.argwhere(got.any(axis=-1))}


def counters(pair, i=0):
    st = pair.st
    return (int(st.cur[i]), int(u32(st.rec)[i]), int(u32(st.rep_n)[i]), int(u32(st.rep_k)[i]))


def feed(pair, names, lr=(1, 1)):
    boards = {"A": A, "CB": CHECKER}
    return [pair.step(np.array([boards[k]] * pair.n, np.uint8), *lr) for k in names.split()]


def _calls_4_and_5(pair):
    c = feed(pair, "A")[0]
    assert (c.acts, c.errs, c.deltas, c.xs, c.rep) == ([2], [-4096], [-2048], [Q2], [True])
    assert c.hits == {(0, 0, 2): (-4096, 2), (0, 0, 0): (-12288, 6)}
    assert entries(pair) == {(0, 0, 2): 0, (0, 0, 0): -2048}
    assert ea_entries(pair) == {(0, 0, 2): (-2048, 2048), (0, 0, 0): (-2048, 2048)}
    c = feed(pair, "A")[0]
    assert (c.errs, c.deltas, c.xs, c.rep) == ([4096], [2048], [Q2], [True])
    assert not entries(pair)  # lut[2] = 2048 and lut[0] = 0: both back at their fresh values
    assert pair.net.lut[0, 0, :3].cpu().tolist() == [0, 1024, 2048]
    assert ea_entries(pair) == {(0, 0, 2): (0, 4096), (0, 0, 0): (0, 4096)}


def test_anchor_1_an_episode_of_two_is_replayed_newest_first(M):
    pair = corner_pair(M, (), 1, 4)
    for k, c in enumerate(feed(pair, "A A")):
        assert (c.acts, c.errs, c.deltas, c.rep) == ([2], [0], [0], [False])
    assert counters(pair) == (0, 2, 0, 0)
    assert pair.st.traj[0, 0, :2].cpu().tolist() == [Q2, Q2]
    assert pair.st.gain[0, 0, :2].cpu().tolist() == [4, 4]
    c = feed(pair, "CB")[0]
    assert (c.acts, c.rep) == ([0], [False]) and not entries(pair) and not ea_entries(pair)
    assert counters(pair) == (1, 0, 2, 0)
    _calls_4_and_5(pair)
    assert counters(pair) == (1, 2, 2, 2)
    c = feed(pair, "A")[0]
    assert (c.rep, c.errs, c.deltas) == ([False], [0], [0]) and not c.hits
    assert not entries(pair) and counters(pair) == (1, 3, 2, 2)


def test_anchor_2_a_longer_episode_keeps_its_last_l(M):
    pair = corner_pair(M, (), 1, 2)
    feed(pair, "A A A CB")
    assert counters(pair) == (1, 0, 3, 0) and not entries(pair)
    _calls_4_and_5(pair)
    c = feed(pair, "A")[0]
    assert c.rep == [False] and not c.hits and counters(pair) == (1, 3, 3, 2)


def test_anchor_3_an_episode_ends_while_a_replay_is_active(M):
    pair = corner_pair(M, (), 1, 4)
    feed(pair, "A A A CB")
    c = feed(pair, "A")[0]
    assert (c.errs, c.deltas, c.rep) == ([-4096], [-2048], [True])
    assert counters(pair) == (1, 1, 3, 1)
    c = feed(pair, "CB")[0]  # the older replay's transition is made, then it is dropped
    assert (c.acts, c.errs, c.deltas, c.rep) == ([0], [4096], [2048], [True])
    assert not entries(pair) and counters(pair) == (0, 0, 1, 0)  # lut[2] = 2048, lut[0] = 0
    c = feed(pair, "A")[0]
    assert (c.errs, c.deltas, c.xs, c.rep) == ([-4096], [-2048], [Q2], [True])
    assert c.ms == {(0, 0, 2): -2048, (0, 0, 0): -2048}  # at rate(0, 4096) = 0
    assert not entries(pair)
    assert ea_entries(pair) == {(0, 0, 2): (-2048, 6144), (0, 0, 0): (-2048, 6144)}
    assert counters(pair) == (0, 1, 1, 1)
    assert feed(pair, "A")[0].rep == [False] and counters(pair) == (0, 2, 1, 1)


def test_anchor_4_a_terminal_board_at_rec_0(M):
    pair = corner_pair(M, (), 1, 4)
    c = feed(pair, "CB")[0]
    assert (c.acts, c.errs, c.deltas, c.rep) == ([0], [0], [0], [False])
    assert counters(pair) == (0, 0, 0, 0) and not entries(pair)
    assert not bool(pair.st.traj.any()) and not bool(pair.st.gain.any())
    feed(pair, "A CB")
    assert counters(pair) == (1, 0, 1, 0)
    c = feed(pair, "CB")[0]
    assert (c.errs, c.deltas, c.rep) == ([-4096], [-2048], [True])
    assert counters(pair) == (1, 0, 1, 1)
    assert feed(pair, "CB")[0].rep == [False] and counters(pair) == (1, 0, 1, 1)


def test_anchor_5_two_boards_of_different_stages_replay_onto_one_index(M):
    pair = corner_pair(M, (3,), 2, 4)
    pair.set_replay(0, [Q2])
    pair.set_replay(1, [Q3])
    c = feed(pair, "CB")[0]
    assert (c.errs, c.deltas, c.xs) == ([-4096, -6144], [-2048, -3072], [Q2, Q3])
    assert c.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert entries(pair) == {(0, 0, 2): 0, (0, 0, 0): -2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    ea = ea_entries(pair)
    assert ea[(0, 0, 0)] == (-2048, 2048) and ea[(1, 0, 0)] == (-3072, 3072)


def test_anchor_6_unset_entries_are_promoted_and_moved_in_one_call(M):
    pair = corner_pair(M, (2,), 1, 4)
    for c in feed(pair, "A CB"):
        assert not c.promoted and not entries(pair)
    c = feed(pair, "CB")[0]
    assert (c.errs, c.deltas, c.xs) == ([-4096], [-2048], [Q2])
    assert c.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0}
    assert entries(pair) == {(1, 0, 2): 0, (1, 0, 0): -2048}


def test_anchor_7_deltas_that_cancel_leave_the_entry_and_its_ea(M):
    pair = corner_pair(M, (), 2, 4, preset={(0, 0, 2): (5, 9)})
    pair.set_replay(0, [Q2])
    pair.set_replay(1, [Q2, Q3], gains=[0, 2], rep_k=1)
    c = feed(pair, "A", lr=(1, 0))[0]
    assert (c.errs, c.deltas, c.xs) == ([-4096, 4096], [-4096, 4096], [Q2, Q2])
    assert c.hits == {(0, 0, 2): (0, 4), (0, 0, 0): (0, 12)}
    assert not entries(pair) and ea_entries(pair) == {(0, 0, 2): (5, 9)}
    assert counters(pair, 0) == (0, 1, 1, 1) and counters(pair, 1) == (0, 1, 2, 2)


# ------------------------------------------------------------------ consequences 1 and 2
def test_a_call_without_a_replay_is_stagedntuplenetwork_act(M):
    """Consequence 1: from the fresh state no board replays; the actions are act's, the recorded
    afterstates are act's `after`, and lut, ea and acc stay as they are."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 770)
    n = 129
    st = M.SB.BackwardState(net, n, 4)
    st.ea.copy_(torch.from_numpy(seeded_ea(tuple(net.lut.shape), 771)))
    lut, ea = net.lut.clone(), st.ea.clone()
    rng = np.random.default_rng(772)
    for t in range(3):
        boards = stage_boards(rng, n)
        if t != 1:  # terminal boards at rec == 0 in call 0; episodes that close in the last call
            boards[(np.arange(n) + t) % 5 == 2] = CHECKER
        b = dev(boards)
        acts, _q, after = net.act(b, q=False, after=True)
        out = outputs(n)
        rec = u32(st.rec).copy()
        cur = st.cur.cpu().numpy().copy()
        st.step(b, *LR, *out)
        assert torch.equal(out[0], acts)
        assert not bool(out[1].any()) and not bool(out[3].any()) and not bool(out[4].any())
        assert bool((out[2] == NOT_WRITTEN).all())
        assert torch.equal(net.lut, lut) and torch.equal(st.ea, ea) and not bool(st.acc.any())
        legal = (boards != np.array(CHECKER, np.uint8)).any(axis=1)
        rows = np.flatnonzero(legal)
        got = st.traj.cpu().numpy()[rows, cur[rows] & 1, rec[rows] % 4]
        assert np.array_equal(got, after.cpu().numpy()[rows])
    assert bool(st.rec.any())


@pytest.mark.parametrize("S", [1, 3])
def test_a_replay_of_last_afterstates_is_libg2048_stagemeantc(M, S):
    """Consequence 2 against the thirteenth library itself: every replaying board at rep_k == 0.
    Its step on terminal boards with prev = x and has_prev = replays leaves the same lut and the
    same ea, from a seeded ea on a half-UNSET table."""
    bounds = (5, 8)[:S - 1]
    n = 257
    nets = [make_net(M.NS, NR.TUPLES_2x4, bounds, 780 + S) for _ in range(2)]
    ea0 = seeded_ea(tuple(nets[0].lut.shape), 785)
    rng = np.random.default_rng(786 + S)
    xs = stage_boards(rng, n)
    has = (np.arange(n) % 5 != 0).astype(np.uint8)
    st = M.SB.BackwardState(nets[0], n, 3)
    st.ea.copy_(torch.from_numpy(ea0))
    # an episode of 2 whose last afterstate is x, in buffer 0 while buffer 1 is recorded
    st.traj[:, 0, 1].copy_(dev(xs))
    st.traj[:, 0, 0].copy_(dev(stage_boards(rng, n)))
    st.cur.fill_(1)
    st.rep_n.copy_(dev(2 * has.astype(np.int32), np.int32))
    out = outputs(n)
    st.step(dev(stage_boards(rng, n)), *LR, *out)
    tc = M.SMTC.StagedMeanTCState(nets[1])
    tc.ea.copy_(torch.from_numpy(ea0))
    prev, has_prev = dev(xs), dev(has)
    tc_out = (torch.zeros(n, dtype=torch.uint8, device=DEV),
              torch.zeros(n, dtype=torch.int32, device=DEV),
              torch.zeros(n, dtype=torch.int64, device=DEV))
    tc.meantc_step(dev(np.array([CHECKER] * n, np.uint8)), prev, has_prev, *LR, *tc_out)
    assert torch.equal(nets[0].lut, nets[1].lut) and torch.equal(st.ea, tc.ea)
    assert torch.equal(out[1], tc_out[1]) and torch.equal(out[4], tc_out[2])
    assert out[3].cpu().tolist() == has.tolist() and bool(out[1].any())
    assert not torch.equal(st.ea, torch.from_numpy(ea0).to(DEV)) and not bool(st.acc.any())
    assert u32(st.rep_k).tolist() == has.tolist()


# ------------------------------------------------------------------ crafted batches
def test_a_block_of_distinct_afterstates_overflows_both_lds_tables(M):
    """T = 8, m = 4, 128 boards all replaying distinct random full afterstates: one block makes
    128 * 64 = 8192 hits on nearly as many distinct staged entries, more than the gather's 4096
    slots hold and, after four probes, more than the apply's 8192 place, so hits go straight to
    memory beside merged ones, in both launches.  Two calls: the second has successors."""
    net = make_net(M.NS, T8M4, (10,), 790, upper=1.0)
    n, L = 128, 2
    pair = Pair(M, net, n, L, seeded_ea(tuple(net.lut.shape), 791))
    rng = np.random.default_rng(792)
    eps = rng.integers(1, 12, (n, 2, 16)).astype(np.uint8)
    for i in range(n):
        pair.set_replay(i, eps[i], gains=rng.integers(0, 64, 2) * 4)
    boards = live_pool(rng, n)
    for k in range(2):
        c = pair.step(boards, 7, 5)
        assert all(c.rep) and all(c.deltas)
        assert sum(cnt for _d, cnt in c.hits.values()) == n * 64 and len(c.hits) > 6000
        assert {key[0] for key in c.hits} == {0, 1}
    assert pair.ref.rep_k == [2] * n and not any(pair.step(boards, 7, 5).rep)
    pair.close()


def test_129_copies_of_one_board(M):
    """One episode on every row: C = 129 times the hits of one board, one block of 128 boards and
    one more; the last afterstate's 8 symmetries coincide."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 800, upper=1.0)
    n, L = 129, 3
    pair = Pair(M, net, n, L, seeded_ea(tuple(net.lut.shape), 801))
    episode = [[7, 1, 0, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 2],
               [8, 1, 0, 1, 2, 0, 2, 1, 0, 0, 3, 0, 1, 0, 0, 2], [5] * 16]
    for i in range(n):
        pair.set_replay(i, episode, gains=[0, 256, 12])
    b = [6, 3, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0, 1, 0, 0, 2]
    c = pair.step(np.array([b] * n, np.uint8), 1, 4)
    assert len(set(c.deltas)) == 1 and c.deltas[0] != 0
    assert sorted(cnt for _d, cnt in c.hits.values()) == [8 * n, 8 * n]
    for _ in range(2):
        c = pair.step(np.array([b] * n, np.uint8), 1, 4)
        assert len(set(c.deltas)) == 1 and c.deltas[0] != 0
        assert all(cnt % n == 0 and d == cnt * c.deltas[0] for d, cnt in c.hits.values())
    assert not any(pair.step(np.array([CHECKER] * n, np.uint8), 1, 4).rep)
    pair.close()


# ------------------------------------------------------------------ the 4 x 6 set
def test_4x6_two_stages_on_played_boards(M):
    """The 4 x 6 table with bounds (11,) (512 MiB, 2 GiB of acc, 2 GiB of ea), 256 boards from a
    rollout, L = 3: every board's replay buffer holds three afterstates of played boards, four
    calls: the touched staged entries of lut and ea (gathered, not a dense copy), the set counts,
    the trajectory and acc.any().  Staged indices reach past 2^24."""
    import g2048

    n, L = 256, 3
    env = g2048.VecEnv2048(n, seed=811, device=DEV)
    played = []
    for _ in range(5):
        env.rollout(60)
        torch.cuda.synchronize()
        played.append(env.board.cpu().numpy().copy())
    env.check_errors()
    played[1][::3] = np.maximum(played[1][::3], 11 * (np.arange(16) == 5)).astype(np.uint8)
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_4x6, (11,), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(812)
    net.lut[0].copy_(torch.randint(-(1 << 20), 1 << 20, net.lut[0].shape, generator=g, device=DEV,
                                   dtype=torch.int32))
    st = M.SB.BackwardState(net, n, L)
    assert st.acc.numel() * 8 == 2 << 30 == st.ea.numel() * 8
    base = SparseBase(net.lut[0])
    ref = R.Backward(SR.StagedNet(net.spec.tuples, net.bounds, base=base), n, L)
    traj = np.stack(played[:3], axis=1)
    gains = 4 * np.random.default_rng(813).integers(0, 128, (n, L)).astype(np.int32)
    st.traj[:, 1].copy_(dev(traj))
    st.gain[:, 1].copy_(dev(gains, np.int32))
    st.rep_n.fill_(L)
    for i in range(n):
        ref.traj[i][1], ref.gain[i][1], ref.rep_n[i] = lists(traj[i]), gains[i].tolist(), L
    want_traj, want_gain = st.traj.cpu().numpy().copy(), st.gain.cpu().numpy().copy()
    stage0 = net.lut.shape[1] * net.lut.shape[2]
    moved = 0
    for t in range(4):
        boards = played[3 + t % 2]
        keys = []
        for b in lists(boards):
            for a in range(4):
                keys += ref.net.indices(NR.E.move(b, a)[0])
        for row in lists(traj.reshape(-1, 16)):
            keys += ref.net.indices(row)
        base.prefetch(keys)
        out = outputs(n)
        cur, rec = list(ref.cur), list(ref.rec)
        st.step(dev(boards), 5, 9, *out)
        acts, errs, deltas, xs, rep = ref.step(lists(boards), 5, 9)
        for i in range(n):  # a played board can be terminal: its episode closes and cur turns
            if ref.rec[i] == rec[i] + 1:
                buf, slot = cur[i] & 1, rec[i] % L
                want_traj[i, buf, slot] = ref.traj[i][buf][slot]
                want_gain[i, buf, slot] = ref.gain[i][buf][slot]
        assert out[0].cpu().tolist() == acts and out[4].cpu().tolist() == errs
        assert out[1].cpu().tolist() == deltas and out[3].cpu().tolist() == [int(r) for r in rep]
        assert out[2].cpu().tolist() == [[NOT_WRITTEN] * 16 if x is None else x for x in xs]
        check_planes(st, ref, want_traj, want_gain, t)
        ent = sorted(ref.net.set_entries())
        if ent:
            idx = [torch.tensor([k[j] for k in ent], dtype=torch.long, device=DEV)
                   for j in range(3)]
            assert net.lut[idx[0], idx[1], idx[2]].cpu().tolist() == [ref.net.stages[s][(t_, i)]
                                                                      for s, t_, i in ent]
            assert st.ea[idx[0], idx[1], idx[2]].cpu().tolist() == [list(ref.get_ea(*k))
                                                                    for k in ent]
        assert net.set_counts() == [stage0, len(ref.net.stages[1])]
        assert int(st.ea[..., 1].count_nonzero()) == sum(1 for a in ref.A.values() if a)
        assert not bool(st.acc.any())
        assert all(rep) == (t < L)
        moved += len(ref.last_hits)
    assert moved > 500 and {k[0] for k in ref.A} == {0, 1}


# ------------------------------------------------------------------ trainer, graph
def late_boards(n, seed):
    """Full boards but for one or two cells, small exponents: games that end within a few moves,
    so that a short run closes episodes and replays them."""
    rng = np.random.default_rng(seed)
    b = rng.integers(1, 6, (n, 16)).astype(np.uint8)
    for row in b:
        row[rng.choice(16, int(rng.integers(1, 3)), replace=False)] = 0
    return b


def late_trainer(M, net, n, seed, **kw):
    tr = M.SB.BackwardTrainer(net, n, seed=seed, **kw)
    tr.env.board.copy_(dev(late_boards(n, seed + 1000)))
    return tr


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """BackwardTrainer at L = 16, 64 boards on the 2x4 set, at its default rate, from late boards,
    next to the reference driving an OracleEnv: actions, err, delta, x, replays, the trajectory,
    the whole table and the whole ea after each of 50 steps, acc all zero.  A low bound besides,
    so stage 1 is reached."""
    for bounds, n, seed in (((7,), 64, 47), ((3,), 64, 48)):
        net = make_net(M.NS, NR.TUPLES_2x4, bounds, 820)
        net.lut[1:].fill_(UNSET)
        base = net.lut.cpu().numpy().copy()
        tr = late_trainer(M, net, n, seed, horizon=16)
        assert (tr.lr_num, tr.lr_shift, tr.state.horizon) == (1, 4, 16)
        ref = R.Backward(SR.StagedNet(NR.TUPLES_2x4, bounds, base=base), n, 16)
        oracle = O.OracleEnv(n, seed)
        oracle.board[:] = late_boards(n, seed + 1000)
        hits = replays = 0
        for t in range(50):
            boards = oracle.board.copy()
            assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
            tr.step(1)
            acts, errs, deltas, xs, rep = ref.step(lists(boards), 1, 4)
            hits += len(ref.last_hits)
            replays += sum(rep)
            oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
            assert tr.actions.cpu().tolist() == acts, t
            assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == deltas, t
            assert tr.replays.cpu().tolist() == [int(r) for r in rep], t
            got_x = tr.x.cpu().tolist()
            assert all(got_x[i] == xs[i] for i in range(n) if rep[i]), t
            check_planes(tr.state, ref, np.array(ref.traj, np.uint8),
                         np.array(ref.gain, np.uint32), t)
            want = base.copy()
            for s, ents in enumerate(ref.net.stages):
                for (k, i), v in ents.items():
                    want[s, k, i] = v
            assert np.array_equal(net.lut.cpu().numpy(), want), t
            want_ea = np.zeros((*base.shape, 2), np.int64)
            for (s, k, i), a in ref.A.items():
                want_ea[s, k, i] = (ref.E[(s, k, i)], a)
            assert np.array_equal(tr.state.ea.cpu().numpy(), want_ea), t
            assert not bool(tr.state.acc.any()), t
        assert hits > 500 and replays > 5 * n and max(ref.rep_n) > 16
        if bounds == (3,):
            assert len(ref.net.stages[1]) > 50 and any(k[0] == 1 for k in ref.A)
        tr.env.check_errors()


TRAJ = ("traj", "gain", "cur", "rec", "rep_n", "rep_k")


def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 830)
        tr = late_trainer(M, net, 1024, 44, horizon=16)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.state.acc.any())
        return (net.lut, tr.state.ea, tr.env.board, tr.delta, tr.x,
                *(getattr(tr.state, k) for k in TRAJ))

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], make_net(M.NS, NR.TUPLES_2x4, (3, 5), 830).lut)
    assert bool(a[1].any()) and bool(a[-2].any())
    ea = a[1]
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all()) and bool((ea[..., 1] >= 0).all())


def test_captured_step_and_env_step_replays(M):
    """step + env.step captured once and replayed 3 times equals 3 eager steps: table (with the
    promotions of each step), ea, the trajectory, boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    def make():
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 841)
        tr = late_trainer(M, net, 192, 45, horizon=8)
        tr.step(20)  # episodes have closed: boards replay, record and idle
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "x", "replays", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {k: getattr(tr.state, k).cpu().clone() for k in ("ea", *TRAJ)} |
                {"lut": net.lut.cpu().clone(), "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(3):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))
    assert bool(want[0]["delta"].any()) and bool(want[0]["replays"].any())

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    before = state(net, tr)
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    after = state(net, tr)  # the capture ran nothing
    assert all(torch.equal(after[k], before[k]) for k in ("lut", "ea", *TRAJ))
    assert not bool(tr.state.acc.any())
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
    tr = late_trainer(M, net, 64, 49, horizon=64, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and all(net.set_counts()) and not bool(tr.state.acc.any())
    assert bool(tr.state.ea[0].any()) and bool(tr.state.ea[1].any())
    with pytest.raises(ValueError):
        M.SB.BackwardTrainer(net, 32, restart=pool)
    with pytest.raises(TypeError):
        M.SB.BackwardTrainer(M.NT.NTupleNetwork(NR.TUPLES_2x4, device=DEV), 64)
    other = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (4,), device=DEV)
    with pytest.raises(ValueError):  # another network's state
        M.SB.BackwardTrainer(other, 64, state=tr.state)
    with pytest.raises(ValueError):  # a state of another board count
        M.SB.BackwardTrainer(net, 32, state=tr.state)
    tr.env.check_errors()


def test_a_run_resumes_bit_for_bit_from_a_saved_state(M, tmp_path):
    """30 steps, save the state, 20 more; a second run of 30 steps takes the file's ea and
    trajectory in a new state and ends where the first did.  With the trajectory reset it does
    not: it holds episodes not yet learned."""
    def start():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 850)
        tr = late_trainer(M, net, 256, 46, horizon=16)
        tr.step(30)
        torch.cuda.synchronize()
        return net, tr

    net, tr = start()
    tr.state.save(tmp_path / "state.pt")
    tr.step(20)
    torch.cuda.synchronize()
    want = (net.lut.clone(), tr.state.ea.clone(), tr.env.board.clone(), tr.state.traj.clone(),
            tr.state.rep_k.clone())

    net, tr = start()
    loaded = M.SB.BackwardState.load(tmp_path / "state.pt", net)
    assert loaded is not tr.state and (loaded.n, loaded.horizon) == (256, 16)
    for name in ("ea", *TRAJ):
        assert torch.equal(getattr(loaded, name), getattr(tr.state, name)), name
        assert getattr(loaded, name).device == net.lut.device
    assert not bool(loaded.acc.any()) and bool(loaded.rep_n.any())
    tr.state = loaded
    tr.step(20)
    torch.cuda.synchronize()
    for x, y in zip(want, (net.lut, tr.state.ea, tr.env.board, tr.state.traj, tr.state.rep_k)):
        assert torch.equal(x, y)

    net, tr = start()
    tr.state.reset()
    assert bool(tr.state.ea.any()) and not any(bool(getattr(tr.state, k).any()) for k in TRAJ)
    tr.step(20)
    torch.cuda.synchronize()
    assert not torch.equal(net.lut, want[0])


def test_from_state_continues_a_staged_batch_mean_tc_run(M):
    """30 steps of the thirteenth library's trainer, then its ea under a fresh trajectory: the
    first call replays nothing and moves nothing, the ea is a copy."""
    net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 860)
    tc = M.SMTC.StagedMeanTCTrainer(net, 256, seed=52)
    tc.step(30)
    torch.cuda.synchronize()
    st = M.SB.BackwardState.from_state(tc.state, net, 256, 8)
    assert torch.equal(st.ea, tc.state.ea) and st.ea.data_ptr() != tc.state.ea.data_ptr()
    lut = net.lut.clone()
    out = outputs(256)
    st.step(tc.env.board, 1, 4, *out)
    torch.cuda.synchronize()
    assert torch.equal(net.lut, lut) and not bool(out[1].any()) and not bool(out[4].any())
    assert not bool(out[3].any()) and bool(st.rec.any()) and not bool(st.acc.any())
    tr = M.SB.BackwardTrainer(net, 256, state=st, seed=53)
    assert tr.state is st and tr.state.horizon == 8


# ------------------------------------------------------------------ it learns
def test_staged_self_play_learns_under_backward_learning(M):
    """The recipe of test_stagedelay_gpu.py::test_staged_self_play_learns_under_delayed_lambda
    with this step: TUPLES_2x4, bounds (7,), 256 boards, p(4) = 0.5, the default rate 2^-4, seed
    61, 4000 steps, horizon 1024.  The mean merge score of the last 200 finished episodes is at
    least twice the random player's mean on the same seed, stage 1 has set entries, no set entry
    exceeds 2^28 in magnitude and |E| <= A everywhere.  The figures are printed.  Measured on an
    MI355X: 7753 over the last 200 of 2953 episodes (random player: 880), 4215 and 19 555 set
    entries in stages 0 and 1 (all of them with A > 0), largest |entry| 684 652."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (7,), device=DEV)
    tr = M.SB.BackwardTrainer(net, 256, horizon=1024, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MTC.default_meantc_lr_shift(net.spec) == 4
    assert tr.state.horizon == 1024
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
    print(f"backward learning L = 1024 on staged batch-mean TC, 2x4, bounds (7,), after 4000 "
          f"steps: {learned:.0f} over the last 200 of {len(scores)} episodes, set entries "
          f"{net.set_counts()}, largest |entry| {largest}, entries with A > 0 per stage "
          f"{ea[..., 1].count_nonzero(dim=(1, 2)).tolist()}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert net.set_counts()[1] > 0
    assert largest <= 1 << 28
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all())
    assert not bool(tr.state.acc.any())
