"""Delayed TD(lambda) on the staged batch-mean TC rule on the GPU (csrc/g2048_stagedelay.hip ->
libg2048_stagedelay.so) against the plain Python restatement tests/stagedelay_ref.py: the table
with its UNSET pattern, ea, the ring (hist, head, depth, g), action, err and the H planes of delta
bit for bit, and acc all zero, after every call -- at the frames' edges for every horizon, for
every T and S, on the hand anchors, on crafted batches, the 4 x 6 set, H = 1 next to
libg2048_stagemeantc.so, the trainer, a captured step, the restart pool, a resumed run, and that
self-play learns."""
import numpy as np
import pytest
import torch

import ntstage_ref as SR
import ntuple_ref as NR
import stagedelay_ref as R
from g2048 import stagedelay as _library
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
X1 = [1, 2] + [0] * 14
X2 = [1, 2] + [0] * 9 + [6, 0, 0, 0, 5]
LR = (3, 6)  # deltas of about 2^20 on a table of +-2^20: nothing leaves int32
# 1: a dead half-wave of the policy frame; 7, 8, 9: around a wave of the gather / apply frame (8
# boards); 63, 64, 65: around eight waves; 127, 128, 129: around their block; 1031: nine blocks
SIZES = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 1031)
HORIZONS = ((1, 1), (2, 31), (3, 1), (8, 4))  # (H, s)


class Modules:
    def __init__(self, ntuple, ntstage, ntmeantc, stagemeantc, stagedelay):
        self.NT, self.NS, self.MTC, self.SMTC, self.SD = (ntuple, ntstage, ntmeantc, stagemeantc,
                                                          stagedelay)


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmeantc, ntstage, ntuple, stagedelay, stagemeantc
    for mod in (ntuple, ntstage, ntmeantc, stagemeantc, stagedelay):
        mod.load()
    return Modules(ntuple, ntstage, ntmeantc, stagemeantc, stagedelay)


def outputs(n, H):
    return (torch.full((n,), 9, dtype=torch.uint8, device=DEV),
            torch.full((H, n), 77, dtype=torch.int32, device=DEV),
            torch.full((n,), 77, dtype=torch.int64, device=DEV))


class Call:
    """What one call did, from the reference."""

    def __init__(self, acts, errs, delta, ref, depth, legal):
        self.acts, self.errs, self.delta = acts, errs, delta
        self.hits, self.ms = dict(ref.last_hits), dict(ref.last_m)
        self.promoted = dict(ref.net.promoted)
        self.depth, self.legal = depth, legal  # the ring's depth before the call; legal(b) != 0

    def applied(self, i):
        return [k for k in range(len(self.delta)) if self.delta[k][i]]


class Pair:
    """A staged network and the rule's state on the GPU next to the reference over host copies of
    the table and of the ea it starts from (ea0: None = zeros)."""

    def __init__(self, M, net, n, H, s, ea0=None):
        self.net, self.n, self.H = net, n, H
        self.st = M.SD.DelayedLambdaState(net, n, H, s)
        self.base = net.lut.cpu().numpy().copy()
        base_ea = None
        if ea0 is not None:
            self.st.ea.copy_(torch.from_numpy(ea0))
            base_ea = lambda s_, t, i: (int(ea0[s_, t, i, 0]), int(ea0[s_, t, i, 1]))  # noqa: E731
        self.ea0 = np.zeros((*self.base.shape, 2), np.int64) if ea0 is None else ea0
        self.ref = R.Delayed(SR.StagedNet(net.spec.tuples, net.bounds, base=self.base), n, H, s,
                             base_ea=base_ea)

    def set_ring(self, hist, head, depth, g):
        """numpy hist u8 [H, n, 16], head [n], depth [n], g i64 [H, n] into both sides."""
        st, ref = self.st, self.ref
        st.hist.copy_(dev(hist))
        st.head.copy_(dev(head))
        st.depth.copy_(dev(depth))
        st.g.copy_(dev(g, np.int64))
        ref.hist = [lists(p) for p in hist]
        ref.head, ref.depth = [int(x) for x in head], [int(x) for x in depth]
        ref.g = [[int(x) for x in p] for p in g]

    def set_board_ring(self, i, afterstates, g=None, head=None):
        """Board i's ring: afterstates[k] is the one k steps back, g[k] its collected sum."""
        hist, hd = self.st.hist.cpu().numpy(), self.st.head.cpu().numpy()
        dp, gs = self.st.depth.cpu().numpy(), self.st.g.cpu().numpy()
        hd[i] = len(afterstates) - 1 if head is None else head
        dp[i] = len(afterstates)
        for k, b in enumerate(afterstates):
            p = (int(hd[i]) - k) % self.H
            hist[p, i] = b
            gs[p, i] = 0 if g is None else g[k]
        self.set_ring(hist, hd, dp, gs)

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
        st, ref = self.st, self.ref
        got, want = self.net.lut.cpu().numpy(), self.want_table()
        assert np.array_equal(got == UNSET, want == UNSET)
        assert np.array_equal(got, want)
        assert np.array_equal(st.ea.cpu().numpy(), self.want_ea())
        assert st.hist.cpu().tolist() == ref.hist
        assert st.head.cpu().tolist() == ref.head and st.depth.cpu().tolist() == ref.depth
        assert st.g.cpu().tolist() == ref.g
        assert not bool(st.acc.any())

    def step(self, boards, lr_num, lr_shift):
        """One step on both sides from the same state; everything is compared."""
        out = outputs(self.n, self.H)
        depth = list(self.ref.depth)
        self.st.step(dev(boards), lr_num, lr_shift, *out)
        acts, errs, delta = self.ref.step(lists(boards), lr_num, lr_shift)
        assert out[0].cpu().tolist() == acts
        assert out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == delta
        self.check_state()
        legal = [bool(x) for x in (np.asarray(boards) != np.array(CHECKER)).any(axis=1)]
        return Call(acts, errs, delta, self.ref, depth, legal)


def random_ring(rng, n, H, caps=(4, 7, 11)):
    """A ring the rule could have built on a table without UNSET: every depth 0..H, every head,
    afterstates of all stages, collected sums of both signs."""
    hist = np.stack([stage_boards(rng, n, caps) for _ in range(H)])
    return (hist, rng.integers(0, H, n).astype(np.uint8),
            rng.integers(0, H + 1, n).astype(np.uint8), rng.integers(-(1 << 22), 1 << 22, (H, n)))


def batch(rng, n, t, caps=(4, 7, 11), period=5):
    """Random boards of all stages; every `period`-th row, moving with the call, is terminal."""
    boards = stage_boards(rng, n, caps)
    boards[(np.arange(n) + t) % period == 2] = CHECKER
    return boards


# ------------------------------------------------------------------ sizes, H, T and S
@pytest.mark.parametrize("H,s", HORIZONS)
@pytest.mark.parametrize("n", SIZES)
def test_step_at_wave_and_block_edges_for_every_horizon(M, n, H, s):
    """Every size class and horizon on the 2 x 4 set with the bounds (5, 8): a table without
    UNSET, a seeded ea and a random ring, so that from the first of three calls boards of every
    depth meet terminal and non-terminal boards."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 501, upper=1.0)
    pair = Pair(M, net, n, H, s, seeded_ea(tuple(net.lut.shape), 502))
    rng = np.random.default_rng(510 + 16 * n + H)
    pair.set_ring(*random_ring(rng, n, H))
    calls = [pair.step(batch(rng, n, t), *LR) for t in range(3)]
    sets = [(len(c.applied(i)), c.legal[i], c.depth[i]) for c in calls for i in range(n)]
    assert all(k <= 1 for k, legal, _d in sets if legal)
    if n >= 127:
        # an episode's end empties a window of several slots; elsewhere the oldest slot leaves
        assert any(k == d >= min(H, 2) and not legal for k, legal, d in sets)
        assert any(k == 1 and legal and d == H for k, legal, d in sets)
        assert {d > 0 for c in calls for p in c.delta for d in p if d} == {True, False}
        assert any(cnt > 8 for c in calls for _d, cnt in c.hits.values())
        assert {k[0] for c in calls for k in c.hits} == {0, 1, 2}


@pytest.mark.parametrize("H,s", HORIZONS)
def test_a_fresh_ring_on_a_half_unset_table_promotes_before_it_adds(M, H, s):
    """129 boards from the fresh state on a table whose upper stages are half UNSET, H + 3 calls:
    the window fills, its oldest slot leaves, head wraps; every entry a call adds into was
    promoted while its afterstate was prev (a hit on UNSET raises in the reference)."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 520)
    pair = Pair(M, net, 129, H, s)
    rng = np.random.default_rng(521 + H)
    calls, heads = [], set()
    for t in range(H + 3):
        # a row ends its episode once in the H + 3 calls, so windows fill in between
        calls.append(pair.step(batch(rng, 129, t, period=H + 3), *LR))
        heads |= set(pair.ref.head)
    assert any(c.promoted for c in calls) and any(c.hits for c in calls)
    assert max(pair.ref.depth) == H and 0 in pair.ref.depth
    assert heads == set(range(H))


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(M, T):
    """Every instantiation of the three kernels: the first T tuples of an 8 x 3 set, H = 3."""
    net = make_net(M.NS, T8M3[:T], (5, 8), 530 + T)
    pair = Pair(M, net, 129, 3, 1, seeded_ea(tuple(net.lut.shape), 535 + T))
    rng = np.random.default_rng(540 + T)
    calls = [pair.step(batch(rng, 129, t), *LR) for t in range(5)]
    assert {k[1] for c in calls for k in c.hits} == set(range(T))
    assert {k[0] for c in calls for k in c.hits} == {0, 1, 2}


@pytest.mark.parametrize("S", [1, 2, 3])
def test_every_stage_count(M, S):
    bounds = (5, 8)[:S - 1]
    net = make_net(M.NS, NR.TUPLES_2x4, bounds, 550 + S, upper=0.25)
    pair = Pair(M, net, 129, 2, 4, seeded_ea(tuple(net.lut.shape), 555 + S))
    rng = np.random.default_rng(560 + S)
    calls = [pair.step(batch(rng, 129, t), *LR) for t in range(4)]
    assert {k[0] for c in calls for k in c.hits} == set(range(S)) == {k[0] for k in pair.ref.A}


# ------------------------------------------------------------------ the anchors, on the device
def corner_pair(M, bounds, n, H, s=1, preset=None, tuples=((0,),), lut0=None):
    net = M.NS.StagedNTupleNetwork(tuples, bounds, device=DEV)
    row = 1024 * np.arange(net.lut.shape[2]) if lut0 is None else np.asarray(lut0)
    net.lut[0, 0].copy_(dev(row, np.int32))
    ea0 = None
    if preset:
        ea0 = np.zeros((*net.lut.shape, 2), np.int64)
        for k, v in preset.items():
            ea0[k] = v
    pair = Pair(M, net, n, H, s, ea0)
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


def pair_lut(values):
    lut0 = [0] * 256
    for i, v in values.items():
        lut0[i] = v
    return lut0


def test_anchor_r_the_shift_rounds_toward_zero(M):
    for values, err, want in (({33: 1}, -1, [[-1], [0], [0]]),
                              ({33: 1, 1: 2}, -3, [[-3], [-1], [0]])):
        pair = corner_pair(M, (), 1, 3, tuples=((0, 1),), lut0=pair_lut(values))
        pair.set_board_ring(0, [X1, Q2, Q3])
        c = pair.step(np.array([CHECKER], np.uint8), 1, 0)
        assert (c.errs, c.delta) == ([err], want)
    assert c.hits == {(0, 0, 33): (-3, 1), (0, 0, 1): (-3, 1), (0, 0, 2): (-2, 2),
                      (0, 0, 0): (-24, 12)}


def test_anchor_w_a_window_fills_applies_its_oldest_slot_and_wraps_head(M):
    pair = corner_pair(M, (), 1, 2)
    a, cb = np.array([A], np.uint8), np.array([CHECKER], np.uint8)
    c = pair.step(a, 1, 1)
    assert (c.acts, c.errs, c.delta) == ([2], [0], [[0], [0]])
    c = pair.step(a, 1, 1)
    assert (c.errs, c.delta) == ([4096], [[0], [0]]) and not entries(pair)
    assert pair.st.g.cpu().tolist() == [[0], [4096]] and pair.st.head.cpu().tolist() == [0]
    c = pair.step(a, 1, 1)
    assert (c.errs, c.delta) == ([4096], [[0], [3072]])
    assert entries(pair) == {(0, 0, 2): 5120, (0, 0, 0): 3072}
    assert ea_entries(pair) == {(0, 0, 2): (3072, 3072), (0, 0, 0): (3072, 3072)}
    assert pair.st.g.cpu().tolist() == [[4096], [0]] and pair.st.head.cpu().tolist() == [1]
    c = pair.step(cb, 1, 1)  # terminal at depth H
    assert (c.errs, c.delta) == ([-28672], [[-14336], [-5120]])
    assert c.hits == {(0, 0, 2): (-38912, 4), (0, 0, 0): (-116736, 12)}
    assert entries(pair) == {(0, 0, 2): -4608, (0, 0, 0): -6656}
    assert ea_entries(pair) == {(0, 0, 2): (-6656, 12800), (0, 0, 0): (-6656, 12800)}
    assert pair.st.depth.cpu().tolist() == [0] and pair.st.g.cpu().tolist() == [[4096], [0]]
    c = pair.step(cb, 1, 1)  # terminal at depth 0
    assert (c.errs, c.delta) == ([0], [[0], [0]]) and not c.hits
    assert entries(pair) == {(0, 0, 2): -4608, (0, 0, 0): -6656}


def test_anchor_t1_a_terminal_call_at_depth_1(M):
    pair = corner_pair(M, (), 1, 2)
    pair.step(np.array([A], np.uint8), 1, 1)
    c = pair.step(np.array([CHECKER], np.uint8), 1, 1)
    assert (c.errs, c.delta) == ([-4096], [[-2048], [0]])
    assert entries(pair) == {(0, 0, 2): 0, (0, 0, 0): -2048}


def test_anchor_c2_two_afterstates_of_one_terminal_board_share_an_entry(M):
    pair = corner_pair(M, (), 1, 2, tuples=((0, 1),), lut0=pair_lut({33: 1, 1: 2}))
    pair.set_board_ring(0, [X1, X2], g=[0, -4])
    c = pair.step(np.array([CHECKER], np.uint8), 1, 0)
    assert (c.errs, c.delta) == ([-3], [[-3], [-5]])
    assert c.hits[(0, 0, 33)] == (-8, 2) and c.ms[(0, 0, 33)] == -4
    assert entries(pair) == {(0, 0, 33): -3, (0, 0, 1): -2, (0, 0, 0): -4, (0, 0, 5): -5,
                             (0, 0, 101): -5}


def test_anchor_s2_two_boards_of_different_stages_address_one_index(M):
    pair = corner_pair(M, (3,), 2, 2)
    pair.set_board_ring(0, [Q2])
    pair.set_board_ring(1, [Q3])
    c = pair.step(np.array([CHECKER, CHECKER], np.uint8), 1, 1)
    assert (c.errs, c.delta) == ([-4096, -6144], [[-2048, -3072], [0, 0]])
    assert c.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert entries(pair) == {(0, 0, 2): 0, (0, 0, 0): -2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    ea = ea_entries(pair)
    assert ea[(0, 0, 0)] == (-2048, 2048) and ea[(1, 0, 0)] == (-3072, 3072)


def test_anchor_p_promoted_while_prev_and_moved_h_minus_1_calls_later(M):
    pair = corner_pair(M, (2,), 1, 2)
    a = np.array([A], np.uint8)
    assert not pair.step(a, 1, 1).promoted
    c = pair.step(a, 1, 1)
    assert c.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0} == entries(pair) and not c.hits
    c = pair.step(a, 1, 1)
    assert not c.promoted and c.delta == [[0], [3072]]
    assert entries(pair) == {(1, 0, 2): 5120, (1, 0, 0): 3072}


def test_anchor_z_a_g_that_cancels_makes_no_hit_and_leaves_ea(M):
    pair = corner_pair(M, (), 1, 2, preset={(0, 0, 3): (5, 9)})
    pair.set_board_ring(0, [Q2, Q3], g=[0, -2048], head=0)
    c = pair.step(np.array([A], np.uint8), 1, 1)
    assert (c.errs, c.delta) == ([4096], [[0], [0]]) and not c.hits
    assert not entries(pair) and ea_entries(pair) == {(0, 0, 3): (5, 9)}
    assert pair.st.g.cpu().tolist() == [[4096], [0]] and pair.st.head.cpu().tolist() == [1]


# ------------------------------------------------------------------ crafted batches
def test_a_block_of_terminal_boards_with_full_rings_overflows_both_lds_tables(M):
    """T = 8, m = 4, H = 8, 128 terminal boards whose rings are full of random full boards: one
    block makes 128 * 8 * 64 = 65 536 hits on more distinct staged entries than the gather's 4096
    slots or the apply's 8192 hold, so hits that find no slot after four probes go straight to
    memory beside merged ones, in both launches.  Then non-terminal boards refill the rings."""
    net = make_net(M.NS, T8M4, (10,), 570, upper=1.0)
    n, H = 128, 8
    pair = Pair(M, net, n, H, 4, seeded_ea(tuple(net.lut.shape), 571))
    rng = np.random.default_rng(572)
    hist = rng.integers(1, 12, (H, n, 16)).astype(np.uint8)
    pair.set_ring(hist, rng.integers(0, H, n).astype(np.uint8), np.full(n, H, np.uint8),
                  rng.integers(-(1 << 22), 1 << 22, (H, n)))
    c = pair.step(np.array([CHECKER] * n, np.uint8), 7, 5)
    assert all(len(c.applied(i)) == H for i in range(n))
    assert sum(cnt for _d, cnt in c.hits.values()) == n * H * 64 and len(c.hits) > 8192
    assert {k[0] for k in c.hits} == {0, 1} and pair.ref.depth == [0] * n
    boards = rng.integers(0, 12, (n, 16)).astype(np.uint8)
    boards[:, 0] = 0  # an empty corner: every board has a legal move
    c = pair.step(boards, 7, 5)
    assert not c.hits and set(pair.ref.depth) == {1}


def test_129_copies_of_one_board(M):
    """One ring on every row: C = 129 times the hits of one board, one block of 128 boards and one
    more; a non-terminal call with a full window, then a terminal one that empties it."""
    net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 580, upper=1.0)
    n, H = 129, 3
    pair = Pair(M, net, n, H, 1, seeded_ea(tuple(net.lut.shape), 581))
    ring = [[7, 1, 0, 1, 2, 0, 2, 1, 0, 0, 0, 0, 1, 0, 0, 2], [5] * 16,
            [8, 1, 0, 1, 2, 0, 2, 1, 0, 0, 3, 0, 1, 0, 0, 2]]
    hist = np.array([[r] * n for r in ring], np.uint8)
    pair.set_ring(hist, np.full(n, 1, np.uint8), np.full(n, H, np.uint8),
                  np.array([[1000] * n, [-70000] * n, [30] * n]))
    b = [6, 3, 0, 1, 2, 0, 0, 1, 0, 0, 3, 0, 1, 0, 0, 2]
    c = pair.step(np.array([b] * n, np.uint8), 1, 4)
    assert len(set(c.delta[2])) == 1 and c.delta[2][0] != 0 and not any(c.delta[0] + c.delta[1])
    assert all(cnt % n == 0 and d == cnt * c.delta[2][0] for d, cnt in c.hits.values())
    c = pair.step(np.array([CHECKER] * n, np.uint8), 1, 4)
    assert all(len(set(p)) == 1 and p[0] != 0 for p in c.delta)
    # the one-valued board's 8 symmetries coincide: one entry per tuple gets 8 * 129 of its hits
    assert sorted(cnt for _d, cnt in c.hits.values())[-2:] == [8 * n, 8 * n]
    assert all(cnt % n == 0 for _d, cnt in c.hits.values())


# ------------------------------------------------------------------ the 4 x 6 set
def test_4x6_two_stages_touched_entries_set_counts_and_ea(M):
    """The 4 x 6 table with bounds (11,) (512 MiB, 2 GiB of acc, 2 GiB of ea), 129 boards, H = 3,
    six calls from the fresh state: the touched staged entries of lut and ea (gathered, not a
    dense copy), the set counts, the ring and acc.any().  Staged indices reach past 2^24."""
    rng = np.random.default_rng(590)
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_4x6, (11,), device=DEV)
    g = torch.Generator(device=DEV).manual_seed(591)
    net.lut[0].copy_(torch.randint(-(1 << 20), 1 << 20, net.lut[0].shape, generator=g, device=DEV,
                                   dtype=torch.int32))
    n, H = 129, 3
    st = M.SD.DelayedLambdaState(net, n, H, 1)
    assert st.acc.numel() * 8 == 2 << 30 == st.ea.numel() * 8
    base = SparseBase(net.lut[0])
    ref = R.Delayed(SR.StagedNet(net.spec.tuples, net.bounds, base=base), n, H, 1)
    stage0 = net.lut.shape[1] * net.lut.shape[2]
    moved = 0
    for t in range(6):
        boards = batch(rng, n, t, caps=(5, 9, 11))
        keys = []
        for b in lists(boards):
            keys += ref.net.indices(b)
            for a in range(4):
                keys += ref.net.indices(NR.E.move(b, a)[0])
        base.prefetch(keys)
        out = outputs(n, H)
        st.step(dev(boards), 5, 9, *out)
        acts, errs, delta = ref.step(lists(boards), 5, 9)
        assert out[0].cpu().tolist() == acts and out[2].cpu().tolist() == errs
        assert out[1].cpu().tolist() == delta
        assert st.hist.cpu().tolist() == ref.hist and st.g.cpu().tolist() == ref.g
        assert st.head.cpu().tolist() == ref.head and st.depth.cpu().tolist() == ref.depth
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
        moved += len(ref.last_hits)
    assert moved > 500 and {k[0] for k in ref.A} == {0, 1}


# ------------------------------------------------------------------ trainer, graph
def test_h1_is_libg2048_stagemeantc_over_50_trainer_steps(M):
    """Consequence 1 against the thirteenth library itself: the two trainers from one seed, lut,
    ea, actions, err and delta equal after every step; plane 0 is prev and depth is has_prev."""
    nets = [make_net(M.NS, NR.TUPLES_2x4, (3, 5), 600) for _ in range(2)]
    tc = M.SMTC.StagedMeanTCTrainer(nets[0], 256, seed=51)
    dl = M.SD.DelayedLambdaTrainer(nets[1], 256, horizon=1, lam_shift=9, seed=51)
    assert (dl.lr_num, dl.lr_shift) == (tc.lr_num, tc.lr_shift) == (1, 4)
    for t in range(50):
        tc.step(1)
        dl.step(1)
        assert torch.equal(nets[0].lut, nets[1].lut), t
        assert torch.equal(tc.state.ea, dl.state.ea), t
        assert torch.equal(tc.actions, dl.actions) and torch.equal(tc.err, dl.err), t
        assert torch.equal(tc.delta, dl.delta[0]), t
        assert torch.equal(tc.has_prev, dl.state.depth) and torch.equal(tc.env.board, dl.env.board)
        assert torch.equal(tc.prev[tc.has_prev != 0], dl.state.hist[0][tc.has_prev != 0]), t
        assert not bool(dl.state.acc.any()) and not bool(dl.state.g.any()), t
    assert bool(dl.state.ea.any()) and bool(dl.delta.any())
    dl.env.check_errors()


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """DelayedLambdaTrainer at H = 3, 64 boards on the 2x4 set, at its default rate, next to the
    reference driving an OracleEnv: actions, err, the delta planes, the ring, the whole table and
    the whole ea after each of 50 steps, acc all zero.  A low bound besides, so stage 1 is
    reached."""
    for bounds, n, seed in (((7,), 64, 47), ((3,), 64, 48)):
        net = make_net(M.NS, NR.TUPLES_2x4, bounds, 610)
        net.lut[1:].fill_(UNSET)
        base = net.lut.cpu().numpy().copy()
        tr = M.SD.DelayedLambdaTrainer(net, n, seed=seed)
        assert (tr.lr_num, tr.lr_shift, tr.state.horizon, tr.state.lam_shift) == (1, 4, 3, 1)
        ref = R.Delayed(SR.StagedNet(NR.TUPLES_2x4, bounds, base=base), n, 3, 1)
        oracle = O.OracleEnv(n, seed)
        hits = 0
        for t in range(50):
            boards = oracle.board.copy()
            assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
            tr.step(1)
            acts, errs, delta = ref.step(lists(boards), 1, 4)
            hits += len(ref.last_hits)
            oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
            assert tr.actions.cpu().tolist() == acts, t
            assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == delta, t
            st = tr.state
            assert st.hist.cpu().tolist() == ref.hist and st.g.cpu().tolist() == ref.g, t
            assert st.head.cpu().tolist() == ref.head and st.depth.cpu().tolist() == ref.depth, t
            want = base.copy()
            for s, ents in enumerate(ref.net.stages):
                for (k, i), v in ents.items():
                    want[s, k, i] = v
            assert np.array_equal(net.lut.cpu().numpy(), want), t
            want_ea = np.zeros((*base.shape, 2), np.int64)
            for (s, k, i), a in ref.A.items():
                want_ea[s, k, i] = (ref.E[(s, k, i)], a)
            assert np.array_equal(st.ea.cpu().numpy(), want_ea), t
            assert not bool(st.acc.any()), t
        assert hits > 1000
        if bounds == (3,):
            assert len(ref.net.stages[1]) > 100 and any(k[0] == 1 for k in ref.A)
        tr.env.check_errors()


def test_e_stays_within_a_over_200_trainer_steps(M):
    net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 620)
    tr = M.SD.DelayedLambdaTrainer(net, 1024, seed=43)
    tr.step(200)
    torch.cuda.synchronize()
    ea = tr.state.ea
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all()) and bool((ea[..., 1] >= 0).all())
    assert bool((ea[..., 0].abs() < ea[..., 1]).any())
    assert bool((ea[..., 1] > 0).any(dim=2).any(dim=1).all())
    assert int(ea[..., 1].max()) <= 200 << 31  # at most 2^31 per call
    assert not bool(tr.state.acc.any())
    tr.env.check_errors()


def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 620)
        tr = M.SD.DelayedLambdaTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.state.acc.any())
        st = tr.state
        return net.lut, st.ea, tr.env.board, st.hist, st.head, st.depth, st.g, tr.delta

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], make_net(M.NS, NR.TUPLES_2x4, (3, 5), 620).lut)
    assert bool(a[1].any()) and bool(a[6].any())


RING = ("hist", "head", "depth", "g")


def test_captured_step_and_env_step_replays(M):
    """step + env.step captured once and replayed 3 times equals 3 eager steps: table (with the
    promotions of each step), ea, the ring, boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    start = stage_boards(np.random.default_rng(630), 192)

    def make():
        net = make_net(M.NS, NR.TUPLES_2x4, (5, 8), 631)
        tr = M.SD.DelayedLambdaTrainer(net, 192, seed=45)
        tr.env.board.copy_(dev(start))
        tr.step(4)  # full windows on the boards that have not ended
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {k: getattr(tr.state, k).cpu().clone() for k in ("ea", *RING)} |
                {"lut": net.lut.cpu().clone(), "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(3):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))
    assert bool(want[0]["delta"].any())

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    before = state(net, tr)
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    after = state(net, tr)  # the capture ran nothing
    assert all(torch.equal(after[k], before[k]) for k in ("lut", "ea", *RING))
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
    tr = M.SD.DelayedLambdaTrainer(net, 64, seed=49, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and all(net.set_counts()) and not bool(tr.state.acc.any())
    assert bool(tr.state.ea[0].any()) and bool(tr.state.ea[1].any())
    with pytest.raises(ValueError):
        M.SD.DelayedLambdaTrainer(net, 32, restart=pool)
    with pytest.raises(TypeError):
        M.SD.DelayedLambdaTrainer(M.NT.NTupleNetwork(NR.TUPLES_2x4, device=DEV), 64)
    other = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (4,), device=DEV)
    with pytest.raises(ValueError):  # another network's state
        M.SD.DelayedLambdaTrainer(other, 64, state=tr.state)
    with pytest.raises(ValueError):  # a state of another board count
        M.SD.DelayedLambdaTrainer(net, 32, state=tr.state)
    tr.env.check_errors()


def test_a_run_resumes_bit_for_bit_from_a_saved_state(M, tmp_path):
    """30 steps, save the state, 20 more; a second run of 30 steps takes the file's ea and ring in
    a new state and ends where the first did.  With the ring reset it does not: the ring holds
    errors not yet applied."""
    def start():
        net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 640)
        tr = M.SD.DelayedLambdaTrainer(net, 256, seed=46)
        tr.step(30)
        torch.cuda.synchronize()
        return net, tr

    net, tr = start()
    tr.state.save(tmp_path / "state.pt")
    tr.step(20)
    torch.cuda.synchronize()
    want = (net.lut.clone(), tr.state.ea.clone(), tr.env.board.clone(), tr.state.g.clone())

    net, tr = start()
    loaded = M.SD.DelayedLambdaState.load(tmp_path / "state.pt", net)
    assert loaded is not tr.state and (loaded.n, loaded.horizon, loaded.lam_shift) == (256, 3, 1)
    for name in ("ea", *RING):
        assert torch.equal(getattr(loaded, name), getattr(tr.state, name)), name
        assert getattr(loaded, name).device == net.lut.device
    assert not bool(loaded.acc.any())
    tr.state = loaded
    tr.step(20)
    torch.cuda.synchronize()
    for x, y in zip(want, (net.lut, tr.state.ea, tr.env.board, tr.state.g)):
        assert torch.equal(x, y)

    net, tr = start()
    tr.state.reset()
    assert bool(tr.state.ea.any()) and not bool(tr.state.depth.any())
    tr.step(20)
    torch.cuda.synchronize()
    assert not torch.equal(net.lut, want[0])


def test_from_state_continues_a_staged_batch_mean_tc_run(M):
    """30 steps of the thirteenth library's trainer, then its ea under a fresh ring: the first
    call has no previous afterstate and moves nothing, the ea is a copy."""
    net = make_net(M.NS, NR.TUPLES_2x4, (3, 5), 650)
    tc = M.SMTC.StagedMeanTCTrainer(net, 256, seed=52)
    tc.step(30)
    torch.cuda.synchronize()
    st = M.SD.DelayedLambdaState.from_state(tc.state, net, 256, 2, 3)
    assert torch.equal(st.ea, tc.state.ea) and st.ea.data_ptr() != tc.state.ea.data_ptr()
    lut = net.lut.clone()
    out = outputs(256, 2)
    st.step(tc.env.board, 1, 4, *out)
    torch.cuda.synchronize()
    assert torch.equal(net.lut, lut) and not bool(out[1].any()) and not bool(out[2].any())
    assert bool(st.depth.any()) and not bool(st.g.any()) and not bool(st.acc.any())


# ------------------------------------------------------------------ it learns
def test_staged_self_play_learns_under_delayed_lambda(M):
    """The recipe of test_stagemeantc_gpu.py::test_staged_self_play_learns_under_batch_mean_tc
    with this step at its defaults (H = 3, lambda = 1 / 2): TUPLES_2x4, bounds (7,), 256 boards,
    p(4) = 0.5, the default rate 2^-4, seed 61, 4000 steps.  The mean merge score of the last 200
    finished episodes is at least twice the random player's mean on the same seed, stage 1 has
    set entries, no set entry exceeds 2^28 in magnitude and |E| <= A everywhere.  The figures are
    printed.  Measured on an MI355X: 6072 over the last 200 of 3627 episodes (random player: 880),
    2726 and 16 417 set entries in stages 0 and 1 (2726 and 16 415 of them with A > 0), largest
    |entry| 741 368."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NS.StagedNTupleNetwork(NR.TUPLES_2x4, (7,), device=DEV)
    tr = M.SD.DelayedLambdaTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MTC.default_meantc_lr_shift(net.spec) == 4
    assert (tr.state.horizon, tr.state.lam_shift) == (3, 1)
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
    print(f"delayed TD(lambda) H = 3, s = 1 on staged batch-mean TC, 2x4, bounds (7,), after 4000 "
          f"steps: {learned:.0f} over the last 200 of {len(scores)} episodes, set entries "
          f"{net.set_counts()}, largest |entry| {largest}, entries with A > 0 per stage "
          f"{ea[..., 1].count_nonzero(dim=(1, 2)).tolist()}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert net.set_counts()[1] > 0
    assert largest <= 1 << 28
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all())
    assert not bool(tr.state.acc.any())
