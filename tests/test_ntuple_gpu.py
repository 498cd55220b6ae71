"""The n-tuple network kernels (csrc/g2048_ntuple.hip -> libg2048_ntuple.so) against the plain
Python restatement tests/ntuple_ref.py: values, policy and whole TD(0) training runs bit for bit
(the table after every step included), the player against the oracle env, a captured step, and
that self-play learns."""
import numpy as np
import pytest
import torch

import ntuple_ref as R
from boards import mask_boards
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
SPECS = {"1x1": ((0,),), "8x3": T8M3, "2x4": R.TUPLES_2x4, "4x6": R.TUPLES_4x6}


@pytest.fixture(scope="module")
def NT():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntuple
    ntuple.load()
    return ntuple


def random_table(NT, tuples, seed):
    """A network whose table holds random int32 in +-2^20."""
    net = NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


@pytest.fixture(scope="module")
def nets(NT):
    """One randomly filled network per spec, shared and never trained."""
    return {name: random_table(NT, tuples, 11 + k) for k, (name, tuples) in enumerate(SPECS.items())}


class DeviceBase:
    """The table as it was at construction, for the reference: entries are gathered from the
    device tensor by index, in batches, so a 256 MiB table is never copied to the host."""

    def __init__(self, lut, clone=False):
        self.lut = lut.clone() if clone else lut
        self.cache = {}

    def prefetch(self, keys):
        miss = sorted(set(keys) - self.cache.keys())
        if miss:
            t = torch.tensor([k[0] for k in miss], device=self.lut.device)
            i = torch.tensor([k[1] for k in miss], device=self.lut.device)
            for k, v in zip(miss, self.lut[t, i].cpu().tolist()):
                self.cache[k] = v

    def __call__(self, t, i):
        if (t, i) not in self.cache:
            self.prefetch([(t, i)])
        return self.cache[(t, i)]


def ref_net(net, boards=(), afterstates=True, clone=False):
    """The reference over net's table, the entries that `boards` (and their afterstates) read
    already gathered."""
    base = DeviceBase(net.lut, clone)
    ref = R.Net(net.spec.tuples, base=base)
    prefetch(ref, boards, afterstates)
    return ref


def prefetch(ref, boards, afterstates=True):
    keys = []
    for b in boards:
        b = [int(x) for x in b]
        keys += ref.indices(b)
        if afterstates:
            for a in range(4):
                keys += ref.indices(R.E.move(b, a)[0])
    ref.base.prefetch(keys)


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def crafted_boards():
    rng = np.random.default_rng(5)
    out = [np.array(b, np.uint8) for b in mask_boards()]
    sq = rng.integers(0, 9, (4, 4))
    out.append(np.triu(sq) + np.triu(sq, 1).T)                    # transpose-symmetric
    out.append(np.concatenate([sq[:, :2], sq[:, 1::-1]], axis=1))  # symmetric under a column flip
    out.append(np.concatenate([sq[:2], sq[1::-1]], axis=0))        # symmetric under a row flip
    half = np.concatenate([sq[:, :2], sq[:, 1::-1]], axis=1)
    out.append(np.concatenate([half[:2], half[1::-1]], axis=0))    # under both flips
    out += [np.full(16, 3), np.full(16, 0), np.full(16, 15), np.full(16, 16)]  # all-equal boards
    # exponents 15, 16 and 17: clamped in the index only, never in the move
    out += [[17, 16, 15, 15, 16, 15, 0, 0, 3, 2, 1, 0, 0, 0, 0, 1],
            [15, 15, 16, 16, 17, 17, 15, 16, 1, 2, 1, 2, 0, 1, 0, 1],
            [16, 16, 17, 0, 15, 15, 15, 15, 2, 1, 2, 1, 1, 2, 1, 2],
            [14, 14, 15, 15, 16, 16, 17, 17, 0, 0, 0, 0, 17, 16, 15, 14]]
    return np.array([np.asarray(b, np.uint8).reshape(16) for b in out], np.uint8)


def ref_policy(ref, boards):
    q = np.full((len(boards), 4), R.INT64_MIN, np.int64)
    acts = np.zeros(len(boards), np.uint8)
    after = np.zeros((len(boards), 16), np.uint8)
    for i, b in enumerate(boards):
        qs, acts[i], after[i] = ref.policy(b)
        for a in range(4):
            if qs[a] is not None:
                q[i, a] = qs[a]
    return q, acts, after


# ------------------------------------------------------------------ 1. values
@pytest.mark.parametrize("name", list(SPECS))
def test_values_bit_for_bit(NT, nets, name):
    net = nets[name]
    rng = np.random.default_rng(21)
    sets = [random_boards(rng, n) for n in (1, 3, 64, 257)] + [crafted_boards()]
    ref = ref_net(net, np.concatenate(sets), afterstates=False)
    for boards in sets:
        got = net.values(dev(boards)).cpu().numpy()
        want = np.array([ref.V(b) for b in boards], np.int64)
        bad = np.flatnonzero(got != want)
        assert len(bad) == 0, (len(boards), boards[bad[0]].tolist(), got[bad[0]], want[bad[0]])
    # a board's value does not depend on where it sits in the batch; the out tensor is used
    boards = sets[3]
    out = torch.zeros(257, dtype=torch.int64, device=DEV)
    assert net.values(dev(boards[::-1].copy()), out=out) is out
    assert np.array_equal(out.cpu().numpy()[::-1], np.array([ref.V(b) for b in boards]))


def test_symmetric_boards_share_indices(nets):
    """The crafted boards really make several (g, t) share an index, and the all-equal board is
    8 T reads of one entry per tuple."""
    ref = R.Net(R.TUPLES_2x4)
    b = crafted_boards()
    n_masks = len(mask_boards())
    for k in range(4):
        keys = ref.indices(b[n_masks + k])
        assert len(set(keys)) < len(keys)
    assert len(set(ref.indices(b[n_masks + 4]))) == 2
    net = nets["2x4"]
    idx = 3 + (3 << 4) + (3 << 8) + (3 << 12)
    want = 8 * int(net.lut[0, idx]) + 8 * int(net.lut[1, idx])
    assert int(net.values(dev(b[n_masks + 4:n_masks + 5]))[0]) == want


# ------------------------------------------------------------------ 2. act
@pytest.mark.parametrize("name", list(SPECS))
def test_act_bit_for_bit(NT, nets, name):
    net = nets[name]
    rng = np.random.default_rng(22)
    sets = [random_boards(rng, n) for n in ((1, 3, 64, 257) if name != "4x6" else (3, 64))]
    sets.append(crafted_boards())
    ref = ref_net(net, np.concatenate(sets))
    for boards in sets:
        acts, q, after = net.act(dev(boards), after=True)
        want_q, want_a, want_after = ref_policy(ref, boards)
        assert np.array_equal(q.cpu().numpy(), want_q), len(boards)
        assert np.array_equal(acts.cpu().numpy(), want_a), len(boards)
        assert np.array_equal(after.cpu().numpy(), want_after), len(boards)


def test_act_covers_every_legal_mask_and_marks_illegal_moves(nets):
    boards = np.array(mask_boards(), np.uint8)
    masks = np.array([O.legal_mask(b) for b in boards])
    assert len(set(masks.tolist())) == 16
    acts, q, after = nets["2x4"].act(dev(boards), after=True)
    acts, q, after = acts.cpu().numpy(), q.cpu().numpy(), after.cpu().numpy()
    legal = ((masks[:, None] >> np.arange(4)) & 1).astype(bool)
    assert ((q != R.INT64_MIN) == legal).all()
    assert (legal[np.arange(len(boards)), acts] | (masks == 0)).all()
    dead = masks == 0
    assert dead.any() and (acts[dead] == 0).all() and np.array_equal(after[dead], boards[dead])
    for i in np.flatnonzero(~dead):
        assert np.array_equal(after[i], O.move(boards[i], acts[i])[0])


def test_act_on_a_zero_table_is_the_gain(NT):
    net = NT.NTupleNetwork(NT.TUPLES_2x4, device=DEV)
    boards = np.concatenate([random_boards(np.random.default_rng(23), 200), crafted_boards()])
    acts, q, _ = net.act(dev(boards))
    acts, q = acts.cpu().numpy(), q.cpu().numpy()
    ties = 0
    for i, b in enumerate(boards):
        gains = []
        for a in range(4):
            after, gain = R.E.move(b, a)
            gains.append(gain << R.F if after != [int(x) for x in b] else None)
        assert [None if x == R.INT64_MIN else int(x) for x in q[i]] == gains
        live = [g for g in gains if g is not None]
        want = gains.index(max(live)) if live else 0  # the smallest move among the largest
        assert acts[i] == want
        ties += live.count(max(live)) > 1 if live else 0
    assert ties > 20


def test_act_output_variants(NT, nets):
    """Each combination of NULL outputs writes the same bytes as the full call, touches nothing
    around an output, and leaves an output that was not asked for alone."""
    import g2048._native as N

    net, n, pad = nets["2x4"], 67, 64
    boards = dev(random_boards(np.random.default_rng(24), n))
    lib = NT.load()

    def call(want_q, want_a, want_after):
        qb = torch.full((pad + 4 * n + pad,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        ab = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        fb = torch.full((pad + 16 * n + pad,), 0xC3, dtype=torch.uint8, device=DEV)
        import ctypes as C
        rc = lib.g2048_ntuple_act(C.byref(net._c), net.lut.data_ptr(), boards.data_ptr(), n,
                                  qb[pad:].data_ptr() if want_q else None,
                                  ab[pad:].data_ptr() if want_a else None,
                                  fb[pad:].data_ptr() if want_after else None, 0,
                                  torch.cuda.current_stream().cuda_stream)
        assert rc == N.G2048_OK, lib.g2048_ntuple_last_error()
        torch.cuda.synchronize()
        return qb.cpu().numpy(), ab.cpu().numpy(), fb.cpu().numpy()

    full = call(True, True, True)
    blank = (np.full_like(full[0], 0x5A5A5A5A5A5A5A5A), np.full_like(full[1], 0xA5),
             np.full_like(full[2], 0xC3))
    for k, size in enumerate((4 * n, n, 16 * n)):
        assert np.array_equal(full[k][:pad], blank[k][:pad])
        assert np.array_equal(full[k][pad + size:], blank[k][pad + size:])
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1)):
        got = call(*want)
        for k in range(3):
            assert np.array_equal(got[k], full[k] if want[k] else blank[k]), (want, k)
    ref = ref_net(net, boards.cpu().numpy())
    want_q, want_a, want_after = ref_policy(ref, boards.cpu().numpy())
    assert np.array_equal(full[0][pad:pad + 4 * n].reshape(n, 4), want_q)
    assert np.array_equal(full[1][pad:pad + n], want_a)
    assert np.array_equal(full[2][pad:pad + 16 * n].reshape(n, 16), want_after)
    # the wrapper returns None for what was not asked for
    acts, q, after = net.act(boards, q=False)
    assert q is None and after is None and np.array_equal(acts.cpu().numpy(), want_a)


# ------------------------------------------------------------------ 3-5. td_step
class Run:
    """A GPU training run (network, env, per-board state) next to the reference driving an
    OracleEnv, stepped together and compared after every step."""

    def __init__(self, NT, net, n, seed, lr_num, lr_shift, boards=None, dense=True):
        import g2048

        self.net, self.n, self.lr = net, n, (lr_num, lr_shift)
        self.dense = dense
        self.base = net.lut.cpu().numpy().copy() if dense else None
        self.ref = R.Net(net.spec.tuples, base=self.base if dense
                         else DeviceBase(net.lut, clone=True))
        self.env = g2048.VecEnv2048(n, seed=seed, device=DEV, reset=boards is None)
        self.oracle = O.OracleEnv(n, seed, reset=boards is None)
        if boards is not None:
            self.env.board.copy_(dev(boards))
            self.oracle.board[:] = boards
        kw = dict(device=DEV)
        self.prev = torch.zeros((n, 16), dtype=torch.uint8, **kw)
        self.has_prev = torch.zeros(n, dtype=torch.uint8, **kw)
        self.actions = torch.full((n,), 9, dtype=torch.uint8, **kw)
        self.delta = torch.full((n,), 77, dtype=torch.int32, **kw)
        self.err = torch.full((n,), 77, dtype=torch.int64, **kw)
        self.ref_prev = [[0] * 16 for _ in range(n)]
        self.ref_has = [0] * n
        self.errs = []

    def step(self, t):
        boards = self.oracle.board.copy()
        assert np.array_equal(self.env.board.cpu().numpy(), boards), t
        if not self.dense:
            prefetch(self.ref, list(boards) + self.ref_prev)
        self.net.td_step(self.env.board, self.prev, self.has_prev, *self.lr, self.actions,
                         self.delta, self.err)
        self.env.step(self.actions)
        acts, errs, deltas = self.ref.td_step(boards, self.ref_prev, self.ref_has, *self.lr)
        self.oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
        assert self.actions.cpu().tolist() == acts, t
        assert self.err.cpu().tolist() == errs, t
        assert self.delta.cpu().tolist() == deltas, t
        assert self.prev.cpu().tolist() == self.ref_prev, t
        assert self.has_prev.cpu().tolist() == self.ref_has, t
        self.errs += errs
        if self.dense:  # the whole table
            want = self.base.copy()
            for (t_, i), v in self.ref.touched.items():
                want[t_, i] = v
            assert np.array_equal(self.net.lut.cpu().numpy(), want), t


def test_td_step_under_heavy_collisions(NT):
    """16 entries, 257 boards: every board adds into the same few entries, within a wave and
    across waves.  The whole table and all per-board state equal the reference after each of
    30 steps."""
    net = random_table(NT, ((0,),), 31)
    run = Run(NT, net, 257, seed=41, lr_num=3, lr_shift=15)
    for t in range(30):
        run.step(t)
    errs = np.array(run.errs)
    assert (errs > 0).any() and (errs < 0).any()
    run.env.check_errors()


def near_terminal_boards(rng, n):
    """Full boards whose neighbours differ in parity (odd exponents 3..9 on one colour of the
    checkerboard, even ones 4..10 on the other, so nothing merges, a spawned tile included),
    with one or two holes."""
    colour = (np.arange(16) // 4 + np.arange(16) % 4) % 2
    b = np.where(colour == 0, 2 * rng.integers(1, 5, (n, 16)) + 1, 2 * rng.integers(2, 6, (n, 16)))
    for row in b:
        row[rng.choice(16, int(rng.integers(1, 3)), replace=False)] = 0
    return b.astype(np.uint8)


def test_td_step_through_episode_ends(NT):
    net = random_table(NT, NT.TUPLES_2x4, 32)
    boards = near_terminal_boards(np.random.default_rng(33), 64)
    run = Run(NT, net, 64, seed=42, lr_num=1, lr_shift=8, boards=boards)
    saw_terminal = 0
    for t in range(16):
        saw_terminal += sum(O.legal_mask(b) == 0 for b in run.oracle.board)
        run.step(t)
    ended = run.env.ep[:, 0].cpu().numpy()
    assert np.array_equal(ended, run.oracle.ep[:, 0].astype(ended.dtype))
    # at least 8 boards ended an episode and played on from a fresh board
    assert saw_terminal >= 8 and (ended > 0).sum() >= 8
    played_on = (ended > 0) & (np.array(run.ref_has) == 1)
    assert played_on.sum() >= 8
    run.env.check_errors()


def test_td_step_4x6_touched_entries_and_table_sum(NT, nets):
    """The 256 MiB table: 64 boards, 20 steps.  The entries the reference touched (a sparse
    dict) and the int64 sum of the whole table are exact."""
    net = NT.NTupleNetwork(NT.TUPLES_4x6, device=DEV)
    net.lut.copy_(nets["4x6"].lut)
    sum0 = int(net.lut.sum(dtype=torch.int64))
    run = Run(NT, net, 64, seed=43, lr_num=5, lr_shift=9, dense=False)
    for t in range(20):
        run.step(t)
    touched = run.ref.touched
    assert len(touched) > 1000
    keys = sorted(touched)
    ti = torch.tensor([k[0] for k in keys], device=DEV)
    ii = torch.tensor([k[1] for k in keys], device=DEV)
    assert net.lut[ti, ii].cpu().tolist() == [touched[k] for k in keys]
    moved = sum(v - run.ref.base(*k) for k, v in touched.items())
    assert moved != 0 and int(net.lut.sum(dtype=torch.int64)) == sum0 + moved
    errs = np.array(run.errs)
    assert (errs > 0).any() and (errs < 0).any()


def test_td_step_with_more_entries_than_the_block_can_merge(NT):
    """T = 8 on unrelated random boards: a block of the update (128 boards) adds into up to
    8192 different entries, as many as its LDS table has slots, so adds that find no slot and
    go straight to memory occur beside merged ones.  Random previous afterstates, some boards
    without one, some terminal; one step, everything compared."""
    net = random_table(NT, T8M3, 36)
    rng = np.random.default_rng(37)
    n = 257
    boards = np.concatenate([random_boards(rng, n - 40, fills=(0.8, 1.0)),
                             np.array(mask_boards(), np.uint8)[:40]])
    prev0 = rng.integers(0, 16, (n, 16)).astype(np.uint8)
    has0 = (rng.random(n) < 0.9).astype(np.uint8)
    base = net.lut.cpu().numpy().copy()
    ref = R.Net(T8M3, base=base)
    ref_prev, ref_has = [list(map(int, p)) for p in prev0], [int(h) for h in has0]
    acts, errs, deltas = ref.td_step(boards, ref_prev, ref_has, 7, 5)
    keys = {k for i in range(n) if has0[i] and deltas[i] for k in ref.indices(prev0[i])}
    assert len(keys) > 8192 and 0 in ref_has and 0 in deltas
    prev, has_prev = dev(prev0), dev(has0)
    out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out_d = torch.zeros(n, dtype=torch.int32, device=DEV)
    out_e = torch.zeros(n, dtype=torch.int64, device=DEV)
    net.td_step(dev(boards), prev, has_prev, 7, 5, out_a, out_d, out_e)
    assert out_a.cpu().tolist() == acts and out_e.cpu().tolist() == errs
    assert out_d.cpu().tolist() == deltas
    assert prev.cpu().tolist() == ref_prev and has_prev.cpu().tolist() == ref_has
    want = base.copy()
    for (t, i), v in ref.touched.items():
        want[t, i] = v
    assert np.array_equal(net.lut.cpu().numpy(), want)
    # err_out is optional: the same step without it
    net2 = random_table(NT, T8M3, 36)
    prev, has_prev = dev(prev0), dev(has0)
    net2.td_step(dev(boards), prev, has_prev, 7, 5, out_a, out_d, None)
    assert torch.equal(net2.lut, net.lut) and out_d.cpu().tolist() == deltas


@pytest.mark.parametrize("T", range(1, 9))
def test_td_step_at_every_tuple_count(NT, T):
    """Every instantiation of the policy and update kernels (T = 1..8, the first T tuples of
    T8M3): 131 boards -- two update blocks, an odd count, a dead half-wave in the policy kernel --
    3 steps from reset boards.  Step 0 has no previous afterstate and adds nothing; the later
    steps add into the few early-game entries all boards share.  Table, prev, has_prev, actions,
    err and delta equal the reference after every step."""
    net = random_table(NT, T8M3[:T], 50 + T)
    run = Run(NT, net, 131, seed=46, lr_num=3, lr_shift=6)
    run.step(0)
    assert not run.ref.touched and run.ref_has == [1] * 131
    for t in (1, 2):
        run.step(t)
    adds = 2 * 8 * T * 131  # (board, g, t) triples that added, at most
    assert 0 < len(run.ref.touched) < adds // 4 and {k[0] for k in run.ref.touched} == set(range(T))
    run.env.check_errors()


# ------------------------------------------------------------------ 6. order-free
def test_two_identical_runs_give_equal_tables(NT):
    def run():
        net = random_table(NT, NT.TUPLES_2x4, 34)
        tr = NT.NTupleTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        return net.lut, tr.env.board, tr.prev

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], random_table(NT, NT.TUPLES_2x4, 34).lut)


# ------------------------------------------------------------------ 7. graph capture
def test_captured_td_step_and_env_step_replays(NT):
    """td_step + env.step captured once and replayed 3 times equals 3 eager steps: table,
    boards and outputs."""
    from g2048.dist import graph_capture

    def make():
        net = random_table(NT, NT.TUPLES_2x4, 35)
        tr = NT.NTupleTrainer(net, 192, seed=45, lr_num=1, lr_shift=7)
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


# ------------------------------------------------------------------ 8. the player
def test_player_matches_oracle_stepped_with_reference_actions(NT, nets):
    """64 games x 40 steps of play("ntuple"): boards, rewards and actions equal an OracleEnv
    stepped with the reference's actions from the same seed."""
    from g2048.player import BatchedPlayer

    n, steps, seed, net = 64, 40, 51, nets["2x4"]
    res = BatchedPlayer(n, device=DEV, seed=seed, ntuple=net, record_games=n,
                        max_moves=steps).play("ntuple")
    assert len(res.trace) == steps
    o = O.OracleEnv(n, seed, flags=O.NO_AUTORESET)
    ref = R.Net(net.spec.tuples, base=net.lut.cpu().numpy())
    for t, (before, act, reward, score_before, after) in enumerate(res.trace):
        assert np.array_equal(before.cpu().numpy(), o.board), t
        want = np.array([ref.policy(b)[1] for b in o.board], np.uint8)
        assert np.array_equal(act.cpu().numpy(), want), t
        assert np.array_equal(score_before.cpu().numpy().astype(np.uint32), o.meta[:, 0]), t
        r = o.step(O.MODE_ACTIONS, actions=want)
        assert np.array_equal(reward.cpu().numpy(), r["reward"]), t
        assert np.array_equal(after.cpu().numpy(), o.board), t
    assert not res.stuck.any()


def test_player_plays_games_to_the_end(NT, nets):
    """Whole games: every game ends on a board without a legal move, with the reference's
    bookkeeping (history length = moves, last history score = merge score)."""
    from g2048.player import BatchedPlayer

    res = BatchedPlayer(32, device=DEV, seed=52, ntuple=nets["2x4"], p4=0.1,
                        record_games=2).play("ntuple")
    assert (res.moves > 14).all() and not res.stuck.any()
    for g, h in enumerate(res.histories):
        assert len(h) == res.moves[g] and h[-1][2] == 0 and h[-1][3] == res.merge_score[g]
        last = np.where(h[-1][0] > 0, np.log2(np.maximum(h[-1][0], 1)), 0).astype(np.uint8)
        assert O.legal_mask(last.reshape(16)) == 0


# ------------------------------------------------------------------ 9. it learns
def test_self_play_learns(NT):
    """NTupleTrainer on TUPLES_2x4, 256 boards, lr 1 / 2^10, 4000 steps: the mean merge score of
    the last 200 finished episodes exceeds twice the random player's mean on the same seed (the
    CPU prototype of the same rule reached 4052 against about 841, a ratio of 4.8, with another
    spawn stream).  Measured on an MI355X: see the printed figures and DESIGN 4.10."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = NT.NTupleNetwork(NT.TUPLES_2x4, device=DEV)
    tr = NT.NTupleTrainer(net, 256, seed=seed, p4=0.5, lr_num=1, lr_shift=10, log_slots=64)
    assert tr.lr_shift == NT.default_lr_shift(256) == 10
    scores = []
    for _chunk in range(4):
        tr.step(1000)
        ep = tr.episodes()
        scores += ep["score"].tolist()
        print(f"steps {1000 * (_chunk + 1)}: {len(scores)} episodes, mean merge score of the "
              f"last 200: {np.mean(scores[-200:]):.0f}")
    tr.env.check_errors()
    rnd = BatchedPlayer(256, device=DEV, seed=seed).play("random")
    learned, random_mean = float(np.mean(scores[-200:])), float(rnd.merge_score.mean())
    print(f"n-tuple 2x4 after 4000 steps: {learned:.0f} over the last 200 of {len(scores)} "
          f"episodes, largest |entry| {int(net.lut.abs().max())}; random player: "
          f"{random_mean:.0f}")
    assert len(scores) >= 200
    assert learned > 2 * random_mean
