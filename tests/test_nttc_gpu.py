"""Temporal-coherence learning on the GPU (csrc/g2048_nttc.hip -> libg2048_nttc.so) against the
plain Python restatement tests/nttc_ref.py: whole training runs bit for bit -- actions, err,
delta, prev, has_prev, the whole table and all accumulators after every step -- the shift path of
the rate on preloaded accumulators, the first step against TD(0), two identical runs, a captured
step, and that self-play learns."""
import numpy as np
import pytest
import torch

import nttc_ref as R
import ntuple_ref as NR
from boards import mask_boards
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))


class Modules:
    def __init__(self, ntuple, nttc):
        self.NT, self.TC = ntuple, nttc


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import nttc, ntuple
    ntuple.load()
    nttc.load()
    return Modules(ntuple, nttc)


def random_table(M, tuples, seed):
    """A network whose table holds random int32 in +-2^20."""
    net = M.NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


def random_ea(rng, shape):
    """In-domain accumulators int64 [*shape, 2]: an eighth each with A = 0, A within 2 of 2^16,
    E = A, E = -A and E = 0; otherwise A of 1..46 bits (up to 2^45) and E uniform in [-A, A]."""
    kind = rng.integers(0, 8, shape)
    a = rng.integers(0, 1 << 45, shape, endpoint=True) >> rng.integers(0, 45, shape)
    a = np.where(kind == 0, 0, np.where(kind == 1, (1 << 16) + rng.integers(-2, 3, shape), a))
    e = rng.integers(-a, a, endpoint=True)
    e = np.where(kind == 2, a, np.where(kind == 3, -a, np.where(kind == 4, 0, e)))
    assert (np.abs(e) <= a).all() and (a >= 0).all()
    return np.stack([e, a], axis=-1).astype(np.int64)


class DeviceBase:
    """The table as it was at construction, for the reference: entries are gathered from the
    device tensor by index, in batches, so a 256 MiB table is never copied to the host."""

    def __init__(self, lut):
        self.lut = lut.clone()
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


def prefetch(ref, boards):
    keys = []
    for b in boards:
        b = [int(x) for x in b]
        keys += ref.indices(b)
        for a in range(4):
            keys += ref.indices(NR.E.move(b, a)[0])
    ref.base.prefetch(keys)


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def ea_base(ea0):
    return lambda t, i: (int(ea0[t, i, 0]), int(ea0[t, i, 1]))


def want_dense(base, touched):
    want = base.copy()
    for (t, i), v in touched.items():
        want[t, i] = v
    return want


def want_ea(ea0, tc):
    want = ea0.copy()
    for (t, i), a in tc.A.items():
        want[t, i] = (tc.E[(t, i)], a)
    return want


class Run:
    """A GPU TC training run (network, accumulators, env, per-board state) next to the reference
    driving an OracleEnv, stepped together and compared after every step."""

    def __init__(self, M, net, n, seed, lr_num, lr_shift, boards=None, dense=True):
        import g2048

        self.net, self.n, self.lr = net, n, (lr_num, lr_shift)
        self.tc = M.TC.TCState(net)
        self.dense = dense
        self.base = net.lut.cpu().numpy().copy() if dense else None
        self.ea0 = np.zeros((*net.lut.shape, 2), np.int64) if dense else None
        self.ref = R.TC(NR.Net(net.spec.tuples, base=self.base if dense else DeviceBase(net.lut)))
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
        self.work = torch.full((M.TC.work_bytes(net.spec, n),), 0xA5, dtype=torch.uint8, **kw)
        self.ref_prev = [[0] * 16 for _ in range(n)]
        self.ref_has = [0] * n
        self.errs = []

    def step(self, t):
        boards = self.oracle.board.copy()
        assert np.array_equal(self.env.board.cpu().numpy(), boards), t
        if not self.dense:
            prefetch(self.ref.net, list(boards) + self.ref_prev)
        self.tc.tc_step(self.env.board, self.prev, self.has_prev, *self.lr, self.actions,
                        self.delta, self.err, self.work)
        self.env.step(self.actions)
        acts, errs, deltas = self.ref.step(boards, self.ref_prev, self.ref_has, *self.lr)
        self.oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
        assert self.actions.cpu().tolist() == acts, t
        assert self.err.cpu().tolist() == errs, t
        assert self.delta.cpu().tolist() == deltas, t
        assert self.prev.cpu().tolist() == self.ref_prev, t
        assert self.has_prev.cpu().tolist() == self.ref_has, t
        self.errs += errs
        if self.dense:  # the whole table and all accumulators
            assert np.array_equal(self.net.lut.cpu().numpy(),
                                  want_dense(self.base, self.ref.net.touched)), t
            assert np.array_equal(self.tc.ea.cpu().numpy(), want_ea(self.ea0, self.ref)), t


# ------------------------------------------------------------------ 1. heavy collisions
def test_tc_step_under_heavy_collisions(M):
    """16 entries, 257 boards: every board adds into the same few entries, within a wave and
    across waves, and after the first step the entries' rates differ from 1 and from each other.
    Table, accumulators and all per-board state equal the reference after each of 30 steps."""
    net = random_table(M, ((0,),), 31)
    run = Run(M, net, 257, seed=41, lr_num=3, lr_shift=15)
    slowed = 0  # steps that read an entry whose rate is below 1
    for t in range(30):
        slowed += any(R.rate(run.ref.E[k], run.ref.A[k]) < R.ONE for k in run.ref.A)
        run.step(t)
    rates = [R.rate(run.ref.E[k], run.ref.A[k]) for k in run.ref.A]
    assert slowed >= 25 and sum(r < R.ONE for r in rates) >= 2 and len(set(rates)) >= 2
    errs = np.array(run.errs)
    assert (errs > 0).any() and (errs < 0).any()
    run.env.check_errors()


@pytest.mark.parametrize("T", range(1, 9))
def test_tc_step_at_every_tuple_count(M, T):
    """Every instantiation of the policy and update kernels (T = 1..8, the first T tuples of
    T8M3): 131 boards -- two update blocks, an odd count, a dead half-wave in the policy kernel --
    3 steps from reset boards.  Step 0 has no previous afterstate and adds nothing; the later
    steps add into the few early-game entries all boards share.  Table, accumulators, prev,
    has_prev, actions, err and delta equal the reference after every step."""
    net = random_table(M, T8M3[:T], 50 + T)
    run = Run(M, net, 131, seed=46, lr_num=3, lr_shift=6)
    run.step(0)
    assert not run.ref.A and not run.ref.net.touched and run.ref_has == [1] * 131
    for t in (1, 2):
        run.step(t)
    adds = 2 * 8 * T * 131  # (board, g, t) triples that added, at most
    assert 0 < len(run.ref.A) < adds // 4 and {k[0] for k in run.ref.A} == set(range(T))
    run.env.check_errors()


# ------------------------------------------------------------------ 2. the shift path
def test_tc_step_rate_shift_path_on_preloaded_accumulators(M):
    """The 2x4 set, 64 boards, one step on accumulators preloaded with seeded in-domain values:
    A = 0, E = +-A, A around 2^16 and A up to 2^45, so the entries the step reads take s = 0 and
    s > 0 and have rates of 0, of 2^16 and in between (asserted on the reference)."""
    net = random_table(M, M.NT.TUPLES_2x4, 38)
    rng = np.random.default_rng(39)
    n = 64
    ea0 = random_ea(rng, net.lut.shape)
    assert ea0[..., 1].max() > 1 << 44
    tc = M.TC.TCState(net)
    tc.ea.copy_(dev(ea0, np.int64))
    boards = random_boards(rng, n, fills=(0.5, 0.8))
    prev0 = rng.integers(0, 16, (n, 16)).astype(np.uint8)
    base = net.lut.cpu().numpy().copy()
    ref = R.TC(NR.Net(net.spec.tuples, base=base), base_ea=ea_base(ea0))
    ref_prev, ref_has = [list(map(int, p)) for p in prev0], [1] * n
    acts, errs, deltas = ref.step(boards, ref_prev, ref_has, 1, 4)
    read = [ref.base_ea(*k) for i in range(n) if deltas[i] for k in ref.net.indices(prev0[i])]
    shifts = {R.shift_of(a) for _e, a in read}
    rates = {R.rate(e, a) for e, a in read}
    assert 0 in shifts and max(shifts) >= 25 and len(shifts) > 10
    assert 0 in rates and R.ONE in rates and any(0 < r < R.ONE for r in rates)
    assert any(a == 0 for _e, a in read) and any(a in (65535, 65536, 65537) for _e, a in read)
    assert any(d < 0 for d in deltas) and any(d > 0 for d in deltas)
    prev, has_prev = dev(prev0), dev(np.ones(n, np.uint8))
    out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out_d = torch.zeros(n, dtype=torch.int32, device=DEV)
    out_e = torch.zeros(n, dtype=torch.int64, device=DEV)
    tc.tc_step(dev(boards), prev, has_prev, 1, 4, out_a, out_d, out_e)
    assert out_a.cpu().tolist() == acts and out_e.cpu().tolist() == errs
    assert out_d.cpu().tolist() == deltas
    assert prev.cpu().tolist() == ref_prev and has_prev.cpu().tolist() == ref_has
    assert np.array_equal(net.lut.cpu().numpy(), want_dense(base, ref.net.touched))
    assert np.array_equal(tc.ea.cpu().numpy(), want_ea(ea0, ref))


# ------------------------------------------------------------------ 3. episode ends
def near_terminal_boards(rng, n):
    """Full boards whose neighbours differ in parity (odd exponents 3..9 on one colour of the
    checkerboard, even ones 4..10 on the other, so nothing merges, a spawned tile included),
    with one or two holes."""
    colour = (np.arange(16) // 4 + np.arange(16) % 4) % 2
    b = np.where(colour == 0, 2 * rng.integers(1, 5, (n, 16)) + 1, 2 * rng.integers(2, 6, (n, 16)))
    for row in b:
        row[rng.choice(16, int(rng.integers(1, 3)), replace=False)] = 0
    return b.astype(np.uint8)


def test_tc_step_through_episode_ends(M):
    net = random_table(M, M.NT.TUPLES_2x4, 32)
    boards = near_terminal_boards(np.random.default_rng(33), 64)
    run = Run(M, net, 64, seed=42, lr_num=1, lr_shift=8, boards=boards)
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


# ------------------------------------------------------------------ 4. the 4x6 set
def test_tc_step_4x6_touched_entries_and_sums(M):
    """The 256 MiB table with its 1 GiB of accumulators: 64 boards, 20 steps.  The entries the
    reference touched (sparse dicts) and the int64 sums of the whole table, of all E and of all
    A are exact."""
    net = random_table(M, M.NT.TUPLES_4x6, 14)
    sum0 = int(net.lut.sum(dtype=torch.int64))
    run = Run(M, net, 64, seed=43, lr_num=5, lr_shift=9, dense=False)
    for t in range(20):
        run.step(t)
    touched, ref = run.ref.net.touched, run.ref
    assert len(touched) > 1000 and set(touched) == set(ref.A) == set(ref.E)
    keys = sorted(touched)
    ti = torch.tensor([k[0] for k in keys], device=DEV)
    ii = torch.tensor([k[1] for k in keys], device=DEV)
    assert net.lut[ti, ii].cpu().tolist() == [touched[k] for k in keys]
    assert run.tc.ea[ti, ii].cpu().tolist() == [[ref.E[k], ref.A[k]] for k in keys]
    moved = sum(v - ref.net.base(*k) for k, v in touched.items())
    assert moved != 0 and int(net.lut.sum(dtype=torch.int64)) == sum0 + moved
    assert int(run.tc.ea[..., 0].sum()) == sum(ref.E.values()) != 0
    assert int(run.tc.ea[..., 1].sum()) == sum(ref.A.values())
    assert any(R.rate(ref.E[k], ref.A[k]) < R.ONE for k in keys)
    errs = np.array(run.errs)
    assert (errs > 0).any() and (errs < 0).any()


# ------------------------------------------------------------------ 5. past the LDS table
def test_tc_step_with_more_entries_than_the_block_can_merge(M):
    """T = 8 on unrelated random boards: a block of the update (128 boards) adds into up to
    8192 different entries, more than its LDS table has slots, so adds that find no slot and go
    straight to memory occur beside merged ones.  Random previous afterstates and preloaded
    accumulators, some boards without a previous afterstate, some terminal; one step, everything
    compared; then the same step without err_out."""
    net = random_table(M, T8M3, 36)
    rng = np.random.default_rng(37)
    n = 257
    boards = np.concatenate([random_boards(rng, n - 40, fills=(0.8, 1.0)),
                             np.array(mask_boards(), np.uint8)[:40]])
    prev0 = rng.integers(0, 16, (n, 16)).astype(np.uint8)
    has0 = (rng.random(n) < 0.9).astype(np.uint8)
    ea0 = random_ea(rng, net.lut.shape)
    base = net.lut.cpu().numpy().copy()
    ref = R.TC(NR.Net(T8M3, base=base), base_ea=ea_base(ea0))
    ref_prev, ref_has = [list(map(int, p)) for p in prev0], [int(h) for h in has0]
    acts, errs, deltas = ref.step(boards, ref_prev, ref_has, 7, 5)
    assert len(ref.A) > 8192 and 0 in ref_has and 0 in deltas
    tc = M.TC.TCState(net)
    tc.ea.copy_(dev(ea0, np.int64))
    prev, has_prev = dev(prev0), dev(has0)
    out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    out_d = torch.zeros(n, dtype=torch.int32, device=DEV)
    out_e = torch.zeros(n, dtype=torch.int64, device=DEV)
    tc.tc_step(dev(boards), prev, has_prev, 7, 5, out_a, out_d, out_e)
    assert out_a.cpu().tolist() == acts and out_e.cpu().tolist() == errs
    assert out_d.cpu().tolist() == deltas
    assert prev.cpu().tolist() == ref_prev and has_prev.cpu().tolist() == ref_has
    assert np.array_equal(net.lut.cpu().numpy(), want_dense(base, ref.net.touched))
    assert np.array_equal(tc.ea.cpu().numpy(), want_ea(ea0, ref))
    # err_out is optional: the same step without it
    net2 = random_table(M, T8M3, 36)
    tc2 = M.TC.TCState(net2)
    tc2.ea.copy_(dev(ea0, np.int64))
    prev, has_prev = dev(prev0), dev(has0)
    out_d.zero_()
    tc2.tc_step(dev(boards), prev, has_prev, 7, 5, out_a, out_d, None)
    assert torch.equal(net2.lut, net.lut) and torch.equal(tc2.ea, tc.ea)
    assert out_d.cpu().tolist() == deltas and out_a.cpu().tolist() == acts


# ------------------------------------------------------------------ 6. fresh ea is TD(0)
def test_first_step_from_fresh_accumulators_is_the_td0_step(M):
    """1 031 boards (an odd size across blocks): from a zero ea every rate is 2^16, so the
    table, the outputs and the per-board state equal NTupleNetwork.td_step's on the same inputs,
    and E and A are the sums of the deltas and of their magnitudes."""
    n = 1031
    rng = np.random.default_rng(40)
    boards = dev(np.concatenate([random_boards(rng, n - 40),
                                 np.array(mask_boards(), np.uint8)[:40]]))
    prev0 = random_boards(rng, n, hi=14)
    has0 = (rng.random(n) < 0.9).astype(np.uint8)

    def outputs():
        return (torch.zeros(n, dtype=torch.uint8, device=DEV),
                torch.zeros(n, dtype=torch.int32, device=DEV),
                torch.zeros(n, dtype=torch.int64, device=DEV))

    td_net, tc_net = random_table(M, M.NT.TUPLES_2x4, 46), random_table(M, M.NT.TUPLES_2x4, 46)
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs()
    td_net.td_step(boards, td_prev, td_has, 3, 6, *td_out)
    tc = M.TC.TCState(tc_net)
    tc_prev, tc_has, tc_out = dev(prev0), dev(has0), outputs()
    tc.tc_step(boards, tc_prev, tc_has, 3, 6, *tc_out)
    assert torch.equal(tc_net.lut, td_net.lut)
    assert not torch.equal(tc_net.lut, random_table(M, M.NT.TUPLES_2x4, 46).lut)
    for a, b in zip(tc_out + (tc_prev, tc_has), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    # the accumulators: 16 pairs per adding board
    d = tc_out[1].to(torch.int64)[dev(has0).bool()]
    assert int(tc.ea[..., 0].sum()) == 16 * int(d.sum())
    assert int(tc.ea[..., 1].sum()) == 16 * int(d.abs().sum()) > 0
    assert bool((tc.ea[..., 0].abs() <= tc.ea[..., 1]).all())
    # a second step is no longer TD(0): some rates have dropped below 1
    td_net.td_step(boards, td_prev, td_has, 3, 6, *td_out)
    tc.tc_step(boards, tc_prev, tc_has, 3, 6, *tc_out)
    assert torch.equal(tc_out[1], td_out[1]) and not torch.equal(tc_net.lut, td_net.lut)


# ------------------------------------------------------------------ 7. order-free
def test_two_identical_runs_give_equal_tables_and_accumulators(M):
    def run():
        net = random_table(M, M.NT.TUPLES_2x4, 34)
        tr = M.TC.TCTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        return net.lut, tr.tc.ea, tr.env.board, tr.prev

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], random_table(M, M.NT.TUPLES_2x4, 34).lut)
    assert bool(a[1].any()) and bool((a[1][..., 0].abs() <= a[1][..., 1]).all())


# ------------------------------------------------------------------ 8. graph capture
def test_captured_tc_step_and_env_step_replays(M):
    """tc_step + env.step captured once and replayed 3 times equals 3 eager steps: table,
    accumulators, boards and outputs."""
    from g2048.dist import graph_capture

    def make():
        net = random_table(M, M.NT.TUPLES_2x4, 35)
        tr = M.TC.TCTrainer(net, 192, seed=45, lr_num=1, lr_shift=7)
        tr.step(2)  # a state with afterstates on every board
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "prev", "has_prev", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {"lut": net.lut.cpu().clone(), "ea": tr.tc.ea.cpu().clone(),
                 "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(3):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    lut0, ea0 = net.lut.clone(), tr.tc.ea.clone()
    st0 = {k: getattr(tr, k).clone() for k in ("prev", "has_prev")}
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert torch.equal(net.lut, lut0) and torch.equal(tr.tc.ea, ea0)
    assert all(torch.equal(getattr(tr, k), v) for k, v in st0.items())
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        got = state(net, tr)
        for name, t in want[k].items():
            assert torch.equal(got[name], t), (k, name)
    tr.env.check_errors()


# ------------------------------------------------------------------ 9. it learns
def test_self_play_learns_under_tc(M):
    """The recipe of test_ntuple_gpu.py::test_self_play_learns with the TC step: TUPLES_2x4, 256
    boards, the default rate 1 / 2^10, seed 61, 4000 steps.  The mean merge score of the last 200
    finished episodes is at least twice the random player's mean on the same seed (the bar of
    that test), and no table entry exceeds 2^28 in magnitude.  Measured on an MI355X: see the
    printed figures and DESIGN 4.12."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    tr = M.TC.TCTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.NT.default_lr_shift(256) == 10
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
    largest = int(net.lut.to(torch.int64).abs().max())
    print(f"TC n-tuple 2x4 after 4000 steps: {learned:.0f} over the last 200 of {len(scores)} "
          f"episodes, largest |entry| {largest}, largest A {int(tr.tc.ea[..., 1].max())}; "
          f"random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert largest <= 1 << 28
