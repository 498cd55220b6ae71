"""Truncated TD(lambda) learning on the GPU (csrc/g2048_ntlambda.hip -> libg2048_ntlambda.so)
against the plain Python restatement tests/ntlambda_ref.py, bit for bit after every step: actions,
err, delta, the ring (hist, head, depth) and the table.  Sizes that cross a lane group, a wave and
the update's block; every tuple count, horizon and a few shifts; H = 1 against TD(0); heavy
collisions; more keys than the merge table has slots; episode ends; the 4x6 table; two identical
runs; a captured step; and that self-play learns."""
import numpy as np
import pytest
import torch

import ntlambda_ref as R
import ntuple_ref as NR
from boards import mask_boards
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# 8 tuples of 4 distinct cells (the offsets 0, 5, 11, 14 differ modulo 16)
T8M4 = tuple((t, (t + 5) % 16, (t + 11) % 16, (t + 14) % 16) for t in range(8))


class Modules:
    def __init__(self, ntuple, ntlambda):
        self.NT, self.L = ntuple, ntlambda


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntlambda, ntuple
    ntuple.load()
    ntlambda.load()
    return Modules(ntuple, ntlambda)


def random_table(M, tuples, seed):
    """A network whose table holds random int32 in +-2^20."""
    net = M.NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


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


def prefetch(net, boards):
    keys = []
    for b in boards:
        b = [int(x) for x in b]
        keys += net.indices(b)
        for a in range(4):
            keys += net.indices(NR.E.move(b, a)[0])
    net.base.prefetch(keys)


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def want_dense(base, touched):
    want = base.copy()
    for (t, i), v in touched.items():
        want[t, i] = v
    return want


class Run:
    """A GPU TD(lambda) run (network, ring, per-board outputs) next to the reference, stepped
    together and compared after every step.  The boards of a step come from `feed(t)` (an array
    [n, 16]) or, without one, from a VecEnv2048 that an OracleEnv shadows (started from `boards`
    or from a reset) and that steps with the chosen actions in between."""

    def __init__(self, M, net, n, H, s, lr_num, lr_shift, seed=0, boards=None, feed=None,
                 dense=True):
        import g2048

        self.net, self.n, self.lr, self.feed = net, n, (lr_num, lr_shift), feed
        self.lam = M.L.TDLambdaState(net, n, H, s)
        self.dense = dense
        self.base = net.lut.cpu().numpy().copy() if dense else None
        self.ref = R.Lam(NR.Net(net.spec.tuples, base=self.base if dense else DeviceBase(net.lut)),
                         n, H, s)
        if feed is None:
            self.env = g2048.VecEnv2048(n, seed=seed, device=DEV, reset=boards is None)
            self.oracle = O.OracleEnv(n, seed, reset=boards is None)
            if boards is not None:
                self.env.board.copy_(dev(boards))
                self.oracle.board[:] = boards
        kw = dict(device=DEV)
        self.actions = torch.full((n,), 9, dtype=torch.uint8, **kw)
        self.delta = torch.full((n,), 77, dtype=torch.int32, **kw)
        self.err = torch.full((n,), 77, dtype=torch.int64, **kw)
        self.errs, self.deltas, self.depths, self.ring = [], [], [], None

    def step(self, t):
        if self.feed is None:
            boards = self.oracle.board.copy()
            assert np.array_equal(self.env.board.cpu().numpy(), boards), t
            gpu_boards = self.env.board
        else:
            boards = self.feed(t)
            gpu_boards = dev(boards)
        self.depths.append(list(self.ref.depth))
        # the afterstates each board has going into this step, latest first
        self.ring = [[self.ref.back(i, k) for k in range(self.ref.depth[i])]
                     for i in range(self.n)]
        if not self.dense:
            prefetch(self.ref.net, list(boards) + [b for r in self.ring for b in r])
        self.lam.step(gpu_boards, *self.lr, self.actions, self.delta, self.err)
        acts, errs, deltas = self.ref.step(boards, *self.lr)
        if self.feed is None:
            self.env.step(self.actions)
            self.oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
        self.compare(t, acts, errs, deltas)
        self.errs += errs
        self.deltas += deltas

    def compare(self, t, acts, errs, deltas):
        assert self.actions.cpu().tolist() == acts, t
        assert self.err.cpu().tolist() == errs, t
        assert self.delta.cpu().tolist() == deltas, t
        assert self.lam.head.cpu().tolist() == self.ref.head, t
        assert self.lam.depth.cpu().tolist() == self.ref.depth, t
        assert self.lam.hist.cpu().tolist() == self.ref.hist, t
        if self.dense:  # the whole table
            assert np.array_equal(self.net.lut.cpu().numpy(),
                                  want_dense(self.base, self.ref.net.touched)), t


def check_spread(run):
    """The run saw errors of both signs and moved the table."""
    errs = np.array(run.errs)
    assert (errs > 0).any() and (errs < 0).any()
    assert run.ref.net.touched


# ------------------------------------------------------------------ 1. boundaries
@pytest.mark.parametrize("n", [1, 7, 9, 129])
def test_lambda_step_at_size_boundaries(M, n):
    """1, 7, 9 and 129 boards: inside a lane group's wave, one short of a wave's 8 boards, one
    past it, one past the update's 128-board block.  Random boards of mixed fill, H = 3, s = 1,
    H + 3 steps with env.step between: the ring wraps, and from step H on the plane the commit
    overwrites is the one the same call read as k = H - 1."""
    H = 3
    net = random_table(M, M.NT.TUPLES_2x4, 70 + n)
    boards = random_boards(np.random.default_rng(90 + n), n)
    run = Run(M, net, n, H, 1, 3, 6, seed=47, boards=boards)
    for t in range(H + 3):
        run.step(t)
    assert max(run.ref.depth) == H and any(d != 0 for d in run.deltas)
    assert run.ref.net.touched
    if n > 1:
        assert len(set(run.ref.head)) > 1 or min(run.ref.depth) == H
    run.env.check_errors()


# ------------------------------------------------------------------ 2. every T, H, shift
@pytest.mark.parametrize("T", range(1, 9))
def test_lambda_step_at_every_tuple_count(M, T):
    """Every instantiation of the two kernels (T = 1..8, the first T tuples of T8M4, m = 4) at
    H = 3, s = 1: 131 boards (two update blocks, an odd count, a dead half-wave in the policy
    kernel), 5 steps from reset boards."""
    net = random_table(M, T8M4[:T], 50 + T)
    run = Run(M, net, 131, 3, 1, 3, 6, seed=46)
    run.step(0)
    assert not run.ref.net.touched and run.ref.depth == [1] * 131
    for t in range(1, 5):
        run.step(t)
    assert {k[0] for k in run.ref.net.touched} == set(range(T))
    check_spread(run)
    run.env.check_errors()


@pytest.mark.parametrize("H", range(1, 9))
def test_lambda_step_at_every_horizon(M, H):
    """H = 1..8 at T = 2, s = 1: 67 boards of mixed fill, H + 3 steps."""
    net = random_table(M, M.NT.TUPLES_2x4, 60 + H)
    boards = random_boards(np.random.default_rng(160 + H), 67)
    run = Run(M, net, 67, H, 1, 3, 6, seed=48, boards=boards)
    for t in range(H + 3):
        run.step(t)
    assert max(run.ref.depth) == H
    check_spread(run)
    run.env.check_errors()


@pytest.mark.parametrize("s,lr_shift", [(2, 18), (4, 13)])
def test_lambda_step_at_other_shifts(M, s, lr_shift):
    """s = 2 and s = 4 at H = 3, T = 2, 67 boards, 6 steps.  The errors on a random table are
    around 2^22, so the rate is chosen to put the deltas around 2^(2 s): some are shifted to 0
    two steps back (the walk ends early) and some are not."""
    net = random_table(M, M.NT.TUPLES_2x4, 80 + s)
    boards = random_boards(np.random.default_rng(180 + s), 67)
    run = Run(M, net, 67, 3, s, 1, lr_shift, seed=49, boards=boards)
    for t in range(6):
        run.step(t)
    mags = [abs(d) for d in run.deltas if d]
    assert any(m >> (2 * s) == 0 for m in mags) and any(m >> (2 * s) for m in mags)
    check_spread(run)
    run.env.check_errors()


# ------------------------------------------------------------------ 3. H = 1 is TD(0)
def test_horizon_one_is_the_td0_step(M):
    """1 031 boards (an odd size across blocks), three steps on three batches of boards, some
    terminal: the outputs and the table equal NTupleNetwork.td_step's bitwise, plane 0 equals
    prev and depth equals has_prev; head stays 0.  lam_shift has no effect at H = 1."""
    n = 1031
    rng = np.random.default_rng(40)
    batches = [dev(np.concatenate([random_boards(rng, n - 40),
                                   np.array(mask_boards(), np.uint8)[:40]])[rng.permutation(n)])
               for _ in range(3)]

    def outputs():
        return (torch.zeros(n, dtype=torch.uint8, device=DEV),
                torch.zeros(n, dtype=torch.int32, device=DEV),
                torch.zeros(n, dtype=torch.int64, device=DEV))

    td_net, lam_net = random_table(M, M.NT.TUPLES_2x4, 46), random_table(M, M.NT.TUPLES_2x4, 46)
    td_prev = torch.zeros((n, 16), dtype=torch.uint8, device=DEV)
    td_has = torch.zeros(n, dtype=torch.uint8, device=DEV)
    lam = M.L.TDLambdaState(lam_net, n, horizon=1, lam_shift=7)
    td_out, lam_out = outputs(), outputs()
    for boards in batches:
        td_net.td_step(boards, td_prev, td_has, 3, 6, *td_out)
        lam.step(boards, 3, 6, *lam_out)
        assert torch.equal(lam_net.lut, td_net.lut)
        for a, b in zip(lam_out + (lam.hist[0], lam.depth), td_out + (td_prev, td_has)):
            assert torch.equal(a, b)
        assert not bool(lam.head.any())
    assert not torch.equal(lam_net.lut, random_table(M, M.NT.TUPLES_2x4, 46).lut)
    assert 0 < int(td_has.sum()) < n and bool((td_out[1] != 0).any())


# ------------------------------------------------------------------ 4. collisions and overflow
def test_lambda_step_under_heavy_collisions(M):
    """129 copies of one board per step (another board each step): every board of a block adds
    into the same 8 T entries per afterstate, so one LDS slot per entry takes up to 128 x 8
    adds, and the 129th board adds from a second block."""
    rng = np.random.default_rng(41)
    net = random_table(M, M.NT.TUPLES_2x4, 31)
    seq = random_boards(rng, 7, fills=(0.5, 0.8))
    run = Run(M, net, 129, 4, 1, 3, 9, feed=lambda t: np.repeat(seq[t:t + 1], 129, axis=0))
    for t in range(7):
        run.step(t)
    assert run.ref.depth == [4] * 129 and len(run.ref.net.touched) <= 7 * 16
    check_spread(run)


def test_lambda_step_with_more_keys_than_the_merge_table_has_slots(M):
    """129 distinct boards of uniformly random exponents, T = 8, H = 4: once the ring is full a
    block adds into more than 16 384 different entries (asserted on the reference), more than
    its LDS table has slots, so adds that find no slot and go straight to memory occur beside
    merged ones."""
    rng = np.random.default_rng(37)
    net = random_table(M, T8M4, 36)
    n = 129
    seq = [rng.integers(0, 12, (n, 16)).astype(np.uint8) for _ in range(6)]
    run = Run(M, net, n, 4, 1, 7, 5, feed=lambda t: seq[t])
    for t in range(6):
        run.step(t)
    # most rings are full (a few random boards had no legal move and started over)
    assert sum(d == 4 for d in run.depths[5][:128]) >= 100
    # the entries block 0 (boards 0..127) added into at the last step
    keys = {key for i in range(128) for k, after in enumerate(run.ring[i])
            if R.shifted(run.deltas[-n:][i], k, 1) != 0 for key in run.ref.net.indices(after)}
    assert len(keys) > 16384
    check_spread(run)


# ------------------------------------------------------------------ 5. episode ends
def near_terminal_boards(rng, n):
    """Full boards whose neighbours differ in parity (odd exponents 3..9 on one colour of the
    checkerboard, even ones 4..10 on the other, so nothing merges, a spawned tile included),
    with one or two holes."""
    colour = (np.arange(16) // 4 + np.arange(16) % 4) % 2
    b = np.where(colour == 0, 2 * rng.integers(1, 5, (n, 16)) + 1, 2 * rng.integers(2, 6, (n, 16)))
    for row in b:
        row[rng.choice(16, int(rng.integers(1, 3)), replace=False)] = 0
    return b.astype(np.uint8)


def test_lambda_step_through_episode_ends(M):
    """Near-terminal boards stepped through their ends with env.step between: a terminal board
    drops its depth to 0 and keeps its head, the fresh board ramps up again, and boards of
    different depth sit in one wave of the update (8 consecutive boards)."""
    net = random_table(M, M.NT.TUPLES_2x4, 32)
    boards = near_terminal_boards(np.random.default_rng(33), 64)
    run = Run(M, net, 64, 3, 1, 1, 8, seed=42, boards=boards)
    saw_terminal = 0
    for t in range(16):
        saw_terminal += sum(O.legal_mask(b) == 0 for b in run.oracle.board)
        run.step(t)
    ended = run.env.ep[:, 0].cpu().numpy()
    assert np.array_equal(ended, run.oracle.ep[:, 0].astype(ended.dtype))
    assert saw_terminal >= 8 and (ended > 0).sum() >= 8
    # steps at which one wave held boards of three different depths, all of them adding
    mixed = sum(len(set(d[w:w + 8])) == 3 for d in run.depths[3:] for w in range(0, 64, 8))
    assert mixed >= 4
    assert len(set(run.ref.head)) >= 2
    check_spread(run)
    run.env.check_errors()


# ------------------------------------------------------------------ 6. the 4x6 set
def test_lambda_step_4x6_touched_entries_and_sum(M):
    """The 256 MiB table: 64 boards, 12 steps at H = 3, s = 1.  The entries the reference
    touched (a sparse dict) and the int64 sum of the whole table are exact."""
    net = random_table(M, M.NT.TUPLES_4x6, 14)
    sum0 = int(net.lut.sum(dtype=torch.int64))
    run = Run(M, net, 64, 3, 1, 5, 9, seed=43, dense=False)
    for t in range(12):
        run.step(t)
    touched = run.ref.net.touched
    assert len(touched) > 1000
    keys = sorted(touched)
    ti = torch.tensor([k[0] for k in keys], device=DEV)
    ii = torch.tensor([k[1] for k in keys], device=DEV)
    assert net.lut[ti, ii].cpu().tolist() == [touched[k] for k in keys]
    moved = sum(v - run.ref.net.base(*k) for k, v in touched.items())
    assert moved != 0 and int(net.lut.sum(dtype=torch.int64)) == sum0 + moved
    check_spread(run)
    run.env.check_errors()


# ------------------------------------------------------------------ 7. order-free
def test_two_identical_runs_give_equal_tables_and_state(M):
    def run():
        net = random_table(M, M.NT.TUPLES_2x4, 34)
        tr = M.L.TDLambdaTrainer(net, 1024, horizon=3, lam_shift=1, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        return net.lut, tr.lam.hist, tr.lam.head, tr.lam.depth, tr.env.board

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], random_table(M, M.NT.TUPLES_2x4, 34).lut)
    assert bool(a[1].any()) and int(a[3].max()) == 3 and len(a[2].unique()) >= 2


# ------------------------------------------------------------------ 8. graph capture
def test_captured_lambda_step_and_env_step_replays(M):
    """lambda step + env.step captured once and replayed 4 times equals 4 eager steps: table,
    ring, boards and outputs."""
    from g2048.dist import graph_capture

    def make():
        net = random_table(M, M.NT.TUPLES_2x4, 35)
        tr = M.L.TDLambdaTrainer(net, 192, horizon=3, lam_shift=1, seed=45, lr_num=1, lr_shift=7)
        tr.step(2)  # a state with afterstates on every board, the ring not yet full
        torch.cuda.synchronize()
        return net, tr

    def state(net, tr):
        names = ("actions", "delta", "err", "reward", "done", "legal")
        return ({k: getattr(tr, k).cpu().clone() for k in names} |
                {"lut": net.lut.cpu().clone(), "hist": tr.lam.hist.cpu().clone(),
                 "head": tr.lam.head.cpu().clone(), "depth": tr.lam.depth.cpu().clone(),
                 "board": tr.env.board.cpu().clone()})

    net, tr = make()
    want = []
    for _k in range(4):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(state(net, tr))

    net, tr = make()
    g = torch.cuda.CUDAGraph()
    lut0 = net.lut.clone()
    st0 = {k: getattr(tr.lam, k).clone() for k in ("hist", "head", "depth")}
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    # the capture ran nothing
    assert torch.equal(net.lut, lut0)
    assert all(torch.equal(getattr(tr.lam, k), v) for k, v in st0.items())
    for k in range(4):
        g.replay()
        torch.cuda.synchronize()
        got = state(net, tr)
        for name, t in want[k].items():
            assert torch.equal(got[name], t), (k, name)
    tr.env.check_errors()


def test_reset_forgets_the_ring(M):
    net = random_table(M, M.NT.TUPLES_2x4, 39)
    tr = M.L.TDLambdaTrainer(net, 64, horizon=2, lam_shift=1, seed=50)
    tr.step(3)
    assert bool(tr.lam.depth.any()) and bool(tr.lam.hist.any())
    tr.lam.reset()
    lut = net.lut.clone()
    tr.step(1)  # no board has a previous afterstate: nothing is added
    torch.cuda.synchronize()
    assert torch.equal(net.lut, lut) and not bool(tr.delta.any())
    assert tr.lam.depth.cpu().tolist() == [1] * 64 and tr.lam.head.cpu().tolist() == [1] * 64


# ------------------------------------------------------------------ 9. it learns
def test_self_play_learns_under_td_lambda(M):
    """The recipe of test_ntuple_gpu.py::test_self_play_learns with the lambda step at H = 3,
    s = 1: TUPLES_2x4, 256 boards, the default rate 1 / 2^10, seed 61, 4000 steps.  The mean merge
    score of the last 200 finished episodes is at least twice the random player's mean on the
    same seed (the bar of that test), and no table entry exceeds 2^28 in magnitude.  Measured on
    an MI355X: see the printed figures and DESIGN 4.13."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    tr = M.L.TDLambdaTrainer(net, 256, horizon=3, lam_shift=1, seed=seed, p4=0.5, log_slots=64)
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
    print(f"TD(lambda) H=3 s=1 n-tuple 2x4 after 4000 steps: {learned:.0f} over the last 200 of "
          f"{len(scores)} episodes, largest |entry| {largest}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert largest <= 1 << 28
