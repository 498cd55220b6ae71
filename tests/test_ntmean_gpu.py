"""Batch-mean TD learning on the GPU (csrc/g2048_ntmean.hip -> libg2048_ntmean.so) against the
plain Python restatement tests/ntmean_ref.py: lut, prev, has_prev, action, err and delta bit for
bit and acc all zero after every call -- on played, identical, symmetric and mixed batches of every
size class, on four specs -- the rule's properties against TD(0) and under repetition, two identical
runs, a trainer run next to the reference, a captured step, and that self-play learns."""
import numpy as np
import pytest
import torch

import ntmean_ref as R
import ntuple_ref as NR
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M2 = tuple((t, (t + 5) % 16) for t in range(8))
SPECS = {"corner": ((0,),), "2x4": NR.TUPLES_2x4, "4x6": NR.TUPLES_4x6, "T8m2": T8M2}
# one board; a partial wave of the policy frame; 63 / 64 / 65 around a wave of the update frame
# (8 boards per wave, 64 boards = 8 waves); 129 = a partial second workgroup of that frame (128
# boards); 1 031 = nine workgroups, so an entry is claimed across workgroups
SIZES = (1, 2, 63, 64, 65, 129, 1031)
LR = (3, 6)  # deltas of about 2^20 on a table of +-2^20: nothing leaves int32


class Modules:
    def __init__(self, ntuple, ntmean):
        self.NT, self.MEAN = ntuple, ntmean


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmean, ntuple
    ntuple.load()
    ntmean.load()
    return Modules(ntuple, ntmean)


class Table:
    """One network per spec for the whole module (the 4x6 set is 256 MiB with 1 GiB of acc): a
    random non-zero table `lut0` that every case starts from, and the workspace, which every case
    must leave all zero."""

    def __init__(self, M, tuples, seed):
        self.net = M.NT.NTupleNetwork(tuples, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.lut0 = torch.randint(-(1 << 20), 1 << 20, self.net.lut.shape, generator=g,
                                  device=DEV, dtype=torch.int32)
        self.mean = M.MEAN.MeanState(self.net)
        self.cache = {}

    def fresh(self):
        self.net.lut.copy_(self.lut0)
        assert not bool(self.mean.acc.any())
        return self.net

    # the reference's view of lut0: entries gathered from the device by index, in batches
    def prefetch(self, keys):
        miss = sorted(set(keys) - self.cache.keys())
        if miss:
            t = torch.tensor([k[0] for k in miss], device=DEV)
            i = torch.tensor([k[1] for k in miss], device=DEV)
            self.cache.update(zip(miss, self.lut0[t, i].cpu().tolist()))

    def __call__(self, t, i):
        if (t, i) not in self.cache:
            self.prefetch([(t, i)])
        return self.cache[(t, i)]

    def expected(self, touched):
        """lut0 with the reference's moved entries, on the device."""
        want = self.lut0.clone()
        if touched:
            keys = sorted(touched)
            t = torch.tensor([k[0] for k in keys], device=DEV)
            i = torch.tensor([k[1] for k in keys], device=DEV)
            want[t, i] = torch.tensor([touched[k] for k in keys], dtype=torch.int32, device=DEV)
        return want


_tables = {}


@pytest.fixture
def table(M, request):
    name = request.param
    if name not in _tables:
        _tables[name] = Table(M, SPECS[name], 100 + list(SPECS).index(name))
    return _tables[name]


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def outputs(n):
    return (torch.full((n,), 9, dtype=torch.uint8, device=DEV),
            torch.full((n,), 77, dtype=torch.int32, device=DEV),
            torch.full((n,), 77, dtype=torch.int64, device=DEV))


def check_step(tb, boards, prev0, has0, lr=LR):
    """One mean_step on the table's fresh copy against the reference: everything bit for bit,
    acc all zero.  Returns (reference hits, deltas)."""
    net = tb.fresh()
    n = len(boards)
    ref = NR.Net(net.spec.tuples, base=tb)
    keys = []
    for b in list(boards) + list(prev0):
        b = [int(x) for x in b]
        keys += ref.indices(b)
        for a in range(4):
            keys += ref.indices(NR.E.move(b, a)[0])
    tb.prefetch(keys)
    ref_prev, ref_has = [[int(x) for x in p] for p in prev0], [int(h) for h in has0]
    acts, errs, deltas = R.step(ref, [list(map(int, b)) for b in boards], ref_prev, ref_has, *lr)
    hits = dict(R.last_hits)
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    tb.mean.mean_step(dev(boards), prev, has_prev, *lr, *out)
    assert out[0].cpu().tolist() == acts
    assert out[2].cpu().tolist() == errs
    assert out[1].cpu().tolist() == deltas
    assert prev.cpu().tolist() == ref_prev and has_prev.cpu().tolist() == ref_has
    assert torch.equal(net.lut, tb.expected(ref.touched))
    assert not bool(tb.mean.acc.any())
    return hits, deltas


# ------------------------------------------------------------------ the four kinds of batch
def played(M, net, n, seed, steps=12):
    """(boards, prev): n boards played `steps` random moves from reset, then one greedy move of
    `net`: prev = that move's afterstate, boards = what the env made of it."""
    import g2048

    env = g2048.VecEnv2048(n, seed=seed, device=DEV)
    for _ in range(steps):
        env.step(None)
    acts, _q, after = net.act(env.board, q=False, after=True)
    env.step(acts)
    torch.cuda.synchronize()
    return env.board.cpu().numpy().copy(), after.cpu().numpy().copy()


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def terminal_boards(rng, n):
    """Full boards whose neighbours differ in parity: nothing merges, no move is legal."""
    colour = (np.arange(16) // 4 + np.arange(16) % 4) % 2
    b = np.where(colour == 0, 2 * rng.integers(1, 5, (n, 16)) + 1, 2 * rng.integers(2, 6, (n, 16)))
    return b.astype(np.uint8)


def symmetric(rng, n):
    """Boards that a symmetry maps to themselves, so pairs (g, t) coincide: a third each under
    the column flip, under the transpose, and under both flips and the transpose."""
    b = random_boards(rng, n, fills=(0.5, 1.0)).reshape(n, 4, 4)
    kind = np.arange(n) % 3
    flip = b.copy()
    flip[:, :, 2:] = flip[:, :, 1::-1]
    tr = np.triu(b) + np.transpose(np.triu(b, 1), (0, 2, 1))
    both = tr.copy()
    both[:, :, :] = tr[:, 0:1, 0:1]  # one value everywhere: all 8 symmetries coincide
    out = np.where((kind == 0)[:, None, None], flip, np.where((kind == 1)[:, None, None], tr, both))
    return out.reshape(n, 16).astype(np.uint8)


CASES = [(s, n) for s in SPECS for n in SIZES]


@pytest.mark.parametrize("table,n", CASES, indirect=["table"])
def test_mean_step_on_played_boards(M, table, n):
    """Boards of a random rollout over a random table: shared early-game entries, D of both
    signs over the module's sizes taken together."""
    boards, prev0 = played(M, table.fresh(), n, seed=200 + n)
    hits, deltas = check_step(table, boards, prev0, np.ones(n, np.uint8))
    assert any(deltas)
    if n >= 63:
        assert any(d > 0 for d in deltas) and any(d < 0 for d in deltas)
        assert any(c > 8 for _d, c in hits.values())  # an entry more than one board hits
        assert any(d % c for d, c in hits.values())   # a quotient that floors


@pytest.mark.parametrize("table,n", CASES, indirect=["table"])
def test_mean_step_on_identical_boards(M, table, n):
    """One board n times: every entry is hit by all n boards, C = 8 n on the hottest, and the
    table moves as for the one board."""
    boards, prev0 = played(M, table.fresh(), 1, seed=300)
    hits, deltas = check_step(table, np.repeat(boards, n, 0), np.repeat(prev0, n, 0),
                              np.ones(n, np.uint8))
    assert deltas[0] != 0 and deltas == [deltas[0]] * n
    assert all(c % n == 0 and d == c * deltas[0] for d, c in hits.values())


@pytest.mark.parametrize("table,n", CASES, indirect=["table"])
def test_mean_step_on_symmetric_boards(M, table, n):
    """Previous afterstates that a flip or the transpose maps to themselves: the coinciding
    pairs of one board are each a hit."""
    rng = np.random.default_rng(400 + n)
    prev0 = symmetric(rng, n)
    hits, deltas = check_step(table, random_boards(rng, n), prev0, np.ones(n, np.uint8))
    T = len(table.net.spec.tuples)
    if any(deltas):
        assert len(hits) < 8 * T * sum(d != 0 for d in deltas)


@pytest.mark.parametrize("table,n", CASES, indirect=["table"])
def test_mean_step_on_a_mix_with_terminal_boards_and_rows_without_prev(M, table, n):
    """Played, random and terminal boards, a quarter of the rows without a previous afterstate,
    previous afterstates with exponents past the clamp to 15;
    then the same batch at lr_num = 0, which changes nothing but prev, has_prev and the outputs."""
    rng = np.random.default_rng(500 + n)
    a, pa = played(M, table.fresh(), n, seed=500 + n)
    kind = (np.arange(n) + 1) % 3
    boards = np.where((kind == 0)[:, None], terminal_boards(rng, n),
                      np.where((kind == 1)[:, None], a, random_boards(rng, n)))
    prev0 = np.where((kind == 1)[:, None], pa, random_boards(rng, n, hi=18))
    has0 = (np.arange(n) % 4 != 1).astype(np.uint8) if n > 2 else np.array([1, 0][:n], np.uint8)
    check_step(table, boards, prev0, has0)
    hits, deltas = check_step(table, boards, prev0, has0, lr=(0, 6))
    assert not hits and not any(deltas)
    assert torch.equal(table.net.lut, table.lut0)


# ------------------------------------------------------------------ properties
def distinct_batch(tuples, n, seed):
    """n previous afterstates whose 8 T n hits are pairwise distinct (checked on the reference's
    indices; boards that would repeat a key are dropped)."""
    rng = np.random.default_rng(seed)
    ref, seen, keep = NR.Net(tuples), set(), []
    while len(keep) < n:
        p = rng.integers(1, 12, 16).astype(np.uint8)
        keys = ref.indices([int(x) for x in p])
        if len(set(keys)) == len(keys) and seen.isdisjoint(keys):
            seen.update(keys)
            keep.append(p)
    return np.stack(keep)


@pytest.mark.parametrize("table", ["2x4", "4x6"], indirect=True)
def test_a_batch_of_pairwise_distinct_hits_is_the_td0_step(M, table):
    n = 129
    rng = np.random.default_rng(600)
    boards, prev0 = dev(random_boards(rng, n)), distinct_batch(table.net.spec.tuples, n, 601)
    has0 = np.ones(n, np.uint8)
    net = table.fresh()
    td_prev, td_has, td_out = dev(prev0), dev(has0), outputs(n)
    net.td_step(boards, td_prev, td_has, *LR, *td_out)
    td_lut = net.lut.clone()
    assert not torch.equal(td_lut, table.lut0)
    net = table.fresh()
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    table.mean.mean_step(boards, prev, has_prev, *LR, *out)
    assert torch.equal(net.lut, td_lut)
    for a, b in zip(out + (prev, has_prev), td_out + (td_prev, td_has)):
        assert torch.equal(a, b)
    assert not bool(table.mean.acc.any())


@pytest.mark.parametrize("table", ["corner", "2x4", "4x6", "T8m2"], indirect=True)
def test_a_batch_repeated_three_times_leaves_the_same_table(M, table):
    n = 129
    boards, prev0 = played(M, table.fresh(), n, seed=700)
    has0 = (np.arange(n) % 5 != 0).astype(np.uint8)
    luts = []
    for k in (1, 3):
        net = table.fresh()
        b, prev, has_prev = dev(np.tile(boards, (k, 1))), dev(np.tile(prev0, (k, 1))), \
            dev(np.tile(has0, k))
        out = outputs(k * n)
        table.mean.mean_step(b, prev, has_prev, *LR, *out)
        luts.append(net.lut.clone())
        assert not bool(table.mean.acc.any())
    assert torch.equal(luts[0], luts[1]) and not torch.equal(luts[0], table.lut0)
    # the sum rule does not have the property
    net = table.fresh()
    net.td_step(dev(np.tile(boards, (3, 1))), dev(np.tile(prev0, (3, 1))), dev(np.tile(has0, 3)),
                *LR, *outputs(3 * n))
    assert not torch.equal(net.lut, luts[0])


def random_net(M, tuples, seed):
    net = M.NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = random_net(M, M.NT.TUPLES_2x4, 34)
        tr = M.MEAN.MeanTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.mean.acc.any())
        return net.lut, tr.env.board, tr.prev, tr.delta

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], random_net(M, M.NT.TUPLES_2x4, 34).lut)


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """MeanTrainer at 256 boards on the 2x4 set, at its default rate, next to the reference
    driving an OracleEnv: actions, err, delta, prev, has_prev and the whole table after each of 50
    steps, acc all zero."""
    n, seed = 256, 47
    net = random_net(M, M.NT.TUPLES_2x4, 48)
    base = net.lut.cpu().numpy().copy()
    tr = M.MEAN.MeanTrainer(net, n, seed=seed)
    assert (tr.lr_num, tr.lr_shift) == (1, 6)
    ref = NR.Net(M.NT.TUPLES_2x4, base=base)
    oracle = O.OracleEnv(n, seed)
    ref_prev, ref_has = [[0] * 16 for _ in range(n)], [0] * n
    moved = 0
    for t in range(50):
        boards = oracle.board.copy()
        assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
        tr.step(1)
        acts, errs, deltas = R.step(ref, boards, ref_prev, ref_has, 1, 6)
        oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
        assert tr.actions.cpu().tolist() == acts, t
        assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == deltas, t
        assert tr.prev.cpu().tolist() == ref_prev and tr.has_prev.cpu().tolist() == ref_has, t
        want = base.copy()
        for (k, i), v in ref.touched.items():
            want[k, i] = v
        assert np.array_equal(net.lut.cpu().numpy(), want), t
        assert not bool(tr.mean.acc.any()), t
        moved += any(d % c for d, c in R.last_hits.values())
    assert moved >= 40 and len(ref.touched) > 100
    tr.env.check_errors()


def test_captured_mean_step_and_env_step_replays(M):
    """mean_step + env.step captured once and replayed 3 times equals 3 eager steps: table,
    boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    def make():
        net = random_net(M, M.NT.TUPLES_2x4, 35)
        tr = M.MEAN.MeanTrainer(net, 192, seed=45)
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

    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    pool = g2048.RestartPool(64, (3, 0, 4), device=DEV, stagger=True)
    tr = M.MEAN.MeanTrainer(net, 64, seed=49, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and bool(net.lut.any()) and not bool(tr.mean.acc.any())
    with pytest.raises(ValueError):
        M.MEAN.MeanTrainer(net, 32, restart=pool)
    tr.env.check_errors()


# ------------------------------------------------------------------ it learns
def last200(tr, steps, chunk):
    scores = []
    for _ in range(steps // chunk):
        tr.step(chunk)
        scores += tr.episodes()["score"].tolist()
    tr.env.check_errors()
    return scores


def test_self_play_learns_under_batch_mean(M):
    """The recipe of test_ntuple_gpu.py::test_self_play_learns with the batch-mean step:
    TUPLES_2x4, 256 boards, the default rate 2^-6, seed 61, 4000 steps.  The mean merge score of
    the last 200 finished episodes is at least twice the random player's mean on the same seed
    (the bar of that test), and no table entry exceeds 2^28 in magnitude.  The numpy prototype
    measured 4 450 and 3.2e5; for the MI355X see the printed figures and DESIGN 4.17."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    tr = M.MEAN.MeanTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MEAN.default_mean_lr_shift(net.spec) == 6
    scores = last200(tr, 4000, 1000)
    rnd = BatchedPlayer(256, device=DEV, seed=seed).play("random")
    learned, random_mean = float(np.mean(scores[-200:])), float(rnd.merge_score.mean())
    largest = int(net.lut.to(torch.int64).abs().max())
    print(f"batch-mean n-tuple 2x4 after 4000 steps: {learned:.0f} over the last 200 of "
          f"{len(scores)} episodes, largest |entry| {largest}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert largest <= 1 << 28


def test_batch_mean_beats_td0_on_a_wide_batch(M):
    """TUPLES_2x4, 4 096 boards, 1 200 steps, seeds 61-63: MeanTrainer at its default (2^-6)
    against NTupleTrainer at its default (2^-14) on the same seeds.  The mean over the seeds of
    the ratio of the last-200-episode means is at least 1.2: under the numpy prototype's 1.45 (one
    seed, another random stream) by more than the 15 % that seeds differ by on this table."""
    ratios = []
    for seed in (61, 62, 63):
        means = []
        for cls in (M.MEAN.MeanTrainer, M.NT.NTupleTrainer):
            net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
            tr = cls(net, 4096, seed=seed, p4=0.5, log_slots=16)
            scores = last200(tr, 1200, 400)
            assert len(scores) >= 200
            means.append(float(np.mean(scores[-200:])))
        assert tr.lr_shift == 14
        ratios.append(means[0] / means[1])
        print(f"seed {seed}: batch-mean {means[0]:.0f}, TD(0) {means[1]:.0f}, ratio "
              f"{ratios[-1]:.3f}")
    print(f"mean ratio {np.mean(ratios):.3f}")
    assert np.mean(ratios) >= 1.2
