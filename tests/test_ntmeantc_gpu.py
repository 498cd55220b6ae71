"""Temporal-coherence learning on the batch-mean rule on the GPU (csrc/g2048_ntmeantc.hip ->
libg2048_ntmeantc.so) against the plain Python restatement tests/ntmeantc_ref.py: lut, ea, prev,
has_prev, action, err and delta bit for bit and acc all zero after every call.  State carries across
calls, so every case makes three consecutive calls, once from a zero ea and once from a seeded one
that holds every branch of the rate -- on played, identical, symmetric and mixed batches of every
size class, on four specs -- then every tuple count, a block with more entries than the LDS tables
hold, the header's consequences next to the batch-mean and the TC library, two identical runs, a
trainer run next to the reference, a captured step, the restart pool, a resumed run, and that
self-play learns."""
import numpy as np
import pytest
import torch

import ntmeantc_ref as R
import nttc_ref as TR
import ntuple_ref as NR
from g2048 import ntmeantc as _library
from oracle import oracle as O

_library.load()  # without the library the file fails here, before any case
pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M2 = tuple((t, (t + 5) % 16) for t in range(8))
T8M4 = tuple((t, t + 1, t + 4, t + 5) for t in range(8))
SPECS = {"corner": ((0,),), "2x4": NR.TUPLES_2x4, "4x6": NR.TUPLES_4x6, "T8m2": T8M2}
# one board; a partial wave of the policy frame (2 boards per wave); 63 / 64 / 65 around a wave
# group of the gather / apply frame (8 boards per wave); 129 = a partial second workgroup of that
# frame (128 boards); 1 031 = nine workgroups, so an entry is claimed across workgroups
SIZES = (1, 2, 63, 64, 65, 129, 1031)
STARTS = ("zero", "seeded")
LR = (3, 6)  # deltas of about 2^20 on a table of +-2^20: nothing leaves int32
ONE = 1 << 16


class Modules:
    def __init__(self, ntuple, ntmean, nttc, ntmeantc):
        self.NT, self.MEAN, self.TC, self.MTC = ntuple, ntmean, nttc, ntmeantc


@pytest.fixture(scope="module")
def M():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntmean, ntmeantc, nttc, ntuple
    ntuple.load()
    ntmean.load()
    nttc.load()
    ntmeantc.load()
    return Modules(ntuple, ntmean, nttc, ntmeantc)


def seeded_ea(shape, gen):
    """int64 [*shape, 2] on the device: random (E, A) with |E| <= A.  A is 0, below 2^16, within 2
    of 2^16, or of 41 to 50 bits; E is 0, A, -A or uniform in [-A, A]: every branch of the rate."""
    def rnd(lo, hi):
        return torch.randint(lo, hi, shape, generator=gen, device=DEV, dtype=torch.int64)
    ak, ek = rnd(0, 4), rnd(0, 4)
    A = torch.where(ak == 1, rnd(1, 1 << 16), torch.zeros((), dtype=torch.int64, device=DEV))
    A = torch.where(ak == 2, (1 << 16) + rnd(-2, 3), A)
    A = torch.where(ak == 3, rnd(1 << 40, 1 << 50), A)
    E = torch.where(ek == 1, A, torch.zeros((), dtype=torch.int64, device=DEV))
    E = torch.where(ek == 2, -A, E)
    E = torch.where(ek == 3, rnd(0, 1 << 62) % (2 * A + 1) - A, E)
    assert bool((E.abs() <= A).all())
    return torch.stack((E, A), dim=-1).contiguous()


class Table:
    """One network per spec for the whole module (the 4x6 set is 256 MiB with 1 GiB of acc and
    1 GiB of ea): a random non-zero table `lut0` and a seeded `ea0` that the cases start from, their
    copies on the host for the reference, and the workspace, which every call must leave zero."""

    def __init__(self, M, tuples, seed):
        self.net = M.NT.NTupleNetwork(tuples, device=DEV)
        g = torch.Generator(device=DEV).manual_seed(seed)
        self.lut0 = torch.randint(-(1 << 20), 1 << 20, self.net.lut.shape, generator=g,
                                  device=DEV, dtype=torch.int32)
        self.ea0 = seeded_ea(self.net.lut.shape, g)
        self.state = M.MTC.MeanTCState(self.net)
        self.lut_host = self.lut0.cpu().numpy()
        self.ea_host = self.ea0.cpu().numpy()

    def fresh(self, start):
        self.net.lut.copy_(self.lut0)
        if start == "seeded":
            self.state.ea.copy_(self.ea0)
        else:
            self.state.ea.zero_()
        assert not bool(self.state.acc.any())
        return self.net

    def reference(self, start):
        host = self.ea_host
        base_ea = (lambda t, i: (int(host[t, i, 0]), int(host[t, i, 1]))) \
            if start == "seeded" else None
        return R.MeanTC(NR.Net(self.net.spec.tuples, base=self.lut_host), base_ea=base_ea)

    def expected(self, start, mt):
        """(lut, ea) of the start with the reference's moved entries, on the device."""
        lut = self.lut0.clone()
        ea = self.ea0.clone() if start == "seeded" else torch.zeros_like(self.ea0)
        if mt.net.touched:
            keys = sorted(mt.net.touched)
            t = torch.tensor([k[0] for k in keys], device=DEV)
            i = torch.tensor([k[1] for k in keys], device=DEV)
            lut[t, i] = torch.tensor([mt.net.touched[k] for k in keys], dtype=torch.int32,
                                     device=DEV)
        if mt.A:
            keys = sorted(mt.A)
            t = torch.tensor([k[0] for k in keys], device=DEV)
            i = torch.tensor([k[1] for k in keys], device=DEV)
            ea[t, i] = torch.tensor([(mt.E[k], mt.A[k]) for k in keys], dtype=torch.int64,
                                    device=DEV)
        return lut, ea


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


def lists(a):
    return [[int(x) for x in row] for row in a]


def check_calls(tb, start, calls, prev0, has0, lrs=None, reset_prev=False):
    """Consecutive meantc_steps, one per batch of `calls`, from the table's fresh copy against the
    reference: everything bit for bit and acc all zero after every call.  prev and has_prev carry
    from call to call (reset_prev: every call starts from prev0 / has0 again).  Returns the
    reference and, per call, (hits, m, deltas)."""
    net = tb.fresh(start)
    mt = tb.reference(start)
    n = len(prev0)
    lrs = lrs or [LR] * len(calls)
    ref_prev, ref_has = lists(prev0), [int(h) for h in has0]
    prev, has_prev = dev(prev0), dev(has0)
    seen = []
    for k, boards in enumerate(calls):
        if reset_prev and k:
            ref_prev, ref_has = lists(prev0), [int(h) for h in has0]
            prev.copy_(dev(prev0))
            has_prev.copy_(dev(has0))
        acts, errs, deltas = mt.step(lists(boards), ref_prev, ref_has, *lrs[k])
        out = outputs(n)
        tb.state.meantc_step(dev(boards), prev, has_prev, *lrs[k], *out)
        assert out[0].cpu().tolist() == acts, k
        assert out[2].cpu().tolist() == errs, k
        assert out[1].cpu().tolist() == deltas, k
        assert prev.cpu().tolist() == ref_prev and has_prev.cpu().tolist() == ref_has, k
        lut, ea = tb.expected(start, mt)
        assert torch.equal(net.lut, lut), k
        assert torch.equal(tb.state.ea, ea), k
        assert not bool(tb.state.acc.any()), k
        seen.append((dict(mt.last_hits), dict(mt.last_m), deltas))
    return mt, seen


def moved_twice(seen):
    """Entries that moved in more than one call: their second move read (E, A) back."""
    first = {k for k, m in seen[0][1].items() if m}
    return [k for _h, ms, _d in seen[1:] for k, m in ms.items() if m and k in first]


def rate_branches(tb, keys):
    """What the seeded (E, A) of these entries are, as a set of words."""
    words = set()
    for t, i in keys:
        e, a = int(tb.ea_host[t, i, 0]), int(tb.ea_host[t, i, 1])
        words.add("A=0" if a == 0 else "A<2^16" if a < (1 << 16) - 2 else
                  "A~2^16" if a <= (1 << 16) + 2 else "A>=2^40")
        if a:
            words.add("E=0" if e == 0 else "E=A" if e == a else "E=-A" if e == -a else "E<A")
            if TR.shift_of(a):
                words.add("s>0")
    return words


ALL_BRANCHES = {"A=0", "A<2^16", "A~2^16", "A>=2^40", "E=0", "E=A", "E=-A", "E<A", "s>0"}


# ------------------------------------------------------------------ the four kinds of batch
def played(M, net, n, seed, steps=12, more=2):
    """(calls, prev): n boards played `steps` random moves from reset, then one greedy move of
    `net`: prev = that move's afterstate, calls[0] = what the env made of it, and calls[1:] the
    same games `more` random moves on."""
    import g2048

    env = g2048.VecEnv2048(n, seed=seed, device=DEV)
    for _ in range(steps):
        env.step(None)
    acts, _q, after = net.act(env.board, q=False, after=True)
    env.step(acts)
    torch.cuda.synchronize()
    calls = [env.board.cpu().numpy().copy()]
    for _ in range(more):
        env.step(None)
        torch.cuda.synchronize()
        calls.append(env.board.cpu().numpy().copy())
    return calls, after.cpu().numpy().copy()


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


CASES = [(s, n, st) for s in SPECS for n in SIZES for st in STARTS]
PARAMS = pytest.mark.parametrize("table,n,start", CASES, indirect=["table"])


@PARAMS
def test_three_calls_on_played_boards(M, table, n, start):
    """Boards of a random rollout over a random table: shared early-game entries, D of both
    signs; entries move again in the later calls, at the rate the first call left them."""
    calls, prev0 = played(M, table.fresh(start), n, seed=200 + n)
    _mt, seen = check_calls(table, start, calls, prev0, np.ones(n, np.uint8))
    hits, ms, deltas = seen[0]
    assert any(deltas)
    if n >= 63:
        assert any(d > 0 for d in deltas) and any(d < 0 for d in deltas)
        assert any(c > 8 for _d, c in hits.values())  # an entry more than one board hits
        assert any(d % c for d, c in hits.values())   # a quotient that floors
        assert moved_twice(seen)
    if start == "seeded" and sum(1 for m in ms.values() if m) >= 400:
        assert rate_branches(table, [k for k, m in ms.items() if m]) == ALL_BRANCHES


@PARAMS
def test_three_calls_on_identical_boards(M, table, n, start):
    """One game n times: every entry is hit by all n boards, C = 8 n on the hottest, and the
    table and ea move as for the one board."""
    calls, prev0 = played(M, table.fresh(start), 1, seed=300)
    _mt, seen = check_calls(table, start, [np.repeat(b, n, 0) for b in calls],
                            np.repeat(prev0, n, 0), np.ones(n, np.uint8))
    for hits, ms, deltas in seen:
        assert deltas == [deltas[0]] * n
        assert all(c % n == 0 and d == c * deltas[0] for d, c in hits.values())
        assert all(m == deltas[0] for m in ms.values())
    assert seen[0][2][0] != 0


@PARAMS
def test_three_calls_on_symmetric_boards(M, table, n, start):
    """Previous afterstates that a flip or the transpose maps to themselves: the coinciding
    pairs of one board are each a hit."""
    rng = np.random.default_rng(400 + n)
    prev0 = symmetric(rng, n)
    calls = [random_boards(rng, n), symmetric(rng, n), symmetric(rng, n)]
    _mt, seen = check_calls(table, start, calls, prev0, np.ones(n, np.uint8))
    hits, _ms, deltas = seen[0]
    T = len(table.net.spec.tuples)
    if any(deltas):
        assert len(hits) < 8 * T * sum(d != 0 for d in deltas)


@PARAMS
def test_three_calls_on_a_mix_with_terminal_boards_and_rows_without_prev(M, table, n, start):
    """Played, random and terminal boards, a quarter of the rows without a previous afterstate,
    previous afterstates with exponents past the clamp to 15; the terminal boards of one call are
    rows without prev in the next.  Then a fourth call at lr_num = 0, which changes nothing but
    prev, has_prev and the outputs."""
    rng = np.random.default_rng(500 + n)
    games, pa = played(M, table.fresh(start), n, seed=500 + n)
    calls = []
    for k, a in enumerate(games):
        kind = (np.arange(n) + 1 + k) % 3
        calls.append(np.where((kind == 0)[:, None], terminal_boards(rng, n),
                              np.where((kind == 1)[:, None], a, random_boards(rng, n))))
    kind = (np.arange(n) + 1) % 3
    prev0 = np.where((kind == 1)[:, None], pa, random_boards(rng, n, hi=18))
    has0 = (np.arange(n) % 4 != 1).astype(np.uint8) if n > 2 else np.array([1, 0][:n], np.uint8)
    calls.append(random_boards(rng, n))
    _mt, seen = check_calls(table, start, calls, prev0, has0, lrs=[LR, LR, LR, (0, 6)])
    assert not seen[3][0] and not any(seen[3][2])  # no hit: lut and ea as the third call left them
    if n >= 3:
        assert any(seen[0][2]) and 0 in seen[1][2]


# ------------------------------------------------------------------ every T, and the direct path
def small_table(M, tuples, seed):
    key = ("small", tuples)
    if key not in _tables:
        _tables[key] = Table(M, tuples, seed)
    return _tables[key]


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(M, T):
    """DISPATCH_T instantiates T = 1..8: 129 boards, a mix with rows without prev, three calls
    from the seeded ea."""
    tb = small_table(M, T8M2[:T], 140 + T)
    n = 129
    calls, prev0 = played(M, tb.fresh("seeded"), n, seed=150 + T)
    has0 = (np.arange(n) % 5 != 2).astype(np.uint8)
    _mt, seen = check_calls(tb, "seeded", calls, prev0, has0)
    assert any(seen[0][2]) and moved_twice(seen)
    assert any(c > 8 for _d, c in seen[0][0].values())


def test_more_entries_than_either_lds_table_holds(M):
    """T = 8, m = 4, 128 random full boards: one block whose distinct entries exceed the gather's
    4096 slots and crowd the apply's 8192, so hits that find no slot after four probes go straight
    to memory beside merged ones, in both launches.  The second call hits the same entries again:
    the owners of the direct path read back the (E, A) they stored."""
    tb = small_table(M, T8M4, 370)
    rng = np.random.default_rng(371)
    n = 128
    prev0 = rng.integers(1, 12, (n, 16)).astype(np.uint8)
    calls = [rng.integers(0, 12, (n, 16)).astype(np.uint8) for _ in range(2)]
    for start in STARTS:
        _mt, seen = check_calls(tb, start, calls, prev0, np.ones(n, np.uint8), lrs=[(7, 5)] * 2,
                                reset_prev=True)
        for hits, ms, _deltas in seen:
            assert len(hits) > 4096 and any(c > 1 for _d, c in hits.values())
        assert len(moved_twice(seen)) > 4096


# ------------------------------------------------------------------ the header's consequences
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
def test_consequence_1_a_zero_ea_is_the_batch_mean_step(M, table):
    n = 1031
    calls, prev0 = played(M, table.fresh("zero"), n, seed=600, more=0)
    boards, has0 = dev(calls[0]), (np.arange(n) % 5 != 0).astype(np.uint8)
    mean = M.MEAN.MeanState(table.net)
    net = table.fresh("zero")
    mn_prev, mn_has, mn_out = dev(prev0), dev(has0), outputs(n)
    mean.mean_step(boards, mn_prev, mn_has, *LR, *mn_out)
    mean_lut = net.lut.clone()
    assert not torch.equal(mean_lut, table.lut0)
    del mean
    net = table.fresh("zero")
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    table.state.meantc_step(boards, prev, has_prev, *LR, *out)
    assert torch.equal(net.lut, mean_lut)
    for a, b in zip(out + (prev, has_prev), mn_out + (mn_prev, mn_has)):
        assert torch.equal(a, b)
    m = mean_lut.to(torch.int64) - table.lut0.to(torch.int64)  # nothing wrapped: |m| < 2^22
    assert torch.equal(table.state.ea, torch.stack((m, m.abs()), dim=-1))
    assert not bool(table.state.acc.any())


@pytest.mark.parametrize("table", ["2x4", "4x6"], indirect=True)
def test_consequence_2_pairwise_distinct_hits_are_the_tc_step(M, table):
    n = 129
    rng = np.random.default_rng(610)
    boards, prev0 = dev(random_boards(rng, n)), distinct_batch(table.net.spec.tuples, n, 611)
    has0 = np.ones(n, np.uint8)
    net = table.fresh("seeded")
    tc = M.TC.TCState(net)
    tc.ea.copy_(table.ea0)
    tc_prev, tc_has, tc_out = dev(prev0), dev(has0), outputs(n)
    tc.tc_step(boards, tc_prev, tc_has, *LR, *tc_out)
    tc_lut, tc_ea = net.lut.clone(), tc.ea
    assert not torch.equal(tc_lut, table.lut0) and not torch.equal(tc_ea, table.ea0)
    net = table.fresh("seeded")
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    table.state.meantc_step(boards, prev, has_prev, *LR, *out)
    assert torch.equal(net.lut, tc_lut) and torch.equal(table.state.ea, tc_ea)
    for a, b in zip(out + (prev, has_prev), tc_out + (tc_prev, tc_has)):
        assert torch.equal(a, b)
    assert not bool(table.state.acc.any())


@pytest.mark.parametrize("table", ["corner", "2x4", "4x6", "T8m2"], indirect=True)
def test_consequences_3_and_4_repetition_and_a_zero_rate(M, table):
    n = 129
    calls, prev0 = played(M, table.fresh("seeded"), n, seed=700, more=0)
    boards = calls[0]
    has0 = (np.arange(n) % 5 != 0).astype(np.uint8)
    got = []
    for k in (1, 3):
        net = table.fresh("seeded")
        b, prev, has_prev = dev(np.tile(boards, (k, 1))), dev(np.tile(prev0, (k, 1))), \
            dev(np.tile(has0, k))
        table.state.meantc_step(b, prev, has_prev, *LR, *outputs(k * n))
        got.append((net.lut.clone(), table.state.ea.clone()))
        assert not bool(table.state.acc.any())
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1])
    assert not torch.equal(got[0][0], table.lut0) and not torch.equal(got[0][1], table.ea0)
    del got
    # lr_num = 0: neither lut nor ea moves, prev and has_prev do
    net = table.fresh("seeded")
    prev, has_prev, out = dev(prev0), dev(has0), outputs(n)
    table.state.meantc_step(dev(boards), prev, has_prev, 0, 6, *out)
    assert torch.equal(net.lut, table.lut0) and torch.equal(table.state.ea, table.ea0)
    assert not bool(out[1].any()) and bool(out[2].any()) and bool(has_prev.all())
    assert not bool(table.state.acc.any())


def random_net(M, tuples, seed):
    net = M.NT.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


def test_consequence_5_e_stays_within_a_over_200_trainer_steps(M):
    net = random_net(M, M.NT.TUPLES_2x4, 33)
    tr = M.MTC.MeanTCTrainer(net, 1024, seed=43)
    tr.step(200)
    torch.cuda.synchronize()
    ea = tr.state.ea
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all()) and bool((ea[..., 1] >= 0).all())
    # errors of both signs met on some entries: a rate below 1 is in use
    assert bool((ea[..., 0].abs() < ea[..., 1]).any())
    # consequence 6: at most 2^31 per call
    assert int(ea[..., 1].max()) <= 200 << 31
    assert not bool(tr.state.acc.any())
    tr.env.check_errors()


# ------------------------------------------------------------------ the trainer
def test_two_runs_of_50_trainer_steps_give_equal_tables(M):
    def run():
        net = random_net(M, M.NT.TUPLES_2x4, 34)
        tr = M.MTC.MeanTCTrainer(net, 1024, seed=44)
        tr.step(50)
        torch.cuda.synchronize()
        assert not bool(tr.state.acc.any())
        return net.lut, tr.state.ea, tr.env.board, tr.prev, tr.delta

    a, b = run(), run()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], random_net(M, M.NT.TUPLES_2x4, 34).lut) and bool(a[1].any())


def test_50_trainer_steps_equal_the_reference_after_every_step(M):
    """MeanTCTrainer at 64 boards on the 2x4 set, at its default rate, next to the reference
    driving an OracleEnv: actions, err, delta, prev, has_prev, the whole table and the whole ea
    after each of 50 steps, acc all zero."""
    n, seed = 64, 47
    net = random_net(M, M.NT.TUPLES_2x4, 48)
    base = net.lut.cpu().numpy().copy()
    tr = M.MTC.MeanTCTrainer(net, n, seed=seed)
    assert (tr.lr_num, tr.lr_shift) == (1, 4)
    mt = R.MeanTC(NR.Net(M.NT.TUPLES_2x4, base=base))
    oracle = O.OracleEnv(n, seed)
    ref_prev, ref_has = [[0] * 16 for _ in range(n)], [0] * n
    slowed = 0
    for t in range(50):
        boards = oracle.board.copy()
        assert np.array_equal(tr.env.board.cpu().numpy(), boards), t
        tr.step(1)
        rates = [TR.rate(*mt.get_ea(*k)) for k in {key for i in range(n) if ref_has[i]
                                                   for key in mt.net.indices(ref_prev[i])}]
        acts, errs, deltas = mt.step(lists(boards), ref_prev, ref_has, 1, 4)
        oracle.step(O.MODE_ACTIONS, actions=np.array(acts, np.uint8))
        assert tr.actions.cpu().tolist() == acts, t
        assert tr.err.cpu().tolist() == errs and tr.delta.cpu().tolist() == deltas, t
        assert tr.prev.cpu().tolist() == ref_prev and tr.has_prev.cpu().tolist() == ref_has, t
        want = base.copy()
        for (k, i), v in mt.net.touched.items():
            want[k, i] = v
        assert np.array_equal(net.lut.cpu().numpy(), want), t
        want_ea = np.zeros((*base.shape, 2), np.int64)
        for (k, i), a in mt.A.items():
            want_ea[k, i] = (mt.E[(k, i)], a)
        assert np.array_equal(tr.state.ea.cpu().numpy(), want_ea), t
        assert not bool(tr.state.acc.any()), t
        slowed += any(0 < r < ONE for r in rates)
    assert slowed >= 30 and len(mt.net.touched) > 100
    tr.env.check_errors()


def test_captured_meantc_step_and_env_step_replays(M):
    """meantc_step + env.step captured once and replayed 3 times equals 3 eager steps: table, ea,
    boards and outputs, acc all zero."""
    from g2048.dist import graph_capture

    def make():
        net = random_net(M, M.NT.TUPLES_2x4, 35)
        tr = M.MTC.MeanTCTrainer(net, 192, seed=45)
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

    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    pool = g2048.RestartPool(64, (3, 0, 4), device=DEV, stagger=True)
    tr = M.MTC.MeanTCTrainer(net, 64, seed=49, restart=pool)
    tr.step(300)
    torch.cuda.synchronize()
    assert sum(pool.counts()) > 0 and bool(net.lut.any()) and bool(tr.state.ea.any())
    assert not bool(tr.state.acc.any())
    with pytest.raises(ValueError):
        M.MTC.MeanTCTrainer(net, 32, restart=pool)
    with pytest.raises(ValueError):  # another network's state
        M.MTC.MeanTCTrainer(M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV), 64, state=tr.state)
    tr.env.check_errors()


def test_a_run_resumes_bit_for_bit_from_a_saved_ea(M, tmp_path):
    """30 steps, save ea, 20 more; a second run of 30 steps takes the file's ea in a new state
    and ends where the first did.  With a zeroed ea it does not."""
    def start():
        net = random_net(M, M.NT.TUPLES_2x4, 36)
        tr = M.MTC.MeanTCTrainer(net, 256, seed=46)
        tr.step(30)
        torch.cuda.synchronize()
        return net, tr

    net, tr = start()
    tr.state.save(tmp_path / "ea.pt")
    tr.step(20)
    torch.cuda.synchronize()
    want = (net.lut.clone(), tr.state.ea.clone(), tr.env.board.clone())

    net, tr = start()
    loaded = M.MTC.MeanTCState.load(tmp_path / "ea.pt", net)
    assert loaded is not tr.state and torch.equal(loaded.ea, tr.state.ea)
    assert loaded.ea.device == net.lut.device and not bool(loaded.acc.any())
    # the file also loads into the TC library's state
    assert torch.equal(M.TC.TCState.load(tmp_path / "ea.pt", net).ea, loaded.ea)
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


# ------------------------------------------------------------------ it learns
def last200(tr, steps, chunk):
    scores = []
    for _ in range(steps // chunk):
        tr.step(chunk)
        scores += tr.episodes()["score"].tolist()
    tr.env.check_errors()
    return scores


def test_self_play_learns_under_batch_mean_tc(M):
    """The recipe of test_ntuple_gpu.py::test_self_play_learns with this step: TUPLES_2x4, 256
    boards, the default rate 2^-4 (8 T lr = 1), seed 61, p(4) = 0.5, 4000 steps.  The mean merge
    score of the last 200 finished episodes is at least twice the random player's mean on the same
    seed (the bar of that test, about 2 x 880), and no table entry exceeds 2^28 in magnitude.
    Measured on an MI355X: 5 994 and 596 078; at 2^-6, the batch-mean rule's default, 5 091 and
    307 547."""
    from g2048.player import BatchedPlayer

    seed = 61
    net = M.NT.NTupleNetwork(M.NT.TUPLES_2x4, device=DEV)
    tr = M.MTC.MeanTCTrainer(net, 256, seed=seed, p4=0.5, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == M.MTC.default_meantc_lr_shift(net.spec) == 4
    assert tr.lr_shift == M.MEAN.default_mean_lr_shift(net.spec) - 2
    scores = last200(tr, 4000, 1000)
    rnd = BatchedPlayer(256, device=DEV, seed=seed).play("random")
    learned, random_mean = float(np.mean(scores[-200:])), float(rnd.merge_score.mean())
    largest = int(net.lut.to(torch.int64).abs().max())
    ea = tr.state.ea
    print(f"batch-mean TC n-tuple 2x4 after 4000 steps: {learned:.0f} over the last 200 of "
          f"{len(scores)} episodes, largest |entry| {largest}; random player: {random_mean:.0f}")
    assert len(scores) >= 200
    assert learned >= 2 * random_mean
    assert largest <= 1 << 28
    assert bool((ea[..., 0].abs() <= ea[..., 1]).all())
