"""The twelve n-tuple libraries at the edges of the domains their headers declare, bit for bit
against the Python references: tables whose values need 38 bits ("full", "max", "min", and UNSET
beside INT32_MIN + 1), boards of exponents up to 27 (a gain of exactly 2^31), deltas of INT32_MIN
and INT32_MAX, the rates 1 / 2^31, 2^16 / 2^31, 1 and 0, and accumulators up to 2^62.  The inputs
come from tests/domain_edge.py; tests/test_domain_edge.py proves on the CPU that every learning
case stays inside the domain, and the reference side of every step here runs inside the same
InDomain guard.

The searches are compared with the definition (ntsearch_ref, stagesearch_ref, deepsearch_ref),
never with each other: the three search libraries share one tree walk.  The wide search takes root
exponents up to 22 at every depth, as its header declares.  The staged networks use the small
specs: two stages of the 4x6 set would be twice the largest allocation."""
import numpy as np
import pytest
import torch

import deepsearch_ref as DR
import domain_edge as DE
import ntsearch_ref as SRCH
import ntstage_ref as SR
import ntuple_ref as NR
import stagesearch_ref as SSR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT64_MIN = NR.INT64_MIN
CASES = DE.learning_cases()


class Modules:
    pass


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import (deepsearch, ntlambda, ntmean, ntmeantc, ntsearch, ntstage, nttc, ntuple,
                       stagemean, stagemeantc, stagesearch)
    m = Modules()
    m.NT, m.TC, m.L, m.NS, m.MEAN, m.MTC, m.SM, m.SMTC, m.D = (
        ntuple, nttc, ntlambda, ntstage, ntmean, ntmeantc, stagemean, stagemeantc, deepsearch)
    for mod in (ntuple, nttc, ntlambda, ntstage, ntmean, ntmeantc, stagemean, stagemeantc,
                ntsearch, stagesearch, deepsearch):
        mod.load()
    return m


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def flat_net(G, name, spec, seed):
    net = G.NT.NTupleNetwork(DE.SPECS[spec], device=DEV)
    net.lut.copy_(DE.table(name, tuple(net.lut.shape), DEV, seed))
    return net


def staged_net(G, name, spec, bounds, seed):
    net = G.NS.StagedNTupleNetwork(DE.SPECS[spec], bounds, device=DEV)
    net.lut.copy_(DE.table(name, tuple(net.lut.shape), DEV, seed))
    return net


class DeviceBase:
    """Entries gathered from the device tensor by index, in batches, so the 4x6 table is never
    copied to the host."""

    def __init__(self, lut):
        self.lut, self.cache = lut, {}

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


def flat_ref(net, name, boards=(), leaves=()):
    """The reference over net's table: a constant for "max" / "min", else the entries that
    `boards`, their afterstates and `leaves` read, gathered in one batch."""
    if name in ("max", "min"):
        const = DE.INT32_MAX if name == "max" else DE.INT32_MIN
        return NR.Net(net.spec.tuples, base=lambda t, i: const)
    ref = NR.Net(net.spec.tuples, base=DeviceBase(net.lut))
    keys = [k for b in leaves for k in ref.indices(b)]
    for b in boards:
        b = [int(x) for x in b]
        keys += ref.indices(b)
        for a in range(4):
            keys += ref.indices(NR.E.move(b, a)[0])
    ref.base.prefetch(keys)
    return ref


def check_values_and_act(net, ref, boards, entry=None):
    """values, q, action and after against the reference; with `entry` (a table of one value)
    also the closed form q = (gain << F) + 8 T * entry."""
    assert net.values(dev(boards)).cpu().tolist() == [ref.V(b) for b in boards]
    acts, q, after = net.act(dev(boards), after=True)
    acts, q, after = acts.cpu().tolist(), q.cpu().tolist(), after.cpu().tolist()
    legal = 0
    for i, b in enumerate(boards):
        qs, a, aft = ref.policy(b)
        assert [INT64_MIN if x is None else x for x in qs] == q[i], (i, b.tolist())
        assert acts[i] == a and after[i] == aft, (i, b.tolist())
        if entry is not None:
            for m in range(4):
                moved, gain = NR.E.move(b, m)
                if moved != [int(x) for x in b]:
                    assert q[i][m] == (gain << DE.F) + 8 * len(net.spec.tuples) * entry
                    legal += 1
    assert entry is None or legal


# ------------------------------------------------------------------ values and act
@pytest.mark.parametrize("spec", ["1x1", "2x4", "8x3", "4x6"])
@pytest.mark.parametrize("name", ["full", "max", "min"])
def test_values_and_act_on_full_range_tables(G, name, spec):
    net = flat_net(G, name, spec, 11)
    rng = np.random.default_rng(21)
    entry = {"max": DE.INT32_MAX, "min": DE.INT32_MIN}.get(name)
    for n in (1, 3, 65):  # a partial wave of the 2-boards-per-wave frame; one past a 64 group
        boards = DE.high_boards(rng, n, DE.CAP_LEARN)
        check_values_and_act(net, flat_ref(net, name, boards), boards, entry)
    if name == "max" and spec == "8x3":
        assert int(net.values(dev(boards[:1]))[0]) == 64 * DE.INT32_MAX
        assert net.act(dev(boards[:1]))[1][0].tolist() == [(1 << 41) + 64 * DE.INT32_MAX] * 4


@pytest.mark.parametrize("bounds", DE.STAGE_BOUNDS, ids=["b16_25", "b27"])
@pytest.mark.parametrize("spec", DE.SMALL)
@pytest.mark.parametrize("name", ["full", "max", "min", "edge_unset"])
def test_staged_values_and_act_on_full_range_tables(G, name, spec, bounds):
    net = staged_net(G, name, spec, bounds, 12)
    ref = SR.StagedNet(net.spec.tuples, bounds, base=net.lut.cpu().numpy())
    rng = np.random.default_rng(22)
    entry = {"max": DE.INT32_MAX, "min": DE.INT32_MIN + 1}.get(name)
    stages = set()
    for n in (1, 3, 65):
        boards = DE.high_boards(rng, n, DE.CAP_LEARN)
        if n == 65:  # nearly every board of exponents up to 27 holds a 16: some of stage 0 too
            boards[-8:] = DE.low_boards(rng, 8, hi=15)
        stages |= {ref.stage(b) for b in boards}
        check_values_and_act(net, ref, boards, entry)
    assert stages == set(range(len(bounds) + 1))
    if name == "edge_unset":  # a value of INT32_MIN + 1 and an UNSET met in one board's reads
        kinds = {ref.raw(ref.stage(b), t, i) for b in boards for t, i in ref.indices(b)
                 if ref.stage(b)}
        assert {None, DE.INT32_MIN + 1} <= kinds


# ------------------------------------------------------------------ the per-wave searches
def search_boards(seed, n, cap):
    """The crafted boards of high_boards (all-cap, stripes, terminal, the 24s row, dense with 0..3
    empties), then nearly full mixed boards: the Python reference stays within seconds."""
    return DE.high_boards(np.random.default_rng(seed), n, cap, fills=(0.9, 1.0))


def same(got, want, what):
    assert got[1].cpu().tolist() == want[1].tolist(), f"{what}: values differ"
    assert got[0].cpu().tolist() == want[0].tolist(), f"{what}: actions differ"


@pytest.mark.parametrize("spec", ["2x4", "8x3"])
@pytest.mark.parametrize("name", ["full", "max", "min"])
def test_ntsearch_against_the_definition(G, name, spec):
    net = flat_net(G, name, spec, 31)
    boards = search_boards(41, 10, DE.SEARCH_CAP[3])
    base = net.lut.cpu().numpy()
    for p4 in (0.5, 0.1):
        s = SRCH.Search(NR.Net(net.spec.tuples, base=base), p4)
        for depth in (1, 2, 3):
            same(net.search(dev(boards), depth, p4), s.root_batch(boards, depth),
                 (name, spec, depth, p4))


def test_ntsearch_4x6_against_the_definition(G):
    net = flat_net(G, "full", "4x6", 32)
    boards = search_boards(42, 8, DE.SEARCH_CAP[3])[4:8]  # the dense ones: 0..3 empty cells
    probe = SRCH.Search(NR.Net(net.spec.tuples), 0.5)
    leaves = {leaf for b in boards for d in (1, 2, 3) for leaf in probe.leaf_boards(b, d)}
    ref = flat_ref(net, "full", leaves=leaves)
    for p4 in (0.5, 0.1):
        s = SRCH.Search(ref, p4)
        for depth in (1, 2, 3):
            same(net.search(dev(boards), depth, p4), s.root_batch(boards, depth), (depth, p4))


@pytest.mark.parametrize("spec,bounds", [("2x4", (16, 25)), ("8x3", (27,)), ("8x3", (16, 25))])
@pytest.mark.parametrize("name", ["full", "max", "min", "edge_unset"])
def test_stagesearch_against_the_definition(G, name, spec, bounds):
    net = staged_net(G, name, spec, bounds, 33)
    boards = search_boards(43, 10, DE.SEARCH_CAP[3])
    base = net.lut.cpu().numpy()
    for p4 in (0.5, 0.1):
        s = SSR.staged_search(net.spec.tuples, bounds, base, p4)
        for depth in (1, 2, 3):
            same(net.expectimax(dev(boards), depth, p4), s.root_batch(boards, depth),
                 (name, spec, bounds, depth, p4))
    if bounds == (16, 25):  # the 24s row merges into a 25: leaves in another stage than the root
        leaves, crossed = SSR.crossing(s, boards[3:4], 2)
        assert 0 < crossed < leaves


# ------------------------------------------------------------------ the wide search
def deep_pair(G, staged, name, seed):
    """(net, search(p4)): the 8x3 set flat, or staged with the bounds (16, 25)."""
    if staged:
        net = staged_net(G, name, "8x3", (16, 25), seed)
        base = net.lut.cpu().numpy()
        return net, lambda p4: SSR.staged_search(net.spec.tuples, (16, 25), base, p4)
    net = flat_net(G, name, "8x3", seed)
    base = net.lut.cpu().numpy()
    return net, lambda p4: SRCH.Search(NR.Net(net.spec.tuples, base=base), p4)


@pytest.mark.parametrize("staged", [False, True], ids=["flat", "staged"])
@pytest.mark.parametrize("name", ["full", "max", "min"])
def test_deepsearch_depths_1_to_3_against_the_definition_at_every_split(G, name, staged):
    net, search = deep_pair(G, staged, "edge_unset" if staged and name == "full" else name, 34)
    boards = search_boards(44, 9, DE.DEEP_CAP)
    for p4 in (0.5, 0.1):
        s = search(p4)
        for depth in (1, 2, 3):
            want = s.root_batch(boards, depth)
            for top in G.D.legal_tops(depth):
                same(G.D.expectimax(net, dev(boards), depth, p4, top=top), want,
                     (name, staged, depth, p4, top))


@pytest.mark.parametrize("staged", [False, True], ids=["flat", "staged"])
@pytest.mark.parametrize("name", ["full", "max"])
def test_deepsearch_depths_4_and_5_against_the_definition(G, name, staged):
    """Depth 4, both splits: a full board of 19..22 and sixteen 22s, whose root values over the max
    table are about 4.1e11.  Depth 5: two 22 / 20 and 21 / 22 checkerboards with one corner
    emptied.  The boards are few because the Python reference takes 1.5 to 2.5 s for each."""
    net, search = deep_pair(G, staged, name, 35)
    deep = DR.Deep(search(0.5))
    four = np.stack([DE.dense_board(np.random.default_rng(45), DE.DEEP_CAP, 0),
                     np.full(16, 22, np.uint8)])
    for top in (1, 2):
        want = deep.root_batch(four, 4, top)
        same(G.D.expectimax(net, dev(four), 4, 0.5, top=top), want, (name, staged, 4, top))
    if name == "max" and not staged:
        assert want[1][-1].max() > 4e11
    five = np.stack([DE.checker(22, 20), DE.checker(21, 22)])
    five[0, 0] = five[1, 15] = 0
    want = deep.root_batch(five, 5, 2)
    same(G.D.expectimax(net, dev(five), 5, 0.5, top=2), want, (name, staged, 5))
    assert np.abs(want[1][want[1] != INT64_MIN]).max() > 1 << 32  # no root value fits int32


# ------------------------------------------------------------------ learning steps
class GpuSide:
    """One library's network and state on the GPU, built from a Case.  Each call sets the
    per-board state from the call's history, as domain_edge.RefSide does."""

    def __init__(self, G, case, lib):
        self.G, self.case, self.lib = G, case, lib
        if case.bounds is None:
            self.net = G.NT.NTupleNetwork(case.tuples, device=DEV)
        else:
            self.net = G.NS.StagedNTupleNetwork(case.tuples, case.bounds, device=DEV)
        self.net.lut.copy_(dev(case.lut, np.int32))
        kind = {"tc": G.TC.TCState, "mean": G.MEAN.MeanState, "meantc": G.MTC.MeanTCState,
                "stagemean": G.SM.StagedMeanState, "stagemeantc": G.SMTC.StagedMeanTCState}
        self.state = kind[lib](self.net) if lib in kind else None
        if case.ea is not None and lib in DE.TC_LIBS:
            self.state.ea.copy_(dev(case.ea, np.int64))

    def step(self, call):
        """(actions, errs, deltas, state) in RefSide.step's format."""
        n = len(call.boards)
        boards = dev(call.boards)
        a = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
        d = torch.full((n,), 77, dtype=torch.int32, device=DEV)
        e = torch.full((n,), 77, dtype=torch.int64, device=DEV)
        if self.lib == "lam":
            st = self.G.L.TDLambdaState(self.net, n, *self.case.lam)
            hist, head, depth = DE.RefSide.ring(call, st.horizon)
            st.hist.copy_(dev(hist))
            st.head.copy_(dev(head))
            st.depth.copy_(dev(depth))
            st.step(boards, *call.lr, a, d, e)
            state = (st.hist.cpu().tolist(), st.head.cpu().tolist(), st.depth.cpu().tolist())
        else:
            prev, has = DE.RefSide.state(call)
            prev, has = dev(prev), dev(has)
            step = {"td": self.net.td_step, "stage": self.net.td_step,
                    "tc": getattr(self.state, "tc_step", None),
                    "mean": getattr(self.state, "mean_step", None),
                    "stagemean": getattr(self.state, "mean_step", None),
                    "meantc": getattr(self.state, "meantc_step", None),
                    "stagemeantc": getattr(self.state, "meantc_step", None)}[self.lib]
            step(boards, prev, has, *call.lr, a, d, e)
            state = (prev.cpu().tolist(), has.cpu().tolist())
        return a.cpu().tolist(), e.cpu().tolist(), d.cpu().tolist(), state


@pytest.mark.parametrize("name,lib,build", CASES, ids=[c[0] for c in CASES])
def test_learning_step_at_the_domain_edge(G, name, lib, build):
    """Everything the libraries' own check_calls helpers compare, after every call: action, err,
    delta, prev and has_prev (lambda: the ring), the whole table with its UNSET pattern, the
    accumulators, and the batch-mean workspace left all zero."""
    case = build()
    gpu, ref = GpuSide(G, case, lib), DE.RefSide(case, lib)
    for c, call in enumerate(case.calls):
        got = gpu.step(call)
        want = ref.step(call)  # inside InDomain
        for what, x, y in zip(("action", "err", "delta"), got, want):
            assert x == list(y), (c, what)
        for what, x, y in zip(("prev / hist", "has_prev / head", "depth"), got[3], want[3]):
            assert x == y, (c, what)
        lut, want_lut = gpu.net.lut.cpu().numpy(), ref.want_lut()
        assert np.array_equal(lut == DE.UNSET, want_lut == DE.UNSET), c
        assert np.array_equal(lut, want_lut), c
        if lib in DE.TC_LIBS:
            assert np.array_equal(gpu.state.ea.cpu().numpy(), ref.want_ea()), c
        if hasattr(gpu.state, "acc"):
            assert not bool(gpu.state.acc.any()), c
        if "exact" in name:
            assert [want[2][i] for i in (1, 2, 3, 5, 6, 7)] == list(DE.DELTAS)
    if "seeds" in name:
        assert int(gpu.state.ea[..., 1].max()) >= 1 << 61
