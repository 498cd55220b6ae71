"""The expectimax over the multi-stage n-tuple network (csrc/g2048_stagesearch.hip ->
libg2048_stagesearch.so) against the reference tests/stagesearch_ref.py: values and actions bit for
bit on tables with UNSET entries at every stage, every tuple count and stage count, the three
identities of the header (depth 1 is StagedNTupleNetwork.act, S = 1 is the single-table search, a
lifted single table searches as the single table), the anchors, the output variants, that the
table is only read, a captured call, the player, and its strength against the greedy policy."""
import numpy as np
import pytest
import torch

import ntuple_ref as NR
import stagesearch_ref as R
from test_ntsearch_gpu import FULL, NEAR, crafted_boards, dense_boards, random_table
from test_ntstage_gpu import make_net, stage_boards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
SPECS = {"1x1": ((0,),), "8x3": T8M3, "2x4": NR.TUPLES_2x4}
BOUNDS = (5, 8)
UNSET = -(1 << 31)
INT64_MIN = R.INT64_MIN


@pytest.fixture(scope="module")
def SS():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntsearch, ntstage, ntuple, stagesearch
    ntuple.load()
    ntsearch.load()
    ntstage.load()
    stagesearch.load()
    return stagesearch


def NSmod():
    from g2048 import ntstage
    return ntstage


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def holes_net(tuples, bounds, seed):
    """Half-set at every stage, stage 0 included: some lookups resolve to 0."""
    net = make_net(NSmod(), tuples, bounds, seed)
    g = torch.Generator(device=DEV).manual_seed(seed + 1000)
    drop = torch.rand(net.lut[0].shape, generator=g, device=DEV) < 0.5
    net.lut[0].masked_fill_(drop, UNSET)
    return net


def big_value(s, t, i):
    """The 4 x 6 table's entry as a formula, so that the reference needs no host copy of the
    512 MiB: a multiplicative hash in +-2^20; at stage 1 the entries with bit 3 of the hash set
    are UNSET."""
    h = (i * 2654435761 + t * 40503 + s * 7919) % (1 << 32)
    if s > 0 and (h >> 3) & 1:
        return None
    return (h >> 8) % (1 << 21) - (1 << 20)


def big_net():
    """TUPLES_4x6 with S = 2 (512 MiB), filled with big_value."""
    net = NSmod().StagedNTupleNetwork(NR.TUPLES_4x6, (6,), device=DEV)
    i = torch.arange(16 ** 6, dtype=torch.int64, device=DEV)
    for s in range(2):
        for t in range(4):
            h = (i * 2654435761 + t * 40503 + s * 7919) % (1 << 32)
            v = ((h >> 8) % (1 << 21) - (1 << 20)).to(torch.int32)
            if s > 0:
                v = torch.where(((h >> 3) & 1) != 0, torch.full_like(v, UNSET), v)
            net.lut[s, t].copy_(v)
    return net


class Shared:
    """One network per (spec, kind) and one memoising reference per (spec, kind, p4) over a host
    copy of its table: built on first use, shared by every test, never written."""

    def __init__(self):
        self.nets, self.bases, self.refs = {}, {}, {}

    def net(self, name, kind="half"):
        key = (name, kind)
        if key not in self.nets:
            seed = 401 + len(self.nets)
            if name == "4x6":
                net, base = big_net(), big_value
            else:
                if kind == "half":
                    net = make_net(NSmod(), SPECS[name], BOUNDS, seed)
                elif kind == "holes":
                    net = holes_net(SPECS[name], BOUNDS, seed)
                else:
                    net = make_net(NSmod(), SPECS[name], BOUNDS)  # fresh: all UNSET
                base = net.lut.cpu().numpy()
            self.nets[key], self.bases[key] = net, base
        return self.nets[key]

    def ref(self, name, kind="half", p4=0.5):
        key = (name, kind, p4)
        if key not in self.refs:
            net = self.net(name, kind)
            self.refs[key] = R.staged_search(net.spec.tuples, net.bounds,
                                             self.bases[(name, kind)], p4)
        return self.refs[key]


@pytest.fixture(scope="module")
def shared(SS):
    return Shared()


def compare(net, ref, boards, depth, p4=0.5, what=""):
    """One launch over `boards` against the reference, values and actions."""
    acts, vals = net.expectimax(dev(boards), depth, p4)
    torch.cuda.synchronize()
    acts, vals = acts.cpu().numpy(), vals.cpu().numpy()
    ref_a, ref_v = ref.root_batch(boards, depth)
    bad = np.flatnonzero((vals != ref_v).any(axis=1) | (acts != ref_a))
    assert len(bad) == 0, (f"{what} depth {depth} p4 {p4}: {len(bad)} of {len(boards)} boards "
                           f"differ; first: board {boards[bad[0]].tolist()} got "
                           f"{vals[bad[0]].tolist()} / {acts[bad[0]]} want "
                           f"{ref_v[bad[0]].tolist()} / {ref_a[bad[0]]}")
    return acts, vals


def check(shared, name, kind, boards, depth, p4=0.5):
    return compare(shared.net(name, kind), shared.ref(name, kind, p4), boards, depth, p4,
                   f"{name} {kind}")


def boards_d1():
    return np.concatenate([stage_boards(np.random.default_rng(411), 257), crafted_boards()])


def boards_d2():
    rng = np.random.default_rng(412)
    return stage_boards(rng, 67), stage_boards(rng, 128)


def boards_d3(n):
    rng = np.random.default_rng(413)
    b = np.concatenate([dense_boards(rng, n - 3, max_empty=4, hi=9),
                        np.array([NEAR, FULL[:15] + [0],
                                  [15, 15, 16, 16, 17, 17, 15, 16, 1, 2, 1, 2, 0, 1, 0, 1]],
                                 np.uint8)])
    return b


TABLES = [("1x1", "half"), ("8x3", "half"), ("2x4", "half"), ("2x4", "holes"), ("2x4", "fresh"),
          ("4x6", "formula")]


# ------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("name,kind", TABLES)
def test_depth_1_bit_for_bit(shared, name, kind):
    """n = 1, 2, 3, 257 (two boards per wave: an odd n has a dead half) and the crafted boards:
    every legal mask, a single empty cell, terminal children, exponents >= 16."""
    boards = boards_d1()
    for n in (1, 2, 3):
        check(shared, name, kind, boards[5:5 + n], 1)
    check(shared, name, kind, boards[:257], 1, p4=0.1)
    acts, vals = check(shared, name, kind, boards[257:], 1)
    masks = np.arange(16)  # the first 16 crafted boards realise the legal masks 0..15
    legal = ((masks[:, None] >> np.arange(4)) & 1).astype(bool)
    assert ((vals[:16] != INT64_MIN) == legal).all()
    assert (legal[np.arange(16), acts[:16]] | (masks == 0)).all() and acts[0] == 0
    assert (vals[0] == INT64_MIN).all()
    if kind == "fresh":  # every value is the gain tree alone: the depth-1 value is the gain
        for b, v in zip(boards[:40], compare(shared.net(name, kind), shared.ref(name, kind),
                                             boards[:40], 1)[1]):
            for a in range(4):
                after, gain = NR.E.move(b, a)
                assert v[a] == (gain << NR.F if after != [int(x) for x in b] else INT64_MIN)


@pytest.mark.parametrize("name,kind", TABLES)
def test_depth_2_bit_for_bit(shared, name, kind):
    """n = 1 and 67 at p(4) = 0.5, 128 at p(4) = 0.1, and the crafted boards."""
    b67, b128 = boards_d2()
    check(shared, name, kind, b67[:1], 2)
    _, v67 = check(shared, name, kind, b67, 2)
    _, v128 = check(shared, name, kind, b128, 2, p4=0.1)
    crafted = crafted_boards()
    acts, vals = check(shared, name, kind, crafted, 2, p4=0.5 if name == "2x4" else 0.1)
    assert (vals[0] == INT64_MIN).all() and acts[0] == 0  # no legal move
    # negative chance sums occur, where the floor differs from a truncation (not on the fresh
    # table, whose values are gains, nor with the 8 reads of a 16-entry table, which the gains
    # outweigh)
    if kind != "fresh" and name != "1x1":
        v = np.concatenate([v67, v128]).ravel()
        assert ((v < 0) & (v != INT64_MIN)).sum() >= 10


@pytest.mark.parametrize("name,kind,p4,n", [("1x1", "half", 0.1, 8), ("8x3", "half", 0.5, 8),
                                            ("2x4", "half", 0.5, 8), ("2x4", "holes", 0.1, 8),
                                            ("2x4", "fresh", 0.5, 8), ("4x6", "formula", 0.1, 8)])
def test_depth_3_bit_for_bit(shared, name, kind, p4, n):
    """n = 1 and 8 on dense boards with at most 4 empty cells (exponents up to 8, so every
    stage of the bounds occurs among the leaves)."""
    boards = boards_d3(n)
    check(shared, name, kind, boards, 3, p4)
    check(shared, name, kind, boards[:1], 3, p4)


def test_the_inputs_exercise_the_stages_and_the_fall_through(shared):
    """The depth-2 boards above on the half-set 2 x 4 table, counted with the reference: at
    least a quarter of the leaves lie in another stage than their root, and lookups that
    resolve 0, 1 and 2 stages down each occur at least 1000 times.  On the table with holes in
    stage 0 lookups that find nothing at any stage (they read as 0) occur as well."""
    b67, b128 = boards_d2()
    boards = np.concatenate([b67, b128])
    ref = shared.ref("2x4", "half")
    assert {ref.net.stage(b) for b in boards} == {0, 1, 2}
    leaves, crossed = R.crossing(ref, boards, 2)
    depths = R.fall_depths(ref, boards, 2)
    print(f"{len(boards)} depth-2 boards: {crossed} of {leaves} leaves in another stage than "
          f"their root; lookups resolved 0 / 1 / 2 stages down: {depths}")
    assert 4 * crossed >= leaves > 10000
    assert len(depths) == 3 and min(depths) >= 1000 and sum(depths) == 16 * leaves
    holes = shared.ref("2x4", "holes").net
    nothing = sum(holes.val(holes.stage(b), t, i) == 0 and holes.raw(0, t, i) is None
                  for b in b67 for t, i in holes.indices(b))
    assert nothing >= 100


# ------------------------------------------------------------------ 2. every T
@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(SS, T):
    """The run-time tuple loop takes bursts of two and a tail of one: the first T tuples of the
    8 x 3 set at depth 2 on 9 boards, and at depth 1 (where T selects the live loads)."""
    net = make_net(NSmod(), T8M3[:T], BOUNDS, 420 + T)
    ref = R.staged_search(T8M3[:T], BOUNDS, net.lut.cpu().numpy())
    boards = stage_boards(np.random.default_rng(430 + T), 9)
    compare(net, ref, boards, 2, what=f"T = {T}")
    compare(net, ref, boards, 1, what=f"T = {T}")


# ------------------------------------------------------------------ 3. every S
def chain_net(tuples, bounds, seed):
    """Stage s is set only where i mod 8 == s: a lookup at stage s with i mod 8 == k <= s falls
    s - k stages, any other falls through every stage to 0."""
    net = make_net(NSmod(), tuples, bounds, seed, upper=1.0)
    i = torch.arange(net.lut.shape[2], device=DEV) % 8
    for s in range(net.n_stages):
        net.lut[s].masked_fill_((i != s)[None, :], UNSET)
    return net


@pytest.mark.parametrize("S", range(1, 9))
def test_every_stage_count(SS, S):
    """S = 1..8 with the bounds 2..S on the chain table: one burst needs up to S - 1 rounds, and
    lanes of one wave need different numbers of them."""
    bounds = tuple(range(2, S + 1))
    net = chain_net(NR.TUPLES_2x4, bounds, 440 + S)
    ref = R.staged_search(NR.TUPLES_2x4, bounds, net.lut.cpu().numpy())
    rng = np.random.default_rng(450 + S)
    caps = np.array([1, 2, 3, 4, 5, 6, 7, 9] * 3)[:, None]  # every largest tile, three times
    boards = np.minimum(stage_boards(rng, 24, caps=(11,)), caps).astype(np.uint8)
    boards[np.arange(24), rng.integers(0, 16, 24)] = caps[:, 0]
    assert {ref.net.stage(b) for b in boards} == set(range(S))
    compare(net, ref, boards, 2, what=f"S = {S}")
    compare(net, ref, boards[:9], 1, what=f"S = {S}")
    if S == 8:
        depths = R.fall_depths(ref, boards, 2)
        assert all(d > 0 for d in depths), depths  # every number of rounds 0..7 occurs
        compare(net, ref, boards_d3(5), 3, what="S = 8")


# ------------------------------------------------------------------ 4. the three identities
def test_depth_1_is_act(shared):
    rng = np.random.default_rng(460)
    boards = dev(np.concatenate([stage_boards(rng, 4099 - 29), crafted_boards()[:29]]))
    for kind in ("half", "holes"):
        net = shared.net("2x4", kind)
        want_a, want_q, _ = net.act(boards)
        for p4 in (0.5, 0.1):
            acts, vals = net.expectimax(boards, 1, p4)
            assert torch.equal(vals, want_q) and torch.equal(acts, want_a)


def test_one_stage_is_the_single_table_search(SS):
    plain = random_table(NR.TUPLES_2x4, 461)
    staged = NSmod().StagedNTupleNetwork.from_network(plain, ())
    rng = np.random.default_rng(462)
    boards = dev(stage_boards(rng, 4099))
    for depth, b in ((1, boards), (2, boards), (3, dev(boards_d3(16)))):
        for p4 in (0.5, 0.1):
            got, want = staged.expectimax(b, depth, p4), plain.search(b, depth, p4)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (depth, p4)


def test_a_lifted_single_table_searches_as_the_single_table(SS):
    """from_network(net, (5, 8)): stage 0 is the table, stages 1 and 2 are UNSET.  Every lookup
    of a board of stage 2 falls two rounds, and the result is the single table's."""
    plain = random_table(NR.TUPLES_2x4, 463)
    staged = NSmod().StagedNTupleNetwork.from_network(plain, BOUNDS)
    rng = np.random.default_rng(464)
    boards = dev(stage_boards(rng, 515))
    assert set(staged.stage_of(boards).tolist()) == {0, 1, 2}
    for depth, b in ((1, boards), (2, boards), (3, dev(boards_d3(8)))):
        got, want = staged.expectimax(b, depth), plain.search(b, depth)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), depth


def test_a_tree_that_stays_in_one_stage_is_that_stage_resolved(shared):
    """Boards that hold a 13 and otherwise exponents <= 6, bounds (13,): no merge makes a second
    13, the whole tree stays in stage 1, and the result is resolved(1).search's."""
    rng = np.random.default_rng(465)
    b = (rng.integers(1, 7, (300, 16)) * (rng.random((300, 16)) < 0.7)).astype(np.uint8)
    b[np.arange(300), rng.integers(0, 16, 300)] = 13
    boards = dev(b)
    net = make_net(NSmod(), NR.TUPLES_2x4, (13,), 466)
    plain = net.resolved(1)
    for depth, n in ((1, 300), (2, 300), (3, 6)):
        got, want = net.expectimax(boards[:n], depth), plain.search(boards[:n], depth)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), depth
    other = net.resolved(0).search(boards, 2)[1]
    assert not torch.equal(other, net.expectimax(boards, 2)[1])  # stage 0 frozen is another search


# ------------------------------------------------------------------ 5. anchors, crafted cases
def anchor_net(bounds, fill):
    net = NSmod().StagedNTupleNetwork(((0,),), bounds, device=DEV)
    i = torch.arange(16, dtype=torch.int32, device=DEV)
    fill(net.lut, i)
    return net


def test_the_anchors_of_the_definition(SS):
    """The hand-checked numbers of tests/stagesearch_ref.py's docstring, from the kernel."""
    m = INT64_MIN

    def table_x(lut, i):
        lut[0, 0] = 1024 * i
        lut[1, 0] = torch.where(i % 2 == 0, 4096 * i + 3, torch.full_like(i, UNSET))

    def table_y(lut, i):
        lut[0, 0] = 1000 * i
        lut[1, 0] = -77

    x = anchor_net((2,), table_x)
    boards = dev(np.array([[1, 1] + [0] * 14, NEAR, NEAR[:15] + [1]], np.uint8))
    want_a = {(1, 0.5): [m, 2048, 20504, 20504], (1, 0.1): [m, 2048, 20504, 20504],
              (2, 0.5): [m, 23136, 24803, 24803], (2, 0.1): [m, 21497, 22126, 22126],
              (3, 0.5): [m, 27020, 28091, 28091], (3, 0.1): [m, 24087, 25024, 25024]}
    want_n = {1: [m, 34834, m, 34834], 2: [m, 51218, m, 51218], 3: [m, 69650, m, 69650]}
    for (depth, p4), v in want_a.items():
        acts, vals = x.expectimax(boards, depth, p4)
        assert vals[0].tolist() == v and acts.tolist() == [2, 1, 0], (depth, p4)
        assert vals[2].tolist() == [m] * 4
        if p4 == 0.5:
            assert vals[1].tolist() == want_n[depth]
    # the single table alone: the anchor of the single-table search
    assert x.resolved(0).search(boards, 1)[1][0].tolist() == [m, 2048, 8192, 8192]
    y = anchor_net((25,), table_y)
    top = dev(np.array([[24, 24, 23, 23, 22, 22, 0, 0, 1, 2, 1, 2, 0, 0, 1, 1]], np.uint8))
    acts, vals = y.expectimax(top, 1)
    assert vals[0].tolist() == [64096, 8096, 60129545624, 60129545624] and acts.tolist() == [2]
    acts, vals = y.expectimax(top, 2)
    assert vals[0].tolist() == [60129555044, 42949684632, 60129549464, 60129556632]
    assert acts.tolist() == [3]


@pytest.mark.parametrize("bounds", [(16,), (17,), (15, 16, 17)])
def test_exponents_past_the_index_clamp_decide_the_stage(SS, bounds):
    """Exponents 12..18 next to bounds at 16 and 17: the stage uses the true exponent, the table
    index the one clamped at 15."""
    net = make_net(NSmod(), NR.TUPLES_2x4, bounds, 470 + len(bounds), upper=0.6)
    ref = R.staged_search(NR.TUPLES_2x4, bounds, net.lut.cpu().numpy())
    rng = np.random.default_rng(471)
    low = (rng.integers(1, 4, (24, 16)) * (rng.random((24, 16)) < 0.6)).astype(np.uint8)
    for k, row in enumerate(low):
        cells = rng.choice(16, 3, replace=False)
        row[cells] = [14 + k % 5, 12 + k % 6, 13]
    boards = np.concatenate([low, crafted_boards()[23:28]])
    assert {ref.net.stage(b) for b in boards} == set(range(len(bounds) + 1))
    assert sum(int(max(b)) >= 16 for b in boards) >= 10
    compare(net, ref, boards, 1, what=str(bounds))
    compare(net, ref, boards, 2, what=str(bounds))


# ------------------------------------------------------------------ 6. outputs and guards
def test_output_variants_guards_and_a_table_that_is_only_read(SS, shared):
    """values-only and action-only calls write the same bytes as the full call, nothing around
    either output is touched, the wrapper fills caller-owned outputs, and the whole table is
    what it was: the search promotes nothing."""
    import ctypes as C

    import g2048._native as N

    net, n, pad = shared.net("2x4", "holes"), 67, 64
    table = net.lut.clone()
    b67, _ = boards_d2()
    boards = dev(b67)
    lib = SS.load()
    V, A = 0x5A5A5A5A5A5A5A5A, 0xA5

    def call(want_values, want_action):
        vbuf = torch.full((pad + 4 * n + pad,), V, dtype=torch.int64, device=DEV)
        abuf = torch.full((pad + n + pad,), A, dtype=torch.uint8, device=DEV)
        rc = lib.g2048_stagesearch_expectimax(
            C.byref(net._c), C.byref(net._cs), net.lut.data_ptr(), boards.data_ptr(), n, 2, 0,
            vbuf[pad:].data_ptr() if want_values else None,
            abuf[pad:].data_ptr() if want_action else None, 0,
            torch.cuda.current_stream().cuda_stream)
        assert rc == N.G2048_OK, lib.g2048_stagesearch_last_error()
        torch.cuda.synchronize()
        return vbuf.cpu().numpy(), abuf.cpu().numpy()

    v_full, a_full = call(True, True)
    v_only, a_none = call(True, False)
    v_none, a_only = call(False, True)
    assert np.array_equal(v_only, v_full) and np.array_equal(a_only, a_full)
    assert (a_none == A).all() and (v_none == V).all()
    assert (v_full[:pad] == V).all() and (v_full[pad + 4 * n:] == V).all()
    assert (a_full[:pad] == A).all() and (a_full[pad + n:] == A).all()
    ref_a, ref_v = shared.ref("2x4", "holes").root_batch(b67, 2)
    assert np.array_equal(v_full[pad:pad + 4 * n].reshape(n, 4), ref_v)
    assert np.array_equal(a_full[pad:pad + n], ref_a)
    # the wrapper: None for what was not asked for, caller-owned outputs are the ones returned
    acts, vals = net.expectimax(boards, 2, values=False)
    assert vals is None and np.array_equal(acts.cpu().numpy(), ref_a)
    acts, vals = SS.expectimax(net, boards, 2, actions=False)
    assert acts is None and np.array_equal(vals.cpu().numpy(), ref_v)
    out_v = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
    out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    acts, vals = net.expectimax(boards, 2, values=False, actions=False, values_out=out_v,
                                actions_out=out_a)
    assert acts is out_a and vals is out_v
    assert np.array_equal(out_v.cpu().numpy(), ref_v) and np.array_equal(out_a.cpu().numpy(), ref_a)
    with pytest.raises(ValueError):
        net.expectimax(boards, 2, values=False, actions=False)
    with pytest.raises(ValueError):
        net.expectimax(boards, 2, values_out=out_v[:5])
    for depth in (1, 3):
        net.expectimax(boards[:8], depth)
    torch.cuda.synchronize()
    assert torch.equal(net.lut, table)


def test_captured_search_replays_on_changed_boards(SS, shared):
    """A call captured once reads the boards of the replay, not those of the capture."""
    from g2048.dist import graph_capture

    net = shared.net("2x4", "half")
    b67, b128 = boards_d2()
    boards = dev(b128[:67])
    out_a = torch.zeros(67, dtype=torch.uint8, device=DEV)
    out_v = torch.zeros((67, 4), dtype=torch.int64, device=DEV)
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        net.expectimax(boards, 2, values_out=out_v, actions_out=out_a)
    torch.cuda.synchronize()
    assert not out_v.any()  # the capture ran nothing
    ref = shared.ref("2x4", "half")
    for b in (b128[:67], b67):
        boards.copy_(dev(b))
        g.replay()
        torch.cuda.synchronize()
        ref_a, ref_v = ref.root_batch(b, 2)
        assert np.array_equal(out_v.cpu().numpy(), ref_v)
        assert np.array_equal(out_a.cpu().numpy(), ref_a)


# ------------------------------------------------------------------ 7. the player
def test_player_plays_to_the_end_with_the_reference_actions(SS):
    """8 games of play("ntstage_search") at depth 2 to the end on a half-set table with bounds
    (3, 5): the first 40 moves of every game are the reference's, no game is left stuck, and
    every game ends on a board without a legal move.  At depth 1 the games are exactly
    play("ntuple")'s."""
    from g2048.player import BatchedPlayer
    from oracle import oracle as O

    net = make_net(NSmod(), NR.TUPLES_2x4, (3, 5), 480)
    ref = R.staged_search(NR.TUPLES_2x4, (3, 5), net.lut.cpu().numpy())
    res = BatchedPlayer(8, device=DEV, seed=481, ntuple=net, search_depth=2,
                        record_games=8).play("ntstage_search")
    stages = set()
    for t, (before, act, _reward, _score, _after) in enumerate(res.trace[:40]):
        b = before.cpu().numpy()
        live = [g for g in range(8) if t < res.moves[g]]
        want = [ref.root(b[g], 2)[1] for g in live]
        assert act.cpu().numpy()[live].tolist() == want, t
        stages |= {ref.net.stage(b[g]) for g in live}
    assert stages == {0, 1, 2}
    assert (res.moves > 14).all() and not res.stuck.any()
    for g, h in enumerate(res.histories):
        assert len(h) == res.moves[g] and h[-1][2] == 0 and h[-1][3] == res.merge_score[g]
        last = np.where(h[-1][0] > 0, np.log2(np.maximum(h[-1][0], 1)), 0).astype(np.uint8)
        assert O.legal_mask(last.reshape(16)) == 0
    one = BatchedPlayer(64, device=DEV, seed=482, ntuple=net, search_depth=1,
                        record_games=2).play("ntstage_search")
    greedy = BatchedPlayer(64, device=DEV, seed=482, ntuple=net, record_games=2).play("ntuple")
    for name in ("merge_score", "moves", "max_tile"):
        assert np.array_equal(getattr(one, name), getattr(greedy, name)), name
    for h1, h2 in zip(one.histories, greedy.histories):
        assert len(h1) == len(h2)
        assert all(x[1] == y[1] and np.array_equal(x[0], y[0]) for x, y in zip(h1, h2))


# ------------------------------------------------------------------ 8. strength
def test_staged_search_is_at_least_as_strong_as_the_greedy_policy(SS):
    """StagedNTupleNetwork(TUPLES_2x4, bounds (7,)) trained as
    tests/test_ntstage_gpu.py::test_staged_self_play_learns trains it (256 boards, 4000 steps,
    seed 61), then 256 games of play("ntuple") and of play("ntstage_search") at depth 2 on the
    same seeds: the search's mean merge score is at least the greedy policy's on the same table
    (the bar of the single-table search's test).  Measured on an MI355X: greedy 4387, depth 2
    10737, ratio 2.45."""
    from g2048 import ntuple
    from g2048.player import BatchedPlayer

    seed = 61
    net = NSmod().StagedNTupleNetwork(ntuple.TUPLES_2x4, (7,), device=DEV)
    tr = ntuple.NTupleTrainer(net, 256, seed=seed, p4=0.5, lr_num=1, lr_shift=10, log_slots=64)
    for _chunk in range(4):
        tr.step(1000)
        tr.episodes()
    tr.env.check_errors()
    table = net.lut.clone()
    greedy = BatchedPlayer(256, device=DEV, seed=seed, ntuple=net).play("ntuple")
    deep = BatchedPlayer(256, device=DEV, seed=seed, ntuple=net,
                         search_depth=2).play("ntstage_search")
    g, d = float(greedy.merge_score.mean()), float(deep.merge_score.mean())
    print(f"staged 2x4, bounds (7,), after 4000 TD steps, 256 games each: greedy {g:.0f} (mean "
          f"moves {greedy.moves.mean():.0f}, max tile {greedy.max_tile.max()}), depth-2 staged "
          f"search {d:.0f} (mean moves {deep.moves.mean():.0f}, max tile {deep.max_tile.max()}), "
          f"ratio {d / g:.2f}")
    assert not deep.stuck.any() and not greedy.stuck.any()
    assert torch.equal(net.lut, table)  # playing promotes nothing
    assert d >= g
