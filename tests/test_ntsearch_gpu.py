"""The expectimax over the n-tuple network (csrc/g2048_ntsearch.hip -> libg2048_ntsearch.so)
against the plain Python restatement tests/ntsearch_ref.py: values and actions bit for bit, depth
1 against NTupleNetwork.act, the output variants, a captured search + step, the searching player
against the oracle env, and its strength against the greedy policy on the same table."""
import numpy as np
import pytest
import torch

import ntsearch_ref as R
import ntuple_ref as NR
from boards import mask_boards
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
SPECS = {"1x1": ((0,),), "8x3": T8M3, "2x4": NR.TUPLES_2x4, "4x6": NR.TUPLES_4x6}
# a full board without equal neighbours
FULL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1]
NEAR = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0]  # most of its children are terminal


@pytest.fixture(scope="module")
def NS():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntsearch, ntuple
    ntuple.load()
    ntsearch.load()
    return ntsearch


def random_table(tuples, seed):
    """A network whose table holds random int32 in +-2^20: chance sums are negative about half
    the time, so the floor is exercised."""
    from g2048 import ntuple

    net = ntuple.NTupleNetwork(tuples, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=g, device=DEV,
                                dtype=torch.int32))
    return net


class Shared:
    """One randomly filled network per spec and one memoising reference per (spec, p4) over a
    host copy of its table: built on first use, shared by every test, never trained."""

    def __init__(self):
        self.nets, self.tables, self.refs = {}, {}, {}

    def net(self, name):
        if name not in self.nets:
            self.nets[name] = random_table(SPECS[name], 71 + len(self.nets))
            self.tables[name] = self.nets[name].lut.cpu().numpy()
        return self.nets[name]

    def ref(self, name, p4=0.5):
        if (name, p4) not in self.refs:
            self.net(name)
            self.refs[(name, p4)] = R.Search(NR.Net(SPECS[name], base=self.tables[name]), p4)
        return self.refs[(name, p4)]


@pytest.fixture(scope="module")
def shared(NS):
    return Shared()


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def dense_boards(rng, n, max_empty, hi=8):
    """Full boards of exponents 1..hi-1 with 1..max_empty cells emptied."""
    b = rng.integers(1, hi, (n, 16)).astype(np.uint8)
    for row in b:
        row[rng.choice(16, int(rng.integers(1, max_empty + 1)), replace=False)] = 0
    return b


def one_board_per_mask():
    by_mask = {}
    for b in mask_boards():
        by_mask.setdefault(int(O.legal_mask(b)), b)
    assert len(by_mask) == 16
    return [by_mask[m] for m in range(16)]


def crafted_boards():
    """Every legal mask (no legal move among them), a single empty cell, children that are
    terminal, exponents >= 16 (clamped in the index, not in the gain) and symmetric boards."""
    out = [np.asarray(b, np.uint8) for b in one_board_per_mask()]
    out += [NEAR, NEAR[:15] + [1], [0] * 16, [1, 1] + [0] * 14]
    for hole in (0, 5, 15):  # a single empty cell in a board that is terminal once it is filled
        b = list(FULL)
        b[hole] = 0
        out.append(b)
    out += [[17, 16, 15, 15, 16, 15, 0, 0, 3, 2, 1, 0, 0, 0, 0, 1],
            [15, 15, 16, 16, 17, 17, 15, 16, 1, 2, 1, 2, 0, 1, 0, 1],
            [16, 16, 17, 0, 15, 15, 15, 15, 2, 1, 2, 1, 1, 2, 1, 2],
            [14, 14, 15, 15, 16, 16, 17, 17, 0, 0, 0, 0, 17, 16, 15, 14],
            [24, 24, 23, 23, 22, 22, 0, 0, 1, 2, 1, 2, 0, 0, 1, 1]]  # the domain's largest tiles
    sq = np.random.default_rng(5).integers(0, 7, (4, 4))
    out.append(np.triu(sq) + np.triu(sq, 1).T)                    # transpose-symmetric
    out.append(np.concatenate([sq[:, :2], sq[:, 1::-1]], axis=1))  # symmetric under a column flip
    return np.array([np.asarray(b, np.uint8).reshape(16) for b in out], np.uint8)


def check(shared, name, boards, depth, p4=0.5):
    """One launch over `boards` against the reference, values and actions."""
    net = shared.net(name)
    acts, vals = net.search(dev(boards), depth, p4)
    torch.cuda.synchronize()
    acts, vals = acts.cpu().numpy(), vals.cpu().numpy()
    ref_a, ref_v = shared.ref(name, p4).root_batch(boards, depth)
    bad = np.flatnonzero((vals != ref_v).any(axis=1) | (acts != ref_a))
    assert len(bad) == 0, (f"{name} depth {depth} p4 {p4}: {len(bad)} of {len(boards)} boards "
                           f"differ; first: board {boards[bad[0]].tolist()} got "
                           f"{vals[bad[0]].tolist()} / {acts[bad[0]]} want "
                           f"{ref_v[bad[0]].tolist()} / {ref_a[bad[0]]}")
    return acts, vals


# ------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize("name", list(SPECS))
def test_depth_1_bit_for_bit(shared, name):
    rng = np.random.default_rng(81)
    check(shared, name, random_boards(rng, 257), 1)
    check(shared, name, random_boards(rng, 1), 1, p4=0.1)
    acts, vals = check(shared, name, crafted_boards(), 1)
    masks = np.arange(16)  # the first 16 crafted boards realise the legal masks 0..15
    legal = ((masks[:, None] >> np.arange(4)) & 1).astype(bool)
    assert ((vals[:16] != R.INT64_MIN) == legal).all()
    assert (legal[np.arange(16), acts[:16]] | (masks == 0)).all() and acts[0] == 0


@pytest.mark.parametrize("name,p4", [("1x1", 0.5), ("8x3", 0.1), ("2x4", 0.5), ("4x6", 0.1)])
def test_depth_2_bit_for_bit(shared, name, p4):
    rng = np.random.default_rng(82)
    other = 0.1 if p4 == 0.5 else 0.5
    _, v67 = check(shared, name, random_boards(rng, 67), 2, p4)
    check(shared, name, random_boards(rng, 3), 2, other)
    _, v128 = check(shared, name, random_boards(rng, 128), 2, other)
    acts, vals = check(shared, name, crafted_boards(), 2, other)
    assert (vals[0] == R.INT64_MIN).all() and acts[0] == 0  # no legal move
    # a negative value has a negative chance node under it (gains are >= 0): there the floor
    # differs from a truncating division
    v = np.concatenate([v67, v128]).ravel()
    assert ((v < 0) & (v != R.INT64_MIN)).sum() >= 10


@pytest.mark.parametrize("name,p4,n", [("1x1", 0.1, 4), ("8x3", 0.5, 4), ("2x4", 0.5, 16),
                                       ("4x6", 0.1, 8)])
def test_depth_3_bit_for_bit(shared, name, p4, n):
    rng = np.random.default_rng(83)
    boards = np.concatenate([dense_boards(rng, n - 3, max_empty=4),
                             np.array([NEAR, FULL[:15] + [0],
                                       [15, 15, 16, 16, 17, 17, 15, 16, 1, 2, 1, 2, 0, 1, 0, 1]],
                                      np.uint8)])
    check(shared, name, boards, 3, p4)
    check(shared, name, boards[:1], 3, p4)  # n = 1


def test_the_anchors_of_the_definition(NS):
    """The hand-checked numbers of tests/ntsearch_ref.py's docstring, from the kernel."""
    from g2048 import ntuple

    a = dev(np.array([[1, 1] + [0] * 14, NEAR], np.uint8))
    net = ntuple.NTupleNetwork(((0,),), device=DEV)
    net.lut.copy_(1024 * torch.arange(16, dtype=torch.int32, device=DEV)[None])
    m = R.INT64_MIN
    want = {(1, 0.5): [m, 2048, 8192, 8192], (2, 0.5): [m, 9069, 11400, 11400],
            (3, 0.5): [m, 15526, 15865, 15865], (2, 0.1): [m, 8835, 9598, 9598],
            (3, 0.1): [m, 11652, 11975, 11975]}
    near = {1: [m, 10240, m, 10240], 2: [m, 33792, m, 33792], 3: [m, 53205, m, 53205]}
    for (depth, p4), v in want.items():
        acts, vals = net.search(a, depth, p4)
        assert vals[0].tolist() == v and acts.tolist() == [2, 1], (depth, p4)
        if p4 == 0.5:
            assert vals[1].tolist() == near[depth]
    net.lut.copy_((-1000 * torch.arange(16, dtype=torch.int32, device=DEV) - 7)[None])
    for depth, v in ((1, [m, -2056, 40, 40]), (2, [m, -256, 1478, 1478]),
                     (3, [m, 4161, 4654, 4654])):
        assert net.search(a, depth)[1][0].tolist() == v
    zero = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    for depth, v in ((1, [m, 0, 4096, 4096]), (2, [m, 4096, 5734, 5734]),
                     (3, [m, 9006, 9152, 9152])):
        acts, vals = zero.search(a, depth)
        assert vals[0].tolist() == v and acts[0] == 2


# ------------------------------------------------------------------ 2. depth 1 is act
@pytest.mark.parametrize("name,n", [("2x4", 4099), ("4x6", 4099), ("8x3", 2048 * 4 + 64 + 5)])
def test_depth_1_equals_act(shared, name, n):
    """Depth 1 has no chance node: q and action of NTupleNetwork.act.  The largest n is more
    boards than the grid has wavefronts (2048 blocks x 4), so the grid-stride loop runs."""
    net = shared.net(name)
    boards = dev(random_boards(np.random.default_rng(84), n))
    want_a, want_q, _ = net.act(boards)
    for p4 in (0.5, 0.1):
        acts, vals = net.search(boards, 1, p4)
        assert torch.equal(vals, want_q) and torch.equal(acts, want_a)


# ------------------------------------------------------------------ 3. zero table
def test_zero_table_is_the_gain_and_ties_go_to_the_smallest_move(NS):
    from g2048 import ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    boards = np.concatenate([random_boards(np.random.default_rng(85), 200), crafted_boards()])
    acts, vals = net.search(dev(boards), 1)
    acts, vals = acts.cpu().numpy(), vals.cpu().numpy()
    for i, b in enumerate(boards):
        gains = []
        for a in range(4):
            after, gain = NR.E.move(b, a)
            gains.append(gain << NR.F if after != [int(x) for x in b] else None)
        assert [None if x == R.INT64_MIN else int(x) for x in vals[i]] == gains
    # a board symmetric under both flips and the transpose: all four moves are worth the same at
    # every depth, and the smallest move wins
    sym = dev(np.array([[1, 2, 2, 1, 2, 0, 0, 2, 2, 0, 0, 2, 1, 2, 2, 1]], np.uint8))
    for depth in (1, 2, 3):
        acts, vals = net.search(sym, depth)
        v = vals[0].tolist()
        assert v[0] == v[1] == v[2] == v[3] != R.INT64_MIN and acts[0] == 0, depth


# ------------------------------------------------------------------ 4. output variants
def test_output_variants_and_guards(NS, shared):
    """values-only and action-only calls write the same bytes as the full call, nothing around
    either output is touched, and the wrapper fills caller-owned outputs."""
    import ctypes as C

    import g2048._native as N

    net, n, pad = shared.net("2x4"), 67, 64
    boards = dev(random_boards(np.random.default_rng(86), n))
    lib = NS.load()
    V, A = 0x5A5A5A5A5A5A5A5A, 0xA5

    def call(want_values, want_action):
        vbuf = torch.full((pad + 4 * n + pad,), V, dtype=torch.int64, device=DEV)
        abuf = torch.full((pad + n + pad,), A, dtype=torch.uint8, device=DEV)
        rc = lib.g2048_ntsearch_expectimax(
            C.byref(net._c), net.lut.data_ptr(), boards.data_ptr(), n, 2, 0,
            vbuf[pad:].data_ptr() if want_values else None,
            abuf[pad:].data_ptr() if want_action else None, 0,
            torch.cuda.current_stream().cuda_stream)
        assert rc == N.G2048_OK, lib.g2048_ntsearch_last_error()
        torch.cuda.synchronize()
        return vbuf.cpu().numpy(), abuf.cpu().numpy()

    v_full, a_full = call(True, True)
    v_only, a_none = call(True, False)
    v_none, a_only = call(False, True)
    assert np.array_equal(v_only, v_full) and np.array_equal(a_only, a_full)
    assert (a_none == A).all() and (v_none == V).all()
    assert (v_full[:pad] == V).all() and (v_full[pad + 4 * n:] == V).all()
    assert (a_full[:pad] == A).all() and (a_full[pad + n:] == A).all()
    ref_a, ref_v = shared.ref("2x4").root_batch(boards.cpu().numpy(), 2)
    assert np.array_equal(v_full[pad:pad + 4 * n].reshape(n, 4), ref_v)
    assert np.array_equal(a_full[pad:pad + n], ref_a)
    # the wrapper: None for what was not asked for, caller-owned outputs are the ones returned
    acts, vals = net.search(boards, 2, values=False)
    assert vals is None and np.array_equal(acts.cpu().numpy(), ref_a)
    acts, vals = NS.expectimax(net, boards, 2, actions=False)
    assert acts is None and np.array_equal(vals.cpu().numpy(), ref_v)
    out_v = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
    out_a = torch.zeros(n, dtype=torch.uint8, device=DEV)
    acts, vals = net.search(boards, 2, values=False, actions=False, values_out=out_v,
                            actions_out=out_a)
    assert acts is out_a and vals is out_v
    assert np.array_equal(out_v.cpu().numpy(), ref_v) and np.array_equal(out_a.cpu().numpy(), ref_a)
    with pytest.raises(ValueError):
        net.search(boards, 2, values=False, actions=False)
    with pytest.raises(ValueError):
        net.search(boards, 2, values_out=out_v[:5])


# ------------------------------------------------------------------ 5. graph capture
def test_captured_search_and_step_replays(NS, shared):
    """Search + env.step captured once (a linear chain) and replayed 3 times equals 3 eager
    steps."""
    import g2048
    from g2048.dist import graph_capture

    n, seed, net = 192, 87, shared.net("2x4")

    def make():
        env = g2048.VecEnv2048(n, seed=seed, device=DEV)
        out = dict(acts=torch.zeros(n, dtype=torch.uint8, device=DEV),
                   vals=torch.zeros((n, 4), dtype=torch.int64, device=DEV),
                   reward=torch.zeros(n, dtype=torch.int32, device=DEV),
                   done=torch.zeros(n, dtype=torch.uint8, device=DEV),
                   legal=torch.zeros(n, dtype=torch.uint8, device=DEV))

        def fn():
            net.search(env.board, 2, actions_out=out["acts"], values_out=out["vals"])
            env.step(out["acts"], reward=out["reward"], done=out["done"], legal=out["legal"])
        return env, out, fn

    eager_env, eager_out, eager = make()
    want = []
    for _k in range(3):
        eager()
        torch.cuda.synchronize()
        want.append({k: v.cpu().clone() for k, v in eager_out.items()} |
                    {"board": eager_env.board.cpu().clone()})

    env, out, fn = make()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        fn()
    torch.cuda.synchronize()
    assert not out["vals"].any()  # the capture ran nothing
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        for name, t in out.items():
            assert torch.equal(t.cpu(), want[k][name]), (k, name)
        assert torch.equal(env.board.cpu(), want[k]["board"]), k
    env.check_errors()


# ------------------------------------------------------------------ 6. the player
def test_player_plays_to_the_end_with_the_reference_actions(NS, shared):
    """64 games of play("ntuple_search") at depth 2 and p(4) = 0.1 to the end.  Over the first 6
    steps boards, rewards and actions equal an OracleEnv stepped with the reference's actions
    from the same seed (the player's p4 reaches the chance nodes); no game is left stuck and
    every game ends on a board without a legal move."""
    from g2048.player import BatchedPlayer

    n, steps, seed, net = 64, 6, 88, shared.net("2x4")
    res = BatchedPlayer(n, device=DEV, seed=seed, ntuple=net, search_depth=2, p4=0.1,
                        record_games=n).play("ntuple_search")
    o = O.OracleEnv(n, seed, flags=O.NO_AUTORESET | O.P4_10)
    ref = shared.ref("2x4", 0.1)
    for t, (before, act, reward, score_before, after) in enumerate(res.trace[:steps]):
        assert np.array_equal(before.cpu().numpy(), o.board), t
        want = np.array([ref.root(b, 2)[1] for b in o.board], np.uint8)
        assert np.array_equal(act.cpu().numpy(), want), t
        r = o.step(O.MODE_ACTIONS, actions=want)
        assert np.array_equal(reward.cpu().numpy(), r["reward"]), t
        assert np.array_equal(after.cpu().numpy(), o.board), t
    assert (res.moves > 14).all() and not res.stuck.any()
    for g, h in enumerate(res.histories):
        assert len(h) == res.moves[g] and h[-1][2] == 0 and h[-1][3] == res.merge_score[g]
        last = np.where(h[-1][0] > 0, np.log2(np.maximum(h[-1][0], 1)), 0).astype(np.uint8)
        assert O.legal_mask(last.reshape(16)) == 0


# ------------------------------------------------------------------ 7. strength
def test_search_is_at_least_as_strong_as_the_greedy_policy(NS):
    """TUPLES_2x4 trained as tests/test_ntuple_gpu.py::test_self_play_learns trains it (256
    boards, 4000 steps, seed 61), then 256 games of play("ntuple") and of play("ntuple_search")
    at depth 2 on the same seeds: the search's mean merge score is at least the greedy policy's
    on the same table.  Measured on an MI355X: see the printed figures and DESIGN 4.11."""
    from g2048 import ntuple
    from g2048.player import BatchedPlayer

    seed = 61
    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    tr = ntuple.NTupleTrainer(net, 256, seed=seed, p4=0.5, lr_num=1, lr_shift=10, log_slots=64)
    for _chunk in range(4):
        tr.step(1000)
        tr.episodes()
    tr.env.check_errors()
    greedy = BatchedPlayer(256, device=DEV, seed=seed, ntuple=net).play("ntuple")
    deep = BatchedPlayer(256, device=DEV, seed=seed, ntuple=net,
                         search_depth=2).play("ntuple_search")
    g, d = float(greedy.merge_score.mean()), float(deep.merge_score.mean())
    print(f"2x4 after 4000 TD steps, 256 games each: greedy {g:.0f} (mean moves "
          f"{greedy.moves.mean():.0f}, max tile {greedy.max_tile.max()}), depth-2 search {d:.0f} "
          f"(mean moves {deep.moves.mean():.0f}, max tile {deep.max_tile.max()}), ratio "
          f"{d / g:.2f}")
    assert not deep.stuck.any() and not greedy.stuck.any()
    assert d >= g
