"""The wide expectimax (csrc/g2048_deepsearch.hip -> libg2048_deepsearch.so) on the device, int64
values and u8 actions compared with torch.equal: depths 1-3 at every split against the two
existing search libraries; depth 4 with one expanded ply against two; depths 4 and 5 against a
one-ply lift, done on the host, of the library one depth below; the CPU anchors of
tests/test_deepsearch.py; workspaces pre-filled with 0xFF and with random bytes; the wrapper's
chunks; a captured call; the two new player policies; and the strength of depth 4 against
depth 2 on one small trained table."""
import numpy as np
import pytest
import torch

import deepsearch_ref as R
import ntuple_ref as NR
from test_deepsearch import A, BOARDS, CHECKER, DEEP_ANCHORS, NEAR, ONE, ONE_MOVE, table_2x4
from test_ntsearch_gpu import SPECS, crafted_boards, random_table
from test_ntstage_gpu import make_net

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT64_MIN = R.INT64_MIN
UNSET = -(1 << 31)
SIZES = (1, 2, 3, 4, 5, 63, 64, 65, 129, 1031)
F = NR.F


@pytest.fixture(scope="module")
def D():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import deepsearch, ntsearch, ntstage, ntuple, stagesearch
    for mod in (ntuple, ntsearch, ntstage, stagesearch, deepsearch):
        mod.load()
    return deepsearch


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def played_boards(n, seed, steps=40):
    """n boards after `steps` random moves of self-play (finished games restart), the crafted
    boards of the search tests written over the first ones where there is room."""
    import g2048

    env = g2048.VecEnv2048(n, seed=seed, device=DEV)
    env.rollout(steps)
    torch.cuda.synchronize()
    env.check_errors()
    boards = env.board.clone()
    if n >= 129:
        c = dev(crafted_boards())
        c = c[(c <= R.MAX_EXPONENT).all(dim=1)]
        boards[:len(c)] = c
    return boards


class Shared:
    """One randomly filled network per spec and the played boards, built once and only read."""

    def __init__(self):
        self.nets, self.boards = {}, {}

    def net(self, name):
        if name not in self.nets:
            self.nets[name] = random_table(SPECS[name], 171 + len(self.nets))
        return self.nets[name]

    def played(self, n):
        if n not in self.boards:
            self.boards[n] = played_boards(n, 500 + n)
        return self.boards[n]


@pytest.fixture(scope="module")
def shared(D):
    return Shared()


def same(got, want, what):
    assert torch.equal(got[1], want[1]), f"{what}: values differ"
    assert torch.equal(got[0], want[0]), f"{what}: actions differ"


# ------------------------------------------------------------------ 1. depths 1-3, every split
@pytest.mark.parametrize("name", list(SPECS))
def test_depths_1_to_3_equal_the_single_table_search_at_every_split(D, shared, name):
    net = shared.net(name)
    for n in SIZES:
        boards = shared.played(n)
        for depth in (1, 2, 3):
            want = net.search(boards, depth)
            for top in D.legal_tops(depth):
                same(D.expectimax(net, boards, depth, top=top), want, (name, n, depth, top))
    boards = shared.played(65)
    for depth in (2, 3):  # both p(4)
        want = net.search(boards, depth, 0.1)
        for top in D.legal_tops(depth):
            same(net.deep_search(boards, depth, 0.1, top), want, (name, depth, top, 0.1))


@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count(D, shared, T):
    net = random_table(SPECS["8x3"][:T], 190 + T)
    boards = shared.played(129)
    for depth in (1, 2, 3):
        want = net.search(boards, depth)
        for top in D.legal_tops(depth):
            same(D.expectimax(net, boards, depth, top=top), want, (T, depth, top))


def staged_net(S, kind, seed):
    """S stages over the 2x4 set; the top stage fresh (no UNSET), half-set or all UNSET."""
    from g2048 import ntstage

    bounds = {1: (), 2: (5,), 3: (5, 8)}[S]
    net = make_net(ntstage, NR.TUPLES_2x4, bounds, seed, upper=0.5 if kind == "half" else 1.0)
    if kind == "unset" and S > 1:
        net.lut[S - 1].fill_(UNSET)
    return net


@pytest.mark.parametrize("kind", ["fresh", "half", "unset"])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_depths_1_to_3_equal_the_staged_search_at_every_split(D, shared, S, kind):
    net = staged_net(S, kind, 600 + S)
    top_stage = net.lut[S - 1]
    if S > 1:
        share = float((top_stage == UNSET).float().mean())
        assert {"fresh": share == 0, "half": 0.4 < share < 0.6, "unset": share == 1}[kind]
    for n in (1, 5, 65, 129, 1031):
        boards = shared.played(n)
        for depth, p4 in ((1, 0.5), (2, 0.1), (3, 0.5)):
            want = net.expectimax(boards, depth, p4)
            for top in D.legal_tops(depth):
                same(D.expectimax(net, boards, depth, p4, top=top), want, (S, kind, n, depth, top))


# ------------------------------------------------------------------ 2. depths 4 and 5
def test_depth_4_with_one_expanded_ply_equals_two(D, shared):
    for name in ("2x4", "4x6"):
        net = shared.net(name)
        for n, p4 in ((1, 0.5), (5, 0.1), (129, 0.5)):
            boards = shared.played(n)
            same(D.expectimax(net, boards, 4, p4, top=1), D.expectimax(net, boards, 4, p4, top=2),
                 (name, n, p4))
    net = staged_net(3, "half", 611)
    boards = shared.played(129)
    same(D.expectimax(net, boards, 4, top=1), D.expectimax(net, boards, 4, top=2), "staged")


def lift(boards, below, p4):
    """One ply on the host over `below(children) -> values i64 [m, 4]`, the search one depth
    less: a child's Vmax is the largest of its legal values (0 with none), a move's value the
    gain plus the floored, weighted mean over the spawns, in Python integers."""
    W, w4 = (2, 1) if p4 == 0.5 else (10, 1)
    rows, children = [], []
    for i, b in enumerate(boards.cpu().numpy()):
        for a in range(4):
            after, gain = NR.E.move(b, a)
            if list(after) == [int(x) for x in b]:
                continue
            cells = [c for c in range(16) if after[c] == 0]
            rows.append((i, a, gain, len(cells), len(children)))
            for c in cells:
                for e in (1, 2):
                    child = list(after)
                    child[c] = e
                    children.append(child)
    v = below(dev(np.array(children, np.uint8)))
    best = v.amax(dim=1)  # an illegal move holds INT64_MIN, below every legal value
    vmax = torch.where(best != INT64_MIN, best, torch.zeros_like(best)).cpu().tolist()
    vals = np.full((len(boards), 4), INT64_MIN, np.int64)
    for i, a, gain, ne, at in rows:
        total = sum((W - w4) * vmax[at + 2 * k] + w4 * vmax[at + 2 * k + 1] for k in range(ne))
        vals[i, a] = (gain << F) + total // (W * ne)
    acts = np.argmax(vals, axis=1).astype(np.uint8)  # the first of the largest
    return dev(acts), dev(vals, np.int64)


@pytest.mark.parametrize("staged", [False, True], ids=["flat", "staged"])
def test_depths_4_and_5_equal_a_one_ply_lift_of_the_depth_below(D, shared, staged):
    net = staged_net(3, "half", 612) if staged else shared.net("2x4")
    three = net.expectimax if staged else net.search
    boards = shared.played(129)
    for p4 in (0.5, 0.1):
        want4 = lift(boards, lambda c: three(c, 3, p4)[1], p4)
        for top in (1, 2):
            same(D.expectimax(net, boards, 4, p4, top=top), want4, (4, top, p4))
    want5 = lift(boards, lambda c: D.expectimax(net, c, 4, top=1)[1], 0.5)
    same(D.expectimax(net, boards, 5), want5, 5)
    assert D.legal_tops(5) == (2,)


def anchor_net(name):
    from g2048 import ntuple

    net = ntuple.NTupleNetwork(SPECS[name], device=DEV)
    i = np.arange(net.lut.shape[1], dtype=np.int64)
    if name == "1x1":
        net.lut.copy_(dev(1024 * i[None], np.int32))
    else:
        net.lut.copy_(dev(np.stack([table_2x4(t, i) for t in range(2)]), np.int32))
    return net


def test_the_cpu_anchors_at_depths_4_and_5(D):
    """tests/test_deepsearch.py's literals from the kernels, the 15-empty root at depth 5 among
    them, and the cases it names: no legal move, one legal move, a tie."""
    nets = {name: anchor_net(name) for name in ("1x1", "2x4")}
    for (name, p4, board), by_depth in DEEP_ANCHORS.items():
        b = dev(np.array([BOARDS[board]], np.uint8))
        for depth, (values, action) in by_depth.items():
            want = [INT64_MIN if v is None else v for v in values]
            for top in D.legal_tops(depth):
                acts, vals = D.expectimax(nets[name], b, depth, p4, top=top)
                assert vals[0].tolist() == want and int(acts[0]) == action, (name, p4, board, top)
    b = dev(np.array([CHECKER, ONE_MOVE, A, ONE, NEAR], np.uint8))
    for depth in (4, 5):
        acts, vals = D.expectimax(nets["1x1"], b, depth)
        assert vals[0].tolist() == [INT64_MIN] * 4 and acts.tolist() == [0, 2, 2, 1, 1]
        assert (vals[1] != INT64_MIN).tolist() == [False, False, True, False]
        assert vals[2, 2] == vals[2, 3] > vals[2, 1]


def test_129_copies_of_one_board(D, shared):
    net = shared.net("4x6")
    one = shared.played(5)[3:4]
    boards = one.repeat(129, 1).contiguous()
    for depth, top in ((3, 2), (4, 1), (4, 2), (5, 2)):
        acts1, vals1 = D.expectimax(net, one, depth, top=top)
        acts, vals = D.expectimax(net, boards, depth, top=top)
        assert torch.equal(vals, vals1.expand(129, 4)) and torch.equal(acts, acts1.expand(129))


def test_a_staged_board_whose_leaves_lie_in_a_later_stage_than_the_root(D):
    """Bounds (5, 8): the root's largest tile is a 4 (stage 0), one merge makes a 5 (stage 1).
    The stage of a leaf is its own: a table that differs only above stage 0 changes the values."""
    net = staged_net(3, "fresh", 613)
    root = dev(np.array([[4, 4, 3, 0, 1, 2, 0, 0, 0, 1, 0, 0, 0, 0, 0, 2]], np.uint8))
    for depth in (2, 3):
        want = net.expectimax(root, depth)
        for top in D.legal_tops(depth)[1:]:
            same(D.expectimax(net, root, depth, top=top), want, (depth, top))
    four = D.expectimax(net, root, 4, top=1)
    same(D.expectimax(net, root, 4, top=2), four, 4)
    five = D.expectimax(net, root, 5)
    frozen = staged_net(3, "fresh", 613)
    frozen.lut[1:].copy_(frozen.lut[:1].expand(2, -1, -1))  # every stage holds stage 0's table
    assert not torch.equal(D.expectimax(frozen, root, 4)[1], four[1])
    assert not torch.equal(D.expectimax(frozen, root, 5)[1], five[1])


# ------------------------------------------------------------------ 3. the workspace
def test_the_result_does_not_depend_on_what_the_workspace_held(D, shared):
    """Every slot a launch reads is written by the call: a workspace of 0xFF bytes (all
    sentinels) and one of random bytes give the result of the module's own."""
    net = shared.net("2x4")
    boards = shared.played(5)
    g = torch.Generator(device=DEV).manual_seed(7)
    for depth, top in ((2, 1), (3, 1), (3, 2), (4, 1), (4, 2), (5, 2)):
        want = D.expectimax(net, boards, depth, top=top)
        nbytes = D.workspace_bytes(len(boards), top)
        for fill in ("ff", "random", "zero"):
            if fill == "random":
                ws = torch.randint(0, 256, (nbytes,), generator=g, device=DEV, dtype=torch.uint8)
            else:
                ws = torch.full((nbytes,), 0xFF if fill == "ff" else 0, dtype=torch.uint8,
                                device=DEV)
            same(D.expectimax(net, boards, depth, top=top, workspace=ws), want, (depth, top, fill))


def test_chunked_boards_equal_one_unchunked_call(D, shared):
    net = shared.net("2x4")
    boards = shared.played(1031)
    for depth, top in ((3, 1), (4, 1), (3, 2)):
        whole = torch.empty(D.workspace_bytes(1031, top), dtype=torch.uint8, device=DEV)
        want = D.expectimax(net, boards, depth, top=top, workspace=whole)
        del whole
        small = torch.empty(D.workspace_bytes(100, top) + 17, dtype=torch.uint8, device=DEV)
        assert len(D.chunks(1031, top, small.numel())) == 11
        same(D.expectimax(net, boards, depth, top=top, workspace=small), want, (depth, top))
        one = torch.empty(D.workspace_bytes(1, top), dtype=torch.uint8, device=DEV)
        same(D.expectimax(net, boards[:65], depth, top=top, workspace=one),
             (want[0][:65], want[1][:65]), (depth, top, "one board per call"))
    # the module's own workspace: 1 031 boards at top 2 are two calls under its cap
    assert len(D.chunks(1031, 2)) == 2
    same(D.expectimax(net, boards, 3, top=2), want, "module workspace")
    with pytest.raises(ValueError, match="workspace"):
        D.expectimax(net, boards, 4, top=2, workspace=torch.empty(64, dtype=torch.uint8,
                                                                  device=DEV))


def test_a_captured_call_replays(D, shared):
    """Depth 4 with two expanded plies is five launches in one chain: captured once, replayed
    twice on changed boards."""
    from g2048.dist import graph_capture

    net, n = shared.net("2x4"), 65
    src = shared.played(129)
    boards = src[:n].clone()
    acts = torch.zeros(n, dtype=torch.uint8, device=DEV)
    vals = torch.zeros((n, 4), dtype=torch.int64, device=DEV)
    ws = torch.empty(D.workspace_bytes(n, 2), dtype=torch.uint8, device=DEV)
    want = [D.expectimax(net, src[k:k + n].contiguous(), 4, top=2) for k in (0, 64)]
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        D.expectimax(net, boards, 4, top=2, values_out=vals, actions_out=acts, workspace=ws)
    torch.cuda.synchronize()
    assert not vals.any()  # the capture ran nothing
    for k, w in zip((0, 64), want):
        boards.copy_(src[k:k + n])
        g.replay()
        torch.cuda.synchronize()
        same((acts, vals), w, k)


# ------------------------------------------------------------------ 4. the player
@pytest.fixture(scope="module")
def trained(D):
    """TUPLES_2x4 trained as tests/test_ntuple_gpu.py::test_self_play_learns trains it: 256
    boards, 4 000 TD steps, seed 61."""
    from g2048 import ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
    tr = ntuple.NTupleTrainer(net, 256, seed=61, p4=0.5, lr_num=1, lr_shift=10, log_slots=64)
    for _chunk in range(4):
        tr.step(1000)
        tr.episodes()
    tr.env.check_errors()
    return net


def test_the_deep_policies_play_the_games_of_the_search_policies(D, trained):
    from g2048 import ntstage
    from g2048.player import BatchedPlayer

    def play(net, policy, depth=2):
        return BatchedPlayer(8, device=DEV, seed=62, ntuple=net, search_depth=depth).play(policy)

    a, b = play(trained, "ntuple_deep"), play(trained, "ntuple_search")
    assert np.array_equal(a.merge_score, b.merge_score) and np.array_equal(a.moves, b.moves)
    assert np.array_equal(a.max_tile, b.max_tile) and not a.stuck.any() and (a.moves > 14).all()
    staged = ntstage.StagedNTupleNetwork.from_network(trained, (5, 8))
    a, b = play(staged, "ntstage_deep"), play(staged, "ntstage_search")
    assert np.array_equal(a.merge_score, b.merge_score) and np.array_equal(a.moves, b.moves)
    with pytest.raises(ValueError, match="search_depth"):
        play(trained, "ntuple_search", 4)


def test_depth_4_is_at_least_as_strong_as_depth_2(D, trained):
    """64 games each of play("ntuple_deep") at depths 2 and 4 on the same table and seeds: the
    mean merge score of depth 4 is at least that of depth 2.  Measured on an MI355X: see the
    printed figures and DESIGN 4.21."""
    from g2048.player import BatchedPlayer

    two = BatchedPlayer(64, device=DEV, seed=61, ntuple=trained, search_depth=2).play("ntuple_deep")
    four = BatchedPlayer(64, device=DEV, seed=61, ntuple=trained,
                         search_depth=4).play("ntuple_deep")
    s2, s4 = float(two.merge_score.mean()), float(four.merge_score.mean())
    print(f"2x4 after 4000 TD steps, 64 games each: depth 2 {s2:.0f} (mean moves "
          f"{two.moves.mean():.0f}, max tile {two.max_tile.max()}), depth 4 {s4:.0f} (mean moves "
          f"{four.moves.mean():.0f}, max tile {four.max_tile.max()}), ratio {s4 / s2:.2f}")
    assert not two.stuck.any() and not four.stuck.any()
    assert s4 >= s2
