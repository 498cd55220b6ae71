"""The on-device n-tuple player (csrc/g2048_ntplay.hip -> libg2048_ntplay.so) against the loop it
replaces: two envs built with equal arguments, one advanced by steps(K), the other by K
iterations of the family's own policy call + env.step.  board, meta, ep, clock, fin and result
are compared with torch.equal: there is no tolerance anywhere.  Then the latch, the guard rows,
the table, a captured call and the two fused policies of the player, game for game."""
import types

import numpy as np
import pytest
import torch

import ntuple_ref as NR
from boards import mask_boards
from test_ntsearch_gpu import random_table
from test_ntstage_gpu import make_net, stage_boards

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M32 = 0xFFFFFFFF
UNSET = -(1 << 31)
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
NEAR = CHECKER[:15] + [0]
FULL = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1]
NS_ = (1, 2, 3, 63, 64, 65, 129)
KS = (1, 2, 7, 33)
KEYS = ("board", "meta", "ep", "clock")
T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import ntplay, ntsearch, ntstage, ntuple, stagesearch
    for m in (ntuple, ntsearch, ntstage, stagesearch, ntplay):
        m.load()
    return g2048


class Shared:
    """One network per name, built on first use, shared by every test, never written."""

    def __init__(self):
        self.nets = {}

    def flat(self, tuples=NR.TUPLES_2x4, seed=501):
        key = ("flat", tuples, seed)
        if key not in self.nets:
            self.nets[key] = random_table(tuples, seed)
        return self.nets[key]

    def staged(self, bounds, kind):
        """Stage 0 random; the top stage free of UNSET, half UNSET or all UNSET."""
        from g2048 import ntstage

        key = ("staged", bounds, kind)
        if key not in self.nets:
            upper = {"set": 1.0, "half": 0.5, "unset": 0.0}[kind]
            net = make_net(ntstage, NR.TUPLES_2x4, bounds, 601 + len(self.nets), upper=0.5)
            if len(bounds):
                g = torch.Generator(device=DEV).manual_seed(77)
                rnd = torch.randint(-(1 << 20), 1 << 20, net.lut[-1].shape, generator=g,
                                    device=DEV, dtype=torch.int32)
                keep = torch.rand(rnd.shape, generator=g, device=DEV) < upper
                net.lut[-1].copy_(torch.where(keep, rnd, torch.full_like(rnd, UNSET)))
            self.nets[key] = net
        return self.nets[key]

    def trained(self):
        """TUPLES_2x4 after 4 000 TD(0) steps of 256 boards, seed 61 (the search tests' table)."""
        from g2048 import ntuple

        if "td" not in self.nets:
            net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device=DEV)
            tr = ntuple.NTupleTrainer(net, 256, seed=61, p4=0.5, lr_num=1, lr_shift=10,
                                      log_slots=64)
            for _chunk in range(4):
                tr.step(1000)
                tr.episodes()
            self.nets["td"] = net
        return self.nets["td"]


@pytest.fixture(scope="module")
def shared(G):
    return Shared()


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def make_env(G, n, autoreset=True, p4=0.5, seed=(7 << 32) | 0x2048, offset=1000, clock=None,
             boards=None):
    """An env with a non-zero board offset and a seed above 2^32; `clock` presets every group's
    clock (the running games then began at that clock), `boards` the boards."""
    env = G.VecEnv2048(n, seed=seed, device=DEV, board_offset=offset, p4=p4, autoreset=autoreset)
    if clock is not None:
        env.clock.fill_(clock)
        env.meta[1].fill_(((clock & M32) + (1 << 31)) % (1 << 32) - (1 << 31))
    if boards is not None:
        env.board.copy_(dev(boards))
    return env


def latch(n):
    return (torch.zeros(n, dtype=torch.uint8, device=DEV),
            torch.zeros((n, 4), dtype=torch.int32, device=DEV))


def host_loop(net, env, K, depth, fin, result):
    """K iterations of the loop the library replaces, with the player's latch in torch."""
    from g2048 import ntsearch, ntstage, stagesearch

    mod = stagesearch if isinstance(net, ntstage.StagedNTupleNetwork) else ntsearch
    p4 = 0.1 if env.flags & 1 else 0.5
    for _ in range(K):
        if depth == 1:
            act = net.act(env.board, q=False)[0]
        else:
            act = mod.expectimax(net, env.board, depth, p4, values=False)[0]
        _, done, _ = env.step(act)
        new = done.bool() & (fin == 0)
        result.copy_(torch.where(new[:, None], env.ep, result))
        fin |= new.to(torch.uint8)


def state(env, fin, result):
    torch.cuda.synchronize()
    return {**{k: getattr(env, k).clone() for k in KEYS}, "fin": fin.clone(),
            "result": result.clone()}


def same(a, b, what=""):
    for k in a:
        if not torch.equal(a[k], b[k]):
            bad = (a[k] != b[k]).nonzero()
            raise AssertionError(f"{what}: {k} differs at {bad[:4].tolist()} "
                                 f"({len(bad)} elements): {a[k][tuple(bad[0])].item()} against "
                                 f"{b[k][tuple(bad[0])].item()}")


def both(G, net, n, K, depth, what="", splits=None, **kw):
    """The fused call(s) on one env, the host loop on its twin; returns the fused state."""
    fused, host = make_env(G, n, **kw), make_env(G, n, **kw)
    (f1, r1), (f2, r2) = latch(n), latch(n)
    for k in splits or (K,):
        net.play_steps(fused, k, depth, f1, r1)
    host_loop(net, host, K, depth, f2, r2)
    fused.check_errors()
    a = state(fused, f1, r1)
    same(a, state(host, f2, r2), f"{what} n={n} K={K} depth={depth} {kw.get('autoreset')}")
    return a


# ------------------------------------------------------------------ 1. state equality
@pytest.mark.parametrize("p4", [0.5, 0.1])
@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_steps_equal_the_move_by_move_loop(G, shared, depth, autoreset, p4):
    """Every n and K of the grid (depth 3 at n <= 65 and K <= 7), on an env with a non-zero
    board offset and a seed above 2^32 whose clocks start 5 below 2^32, so that every window of
    K >= 7 crosses it."""
    net, t0 = shared.flat(), (1 << 32) - 5
    for n in NS_:
        for K in KS:
            if depth == 3 and (n > 65 or K > 7):
                continue
            a = both(G, net, n, K, depth, autoreset=autoreset, p4=p4, clock=t0)
            assert int(a["clock"][0]) == t0 + K and int(a["clock"][-1]) == t0 + K


# ------------------------------------------------------------------ 2. late-game boards
def late_boards():
    """129 boards: live and terminal ones interleaved (boards 2j and 2j + 1 share a wave at depth
    1), boards with a single legal move, boards of every legal mask a few moves from their end."""
    live = ([b for b in mask_boards()][::5][:55] + [NEAR] * 3 + [NEAR[:14] + [0, 0]] * 2
            + [[1, 1] + [0] * 14] * 5)
    out = []
    for j, b in enumerate(live):
        out.append(np.asarray(b, np.uint8))
        out.append(np.asarray(CHECKER if j % 2 else FULL, np.uint8))
    return np.stack(out[:129])


@pytest.mark.parametrize("autoreset", [True, False])
@pytest.mark.parametrize("depth", [1, 2])
def test_terminal_steps_inside_the_window(G, shared, depth, autoreset):
    boards = late_boards()
    n, K = len(boards), 33
    a = both(G, shared.flat(), n, K, depth, "late", autoreset=autoreset, boards=boards, clock=90)
    ep = a["ep"].cpu().numpy()
    assert bool(a["fin"][1::2].all())              # the terminal boards end at the first step
    print(f"late boards, depth {depth}, autoreset {autoreset}: {(ep[::2, 0] > 0).sum()} of "
          f"{len(ep[::2])} live boards ended inside the window")
    assert (ep[::2, 0] > 0).sum() > 0              # and live ones inside the window
    if autoreset:
        # a board dealt again at move k < K plays on: its new game began inside the window
        start = a["meta"][1].cpu().numpy()
        again = (ep[:, 0] > 0) & (start > 91) & (start < 90 + K)
        assert again.sum() > 0 and (a["board"].cpu().numpy()[again] > 0).sum(axis=1).min() >= 2
        assert (ep[1::2, 0] >= 1).all()
    else:
        assert (ep[1::2, 0] == K).all()            # a terminal board ends again at every step
        assert (ep[1::2, 2] == K).all()


# ------------------------------------------------------------------ 3. two calls are one
@pytest.mark.parametrize("autoreset", [True, False])
def test_two_calls_equal_one(G, shared, autoreset):
    boards = late_boards()
    for depth, (k1, k2) in ((1, (5, 28)), (2, (1, 6)), (3, (2, 2))):
        n = 129 if depth < 3 else 33
        both(G, shared.flat(), n, k1 + k2, depth, "split", splits=(k1, k2), autoreset=autoreset,
             boards=boards[:n], clock=(1 << 32) - 3)


# ------------------------------------------------------------------ 4. staged tables
STAGED = [((), "set")] + [(b, k) for b in ((5,), (5, 8)) for k in ("set", "half", "unset")]


@pytest.mark.parametrize("bounds,kind", STAGED)
def test_staged_tables(G, shared, bounds, kind):
    """S = 1..3 with the top stage free of UNSET, half UNSET and all UNSET (a single stage has
    no stage above stage 0), from boards capped just below a bound, so that merges inside the
    window and inside the tree cross it."""
    net = shared.staged(bounds, kind)
    boards = stage_boards(np.random.default_rng(len(bounds)), 65)
    boards[::2] = np.concatenate([late_boards()[:32], boards[:1]])[:33]
    for depth, K in ((1, 33), (2, 7), (3, 2)):
        n = 65 if depth < 3 else 17
        both(G, net, n, K, depth, f"staged {bounds} {kind}", autoreset=depth != 2,
             boards=boards[:n])


# ------------------------------------------------------------------ 5. tuple counts, the 4x6 set
@pytest.mark.parametrize("T", range(1, 9))
def test_every_tuple_count_at_depth_1(G, shared, T):
    net = shared.flat(T8M3[:T], 700 + T)
    both(G, net, 65, 33, 1, f"T={T}", autoreset=False, boards=late_boards()[:65])
    both(G, net, 3, 7, 1, f"T={T}", autoreset=True)


def test_the_4x6_set(G, shared):
    net = shared.flat(NR.TUPLES_4x6, 751)
    both(G, net, 65, 7, 1, "4x6", autoreset=True, p4=0.1)
    both(G, net, 33, 3, 2, "4x6", autoreset=False, boards=late_boards()[:33])


# ------------------------------------------------------------------ 6. the latch
def test_rows_finished_on_entry_keep_their_result(G, shared):
    """Rows with fin = 1 on entry keep result; the others take the ep row of their first terminal
    step, not of a later one."""
    boards = late_boards()
    n, K, net = len(boards), 9, shared.flat()
    env = make_env(G, n, autoreset=False, boards=boards)
    fin, result = latch(n)
    fin[::3] = 1
    result[::3] = 0x5A5A5A5A
    net.play_steps(env, 1, 1, fin, result)
    first = state(env, fin, result)
    net.play_steps(env, K - 1, 1, fin, result)
    last = state(env, fin, result)
    keep = torch.zeros(n, dtype=torch.bool, device=DEV)
    keep[::3] = True
    assert bool((last["result"][keep] == 0x5A5A5A5A).all()) and bool(last["fin"][keep].all())
    term = torch.zeros(n, dtype=torch.bool, device=DEV)
    term[1::2] = True
    rows = term & ~keep
    # a terminal board ended K times; the latch holds the first of them
    assert bool((last["ep"][rows, 0] == K).all())
    assert bool((last["result"][rows, 0] == 1).all())
    assert torch.equal(last["result"][rows], first["ep"][rows])
    assert torch.equal(last["result"][rows, 2], last["ep"][rows, 2] - (K - 1))
    # without a latch the env moves the same way
    twin = make_env(G, n, autoreset=False, boards=boards)
    net.play_steps(twin, K, 1)
    torch.cuda.synchronize()
    for k in KEYS:
        assert torch.equal(getattr(twin, k), last[k]), k


# ------------------------------------------------------------------ 7. guard rows, the table
PATTERN = 0x6B


def guarded(src, guard):
    """A copy of `src` between two guard runs of `guard` elements; returns (buffer, view)."""
    flat = src.reshape(-1)
    buf = torch.full((flat.numel() + 2 * guard,), PATTERN, dtype=src.dtype, device=DEV)
    view = buf[guard:guard + flat.numel()].view(src.shape)
    view.copy_(src)
    return buf, view


@pytest.mark.parametrize("depth", [1, 2])
def test_guard_rows_and_the_table_stay_intact(G, shared, depth):
    """The env's buffers, fin and result laid between guard runs: for every n of the grid the
    call writes inside them what it writes on an env of its own, and nothing outside; the table
    is byte-equal before and after."""
    net = shared.flat()
    before = net.lut.clone()
    for n in NS_:
        K = 7
        boards = late_boards()[:n]
        real = make_env(G, n, autoreset=n % 2 == 0, boards=boards, clock=(1 << 32) - 2)
        fin, result = latch(n)
        bufs, views = {}, {}
        for name, t, g in (("board", real.board, 64), ("meta", real.meta, 16),
                           ("ep", real.ep, 16), ("clock", real.clock, 2), ("fin", fin, 16),
                           ("result", result, 16)):
            bufs[name], views[name] = guarded(t, g)
        fake = types.SimpleNamespace(n=n, seed=real.seed, board_offset=real.board_offset,
                                     flags=real.flags, episode_log=None,
                                     **{k: views[k] for k in KEYS})
        net.play_steps(fake, K, depth, views["fin"], views["result"])
        net.play_steps(real, K, depth, fin, result)
        torch.cuda.synchronize()
        want = {**{k: getattr(real, k) for k in KEYS}, "fin": fin, "result": result}
        for name, g in (("board", 64), ("meta", 16), ("ep", 16), ("clock", 2), ("fin", 16),
                        ("result", 16)):
            assert torch.equal(views[name], want[name]), (n, name)
            assert bool((bufs[name][:g] == bufs[name][:1]).all()), (n, name, "front guard")
            assert bool((bufs[name][-g:] == bufs[name][:1]).all()), (n, name, "back guard")
            assert torch.equal(bufs[name][:1], torch.full_like(bufs[name][:1], PATTERN))
    assert torch.equal(net.lut, before)


# ------------------------------------------------------------------ 8. one board, 129 games
def test_copies_of_one_board_play_different_games(G, shared):
    """129 copies of one board: every copy draws its own spawns (its own Philox subsequence), as
    in the host loop."""
    a = both(G, shared.flat(), 129, 33, 1, "copies", autoreset=False,
             boards=np.tile(np.asarray([1, 1] + [0] * 14, np.uint8), (129, 1)))
    assert len({bytes(b) for b in a["board"].cpu().numpy()}) > 120


# ------------------------------------------------------------------ 9-12. the player
def same_games(a, b):
    for k in ("max_tile", "merge_score", "moves", "stuck"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.histories == [] and a.trace == []


@pytest.mark.parametrize("table", ["random", "trained"])
def test_fused_player_plays_the_games_of_the_move_by_move_player(G, shared, table):
    from g2048.player import BatchedPlayer

    net = shared.flat() if table == "random" else shared.trained()
    kw = dict(device=DEV, seed=61, ntuple=net)
    for p4 in (0.5, 0.1):
        same_games(BatchedPlayer(64, search_depth=1, p4=p4, **kw).play("ntuple_fused"),
                   BatchedPlayer(64, p4=p4, **kw).play("ntuple"))
    fused = BatchedPlayer(64, search_depth=2, **kw).play("ntuple_fused")
    same_games(fused, BatchedPlayer(64, search_depth=2, **kw).play("ntuple_search"))
    assert fused.policy == "ntuple_fused" and (fused.moves > 0).all()
    assert not fused.stuck.any() and len(fused) == 64


def test_fused_staged_player(G, shared):
    from g2048.player import BatchedPlayer

    net = shared.staged((5, 8), "half")
    kw = dict(device=DEV, seed=62, ntuple=net)
    for depth in (1, 2):
        fused = BatchedPlayer(64, search_depth=depth, **kw).play("ntstage_fused")
        same_games(fused, BatchedPlayer(64, search_depth=depth, **kw).play("ntstage_search"))
        assert (fused.moves > 0).all()


def test_max_moves_cuts_games_short(G, shared):
    """max_moves = 40 with check_every = 32: the second call is shortened to 8 moves; games
    unfinished by then keep zeros, in both players."""
    from g2048.player import BatchedPlayer

    kw = dict(device=DEV, seed=63, ntuple=shared.trained(), max_moves=40, check_every=32)
    fused = BatchedPlayer(64, search_depth=1, **kw).play("ntuple_fused")
    same_games(fused, BatchedPlayer(64, **kw).play("ntuple"))
    assert (fused.moves == 0).any() and fused.moves.max() <= 40


def test_record_games_is_refused(G, shared):
    from g2048.player import BatchedPlayer

    with pytest.raises(ValueError, match="record_games"):
        BatchedPlayer(8, device=DEV, ntuple=shared.flat(), record_games=1).play("ntuple_fused")
    env = make_env(G, 4)
    env.attach_episode_log(4)
    with pytest.raises(ValueError, match="episode log"):
        shared.flat().play_steps(env, 1)


# ------------------------------------------------------------------ 13. a captured call
def test_a_captured_call_replayed_on_a_changed_env(G, shared):
    """steps is stream-ordered, allocates nothing and syncs nothing: one captured call, replayed
    after the env's buffers were overwritten, equals the eager call on a twin."""
    net, n, K, depth = shared.flat(), 65, 7, 2
    env, twin = make_env(G, n, autoreset=True), make_env(G, n, autoreset=True)
    (f1, r1), (f2, r2) = latch(n), latch(n)
    net.play_steps(twin, K, depth, f2, r2)  # warm-up of the library on another env
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        net.play_steps(env, K, depth, f1, r1)
    torch.cuda.synchronize()
    # the capture ran nothing; now change both envs the same way and run each once
    boards = dev(late_boards()[:n])
    for e, f, r in ((env, f1, r1), (twin, f2, r2)):
        e.board.copy_(boards)
        e.meta.zero_()
        e.ep.zero_()
        e.clock.fill_((1 << 32) - 3)
        f.zero_()
        r.zero_()
    graph.replay()
    net.play_steps(twin, K, depth, f2, r2)
    same(state(env, f1, r1), state(twin, f2, r2), "captured")
    assert int(env.clock[0]) == (1 << 32) - 3 + K and int(f1.sum()) > 0
