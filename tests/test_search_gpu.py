"""The expectimax search kernel (csrc/g2048_search.hip -> libg2048_search.so) against the plain
Python restatement tests/expectimax_ref.py: values and actions bit for bit on crafted and random
boards, the output variants, the searching player and the replay pre-fill against the oracle env
stepped with the reference's actions, a captured search + step, and a strength sanity check."""
import numpy as np
import pytest
import torch

import expectimax_ref as R
from boards import mask_boards
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

A = [1, 1] + [0] * 14
B = [1, 2, 3, 4, 8, 7, 6, 5, 1, 2, 3, 4, 2, 1, 2, 0]
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
D = [11, 10, 9, 8, 4, 5, 6, 7, 3, 2, 1, 1, 0, 0, 0, 0]
# a full board without equal neighbours, for the one-legal-axis / one-legal-direction boards
T = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 1]


def _with(board, **cells):
    b = list(board)
    for k, v in cells.items():
        b[int(k[1:])] = v
    return b


def crafted_boards():
    out = [A, B, CHECKER, D]
    out += [_with([0] * 16, c0=1), _with([0] * 16, c6=2), _with([0] * 16, c15=7)]  # 15 empties
    # full boards whose only legal moves are the two directions of one equal pair
    out += [_with(T, c1=1), _with(T, c4=1), _with(T, c14=15), _with(T, c11=8)]
    # one legal move: the terminal pattern with one empty edge row / column
    out += [_with(T, c0=0, c1=0, c2=0, c3=0), _with(T, c12=0, c13=0, c14=0, c15=0),
            _with(T, c0=0, c4=0, c8=0, c12=0), _with(T, c3=0, c7=0, c11=0, c15=0)]
    # a hole in a terminal pattern; exponents 15-17 (the largest a 4x4 game reaches)
    out += [_with(T, c5=0), _with(T, c15=0), _with(T, c15=2)]
    out += [[17, 16, 15, 15, 16, 15, 0, 0, 3, 2, 1, 0, 0, 0, 0, 1],
            [15, 15, 16, 16, 17, 17, 15, 16, 1, 2, 1, 2, 0, 1, 0, 1],
            [16, 16, 17, 0, 15, 15, 15, 15, 2, 1, 2, 1, 1, 2, 1, 2]]
    # tiles past 2^27: merge gains beyond 32 bits
    out += [[30, 30, 30, 30, 29, 29, 28, 28, 30, 1, 30, 1, 27, 27, 27, 27],
            [28, 28, 29, 29, 30, 3, 30, 2, 1, 2, 1, 2, 2, 1, 2, 1]]
    return np.array(out, np.uint8)


def random_boards(rng, n, fills=(0.2, 0.5, 0.8, 1.0), hi=12):
    """Boards of mixed fill levels: a fraction `fill` of the cells holds an exponent 1..hi-1."""
    fill = rng.choice(fills, size=(n, 1))
    return (rng.integers(1, hi, (n, 16)) * (rng.random((n, 16)) < fill)).astype(np.uint8)


def dense_boards(rng, n, max_empty, hi=8):
    """Full boards of exponents 1..hi-1 with 1..max_empty cells emptied."""
    b = rng.integers(1, hi, (n, 16)).astype(np.uint8)
    for row in b:
        row[rng.choice(16, int(rng.integers(1, max_empty + 1)), replace=False)] = 0
    return b


@pytest.fixture(scope="module")
def S():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    from g2048 import search
    search.load()
    return search


def gpu_search(S, boards, depth, p4=0.5, weights=None):
    t = torch.from_numpy(np.ascontiguousarray(boards, dtype=np.uint8)).to(DEV)
    w = None if weights is None else S.SearchWeights(*weights)
    acts, vals = S.expectimax(t, depth, w, p4)
    torch.cuda.synchronize()
    return acts.cpu().numpy(), vals.cpu().numpy()


def check(S, boards, depth, p4=0.5, weights=None):
    acts, vals = gpu_search(S, boards, depth, p4, weights)
    ref_a, ref_v = R.expectimax_batch(boards, depth, weights or R.DEFAULT, p4)
    bad = np.flatnonzero((vals != ref_v).any(axis=1) | (acts != ref_a))
    assert len(bad) == 0, (f"{len(bad)} of {len(boards)} boards differ; first: board "
                           f"{boards[bad[0]].tolist()} got {vals[bad[0]].tolist()} / "
                           f"{acts[bad[0]]} want {ref_v[bad[0]].tolist()} / {ref_a[bad[0]]}")
    return acts, vals


# ------------------------------------------------------------------ values and actions
@pytest.mark.parametrize("p4", [0.5, 0.1])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_crafted_boards(S, depth, p4):
    boards = crafted_boards()
    acts, vals = check(S, boards, depth, p4)
    # the anchors of the definition, spelled out
    if (depth, p4) == (1, 0.5):
        assert vals[0].tolist() == [R.INT64_MIN, 23506, 26982, 26982] and acts[0] == 2
        assert vals[1].tolist() == [R.INT64_MIN, -1000000, R.INT64_MIN, -29696] and acts[1] == 3
    if (depth, p4) == (3, 0.5):  # a tie: the smaller move wins
        assert vals[3].tolist() == [R.INT64_MIN, -25619, 7231, 7231] and acts[3] == 2
    assert (vals[2] == R.INT64_MIN).all() and acts[2] == 0  # the checkerboard: no legal move


def test_every_legal_mask(S):
    """Boards realising all 16 legal masks: an illegal move's value is INT64_MIN, a legal one's
    is not, and the action is a legal move."""
    boards = np.array(mask_boards(), np.uint8)
    acts, vals = check(S, boards, 1)
    masks = np.array([O.legal_mask(b) for b in boards])
    assert len(set(masks.tolist())) == 16
    legal = ((masks[:, None] >> np.arange(4)) & 1).astype(bool)
    assert ((vals != R.INT64_MIN) == legal).all()
    assert (legal[np.arange(len(boards)), acts] | (masks == 0)).all()


@pytest.mark.parametrize("n", [1, 3, 64, 257])
def test_random_boards_depth1(S, n):
    boards = random_boards(np.random.default_rng(100 + n), n)
    check(S, boards, 1, p4=0.5 if n != 3 else 0.1)


@pytest.mark.parametrize("p4", [0.5, 0.1])
def test_random_boards_depth2(S, p4):
    check(S, random_boards(np.random.default_rng(7), 64, fills=(0.5, 0.8, 1.0), hi=10), 2, p4)


def test_random_boards_depth3(S):
    check(S, dense_boards(np.random.default_rng(8), 8, max_empty=4), 3)


def test_random_boards_depth4(S):
    check(S, dense_boards(np.random.default_rng(9), 2, max_empty=2), 4)


def test_non_default_weights(S):
    """Weights far from the defaults, one of them zero, and the largest ones allowed."""
    boards = random_boards(np.random.default_rng(10), 64, hi=9)
    check(S, boards, 1, 0.1, R.Weights(3, 0, 77, 1 << 24, 5, 123456))
    check(S, boards[:16], 2, 0.5, R.Weights(1 << 20, 1 << 24, 1 << 24, 1 << 24, 1 << 24, 1 << 30))


def test_grid_stride_remainder(S):
    """More boards than the grid has wavefronts (2048 blocks x 4): every board still gets its
    result, and a board's result does not depend on where it sits in the batch."""
    base = random_boards(np.random.default_rng(11), 64)
    n = 2048 * 4 + 64 + 5
    boards = np.tile(base, (n // 64 + 1, 1))[:n]
    acts, vals = gpu_search(S, boards, 1)
    ref_a, ref_v = R.expectimax_batch(base, 1)
    idx = np.arange(n) % 64
    assert np.array_equal(vals, ref_v[idx]) and np.array_equal(acts, ref_a[idx])


# ------------------------------------------------------------------ output variants
def test_output_variants_and_sentinels(S):
    """values-only and action-only calls write the same bytes as the full call, and nothing
    around either output is touched."""
    import ctypes as C

    import g2048._native as N

    n, pad = 67, 64
    boards = torch.from_numpy(random_boards(np.random.default_rng(12), n)).to(DEV)
    lib = S.load()

    def call(want_values, want_action):
        vbuf = torch.full((pad + 4 * n + pad,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        abuf = torch.full((pad + n + pad,), 0xA5, dtype=torch.uint8, device=DEV)
        rc = lib.g2048_search_expectimax(
            boards.data_ptr(), n, 2, 0, None,
            vbuf[pad:].data_ptr() if want_values else None,
            abuf[pad:].data_ptr() if want_action else None, 0,
            torch.cuda.current_stream().cuda_stream)
        assert rc == N.G2048_OK, lib.g2048_search_last_error()
        torch.cuda.synchronize()
        return vbuf.cpu().numpy(), abuf.cpu().numpy()

    v_full, a_full = call(True, True)
    v_only, a_none = call(True, False)
    v_none, a_only = call(False, True)
    assert np.array_equal(v_only, v_full) and np.array_equal(a_only, a_full)
    assert (a_none == 0xA5).all() and (v_none == 0x5A5A5A5A5A5A5A5A).all()
    for v in (v_full,):
        assert (v[:pad] == 0x5A5A5A5A5A5A5A5A).all() and (v[pad + 4 * n:] == 0x5A5A5A5A5A5A5A5A).all()
    assert (a_full[:pad] == 0xA5).all() and (a_full[pad + n:] == 0xA5).all()
    ref_a, ref_v = R.expectimax_batch(boards.cpu().numpy(), 2)
    assert np.array_equal(v_full[pad:pad + 4 * n].reshape(n, 4), ref_v)
    assert np.array_equal(a_full[pad:pad + n], ref_a)
    # the Python wrapper: values=False returns None for the values and the same actions
    acts, vals = S.expectimax(boards, 2, values=False)
    assert vals is None and np.array_equal(acts.cpu().numpy(), ref_a)
    assert C.sizeof(S._Weights) == 24


# ------------------------------------------------------------------ player and pre-fill
def test_player_matches_oracle_stepped_with_reference_actions(S):
    """64 games x 40 steps of play("expectimax") at depth 1: boards, rewards and actions equal
    an OracleEnv stepped with the reference's actions from the same seed."""
    from g2048.player import BatchedPlayer

    n, steps, seed = 64, 40, 31
    res = BatchedPlayer(n, device=DEV, seed=seed, search_depth=1, record_games=n,
                        max_moves=steps).play("expectimax")
    assert len(res.trace) == steps
    o = O.OracleEnv(n, seed, flags=O.NO_AUTORESET)
    ref = R.Search()
    for t, (before, act, reward, score_before, after) in enumerate(res.trace):
        assert np.array_equal(before.cpu().numpy(), o.board), t
        want = np.array([ref.root(b, 1)[1] for b in o.board], np.uint8)
        assert np.array_equal(act.cpu().numpy(), want), t
        assert np.array_equal(score_before.cpu().numpy().astype(np.uint32), o.meta[:, 0]), t
        r = o.step(O.MODE_ACTIONS, actions=want)
        assert np.array_equal(reward.cpu().numpy(), r["reward"]), t
        assert np.array_equal(after.cpu().numpy(), o.board), t
    assert not res.stuck.any()


def test_player_plays_games_to_the_end(S):
    """Whole games at depth 1 and p(4) = 0.1: every game ends on a board without a legal move,
    with the reference's bookkeeping (history length = moves, last history score = merge score)."""
    from g2048.player import BatchedPlayer

    res = BatchedPlayer(32, device=DEV, seed=5, search_depth=1, p4=0.1,
                        record_games=2).play("expectimax")
    # a game cannot end before the board is full: 14 spawns after the two dealt tiles
    assert (res.moves > 14).all() and not res.stuck.any()
    for g, h in enumerate(res.histories):
        assert len(h) == res.moves[g] and h[-1][2] == 0 and h[-1][3] == res.merge_score[g]
        last = np.where(h[-1][0] > 0, np.log2(np.maximum(h[-1][0], 1)), 0).astype(np.uint8)
        assert O.legal_mask(last.reshape(16)) == 0


def test_prefill_ring_equals_the_oracle_ring(S):
    n, steps, cap, seed = 64, 8, 512, 77
    rb = S.generate_replay_buffer_using_expectimax(n, steps, cap, depth=1, device=DEV, seed=seed)
    o, orb, ref = O.OracleEnv(n, seed), O.OracleReplay(cap), R.Search()
    for _t in range(steps):
        acts = np.array([ref.root(b, 1)[1] for b in o.board], np.uint8)
        o.step(O.MODE_ACTIONS, actions=acts, replay=orb)
    assert int(rb.count.item()) == int(orb.count[0]) == n * steps
    for name in ("s", "a", "r", "s2", "d"):
        assert np.array_equal(getattr(rb, name).cpu().numpy(), getattr(orb, name)), name
    with pytest.raises(ValueError):
        S.generate_replay_buffer_using_expectimax(64, 8, 500, device=DEV)


def test_captured_search_and_step_replays(S):
    """Search + step captured once (a linear chain) and replayed 3 times equals 3 eager steps."""
    import g2048
    from g2048.dist import graph_capture

    n, seed = 192, 13

    def make():
        env = g2048.VecEnv2048(n, seed=seed, device=DEV)
        out = dict(acts=torch.zeros(n, dtype=torch.uint8, device=DEV),
                   vals=torch.zeros((n, 4), dtype=torch.int64, device=DEV),
                   reward=torch.zeros(n, dtype=torch.int32, device=DEV),
                   done=torch.zeros(n, dtype=torch.uint8, device=DEV),
                   legal=torch.zeros(n, dtype=torch.uint8, device=DEV))

        def fn():
            S.expectimax(env.board, 2, actions_out=out["acts"], values_out=out["vals"])
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
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        for name, t in out.items():
            assert torch.equal(t.cpu(), want[k][name]), (k, name)
        assert torch.equal(env.board.cpu(), want[k]["board"]), k
    env.check_errors()


# ------------------------------------------------------------------ strength
def test_search_beats_the_random_player(S):
    """256 full games at depth 1 against play("random") on the same seeds: a higher mean merge
    score (the CPU prototype gave 12 862 against 841 over 8 games; no ratio is fixed here)."""
    from g2048.player import BatchedPlayer

    s = BatchedPlayer(256, device=DEV, seed=3, search_depth=1).play("expectimax")
    r = BatchedPlayer(256, device=DEV, seed=3).play("random")
    print(f"expectimax depth 1: mean merge score {s.merge_score.mean():.0f}, mean moves "
          f"{s.moves.mean():.0f}, max tile {s.max_tile.max()}; random: {r.merge_score.mean():.0f}")
    assert s.merge_score.mean() > r.merge_score.mean()
    assert not s.stuck.any()
