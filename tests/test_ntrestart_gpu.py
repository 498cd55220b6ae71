"""The restart-pool kernel (csrc/g2048_ntrestart.hip -> libg2048_ntrestart.so) against the plain
Python restatement tests/ntrestart_ref.py, bit for bit after every call: snap, valid, top, turn,
the rotation, board, meta and restored_out.  Crafted arrays at the sizes where the indexing can go
wrong, a played run with its episode log, the trainers with a pool against their own references,
restart=None against the plain loop, a captured step, reproducibility, and that staged self-play
with a pool learns."""
import types

import numpy as np
import pytest
import torch

import ntlambda_ref as LR
import ntrestart_ref as R
import nttc_ref as TR
import ntuple_ref as NR
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U32 = 0xFFFFFFFF
# levels 0, 1, 15 and middle values; L = 1 .. 8 takes the first L (L = 1 gets a second rotation)
BASE = (7, 0, 15, 1, 4, 15, 0, 9)


@pytest.fixture(scope="module")
def G():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X")
    import g2048
    g2048.load_native()
    g2048.ntuple.load()
    g2048.ntrestart.load()
    return g2048


def dev(a, dtype=np.uint8):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def host_state(pool):
    return {"snap": pool.snap.cpu().numpy(), "valid": pool.valid.cpu().numpy().view(np.uint16),
            "top": pool.top.cpu().numpy(), "turn": pool.turn.cpu().numpy().view(np.uint32)}


def load_state(pool, state):
    arrays = R.dense(state)
    pool.snap.copy_(dev(arrays["snap"]))
    pool.valid.copy_(dev(arrays["valid"].view(np.int16), np.int16))
    pool.top.copy_(dev(arrays["top"]))
    pool.turn.copy_(dev(arrays["turn"].view(np.int32), np.int32))


class Pair:
    """A RestartPool on the GPU next to the reference state: `apply` runs both from the env's own
    board / meta / clock / done and compares everything.  `kinds` counts what the boards did."""

    def __init__(self, G, n, levels, stagger=False, state=None):
        self.pool = G.RestartPool(n, levels, device=DEV, stagger=stagger)
        self.levels, self.n = tuple(levels), n
        self.state = R.fresh(n, stagger) if state is None else state
        if state is not None:
            load_state(self.pool, state)
        self.want_snap = R.dense(self.state)["snap"]
        self.kinds = {"capture": {}, "restore": {}, "fallback": {}, "idle": 0}
        self.out = torch.empty(n, dtype=torch.uint8, device=DEV)

    def apply(self, env, done, tag=None):
        board = env.board.cpu().tolist()
        meta = (env.meta.cpu().numpy().view(np.uint32)).tolist()
        clock = [int(c) & ((1 << 64) - 1) for c in env.clock.cpu().tolist()]
        flags = done.cpu().tolist()
        self.out.fill_(77)
        self.pool.apply(env, done, self.out)
        old = self.state
        self.state, wboard, wmeta, back = R.apply(self.levels, old, board, meta, clock, flags)
        for i in range(self.n):
            new = self.state["snap"][i]
            if flags[i]:
                e = self.levels[old["turn"][i] % len(self.levels)]
                kind = self.kinds["restore" if back[i] else "fallback"]
                kind[e] = kind.get(e, 0) + 1
            elif new != old["snap"][i]:
                e = self.state["top"][i]
                self.kinds["capture"][e] = self.kinds["capture"].get(e, 0) + 1
                b, s, moves = new[e]
                self.want_snap[i, e, :16] = b
                self.want_snap[i, e, 16:24] = np.array([s, moves], "<u4").view(np.uint8)
            else:
                self.kinds["idle"] += 1
        got = host_state(self.pool)
        assert np.array_equal(got["snap"], self.want_snap), tag
        assert got["valid"].tolist() == self.state["valid"], tag
        assert got["top"].tolist() == self.state["top"], tag
        assert got["turn"].tolist() == self.state["turn"], tag
        assert self.pool.levels == self.levels
        assert env.board.cpu().tolist() == wboard, tag
        assert env.meta.cpu().numpy().view(np.uint32).tolist() == wmeta, tag
        assert self.out.cpu().tolist() == back, tag
        return wboard, wmeta, back

    def check_dense(self):
        """The incrementally kept image of snap is the reference's own."""
        assert np.array_equal(self.want_snap, R.dense(self.state)["snap"])


# ------------------------------------------------------------------ crafted arrays
def capped_boards(rng, n, caps):
    """Random boards whose largest exponent is exactly caps[i] (>= 1)."""
    b = rng.integers(0, 16, (n, 16)) * (rng.random((n, 16)) < 0.7)
    b = np.minimum(b, np.asarray(caps)[:, None])
    b[np.arange(n), rng.integers(0, 16, n)] = caps
    return b.astype(np.uint8)


def crafted_state(rng, n):
    """A state with random valid bits 1..15, every valid slot a board of that level with random
    u32 score and moves, random top and turn (some turns about to wrap)."""
    valid = [int(v) & 0xFFFE for v in rng.integers(0, 1 << 16, n)]
    snap = []
    for v in valid:
        levels = [e for e in range(16) if (v >> e) & 1]
        boards = capped_boards(rng, len(levels), levels) if levels else []
        snap.append({e: (tuple(int(x) for x in b), int(rng.integers(0, 1 << 32)),
                         int(rng.integers(0, 1 << 32))) for e, b in zip(levels, boards)})
    turn = [int(t) for t in rng.integers(0, 1 << 32, n)]
    for i in range(0, n, 5):
        turn[i] = U32 - (i % 3)
    return {"snap": snap, "valid": valid, "top": [int(t) for t in rng.integers(0, 16, n)],
            "turn": turn}


def crafted_env(rng, n):
    """Boards of every level 1..15 (and, from 8 boards on, one with a 16 and one with a 17, out
    of the domain), random u32 meta, one clock word per 64 boards, each different and some past
    2^32."""
    caps = rng.integers(1, 16, n)
    board = capped_boards(rng, n, caps)
    if n >= 8:
        board[3, 5], board[6, 0] = 16, 17
    meta = rng.integers(0, 1 << 32, (2, n)).astype(np.uint32)
    clock = rng.integers(0, 1 << 34, (n + 63) // 64).astype(np.int64)
    return types.SimpleNamespace(board=dev(board), meta=dev(meta.view(np.int32), np.int32),
                                 clock=dev(clock, np.int64))


def rotations():
    return [BASE[:k] for k in range(1, 9)] + [(0,), (15,), (1,)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_crafted_arrays_every_path_in_one_call(G, n):
    """Every rotation length on crafted state at the sizes of a lone board, a partial wave, the
    clock-group boundary and a second group.  Two calls in a row on the same pool, so the second
    reads what the first wrote.  From 63 boards on, every call has lanes that capture, restore,
    fall back and do nothing."""
    rng = np.random.default_rng(1000 + n)
    total = {"capture": 0, "restore": 0, "fallback": 0, "idle": 0}
    for levels in rotations():
        pair = Pair(G, n, levels, state=crafted_state(rng, n))
        for call in range(2):
            env = crafted_env(rng, n)
            done = dev((rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, n))
            before = {k: (sum(v.values()) if isinstance(v, dict) else v)
                      for k, v in pair.kinds.items()}
            pair.apply(env, done, (levels, call))
            now = {k: (sum(v.values()) if isinstance(v, dict) else v)
                   for k, v in pair.kinds.items()}
            if n >= 63 and any(levels):
                assert all(now[k] > before[k] for k in now), (levels, call, before, now)
        pair.check_dense()
        for k in total:
            v = pair.kinds[k]
            total[k] += sum(v.values()) if isinstance(v, dict) else v
    assert all(total.values()), total  # n = 1: over the rotations, every path


def test_restored_out_may_be_null_and_done_is_any_nonzero_byte(G):
    rng = np.random.default_rng(7)
    n = 70
    state = crafted_state(rng, n)
    pair = Pair(G, n, (5, 0, 9), state=state)
    other = G.RestartPool(n, (5, 0, 9), device=DEV)
    load_state(other, state)
    env = crafted_env(rng, n)
    env2 = types.SimpleNamespace(board=env.board.clone(), meta=env.meta.clone(),
                                 clock=env.clock.clone())
    done = dev(rng.choice([0, 1, 2, 128, 255], n))
    pair.apply(env, done)
    assert other.apply(env2, done) is None
    for name in ("snap", "valid", "top", "turn"):
        assert torch.equal(getattr(other, name), getattr(pair.pool, name)), name
    assert torch.equal(env2.board, env.board) and torch.equal(env2.meta, env.meta)


def test_129_copies_of_one_board_with_different_turns(G):
    """Equal boards, slots and flags; only turn differs, so equal data takes the restore, the
    fresh and the fallback path side by side in every wave."""
    n = 129
    slot5 = (tuple([5, 4, 3] + [0] * 13), 1234, 77)
    slot9 = (tuple([9, 1] + [0] * 14), 99999, 4000)
    state = {"snap": [{5: slot5, 9: slot9} for _ in range(n)],
             "valid": [(1 << 5) | (1 << 9)] * n, "top": [9] * n, "turn": list(range(n))}
    pair = Pair(G, n, (5, 0, 9, 11), state=state)
    fresh = [1, 0, 0, 2] + [0] * 12
    env = types.SimpleNamespace(board=dev([fresh] * n),
                                meta=dev(np.array([[0] * n, [50] * n], np.int32), np.int32),
                                clock=dev([50, 50, 50], np.int64))
    board, meta, back = pair.apply(env, dev([1] * n))
    assert back == [(5, 0, 9, 0)[i % 4] for i in range(n)]
    assert pair.kinds["restore"] == {5: 33, 9: 32} and pair.kinds["fallback"] == {0: 32, 11: 32}
    assert board[0] == list(slot5[0]) and board[1] == fresh and board[2] == list(slot9[0])
    assert meta[0][:4] == [1234, 0, 99999, 0]
    assert meta[1][:4] == [(50 - 77) & U32, 50, (50 - 4000) & U32, 50]
    assert pair.state["top"][:4] == [5, 2, 9, 2]
    # the same 129 boards move on: the copies restored at 5 climb to 6 and capture, the rest idle
    env.board.copy_(dev([[6, 4, 3] + [0] * 13 if i % 4 == 0 else b
                         for i, b in enumerate(board)]))
    env.clock += 3
    pair.apply(env, dev([0] * n))
    assert pair.kinds["capture"] == {6: 33} and pair.kinds["idle"] == 96
    assert pair.state["snap"][0][6] == ((6, 4, 3) + (0,) * 13, 1234, 80)
    pair.check_dense()


# ------------------------------------------------------------------ a played run and its log
class Played:
    """VecEnv2048 under the greedy policy of a zero table (lr = 0), with a pool: every step is
    (td_step, env.step, apply), the pool checked after each one, and the episode log predicted
    from the reference alone."""

    def __init__(self, G, n, seed, levels, steps):
        self.env = G.VecEnv2048(n, seed=seed, device=DEV)
        self.log = self.env.attach_episode_log(64)
        self.net = G.NTupleNetwork(G.TUPLES_2x4, device=DEV)
        self.pair = Pair(G, n, levels)
        kw = dict(device=DEV)
        prev = torch.zeros((n, 16), dtype=torch.uint8, **kw)
        has_prev = torch.zeros(n, dtype=torch.uint8, **kw)
        actions = torch.zeros(n, dtype=torch.uint8, **kw)
        delta = torch.zeros(n, dtype=torch.int32, **kw)
        done = torch.zeros(n, dtype=torch.uint8, **kw)
        board = self.env.board.cpu().tolist()
        meta = self.env.meta.cpu().numpy().view(np.uint32).tolist()
        self.records = []       # (step, board, score, moves, max_exp) the reference predicts
        self.restarted = set()  # (step, board) of logged episodes that began from a snapshot
        from_snapshot = [False] * n
        for t in range(steps):
            self.net.td_step(self.env.board, prev, has_prev, 0, 10, actions, delta)
            self.env.step(actions, done=done)
            # a terminal board does not move: the record is the state the previous apply left
            now = self.env.clock.cpu().tolist()
            for i in np.flatnonzero(done.cpu().numpy()):
                i = int(i)
                self.records.append((now[i >> 6] - 1, i, meta[0][i],
                                     (now[i >> 6] - meta[1][i]) & U32, max(board[i])))
                if from_snapshot[i]:
                    self.restarted.add((now[i >> 6] - 1, i))
            flags = done.cpu().tolist()
            board, meta, back = self.pair.apply(self.env, done, t)
            from_snapshot = [bool(b) if f else s for b, f, s in zip(back, flags, from_snapshot)]
        assert not bool(self.net.lut.any())
        self.env.check_errors()
        self.pair.check_dense()


@pytest.fixture(scope="module")
def played(G):
    return Played(G, 257, 61, (0, 5, 6), 600)


def test_played_run_matches_the_reference_after_every_step(played):
    """VecEnv2048(257, seed 61), zero table, lr = 0, levels (0, 5, 6), 600 steps.  On the CPU
    (the oracle env under the same policy with ntrestart_ref) seed 61 gives 758 finished
    episodes, captures at the levels 1..10 (21, 326, 588, 587, 585, 816, 875, 505, 97, 4), 251
    restores at 5, 175 at 6, and 332 turns of the rotation that start fresh (level 0, the
    fall-back branch).  Under this policy every first game of a board passes 64, so a turn at 5
    or 6 never finds its slot unset -- with seed 61 and with each of the seeds 1..128; the run
    with a level no game reaches, below, has those."""
    kinds = played.pair.kinds
    print(kinds)
    for e in (5, 6):
        assert kinds["capture"].get(e, 0) > 0 and kinds["restore"].get(e, 0) > 0, kinds
    assert kinds["fallback"].get(0, 0) > 0 and kinds["idle"] > 0
    assert set(kinds["restore"]) == {5, 6}
    assert played.pair.pool.counts()[5] == played.pair.pool.counts()[6] == 257


def test_played_run_with_a_level_no_game_reaches_falls_back(G):
    """The same run with levels (13, 5, 0): no game reaches 8192 in 300 steps, so every turn at
    13 finds the slot unset, leaves the fresh board and still advances the rotation."""
    run = Played(G, 257, 61, (13, 5, 0), 300)
    kinds = run.pair.kinds
    print(kinds)
    assert kinds["fallback"].get(13, 0) > 0 and kinds["restore"].get(5, 0) > 0
    assert set(kinds["restore"]) == {5} and run.pair.pool.counts()[13] == 0


def test_played_run_logs_the_whole_virtual_game(played):
    """Every record of the env's episode log has the score, moves and largest tile the reference
    predicts: those of the snapshot's past plus the play since the restart."""
    ep = played.log.read()
    got = sorted(zip(ep["step"].tolist(), ep["board"].tolist(), ep["score"].tolist(),
                     ep["moves"].tolist(), ep["max_exp"].tolist()))
    assert got == sorted(played.records) and len(got) > 257
    assert played.restarted
    # an episode that began from a snapshot at level e >= 5 logs a largest tile of at least 2^e,
    # and some of them log more moves than the whole run has steps since its first restart
    by_key = {(r[0], r[1]): r for r in got}
    assert all(by_key[k][4] >= 5 for k in played.restarted)
    assert any(by_key[k][3] > 0 and by_key[k][2] > 0 for k in played.restarted)


# ------------------------------------------------------------------ the trainers
def table_and_env(tr):
    names = ("prev", "has_prev", "actions", "delta", "err", "reward", "done", "legal")
    out = {k: getattr(tr, k).cpu().clone() for k in names}
    out |= {"lut": tr.net.lut.cpu().clone(), "board": tr.env.board.cpu().clone(),
            "meta": tr.env.meta.cpu().clone(), "ep": tr.env.ep.cpu().clone(),
            "clock": tr.env.clock.cpu().clone()}
    if tr.restart is not None:
        out |= {k: getattr(tr.restart, k).cpu().clone() for k in ("snap", "valid", "top", "turn")}
    return out


def assert_same(a, b, tag=None):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), (tag, k)


def test_restart_none_is_the_plain_loop(G):
    """A trainer built without the keyword and one with restart=None: bit-identical tables and
    env state after 200 steps."""
    def run(**kw):
        tr = G.NTupleTrainer(G.NTupleNetwork(G.TUPLES_2x4, device=DEV), 256, seed=81, **kw)
        assert tr.restart is None
        tr.step(200)
        torch.cuda.synchronize()
        return table_and_env(tr)

    a, b = run(), run(restart=None)
    assert_same(a, b)
    assert bool(a["lut"].any()) and int(a["ep"][:, 0].sum()) > 0


def test_trainer_refuses_a_pool_of_another_size(G):
    net = G.NTupleNetwork(G.TUPLES_2x4, device=DEV)
    with pytest.raises(ValueError):
        G.NTupleTrainer(net, 64, restart=G.RestartPool(65, (0, 5), device=DEV))
    with pytest.raises(ValueError):
        G.NTupleTrainer(net, 64, restart=G.RestartPool(64, (0, 5), device="cpu"))
    with pytest.raises(TypeError):
        G.TCTrainer(net, 64, restart=object())


def make_trainer(G, n, seed, levels, stagger=False, **kw):
    net = G.NTupleNetwork(G.TUPLES_2x4, device=DEV)
    pool = G.RestartPool(n, levels, device=DEV, stagger=stagger)
    return G.NTupleTrainer(net, n, seed=seed, restart=pool, **kw)


def test_two_identical_runs_of_300_steps_with_a_pool(G):
    def run():
        tr = make_trainer(G, 256, 82, (3, 0, 4), stagger=True)
        tr.step(300)
        torch.cuda.synchronize()
        return table_and_env(tr), tr

    (a, tr), (b, _) = run(), run()
    assert_same(a, b)
    turns = a["turn"].to(torch.int64) - torch.arange(256)
    assert int(turns.sum()) == int(a["ep"][:, 0].sum()) > 0
    assert tr.restart.counts()[3] > 0 and tr.restart.counts()[4] > 0
    tr.env.check_errors()


def test_captured_step_with_a_pool_replays(G):
    """(td_step, env.step, apply) captured once and replayed 50 times equals 50 eager
    iterations: table, pool, env and outputs after every one.  The window holds episode ends, so
    the replays restore."""
    from g2048.dist import graph_capture

    def make():
        tr = make_trainer(G, 256, 83, (3, 0, 4))
        tr.step(150)
        torch.cuda.synchronize()
        return tr

    tr = make()
    want = []
    for _k in range(50):
        tr.step(1)
        torch.cuda.synchronize()
        want.append(table_and_env(tr))
    ended = want[-1]["turn"].to(torch.int64).sum() - want[0]["turn"].to(torch.int64).sum()
    assert int(ended) > 0

    tr = make()
    start = table_and_env(tr)
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        tr.step(1)
    torch.cuda.synchronize()
    assert_same(table_and_env(tr), start, "the capture ran nothing")
    for k in range(50):
        g.replay()
        torch.cuda.synchronize()
        assert_same(table_and_env(tr), want[k], k)
    tr.env.check_errors()


class Shadow:
    """The env with a pool on the CPU: the oracle env stepped with the learner reference's
    actions, then ntrestart_ref on its arrays."""

    def __init__(self, n, seed, levels):
        self.n, self.levels = n, levels
        self.env = O.OracleEnv(n, seed)
        self.state = R.fresh(n)
        self.restores = self.ended = 0

    def starts(self, now):
        return [(now[i >> 6] - int(self.env.meta[i, 1])) & U32 for i in range(self.n)]

    def step(self, actions):
        o = self.env.step(O.MODE_ACTIONS, actions=np.array(actions, np.uint8))
        now = [int(c) for c in self.env.clock]
        meta = [[int(x) for x in self.env.meta[:, 0]], self.starts(now)]
        self.state, board, meta, back = R.apply(self.levels, self.state, self.env.board.tolist(),
                                                meta, now, o["done"].tolist())
        self.env.board[:] = np.array(board, np.uint8)
        self.env.meta[:, 0] = np.array(meta[0], np.uint32)
        self.env.meta[:, 1] = np.array([(now[i >> 6] - s) & U32 for i, s in enumerate(meta[1])],
                                       np.uint32)
        self.restores += sum(1 for b in back if b)
        self.ended += int(o["done"].sum())

    def check(self, tr, t):
        got = host_state(tr.restart)
        want = R.dense(self.state)
        for k in want:
            assert np.array_equal(got[k], want[k]), (t, k)
        assert np.array_equal(tr.env.board.cpu().numpy(), self.env.board), t
        now = [int(c) for c in self.env.clock]
        meta = tr.env.meta.cpu().numpy().view(np.uint32)
        assert meta[0].tolist() == self.env.meta[:, 0].tolist() and meta[1].tolist() == \
            self.starts(now), t


def want_lut(touched):
    want = np.zeros((2, 65536), np.int32)
    for (t, i), v in touched.items():
        want[t, i] = v
    return want


def test_tc_trainer_with_a_pool_matches_its_reference(G):
    """TCTrainer on 65 boards with levels (3, 0, 4), 200 steps, next to nttc_ref driving the
    oracle env with ntrestart_ref: actions, prev, has_prev, table, accumulators, pool, boards and
    meta after every step."""
    n, levels = 65, (3, 0, 4)
    net = G.NTupleNetwork(G.TUPLES_2x4, device=DEV)
    tr = G.TCTrainer(net, n, seed=84, restart=G.RestartPool(n, levels, device=DEV))
    lr = (tr.lr_num, tr.lr_shift)
    ref = TR.TC(NR.Net(NR.TUPLES_2x4))
    shadow = Shadow(n, 84, levels)
    prev, has_prev = [[0] * 16 for _ in range(n)], [0] * n
    for t in range(200):
        tr.step(1)
        acts, _errs, deltas = ref.step(shadow.env.board.tolist(), prev, has_prev, *lr)
        shadow.step(acts)
        assert tr.actions.cpu().tolist() == acts and tr.delta.cpu().tolist() == deltas, t
        assert tr.prev.cpu().tolist() == prev and tr.has_prev.cpu().tolist() == has_prev, t
        shadow.check(tr, t)
        if t % 20 == 19:
            assert np.array_equal(net.lut.cpu().numpy(), want_lut(ref.net.touched)), t
            ea = tr.tc.ea.cpu().numpy()
            assert int(ea[..., 1].sum()) == sum(ref.A.values()), t
            assert int(ea[..., 0].sum()) == sum(ref.E.values()), t
    print(f"TC: {shadow.ended} episodes ended, {shadow.restores} restored")
    assert shadow.restores > 0 and ref.net.touched
    tr.env.check_errors()


def test_lambda_trainer_with_a_pool_matches_its_reference(G):
    """TDLambdaTrainer(H = 3) on 65 boards with levels (3, 0, 4), 200 steps, next to
    ntlambda_ref: actions, delta, the ring (hist, head, depth), table, pool, boards and meta after
    every step.  depth = 0 after a terminal board, so no afterstate of the finished game is
    updated from the restored one."""
    n, levels = 65, (3, 0, 4)
    net = G.NTupleNetwork(G.TUPLES_2x4, device=DEV)
    tr = G.TDLambdaTrainer(net, n, horizon=3, lam_shift=1, seed=85,
                           restart=G.RestartPool(n, levels, device=DEV))
    lr = (tr.lr_num, tr.lr_shift)
    ref = LR.Lam(NR.Net(NR.TUPLES_2x4), n, 3, 1)
    shadow = Shadow(n, 85, levels)
    for t in range(200):
        tr.step(1)
        acts, _errs, deltas = ref.step(shadow.env.board.tolist(), *lr)
        shadow.step(acts)
        assert tr.actions.cpu().tolist() == acts and tr.delta.cpu().tolist() == deltas, t
        assert tr.lam.head.cpu().tolist() == ref.head, t
        assert tr.lam.depth.cpu().tolist() == ref.depth, t
        hist = tr.lam.hist.cpu().tolist()
        for i in range(n):
            for k in range(ref.depth[i]):
                assert hist[(ref.head[i] - k) % 3][i] == ref.back(i, k), (t, i, k)
        shadow.check(tr, t)
        if t % 20 == 19:
            assert np.array_equal(net.lut.cpu().numpy(), want_lut(ref.net.touched)), t
    print(f"lambda: {shadow.ended} episodes ended, {shadow.restores} restored")
    assert shadow.restores > 0 and ref.net.touched
    tr.env.check_errors()


# ------------------------------------------------------------------ it learns
def test_staged_self_play_with_a_pool_learns(G):
    """NTupleTrainer on StagedNTupleNetwork(TUPLES_2x4, bounds = (7,)) with levels (0, 7), 256
    boards, seed 61, the default rate, 4000 steps: play("ntuple") over 256 games scores at least
    twice what play("random") scores over 256 games of the same seed, no set entry exceeds 2^28
    and stage 1 holds set entries.  Measured on an MI355X: play("ntuple") 4451 against
    play("random") 880, 4294 and 17 422 set entries in stages 0 and 1, largest |entry| 317 443,
    every board's slots 2..9 set and 71 boards' slot 10."""
    from g2048.ntstage import UNSET
    from g2048.player import BatchedPlayer

    net = G.StagedNTupleNetwork(G.TUPLES_2x4, (7,), device=DEV)
    pool = G.RestartPool(256, (0, 7), device=DEV)
    tr = G.NTupleTrainer(net, 256, seed=61, restart=pool, log_slots=64)
    assert tr.lr_num == 1 and tr.lr_shift == G.ntuple.default_lr_shift(256) == 10
    for _chunk in range(4):
        tr.step(1000)
        tr.episodes()
    tr.env.check_errors()
    random = BatchedPlayer(256, device=DEV, seed=61).play("random")
    played = BatchedPlayer(256, device=DEV, seed=61, ntuple=net).play("ntuple")
    is_set = net.lut != UNSET
    largest = int(torch.where(is_set, net.lut, torch.zeros_like(net.lut)).to(torch.int64)
                  .abs().max())
    print(f"staged 2x4, bounds (7,), levels (0, 7), 4000 steps: play(ntuple) "
          f"{played.merge_score.mean():.0f} against play(random) {random.merge_score.mean():.0f}; "
          f"set entries {net.set_counts()}, largest |entry| {largest}, slots set {pool.counts()}")
    assert not played.stuck.any()
    assert played.merge_score.mean() >= 2 * random.merge_score.mean()
    assert largest <= 1 << 28
    assert net.set_counts()[1] > 0
