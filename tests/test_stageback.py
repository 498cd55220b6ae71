"""CPU-side checks of backward episode learning on the staged batch-mean TC rule: the Python
restatement (tests/stageback_ref.py) reproduces its hand-computed anchors and has the header's six
consequences next to stagemeantc_ref, and the boundary of libg2048_stageback.so (header == exports
== SIGNATURES, build stamps, argument validation without a GPU, the Python side's refusals, its
save / load and from_state, the store audit and no scratch)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest
import torch

import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR
import stageback_ref as R
import stagemeantc_ref as SMT
from g2048 import stageback as _library

_library.load()  # every test of this file belongs to the library: without it the file fails here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_stageback.h")
NAMES = ["g2048_stageback_acc_bytes", "g2048_stageback_last_error", "g2048_stageback_rate",
         "g2048_stageback_step", "g2048_stageback_traj_bytes"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
ONE = 1 << 16


def corner(bounds, n, L, base_ea=None):
    """Spec ((0,),), lut0[i] = 1024 i, the upper stages UNSET."""
    net = SR.StagedNet(((0,),), bounds, base=lambda st, t, i: 1024 * i if st == 0 else None)
    return R.Backward(net, n, L, base_ea=base_ea)


def set_replay(d, i, episode, gains=None, rep_k=0):
    """Board i's replay buffer: a closed episode of these afterstates (fewer than L)."""
    buf = (d.cur[i] & 1) ^ 1
    for k, b in enumerate(episode):
        d.traj[i][buf][k] = list(b)
        d.gain[i][buf][k] = 0 if gains is None else gains[k]
    d.rep_n[i], d.rep_k[i] = len(episode), rep_k


def table(net):
    return {(s, t, i): v for s, d in enumerate(net.stages) for (t, i), v in d.items()}


def ea_of(d):
    return {k: (d.E[k], d.A[k]) for k in d.A}


def counters(d, i=0):
    return d.cur[i], d.rec[i], d.rep_n[i], d.rep_k[i]


# ------------------------------------------------------------------ the issue's anchors
def _calls_4_to_6(d, call5_rec):
    """Calls 4 and 5 of anchor 1 on the board A, with whatever slots the episode lives in."""
    assert d.step([A], 1, 1) == ([2], [-4096], [-2048], [Q2], [True])
    assert d.last_hits == {(0, 0, 2): (-4096, 2), (0, 0, 0): (-12288, 6)}
    assert d.last_m == {(0, 0, 2): -2048, (0, 0, 0): -2048}
    assert table(d.net) == {(0, 0, 2): 0, (0, 0, 0): -2048}
    assert ea_of(d) == {(0, 0, 2): (-2048, 2048), (0, 0, 0): (-2048, 2048)}
    assert (d.rep_k, d.rec) == ([1], [call5_rec - 1])
    assert d.step([A], 1, 1) == ([2], [4096], [2048], [Q2], [True])
    assert d.last_m == {(0, 0, 2): 2048, (0, 0, 0): 2048}
    assert TR.rate(-2048, 2048) == ONE
    assert table(d.net) == {(0, 0, 2): 2048, (0, 0, 0): 0}
    assert ea_of(d) == {(0, 0, 2): (0, 4096), (0, 0, 0): (0, 4096)}
    assert (d.rep_k, d.rec) == ([2], [call5_rec])


def test_anchor_1_an_episode_of_two_is_replayed_newest_first():
    d = corner((), 1, 4)
    for k in (1, 2):
        assert d.step([A], 1, 1) == ([2], [0], [0], [None], [False])
        assert counters(d) == (0, k, 0, 0) and not d.last_hits
    assert d.traj[0][0][:2] == [Q2, Q2] and d.gain[0][0][:2] == [4, 4]
    assert d.step([CHECKER], 1, 1) == ([0], [0], [0], [None], [False])
    assert counters(d) == (1, 0, 2, 0) and not table(d.net) and not ea_of(d)
    _calls_4_to_6(d, 2)
    before = (table(d.net), ea_of(d))
    assert d.step([A], 1, 1) == ([2], [0], [0], [None], [False])
    assert (table(d.net), ea_of(d)) == before and not d.last_hits
    assert counters(d) == (1, 3, 2, 2)
    assert d.traj[0][1][:3] == [Q2, Q2, Q2] and d.traj[0][0][:2] == [Q2, Q2]


def test_anchor_2_a_longer_episode_keeps_its_last_l():
    d = corner((), 1, 2)
    for _ in range(3):
        d.step([A], 1, 1)
    d.step([CHECKER], 1, 1)
    assert counters(d) == (1, 0, 3, 0) and not table(d.net)
    _calls_4_to_6(d, 2)
    before = (table(d.net), ea_of(d))
    assert d.step([A], 1, 1) == ([2], [0], [0], [None], [False])
    assert (table(d.net), ea_of(d)) == before and counters(d) == (1, 3, 3, 2)


def test_anchor_3_an_episode_ends_while_a_replay_is_active():
    d = corner((), 1, 4)
    for _ in range(3):
        d.step([A], 1, 1)
    d.step([CHECKER], 1, 1)
    assert counters(d) == (1, 0, 3, 0)
    assert d.step([A], 1, 1) == ([2], [-4096], [-2048], [Q2], [True])
    assert counters(d) == (1, 1, 3, 1)
    # the older replay's transition of this call is made, then it is dropped
    assert d.step([CHECKER], 1, 1) == ([0], [4096], [2048], [Q2], [True])
    assert table(d.net) == {(0, 0, 2): 2048, (0, 0, 0): 0}
    assert counters(d) == (0, 0, 1, 0)
    assert d.step([A], 1, 1) == ([2], [-4096], [-2048], [Q2], [True])
    assert d.last_m == {(0, 0, 2): -2048, (0, 0, 0): -2048} and TR.rate(0, 4096) == 0
    assert table(d.net) == {(0, 0, 2): 2048, (0, 0, 0): 0}
    assert ea_of(d) == {(0, 0, 2): (-2048, 6144), (0, 0, 0): (-2048, 6144)}
    assert counters(d) == (0, 1, 1, 1)
    assert d.step([A], 1, 1) == ([2], [0], [0], [None], [False])
    assert counters(d) == (0, 2, 1, 1)


def test_anchor_4_a_terminal_board_at_rec_0():
    d = corner((), 1, 4)
    assert d.step([CHECKER], 1, 1) == ([0], [0], [0], [None], [False])
    assert counters(d) == (0, 0, 0, 0) and not table(d.net) and not d.last_hits
    d.step([A], 1, 1)
    d.step([CHECKER], 1, 1)
    assert counters(d) == (1, 0, 1, 0)
    assert d.step([CHECKER], 1, 1) == ([0], [-4096], [-2048], [Q2], [True])
    assert counters(d) == (1, 0, 1, 1)
    assert d.step([CHECKER], 1, 1) == ([0], [0], [0], [None], [False])
    assert counters(d) == (1, 0, 1, 1)


def test_anchor_5_two_boards_of_different_stages_replay_onto_one_index():
    d = corner((3,), 2, 4)
    set_replay(d, 0, [Q2])
    set_replay(d, 1, [Q3])
    assert d.step([CHECKER, CHECKER], 1, 1) == ([0, 0], [-4096, -6144], [-2048, -3072], [Q2, Q3],
                                                [True, True])
    assert d.net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(d.net) == {(0, 0, 2): 0, (0, 0, 0): -2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    assert ea_of(d)[(0, 0, 0)] == (-2048, 2048) and ea_of(d)[(1, 0, 0)] == (-3072, 3072)
    assert d.rep_k == [1, 1] and d.rec == [0, 0] and d.cur == [0, 0]


def test_anchor_6_unset_entries_are_promoted_and_moved_in_one_call():
    d = corner((2,), 1, 4)
    d.step([A], 1, 1)
    d.step([CHECKER], 1, 1)
    assert not table(d.net) and not d.net.promoted
    assert d.step([CHECKER], 1, 1) == ([0], [-4096], [-2048], [Q2], [True])
    assert d.net.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0}
    assert table(d.net) == {(1, 0, 2): 0, (1, 0, 0): -2048}


def test_anchor_7_deltas_that_cancel_leave_the_entry_and_its_ea():
    d = corner((), 2, 4, base_ea=lambda s, t, i: (5, 9) if (s, t, i) == (0, 0, 2) else (0, 0))
    set_replay(d, 0, [Q2])
    set_replay(d, 1, [Q2, Q3], gains=[0, 2], rep_k=1)
    assert d.step([A, A], 1, 0) == ([2, 2], [-4096, 4096], [-4096, 4096], [Q2, Q2], [True, True])
    assert d.last_hits == {(0, 0, 2): (0, 4), (0, 0, 0): (0, 12)}
    assert d.last_m == {(0, 0, 2): 0, (0, 0, 0): 0}
    assert not table(d.net) and not ea_of(d) and d.get_ea(0, 0, 2) == (5, 9)
    assert d.rep_k == [1, 2] and d.rec == [1, 1]


# ------------------------------------------------------------------ consequences, on the reference
T3 = ((0, 1), (1, 5), (2, 7))
BOUNDS = {1: (), 2: (5,), 3: (5, 8)}


def _boards(rng, n, hi=10, fill=0.6):
    return [[rng.randrange(1, hi) if rng.random() < fill else 0 for _ in range(16)]
            for _ in range(n)]


def _staged(rng, n, fill=0.6):
    return [_boards(rng, 1, hi=(5, 8, 11)[k % 3], fill=fill)[0] for k in range(n)]


def _base(seed, S, T, m, upper=None):
    rng = random.Random(seed)
    vals = [[[rng.randrange(-(1 << 20), 1 << 20) for _ in range(16 ** m)] for _ in range(T)]
            for _ in range(S)]
    if upper is not None:
        for s in range(1, S):
            for t in range(T):
                for i in range(16 ** m):
                    if rng.random() >= upper:
                        vals[s][t][i] = SR.UNSET
    return vals


def seeded_ea(seed):
    def ea(s, t, i):
        r = random.Random(seed * 1000003 + s * 7919 + t * 65537 + i)
        a = (0, r.randrange(1, 1 << 16), (1 << 16) + r.randrange(-2, 3),
             r.randrange(1 << 40, 1 << 50))[r.randrange(4)]
        e = (0, a, -a, r.randrange(-a, a + 1))[r.randrange(4)]
        return e, a
    return ea


def _batches(rng, n, calls, period=4):
    """Fresh boards per call; board i is terminal in the calls t with (t + i) % period == period
    - 1, so episodes of period - 1 afterstates close at different times across the batch."""
    out = []
    for t in range(calls):
        boards = _staged(rng, n)
        for i in range(n):
            if (t + i) % period == period - 1:
                boards[i] = list(CHECKER)
        out.append(boards)
    return out


def _state(d):
    return ([[[list(b) for b in buf] for buf in per] for per in d.traj],
            [[list(buf) for buf in per] for per in d.gain], list(d.cur), list(d.rec),
            list(d.rep_n), list(d.rep_k))


@pytest.mark.parametrize("S", [1, 2, 3])
def test_consequence_1_a_call_without_a_replay_only_plays(S):
    rng = random.Random(40 + S)
    base = _base(41 + S, S, 3, 2, upper=0.5)
    n = 12
    d = R.Backward(SR.StagedNet(T3, BOUNDS[S], base=base), n, 8, base_ea=seeded_ea(42))
    plain = SR.StagedNet(T3, BOUNDS[S], base=base)
    for _ in range(3):  # no episode has closed yet
        boards = _staged(rng, n)
        acts, errs, deltas, xs, rep = d.step(boards, 3, 5)
        assert acts == [plain.policy(b)[1] for b in boards]
        assert not any(rep) and not any(errs) and not any(deltas) and xs == [None] * n
        assert not table(d.net) and not ea_of(d) and not d.last_hits and not d.net.promoted
    assert d.rec == [3] * n


@pytest.mark.parametrize("S", [1, 2, 3])
def test_consequence_2_a_replay_of_last_afterstates_is_the_staged_batch_mean_tc_step(S):
    rng = random.Random(50 + S)
    base = _base(51 + S, S, 3, 2, upper=0.5)
    n = 24
    d = R.Backward(SR.StagedNet(T3, BOUNDS[S], base=base), n, 4, base_ea=seeded_ea(52))
    mt = SMT.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base), base_ea=seeded_ea(52))
    xs = _staged(rng, n)
    has = [1 if i % 5 else 0 for i in range(n)]
    for i in range(n):
        if has[i]:
            set_replay(d, i, [_staged(rng, 1)[0], xs[i]])
    boards = _staged(rng, n)  # the backward rule's targets do not depend on the boards played
    _a, errs, deltas, got_x, rep = d.step(boards, 3, 5)
    prev = [list(x) for x in xs]
    want = mt.step([CHECKER] * n, prev, list(has), 3, 5)
    assert (errs, deltas) == want[1:] and rep == [bool(h) for h in has]
    assert [x for x in got_x if x is not None] == [xs[i] for i in range(n) if has[i]]
    assert d.last_hits == mt.last_hits and d.last_m == mt.last_m
    assert d.net.stages == mt.net.stages and d.net.promoted == mt.net.promoted
    assert ea_of(d) == ea_of(mt) and d.A
    assert d.net.promoted or S == 1


def test_consequence_3_an_episode_is_replayed_newest_first_against_the_updated_table():
    """One board, an episode of M afterstates, L = 4: min(M, L) replaying calls that walk j =
    M - 1 .. M - min(M, L), then idling; the target of j is read from the table that holds the
    update of j + 1."""
    for M in (1, 3, 4, 5, 9):
        rng = random.Random(60 + M)
        base = _base(61, 2, 3, 2, upper=0.5)
        d = R.Backward(SR.StagedNet(T3, (5,), base=base), 1, 4)
        episode = _staged(rng, M)
        afters = []
        for b in episode:
            d.step([b], 3, 5)
            afters.append(list(d.traj[0][0][(d.rec[0] - 1) % 4]))
        gains = [R.E.move(list(b), d.net.policy(b)[1])[1] for b in episode]
        d.step([CHECKER], 3, 5)
        assert counters(d) == (1, 0, M, 0)
        for k in range(min(M, 4)):
            j = M - 1 - k
            target = 0 if k == 0 else (gains[j + 1] << 10) + d.net.V(afters[j + 1])
            want = target - d.net.V(afters[j])
            _a, errs, _d, xs, rep = d.step([A], 3, 5)
            assert rep == [True] and xs == [afters[j]] and errs == [want]
        for _ in range(2):
            assert d.step([A], 3, 5)[4] == [False] and not d.last_hits
        assert d.rep_k == [min(M, 4)]


def test_consequence_4_the_hits_of_a_call_and_a_replaced_table():
    """sum of C = 8 T per replaying board with a non-zero delta.  Every upper-stage entry starts
    UNSET and the table is replaced by another one half-way, the state kept: a hit on an UNSET
    entry raises in the reference, so twelve calls without that are consequence 4."""
    rng = random.Random(70)
    n = 24
    d = R.Backward(SR.StagedNet(T3, (5, 8), base=_base(71, 3, 3, 2, upper=0.0)), n, 3)
    seen = 0
    for t, boards in enumerate(_batches(rng, n, 12)):
        if t == 6:
            d.net = SR.StagedNet(T3, (5, 8), base=_base(72, 3, 3, 2, upper=0.0))
        _a, _e, deltas, _x, rep = d.step(boards, 3, 5)
        assert all(r or dl == 0 for r, dl in zip(rep, deltas))
        assert sum(c for _d, c in d.last_hits.values()) == 8 * 3 * sum(1 for x in deltas if x)
        seen += sum(rep)
    assert seen > 3 * n and len(d.net.stages[1]) > 20 and len(d.net.stages[2]) > 20


@pytest.mark.parametrize("S", [2, 3])
def test_consequence_5_e_within_a_order_and_repetition(S):
    rng = random.Random(80 + S)
    base = _base(81, S, 3, 2, upper=0.5)
    n = 20
    batches = _batches(rng, n, 10)
    perm = list(range(n))
    rng.shuffle(perm)
    runs = []
    for k, order in ((1, None), (3, None), (1, perm)):
        d = R.Backward(SR.StagedNet(T3, BOUNDS[S], base=base), n * k, 3, base_ea=seeded_ea(82))
        for boards in batches:
            if order is not None:
                boards = [boards[j] for j in order]
            d.step([list(b) for b in boards] * k, 3, 5)
            assert all(abs(e) <= a for e, a in ea_of(d).values())
        runs.append(d)
    one, three, shuffled = runs
    assert one.A and one.last_hits
    assert one.net.stages == three.net.stages == shuffled.net.stages
    assert ea_of(one) == ea_of(three) == ea_of(shuffled)
    assert all(three.last_hits[k] == (3 * dd, 3 * c) for k, (dd, c) in one.last_hits.items())
    assert _state(three)[2:] == tuple(x * 3 for x in _state(one)[2:])
    assert _state(shuffled)[5] == [_state(one)[5][j] for j in perm]


def test_consequence_6_recording_and_replay_never_share_a_buffer():
    rng = random.Random(90)
    n = 8
    d = R.Backward(SR.StagedNet(T3, (5,), base=_base(91, 2, 3, 2, upper=0.5)), n, 2)
    for boards in _batches(rng, n, 12, period=3):
        before = _state(d)
        rep = [d.replays(i) for i in range(n)]
        d.step(boards, 3, 5)
        after = _state(d)
        for i in range(n):
            read = (before[2][i] & 1) ^ 1
            assert after[0][i][read] == before[0][i][read]  # the buffer a replay reads is kept
            assert after[1][i][read] == before[1][i][read]
            assert rep[i] or before[5][i] == after[5][i] or boards[i] == CHECKER


def test_the_reference_refuses_parameters_outside_the_domain():
    net = SR.StagedNet(T3, ())
    for n, L in ((4, 0), (4, (1 << 20) + 1), (0, 4), ((1 << 11) + 1, 1 << 20)):
        with pytest.raises(ValueError):
            R.Backward(net, n, L)
    R.Backward(net, 4, 1)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (deepsearch, ntlambda, ntmean, ntmeantc, ntrestart, ntsearch, ntstage, nttc,
                       ntuple, search, stagedelay, stagemean, stagemeantc, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean, ntmeantc, stagemeantc, deepsearch, stagedelay)


def test_header_equals_exports_equals_signatures():
    from g2048 import stageback

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = stageback.load()
    assert set(names) == set(stageback.SIGNATURES)
    assert _exported(stageback.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_stageback_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(stageback.SIGNATURES["g2048_stageback_step"][1]) == 23
    # g2048_stagemeantc_step's arguments with the trajectory in the place of prev / has_prev and
    # the three hand-over outputs before err
    args = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    tc = open(os.path.join(ROOT, "include", "g2048_stagemeantc.h")).read()
    tc_args = [a.split()[-1].lstrip("*") for a in
               re.search(r"g2048_stagemeantc_step\((.*?)\);", tc, re.S).group(1).split(",")]
    k, e = tc_args.index("prev_dev"), tc_args.index("err_out_dev")
    assert args == (tc_args[:k] + ["traj_dev", "gain_dev", "cur_dev", "rec_dev", "rep_n_dev",
                                   "rep_k_dev", "horizon"] + tc_args[k + 2:e]
                    + ["x_out_dev", "replay_out_dev"] + tc_args[e:])
    for name, value in (("MAX_HORIZON", "(1 << 20)"), ("RATE_BITS", "16")):
        assert f"#define G2048_STAGEBACK_{name} {value}" in src
        assert getattr(stageback, name) == eval(value)
    assert "#define G2048_STAGEBACK_MAX_SLOTS ((int64_t)1 << 31)" in src
    assert stageback.MAX_SLOTS == 1 << 31
    # the other fifteen libraries keep their ABI: none of the new symbols
    assert len(_others()) == 15
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_stageback")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import stageback

    out = subprocess.run(["readelf", "-d", stageback.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other fifteen stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash(), G.deepsearch_source_hash(), G.stagedelay_source_hash(),
            G.stageback_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS, G.NTMEAN_SHARED,
                  G.STAGEMEAN_SRCS, G.NTMEANTC_SRCS, G.STAGEMEANTC_SRCS, G.DEEPSEARCH_SRCS,
                  G.STAGEDELAY_SRCS):
        assert set(G.STAGEBACK_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.STAGEBACK_SRCS[0]))
    assert open(G.STAGEBACK_STAMP).read().strip() == G.stageback_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.STAGEMEANTC_STAMP).read().strip() == G.stagemeantc_source_hash()
    assert open(G.STAGEDELAY_STAMP).read().strip() == G.stagedelay_source_hash()
    assert len(set(_hashes(G))) == 16


def test_stamp_follows_its_source_the_shared_headers_and_the_four_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp -- source_hash() included, which
    lists the file among the sources with stamps of their own; a change to each shared csrc header
    it includes changes the new stamp; a change to each of g2048.h, g2048_ntuple.h,
    g2048_ntstage.h and g2048_stageback.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.STAGEBACK_SRCS[0])).read()
    includes = re.findall(r'#include\s+"([^"]+)"', src)
    assert includes == ["../../include/g2048_stageback.h", "g2048_board.hpp", G.NTUPLE_SHARED[0],
                        G.NTSTAGE_SHARED[0], G.NTMEAN_SHARED[0]]
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.STAGEBACK_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:15] == before[:15] and after[15] != before[15]
    last = after
    for shared in (G.NTMEAN_SHARED[0], G.NTUPLE_SHARED[0], G.NTSTAGE_SHARED[0],
                   "g2048_board.hpp"):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
        now = _hashes(G)
        assert now[15] != last[15] and now[12] != last[12], shared  # the thirteenth follows too
        if shared != "g2048_board.hpp":  # that one the main library includes too
            assert now[0] == before[0]
        last = now
    shared, include = last, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntstage.h",
                                "g2048_stageback.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[15] != shared[15] and now[15] != last[15], header
        if header == "g2048_stageback.h":
            assert now[:15] == shared[:15]
        last = now


def test_kernels_have_no_store_data_hazard_and_no_scratch(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's flags,
    as the other libraries' tests audit theirs; and none of the 24 kernels (policy, gather and
    apply for T = 1..8) uses scratch."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.STAGEBACK_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", open(out).read())
        assert len(sizes) == 24 and set(sizes) == {"0"}


def _spec(tuples, n_tuples=None, n_cells=None):
    from g2048 import ntuple

    s = ntuple._Spec(len(tuples) if n_tuples is None else n_tuples,
                     len(tuples[0]) if n_cells is None else n_cells)
    for t, cells in enumerate(tuples):
        for k, c in enumerate(cells):
            s.cells[t][k] = c
    return s


def _stages(bounds, n_stages=None):
    from g2048 import ntstage

    s = ntstage._Stages(len(bounds) + 1 if n_stages is None else n_stages)
    for k, b in enumerate(bounds):
        s.bounds[k] = b
    return s


def test_acc_bytes_rate_and_traj_bytes():
    import g2048._native as N
    from g2048 import stageback, stagemeantc

    lib, tc = stageback.load(), stagemeantc.load()
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6):
        for bounds in ((), (11,), (5, 8), tuple(range(1, 8))):
            want = 16 * (len(bounds) + 1) * len(tuples) * 16 ** len(tuples[0])
            assert lib.g2048_stageback_acc_bytes(C.byref(_spec(tuples)),
                                                 C.byref(_stages(bounds))) == want
            assert stageback.acc_bytes(tuples, bounds) == want
    assert lib.g2048_stageback_acc_bytes(None, C.byref(_stages(()))) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_stageback_last_error()
    assert lib.g2048_stageback_acc_bytes(C.byref(_spec(NR.TUPLES_2x4)), None) == N.G2048_EINVAL
    assert b"stages" in lib.g2048_stageback_last_error()
    with pytest.raises(ValueError):
        stageback.acc_bytes(NR.TUPLES_2x4, (8, 5))
    rng = random.Random(8)
    for a in (0, 1, 3, 255, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, 1 << 31, (1 << 40) + 12345,
              (1 << 62) - 1):
        for e in {0, a, -a, a // 3} | {rng.randrange(-a, a + 1) for _ in range(6)}:
            want = TR.rate(e, a)
            assert lib.g2048_stageback_rate(e, a) == want == tc.g2048_stagemeantc_rate(e, a)
            assert stageback.rate(e, a) == want == stageback.BackwardState.rate(e, a)
    for e, a, word in ((0, -1, b"A ="), (0, 1 << 62, b"A ="), (2, 1, b"exceeds"),
                       (-(1 << 63), 5, b"exceeds")):
        assert lib.g2048_stageback_rate(e, a) == N.G2048_EINVAL
        assert word in lib.g2048_stageback_last_error()
        assert b"stageback_rate" in lib.g2048_stageback_last_error()
        with pytest.raises(ValueError):
            stageback.rate(e, a)
    for n, L in ((1, 1), (7, 3), (4096, 8192), (2048, 1 << 20), (1 << 30, 2)):
        assert lib.g2048_stageback_traj_bytes(n, L) == 32 * n * L == stageback.traj_bytes(n, L)
    for n, L, word in ((0, 4, b"n ="), (N.MAX_BOARDS + 1, 1, b"n ="), (4, 0, b"horizon"),
                       (4, -1, b"horizon"), (4, (1 << 20) + 1, b"horizon"),
                       (2049, 1 << 20, b"n * horizon"), ((1 << 30) + 1, 2, b"n * horizon")):
        assert lib.g2048_stageback_traj_bytes(n, L) == N.G2048_EINVAL
        msg = lib.g2048_stageback_last_error()
        assert word in msg and b"stageback_traj_bytes" in msg
        with pytest.raises(ValueError):
            stageback.traj_bytes(n, L)


FAKE, FAKE_EA = 1 << 20, 1 << 30  # aligned addresses that stand in for device memory


def _step(lib, spec, stages, lut=FAKE, acc=FAKE, ea=FAKE_EA, boards=FAKE, n=4, traj=FAKE,
          gain=FAKE, cur=FAKE, rec=FAKE, rep_n=FAKE, rep_k=FAKE, horizon=3, lr_num=1, lr_shift=10,
          action=FAKE, delta=FAKE, x=FAKE, replay=FAKE, err=FAKE):
    return lib.g2048_stageback_step(C.byref(spec) if spec is not None else None,
                                    C.byref(stages) if stages is not None else None, lut, acc,
                                    ea, boards, n, traj, gain, cur, rec, rep_n, rep_k, horizon,
                                    lr_num, lr_shift, action, delta, x, replay, err, 1 << 20, None)


BAD_SPECS = [
    (dict(tuples=((0,),), n_tuples=0), b"n_tuples"),
    (dict(tuples=((0,),), n_tuples=9), b"n_tuples"),
    (dict(tuples=((0,),), n_cells=0), b"n_cells"),
    (dict(tuples=((0,),), n_cells=7), b"n_cells"),
    (dict(tuples=((0, 1), (2, 16))), b"not a board cell"),
    (dict(tuples=((0, 1, 2), (3, 4, 3))), b"twice"),
]

BAD_STAGES = [
    (dict(bounds=(), n_stages=0), b"n_stages"),
    (dict(bounds=(1, 2, 3, 4, 5, 6, 7), n_stages=9), b"n_stages"),
    (dict(bounds=(0,)), b"outside [1, 27]"),
    (dict(bounds=(28,)), b"outside [1, 27]"),
    (dict(bounds=(5, 5)), b"strictly increasing"),
    (dict(bounds=(8, 5)), b"strictly increasing"),
    (dict(bounds=(5, 8), n_stages=2), b"unused bound"),
]


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused_by_every_entry_point(kw, word):
    import g2048._native as N
    from g2048 import stageback

    lib, s, st = stageback.load(), _spec(**kw), _stages((5, 8))
    for call in (lambda: lib.g2048_stageback_acc_bytes(C.byref(s), C.byref(st)),
                 lambda: _step(lib, s, st)):
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_stageback_last_error()


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused_by_every_entry_point(kw, word):
    import g2048._native as N
    from g2048 import stageback

    lib, s, st = stageback.load(), _spec(NR.TUPLES_2x4), _stages(**kw)
    for call in (lambda: lib.g2048_stageback_acc_bytes(C.byref(s), C.byref(st)),
                 lambda: _step(lib, s, st)):
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_stageback_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    """Argument checks run before any device work: G2048_EINVAL with a message, on a machine
    without a GPU, for a device id that does not exist.  The pointers are never dereferenced (fake
    aligned addresses stand in for device memory)."""
    import g2048._native as N
    from g2048 import stageback

    lib = stageback.load()
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))
    size = stageback.acc_bytes(NR.TUPLES_2x4, (5, 8))
    assert size == 3 * 16 * 2 * 65536
    cases = [(dict(spec=None), b"spec"), (dict(stages=None), b"stages"),
             (dict(lut=None), b"NULL"), (dict(acc=None), b"acc_dev is NULL"),
             (dict(ea=None), b"ea_dev is NULL"), (dict(boards=None), b"NULL"),
             (dict(traj=None), b"traj_dev is NULL"), (dict(gain=None), b"gain_dev is NULL"),
             (dict(cur=None), b"cur_dev is NULL"), (dict(rec=None), b"rec_dev is NULL"),
             (dict(rep_n=None), b"rep_n_dev is NULL"), (dict(rep_k=None), b"rep_k_dev is NULL"),
             (dict(x=None), b"x_out_dev is NULL"), (dict(replay=None), b"replay_out_dev is NULL"),
             (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(horizon=0), b"horizon"), (dict(horizon=(1 << 20) + 1), b"horizon"),
             (dict(horizon=-1), b"horizon"),
             (dict(n=2049, horizon=1 << 20), b"n * horizon"),
             (dict(n=(1 << 30) + 1, horizon=2), b"n * horizon"),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=FAKE + 2), b"aligned"), (dict(acc=FAKE + 8), b"acc_dev must be 16-byte"),
             (dict(ea=FAKE_EA + 8), b"ea_dev must be 16-byte"),
             (dict(ea=FAKE), b"overlaps"), (dict(ea=FAKE + size - 16), b"overlaps"),
             (dict(acc=FAKE_EA + size - 16), b"overlaps"),
             (dict(boards=FAKE + 4), b"aligned"),
             (dict(traj=FAKE + 8), b"traj_dev must be 16-byte"),
             (dict(gain=FAKE + 2), b"gain_dev must be 4-byte"),
             (dict(rec=FAKE + 2), b"rec_dev must be 4-byte"),
             (dict(rep_n=FAKE + 1), b"rep_n_dev must be 4-byte"),
             (dict(rep_k=FAKE + 3), b"rep_k_dev must be 4-byte"),
             (dict(x=FAKE + 8), b"x_out_dev must be 16-byte"),
             (dict(delta=FAKE + 2), b"aligned"), (dict(err=FAKE + 4), b"aligned")]
    for kw, word in cases:
        assert _step(lib, **{"spec": s, "stages": st, **kw}) == N.G2048_EINVAL, kw
        msg = lib.g2048_stageback_last_error()
        assert word in msg and b"stageback_step" in msg, (kw, msg)
    # the edges of the domain pass the checks and fail only at the device that does not exist
    for kw in (dict(horizon=1), dict(horizon=1 << 20), dict(n=2048, horizon=1 << 20),
               dict(n=1 << 30, horizon=2), dict(cur=FAKE + 1), dict(replay=FAKE + 3),
               dict(err=None)):
        assert _step(lib, s, st, **kw) != N.G2048_EINVAL, kw


# ------------------------------------------------------------------ the Python side
TRAJ = ("traj", "gain", "cur", "rec", "rep_n", "rep_k")


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmeantc, ntstage, ntuple, stageback

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stageback.BackwardState(net, 4, 8)
    assert (st.horizon, st.n) == (8, 4)
    assert "horizon: int = 4096" in open(stageback.__file__).read()
    for t in (st.acc, st.ea):
        assert t.shape == (3, 2, 65536, 2) and t.dtype == torch.int64 and not t.any()
        assert t.data_ptr() % 16 == 0
    assert st.traj.shape == (4, 2, 8, 16) and st.traj.dtype == torch.uint8
    assert st.traj.data_ptr() % 16 == 0
    assert st.gain.shape == (4, 2, 8) and st.gain.dtype == torch.int32
    assert st.cur.shape == (4,) and st.cur.dtype == torch.uint8
    for t in (st.rec, st.rep_n, st.rep_k):
        assert t.shape == (4,) and t.dtype == torch.int32
    assert not any(bool(getattr(st, k).any()) for k in TRAJ)
    assert st.traj.numel() == stageback.traj_bytes(4, 8) == 32 * 4 * 8
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        st.step(boards, 1, 6, u8, i32, boards.clone(), u8.clone())
    with pytest.raises(g2048.NativeError):
        stageback.BackwardTrainer(net, 256, 8)
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for bad in (None, plain):  # staged networks only; the message points to from_network
        with pytest.raises(TypeError, match="from_network"):
            stageback.BackwardState(bad, 4)
        with pytest.raises(TypeError, match="from_network"):
            stageback.BackwardTrainer(bad, 256)
    for kw in (dict(n_boards=0), dict(horizon=0), dict(horizon=-2), dict(horizon=(1 << 20) + 1),
               dict(n_boards=2049, horizon=1 << 20)):
        with pytest.raises(ValueError):
            stageback.BackwardState(net, **{"n_boards": 4, **kw})
        with pytest.raises(ValueError):  # before the env is made, so without a GPU
            stageback.BackwardTrainer(net, **{"n_boards": 4, **kw})
    stageback.BackwardState(net, 4, 1)
    assert stageback.default_meantc_lr_shift is ntmeantc.default_meantc_lr_shift
    assert "lr_shift = default_meantc_lr_shift(net.spec)" in open(stageback.__file__).read()
    assert g2048.stageback is stageback
    assert g2048.BackwardState is stageback.BackwardState
    assert g2048.BackwardTrainer is stageback.BackwardTrainer
    assert issubclass(stageback.BackwardTrainer, ntuple.NTupleTrainer)
    assert {"stageback", "BackwardState", "BackwardTrainer"} <= set(g2048.__all__)


def _fill(st, seed):
    g = torch.Generator().manual_seed(seed)
    st.ea[..., 1] = torch.randint(0, 1 << 50, st.ea.shape[:-1], generator=g)
    st.ea[..., 0] = st.ea[..., 1] // 3 - 5
    st.traj.copy_(torch.randint(0, 12, st.traj.shape, generator=g).to(torch.uint8))
    st.gain.copy_(torch.randint(0, 1 << 16, st.gain.shape, generator=g).to(torch.int32))
    st.cur.copy_(torch.randint(0, 2, st.cur.shape, generator=g).to(torch.uint8))
    for name in ("rec", "rep_n", "rep_k"):
        getattr(st, name).copy_(torch.randint(0, 40, (st.n,), generator=g).to(torch.int32))


def test_the_state_round_trips_through_a_file_and_reset_keeps_ea(tmp_path):
    from g2048 import ntstage, ntuple, stageback, stagemeantc

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stageback.BackwardState(net, 9, 5)
    _fill(st, 9)
    keys = {"tuples", "bounds", "ea", *TRAJ}
    assert set(st.state_dict()) == keys
    st.save(tmp_path / "own.pt")
    back = stageback.BackwardState.load(tmp_path / "own.pt", net)
    assert (back.n, back.horizon) == (9, 5) and not back.acc.any()
    for name in ("ea", *TRAJ):
        assert torch.equal(getattr(back, name), getattr(st, name)), name
        assert getattr(back, name) is not getattr(st, name)
    assert set(torch.load(tmp_path / "own.pt", weights_only=True)) == keys
    # ea under StagedMeanTCState's keys: the thirteenth library's state reads the file
    tc = stagemeantc.StagedMeanTCState.load(tmp_path / "own.pt", net)
    assert torch.equal(tc.ea, st.ea)
    for other in (ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu"),
                  ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 9), device="cpu")):
        with pytest.raises(ValueError):
            stageback.BackwardState.load(tmp_path / "own.pt", other)
    good = st.state_dict()
    for bad in (dict(good, ea=st.ea.to(torch.int32)), dict(good, gain=st.gain[:, :, :2]),
                dict(good, traj=st.traj[:4]), dict(good, rec=st.rec.to(torch.int64)),
                dict(good, cur=st.cur.to(torch.int32))):
        with pytest.raises(ValueError):
            st.load_state_dict(bad)
    ea = st.ea.clone()
    st.reset()
    assert torch.equal(st.ea, ea) and not any(bool(getattr(st, k).any()) for k in TRAJ)


def test_from_state_carries_over_a_staged_or_a_single_tables_ea():
    from g2048 import ntmeantc, ntstage, ntuple, stageback, stagemeantc

    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    one = ntmeantc.MeanTCState(plain)
    one.ea[..., 1] = torch.arange(one.ea[..., 1].numel()).reshape(one.ea.shape[:-1]) + 7
    one.ea[..., 0] = 3
    staged = ntstage.StagedNTupleNetwork.from_network(plain, (5, 8))
    st = stageback.BackwardState.from_state(one, staged, 6, 2)
    assert st.net is staged and (st.n, st.horizon) == (6, 2)
    assert torch.equal(st.ea[0], one.ea) and not st.ea[1:].any() and not st.acc.any()
    assert not any(bool(getattr(st, k).any()) for k in TRAJ)
    tc = stagemeantc.StagedMeanTCState.from_state(one, staged)
    tc.ea[2] += 11
    st = stageback.BackwardState.from_state(tc, staged, 6, 16)
    assert torch.equal(st.ea, tc.ea) and st.ea.data_ptr() != tc.ea.data_ptr()
    assert st.horizon == 16
    other = ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu")
    with pytest.raises(ValueError):
        stageback.BackwardState.from_state(one, other, 6, 2)
    with pytest.raises(ValueError):  # the staged state's bounds must be the network's
        stageback.BackwardState.from_state(
            tc, ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5,), device="cpu"), 6, 2)
    with pytest.raises(TypeError):
        stageback.BackwardState.from_state(st, staged, 6, 2)
    with pytest.raises(TypeError):
        stageback.BackwardState.from_state(one, plain, 6, 2)
