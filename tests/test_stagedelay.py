"""CPU-side checks of delayed TD(lambda) on the staged batch-mean TC rule: the Python restatement
(tests/stagedelay_ref.py) reproduces its hand-computed anchors and has the header's six
consequences next to stagemeantc_ref, and the boundary of libg2048_stagedelay.so (header == exports
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
import stagedelay_ref as R
import stagemeantc_ref as SMT
from g2048 import stagedelay as _library

_library.load()  # every test of this file belongs to the library: without it the file fails here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_stagedelay.h")
NAMES = ["g2048_stagedelay_acc_bytes", "g2048_stagedelay_last_error", "g2048_stagedelay_rate",
         "g2048_stagedelay_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
X1 = [1, 2] + [0] * 14
X2 = [1, 2] + [0] * 9 + [6, 0, 0, 0, 5]
ONE = 1 << 16


def corner(bounds, n, H, s=1, base_ea=None):
    """Spec ((0,),), lut0[i] = 1024 i, the upper stages UNSET."""
    net = SR.StagedNet(((0,),), bounds, base=lambda st, t, i: 1024 * i if st == 0 else None)
    return R.Delayed(net, n, H, s, base_ea=base_ea)


def pair_spec(lut, n, H, s=1):
    """Spec ((0, 1),), one stage, the entries of `lut` and zeros."""
    net = SR.StagedNet(((0, 1),), (), base=lambda st, t, i: lut.get(i, 0))
    return R.Delayed(net, n, H, s)


def set_ring(d, i, afterstates, g=None, head=None):
    """Board i's ring: afterstates[k] is the one k steps back, g[k] its collected sum."""
    depth = len(afterstates)
    d.head[i] = depth - 1 if head is None else head
    d.depth[i] = depth
    for k, b in enumerate(afterstates):
        d.hist[d.plane(i, k)][i] = list(b)
        d.g[d.plane(i, k)][i] = 0 if g is None else g[k]


def table(net):
    return {(s, t, i): v for s, d in enumerate(net.stages) for (t, i), v in d.items()}


def ea_of(d):
    return {k: (d.E[k], d.A[k]) for k in d.A}


# ------------------------------------------------------------------ the reference's anchors
def test_anchor_r_the_shift_rounds_toward_zero():
    assert [R.collect(0, -1, k, 1) for k in range(3)] == [-1, 0, 0]
    assert [R.collect(0, -3, k, 1) for k in range(3)] == [-3, -1, 0]
    assert [(-1) >> k for k in range(3)] == [-1, -1, -1]  # what a shift of err itself would give
    assert [(-3) >> k for k in range(3)] == [-3, -2, -1]
    assert [R.collect(7, 3, k, 1) for k in range(3)] == [10, 8, 7]
    for lut, err, want in (({33: 1}, -1, [[-1], [0], [0]]), ({33: 1, 1: 2}, -3, [[-3], [-1], [0]])):
        d = pair_spec(lut, 1, 3)
        set_ring(d, 0, [X1, Q2, Q3])
        acts, errs, delta = d.step([CHECKER], 1, 0)
        assert (acts, errs, delta) == ([0], [err], want)
        assert d.depth == [0] and d.head == [2]
    # err = -3: X1 moved by -3, Q2 (index 2 twice, 0 six times) by -1, Q3 by nothing
    assert d.last_hits == {(0, 0, 33): (-3, 1), (0, 0, 1): (-3, 1), (0, 0, 2): (-2, 2),
                           (0, 0, 0): (-18 - 6, 12)}


def test_anchor_w_a_window_fills_applies_its_oldest_slot_and_wraps_head():
    d = corner((), 1, 2)
    assert d.step([A], 1, 1) == ([2], [0], [[0], [0]])
    assert (d.head, d.depth, d.hist[1], d.g) == ([1], [1], [Q2], [[0], [0]])
    assert d.step([A], 1, 1) == ([2], [4096], [[0], [0]])
    assert (d.head, d.depth, d.hist[0], d.g) == ([0], [2], [Q2], [[0], [4096]])
    assert not d.last_hits and not table(d.net)
    assert d.step([A], 1, 1) == ([2], [4096], [[0], [3072]])
    assert d.last_hits == {(0, 0, 2): (6144, 2), (0, 0, 0): (18432, 6)}
    assert table(d.net) == {(0, 0, 2): 5120, (0, 0, 0): 3072}
    assert ea_of(d) == {(0, 0, 2): (3072, 3072), (0, 0, 0): (3072, 3072)}
    assert (d.head, d.depth, d.hist[1], d.g) == ([1], [2], [Q2], [[4096], [0]])
    # terminal at depth H: both slots applied, two afterstates of one board in one mean
    assert d.step([CHECKER], 1, 1) == ([0], [-28672], [[-14336], [-5120]])
    assert d.last_hits == {(0, 0, 2): (-38912, 4), (0, 0, 0): (-116736, 12)}
    assert d.last_m == {(0, 0, 2): -9728, (0, 0, 0): -9728}
    assert table(d.net) == {(0, 0, 2): -4608, (0, 0, 0): -6656}
    assert ea_of(d) == {(0, 0, 2): (-6656, 12800), (0, 0, 0): (-6656, 12800)}
    assert (d.head, d.depth, d.g) == ([1], [0], [[4096], [0]])
    # terminal at depth 0
    before = (table(d.net), ea_of(d), [list(p) for p in d.hist])
    assert d.step([CHECKER], 1, 1) == ([0], [0], [[0], [0]])
    assert (table(d.net), ea_of(d), d.hist) == before and not d.last_hits
    assert (d.head, d.depth, d.g) == ([1], [0], [[4096], [0]])


def test_anchor_t1_a_terminal_call_at_depth_1():
    d = corner((), 1, 2)
    d.step([A], 1, 1)
    assert d.step([CHECKER], 1, 1) == ([0], [-4096], [[-2048], [0]])
    assert table(d.net) == {(0, 0, 2): 0, (0, 0, 0): -2048}
    assert (d.head, d.depth) == ([1], [0])


def test_anchor_c2_two_afterstates_of_one_terminal_board_share_an_entry():
    d = pair_spec({33: 1, 1: 2}, 1, 2)
    set_ring(d, 0, [X1, X2], g=[0, -4])
    assert d.step([CHECKER], 1, 0) == ([0], [-3], [[-3], [-5]])
    assert d.last_hits == {(0, 0, 33): (-8, 2), (0, 0, 1): (-8, 2), (0, 0, 0): (-38, 10),
                           (0, 0, 5): (-5, 1), (0, 0, 101): (-5, 1)}
    assert d.last_m == {(0, 0, 33): -4, (0, 0, 1): -4, (0, 0, 0): -4, (0, 0, 5): -5,
                        (0, 0, 101): -5}
    assert table(d.net) == {(0, 0, 33): -3, (0, 0, 1): -2, (0, 0, 0): -4, (0, 0, 5): -5,
                            (0, 0, 101): -5}
    assert ea_of(d) == {k: (m, -m) for k, m in d.last_m.items()}


def test_anchor_s2_two_boards_of_different_stages_address_one_index():
    d = corner((3,), 2, 2)
    set_ring(d, 0, [Q2])
    set_ring(d, 1, [Q3])
    assert d.step([CHECKER, CHECKER], 1, 1) == ([0, 0], [-4096, -6144],
                                                [[-2048, -3072], [0, 0]])
    assert d.net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(d.net) == {(0, 0, 2): 0, (0, 0, 0): -2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    assert ea_of(d)[(0, 0, 0)] == (-2048, 2048) and ea_of(d)[(1, 0, 0)] == (-3072, 3072)


def test_anchor_p_promoted_while_prev_and_moved_h_minus_1_calls_later():
    d = corner((2,), 1, 2)
    d.step([A], 1, 1)
    assert not d.net.promoted and not table(d.net)
    assert d.step([A], 1, 1) == ([2], [4096], [[0], [0]])
    assert d.net.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0} == table(d.net)
    assert d.step([A], 1, 1) == ([2], [4096], [[0], [3072]])
    assert not d.net.promoted
    assert table(d.net) == {(1, 0, 2): 5120, (1, 0, 0): 3072}


def test_anchor_z_a_g_that_cancels_makes_no_hit_and_leaves_ea():
    d = corner((), 1, 2, base_ea=lambda s, t, i: (5, 9) if (s, t, i) == (0, 0, 3) else (0, 0))
    set_ring(d, 0, [Q2, Q3], g=[0, -2048], head=0)
    assert d.step([A], 1, 1) == ([2], [4096], [[0], [0]])
    assert not d.last_hits and not table(d.net) and not ea_of(d)
    assert d.get_ea(0, 0, 3) == (5, 9)
    assert (d.head, d.depth, d.hist[1], d.g) == ([1], [2], [Q2], [[4096], [0]])


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


def _batches(rng, n, calls):
    """Fresh boards per call, a terminal one moving through the batch."""
    out = []
    for t in range(calls):
        boards = _staged(rng, n)
        boards[(3 * t + 1) % n] = list(CHECKER)
        out.append(boards)
    return out


def _ring(d):
    return ([[list(b) for b in p] for p in d.hist], list(d.head), list(d.depth),
            [list(p) for p in d.g])


@pytest.mark.parametrize("S", [1, 2, 3])
def test_consequence_1_h1_is_the_staged_batch_mean_tc_step(S):
    rng = random.Random(50 + S)
    base = _base(51 + S, S, 3, 2, upper=0.5)
    n = 24
    d = R.Delayed(SR.StagedNet(T3, BOUNDS[S], base=base), n, 1, 7, base_ea=seeded_ea(52))
    mt = SMT.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base), base_ea=seeded_ea(52))
    prev, has = [[0] * 16 for _ in range(n)], [0] * n
    for boards in _batches(rng, n, 6):
        acts, errs, delta = d.step(boards, 3, 5)
        assert (acts, errs, delta[0]) == mt.step(boards, prev, has, 3, 5)
        assert d.last_hits == mt.last_hits and d.last_m == mt.last_m
        assert d.net.stages == mt.net.stages and d.net.promoted == mt.net.promoted
        assert ea_of(d) == ea_of(mt)
        assert d.depth == has and d.g == [[0] * n] and d.head == [0] * n
        assert all(d.hist[0][i] == prev[i] for i in range(n) if has[i])
    assert d.A and any(c > 8 for _d, c in d.last_hits.values())


def test_consequence_2_the_weights_of_a_full_window_and_the_one_call_delay():
    """H = 3, s = 1 on one board: the slot that leaves holds err_0 + err_1 / 2 + err_2 / 4 of its
    three calls.  H = 2, s = 31: what is applied in call t is delta_of(err of call t - 1)."""
    rng = random.Random(60)
    base = _base(61, 2, 3, 2, upper=0.5)
    n = 16
    d = R.Delayed(SR.StagedNet(T3, (5,), base=base), n, 3, 1)
    errs = []
    for t, boards in enumerate(_batches(rng, n, 7)):
        boards = [b if b != CHECKER else _boards(rng, 1)[0] for b in boards]
        depth = list(d.depth)
        _a, e, delta = d.step(boards, 3, 5)
        errs.append(e)
        for i in range(n):
            if depth[i] == 3:
                G = R.collect(R.collect(errs[t - 2][i], errs[t - 1][i], 1, 1), errs[t][i], 2, 1)
                assert delta[2][i] == NR.delta_of(G, 3, 5) and delta[0][i] == delta[1][i] == 0
    assert d.depth == [3] * n and any(any(p) for p in delta)
    d = R.Delayed(SR.StagedNet(T3, (5,), base=base), n, 2, 31)
    last = None
    for boards in _batches(rng, n, 5):
        legal = [b != CHECKER for b in boards]
        depth = list(d.depth)
        _a, e, delta = d.step(boards, 3, 5)
        for i in range(n):
            if depth[i] == 2 and legal[i]:
                assert delta[1][i] == NR.delta_of(last[i], 3, 5) and delta[0][i] == 0
        last = e
    assert all(abs(x) < 1 << 31 for x in e) and any(delta[1])


def test_consequences_3_and_4_the_hits_of_a_call_and_no_add_on_unset():
    """sum of C = 8 T per applied slot with a non-zero delta: at most one per non-terminal board,
    depth per terminal board.  Every upper-stage entry starts UNSET: a hit on one raises in the
    reference, so ten calls without that are consequence 4."""
    rng = random.Random(70)
    base = _base(71, 3, 3, 2, upper=0.0)
    n = 24
    d = R.Delayed(SR.StagedNet(T3, (5, 8), base=base), n, 3, 1)
    terminal_sets = 0
    for boards in _batches(rng, n, 10):
        depth = list(d.depth)
        _a, _e, delta = d.step(boards, 3, 5)
        sets = 0
        for i in range(n):
            mine = sum(1 for k in range(3) if delta[k][i])
            if boards[i] == CHECKER:
                assert mine <= depth[i]
                terminal_sets = max(terminal_sets, mine)
            else:
                assert mine <= 1 and (mine == 0 or depth[i] == 3)
            sets += mine
        assert sum(c for _d, c in d.last_hits.values()) == 8 * 3 * sets
    assert terminal_sets == 3 and len(d.net.stages[1]) > 20 and len(d.net.stages[2]) > 20


@pytest.mark.parametrize("S", [2, 3])
def test_consequence_5_e_within_a_the_unset_pattern_and_repetition(S):
    import copy

    rng = random.Random(80 + S)
    base = _base(81, S, 3, 2, upper=0.5)
    n = 20
    batches = _batches(rng, n, 6)
    runs = []
    for k in (1, 3):
        d = R.Delayed(SR.StagedNet(T3, BOUNDS[S], base=base), n * k, 3, 1)
        for boards in batches:
            d.step([list(b) for b in boards] * k, 3, 5)
            assert all(abs(e) <= a for e, a in ea_of(d).values())
        runs.append(d)
    one, three = runs
    assert one.net.stages == three.net.stages and ea_of(one) == ea_of(three)
    assert all(three.last_hits[k] == (3 * dd, 3 * c) for k, (dd, c) in one.last_hits.items())
    assert one.last_hits and _ring(three)[1] == _ring(one)[1] * 3
    assert _ring(three)[3] == [p * 3 for p in _ring(one)[3]]
    # one more call from this state, and from the same table and ring under another ea and
    # another g: other moves, the same entries set
    other = copy.deepcopy(one)
    other.base_ea, other.E, other.A = seeded_ea(82), {}, {}
    other.g = [[x + 12345 for x in p] for p in other.g]
    boards = _batches(rng, n, 1)[0]
    one.step(boards, 3, 5)
    other.step(boards, 3, 5)
    pattern = lambda d: {(s, t, i) for s in range(S) for (t, i) in d.net.stages[s]}  # noqa: E731
    assert pattern(one) == pattern(other) and one.net.promoted == other.net.promoted
    assert one.net.promoted and one.net.stages != other.net.stages


def test_consequence_6_the_order_of_the_boards_does_not_matter():
    rng = random.Random(90)
    base = _base(91, 3, 3, 2, upper=0.5)
    n = 20
    perm = list(range(n))
    rng.shuffle(perm)
    a = R.Delayed(SR.StagedNet(T3, (5, 8), base=base), n, 3, 1, base_ea=seeded_ea(92))
    b = R.Delayed(SR.StagedNet(T3, (5, 8), base=base), n, 3, 1, base_ea=seeded_ea(92))
    for boards in _batches(rng, n, 6):
        oa = a.step(boards, 3, 5)
        ob = b.step([boards[j] for j in perm], 3, 5)
        assert [oa[0][j] for j in perm] == ob[0] and [oa[1][j] for j in perm] == ob[1]
        assert [[p[j] for j in perm] for p in oa[2]] == ob[2]
        assert a.net.stages == b.net.stages and ea_of(a) == ea_of(b)
        assert [[p[j] for j in perm] for p in a.g] == b.g
    assert a.A


def test_the_reference_refuses_parameters_outside_the_domain():
    net = SR.StagedNet(T3, ())
    for H, s in ((0, 1), (9, 1), (2, 0), (2, 32), (3, 16), (8, 5)):
        with pytest.raises(ValueError):
            R.Delayed(net, 4, H, s)
    R.Delayed(net, 4, 2, 31), R.Delayed(net, 4, 8, 4), R.Delayed(net, 4, 1, 31)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (deepsearch, ntlambda, ntmean, ntmeantc, ntrestart, ntsearch, ntstage, nttc,
                       ntuple, search, stagemean, stagemeantc, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean, ntmeantc, stagemeantc, deepsearch)


def test_header_equals_exports_equals_signatures():
    from g2048 import stagedelay

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = stagedelay.load()
    assert set(names) == set(stagedelay.SIGNATURES)
    assert _exported(stagedelay.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_stagedelay_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(stagedelay.SIGNATURES["g2048_stagedelay_step"][1]) == 20
    # g2048_stagemeantc_step's arguments with the ring in the place of prev / has_prev
    args = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    tc = open(os.path.join(ROOT, "include", "g2048_stagemeantc.h")).read()
    tc_args = [a.split()[-1].lstrip("*") for a in
               re.search(r"g2048_stagemeantc_step\((.*?)\);", tc, re.S).group(1).split(",")]
    k = tc_args.index("prev_dev")
    assert tc_args[k:k + 2] == ["prev_dev", "has_prev_dev"]
    assert args == tc_args[:k] + ["hist_dev", "head_dev", "depth_dev", "g_dev", "horizon",
                                  "lam_shift"] + tc_args[k + 2:]
    # the constants are the sixth library's and the thirteenth's
    for name, value in (("MAX_HORIZON", 8), ("MAX_LAM_SHIFT", 31), ("RATE_BITS", 16)):
        assert re.search(rf"#define G2048_STAGEDELAY_{name} {value}\b", src)
        assert getattr(stagedelay, name) == value
    # the other fourteen libraries keep their ABI: none of the new symbols
    assert len(_others()) == 14
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_stagedelay")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import stagedelay

    out = subprocess.run(["readelf", "-d", stagedelay.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other fourteen stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash(), G.deepsearch_source_hash(), G.stagedelay_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS, G.NTMEAN_SHARED,
                  G.STAGEMEAN_SRCS, G.NTMEANTC_SRCS, G.STAGEMEANTC_SRCS, G.DEEPSEARCH_SRCS):
        assert set(G.STAGEDELAY_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.STAGEDELAY_SRCS[0]))
    assert open(G.STAGEDELAY_STAMP).read().strip() == G.stagedelay_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.STAGEMEANTC_STAMP).read().strip() == G.stagemeantc_source_hash()
    assert len(set(_hashes(G))) == 15


def test_stamp_follows_its_source_the_shared_headers_and_the_four_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp -- source_hash() included, which
    lists the file among the sources with stamps of their own; a change to each shared csrc header
    it includes changes the new stamp; a change to each of g2048.h, g2048_ntuple.h,
    g2048_ntstage.h and g2048_stagedelay.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.STAGEDELAY_SRCS[0])).read()
    includes = re.findall(r'#include\s+"([^"]+)"', src)
    assert includes == ["../../include/g2048_stagedelay.h", "g2048_board.hpp", G.NTUPLE_SHARED[0],
                        G.NTSTAGE_SHARED[0], G.NTMEAN_SHARED[0]]
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.STAGEDELAY_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:14] == before[:14] and after[14] != before[14]
    last = after
    for shared in (G.NTMEAN_SHARED[0], G.NTUPLE_SHARED[0], G.NTSTAGE_SHARED[0],
                   "g2048_board.hpp"):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
        now = _hashes(G)
        assert now[14] != last[14] and now[12] != last[12], shared  # the thirteenth follows too
        if shared != "g2048_board.hpp":  # that one the main library includes too
            assert now[0] == before[0]
        last = now
    shared, include = last, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntstage.h",
                                "g2048_stagedelay.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[14] != shared[14] and now[14] != last[14], header
        if header == "g2048_stagedelay.h":
            assert now[:14] == shared[:14]
        last = now


def test_kernels_have_no_store_data_hazard_and_no_scratch(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's flags,
    as the other libraries' tests audit theirs; and none of the 24 kernels (policy, gather and
    apply for T = 1..8) uses scratch."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.STAGEDELAY_SRCS:
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


def test_acc_bytes_and_rate_are_the_thirteenth_librarys():
    import g2048._native as N
    from g2048 import stagedelay, stagemeantc

    lib, tc = stagedelay.load(), stagemeantc.load()
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6):
        for bounds in ((), (11,), (5, 8), tuple(range(1, 8))):
            want = 16 * (len(bounds) + 1) * len(tuples) * 16 ** len(tuples[0])
            assert lib.g2048_stagedelay_acc_bytes(C.byref(_spec(tuples)),
                                                  C.byref(_stages(bounds))) == want
            assert stagedelay.acc_bytes(tuples, bounds) == want
    assert lib.g2048_stagedelay_acc_bytes(None, C.byref(_stages(()))) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_stagedelay_last_error()
    assert lib.g2048_stagedelay_acc_bytes(C.byref(_spec(NR.TUPLES_2x4)), None) == N.G2048_EINVAL
    assert b"stages" in lib.g2048_stagedelay_last_error()
    with pytest.raises(ValueError):
        stagedelay.acc_bytes(NR.TUPLES_2x4, (8, 5))
    rng = random.Random(8)
    for a in (0, 1, 3, 255, (1 << 16) - 1, 1 << 16, (1 << 16) + 1, 1 << 31, (1 << 40) + 12345,
              (1 << 62) - 1):
        for e in {0, a, -a, a // 3} | {rng.randrange(-a, a + 1) for _ in range(6)}:
            want = TR.rate(e, a)
            assert lib.g2048_stagedelay_rate(e, a) == want == tc.g2048_stagemeantc_rate(e, a)
            assert stagedelay.rate(e, a) == want == stagedelay.DelayedLambdaState.rate(e, a)
    for e, a, word in ((0, -1, b"A ="), (0, 1 << 62, b"A ="), (2, 1, b"exceeds"),
                       (-(1 << 63), 5, b"exceeds")):
        assert lib.g2048_stagedelay_rate(e, a) == N.G2048_EINVAL
        assert word in lib.g2048_stagedelay_last_error()
        assert b"stagedelay_rate" in lib.g2048_stagedelay_last_error()
        with pytest.raises(ValueError):
            stagedelay.rate(e, a)


FAKE, FAKE_EA = 1 << 20, 1 << 30  # aligned addresses that stand in for device memory


def _step(lib, spec, stages, lut=FAKE, acc=FAKE, ea=FAKE_EA, boards=FAKE, n=4, hist=FAKE,
          head=FAKE, depth=FAKE, g=FAKE, horizon=3, lam_shift=1, lr_num=1, lr_shift=10,
          action=FAKE, delta=FAKE, err=FAKE):
    return lib.g2048_stagedelay_step(C.byref(spec) if spec is not None else None,
                                     C.byref(stages) if stages is not None else None, lut, acc,
                                     ea, boards, n, hist, head, depth, g, horizon, lam_shift,
                                     lr_num, lr_shift, action, delta, err, 1 << 20, None)


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
    from g2048 import stagedelay

    lib, s, st = stagedelay.load(), _spec(**kw), _stages((5, 8))
    for call in (lambda: lib.g2048_stagedelay_acc_bytes(C.byref(s), C.byref(st)),
                 lambda: _step(lib, s, st)):
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_stagedelay_last_error()


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused_by_every_entry_point(kw, word):
    import g2048._native as N
    from g2048 import stagedelay

    lib, s, st = stagedelay.load(), _spec(NR.TUPLES_2x4), _stages(**kw)
    for call in (lambda: lib.g2048_stagedelay_acc_bytes(C.byref(s), C.byref(st)),
                 lambda: _step(lib, s, st)):
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_stagedelay_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    """Argument checks run before any device work: G2048_EINVAL with a message, on a machine
    without a GPU, for a device id that does not exist.  The pointers are never dereferenced (fake
    aligned addresses stand in for device memory)."""
    import g2048._native as N
    from g2048 import stagedelay

    lib = stagedelay.load()
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))
    size = stagedelay.acc_bytes(NR.TUPLES_2x4, (5, 8))
    assert size == 3 * 16 * 2 * 65536
    cases = [(dict(spec=None), b"spec"), (dict(stages=None), b"stages"),
             (dict(lut=None), b"NULL"), (dict(acc=None), b"acc_dev is NULL"),
             (dict(ea=None), b"ea_dev is NULL"), (dict(boards=None), b"NULL"),
             (dict(hist=None), b"hist_dev is NULL"), (dict(head=None), b"head_dev"),
             (dict(depth=None), b"depth_dev"), (dict(g=None), b"g_dev is NULL"),
             (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(horizon=0), b"horizon"), (dict(horizon=9), b"horizon"),
             (dict(horizon=-1), b"horizon"),
             (dict(lam_shift=0), b"lam_shift"), (dict(lam_shift=32), b"lam_shift"),
             (dict(horizon=3, lam_shift=16), b"(horizon - 1) * lam_shift"),
             (dict(horizon=8, lam_shift=5), b"(horizon - 1) * lam_shift"),
             (dict(horizon=2, lam_shift=32), b"lam_shift"),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=FAKE + 2), b"aligned"), (dict(acc=FAKE + 8), b"acc_dev must be 16-byte"),
             (dict(ea=FAKE_EA + 8), b"ea_dev must be 16-byte"),
             (dict(ea=FAKE), b"overlaps"), (dict(ea=FAKE + size - 16), b"overlaps"),
             (dict(acc=FAKE_EA + size - 16), b"overlaps"),
             (dict(boards=FAKE + 4), b"aligned"), (dict(hist=FAKE + 8), b"hist_dev must be 16-byte"),
             (dict(g=FAKE + 4), b"g_dev must be 8-byte"),
             (dict(delta=FAKE + 2), b"aligned"), (dict(err=FAKE + 4), b"aligned")]
    for kw, word in cases:
        assert _step(lib, **{"spec": s, "stages": st, **kw}) == N.G2048_EINVAL, kw
        msg = lib.g2048_stagedelay_last_error()
        assert word in msg and b"stagedelay_step" in msg, (kw, msg)
    # the edges of the domain pass the checks and fail only at the device that does not exist
    for kw in (dict(horizon=1, lam_shift=31), dict(horizon=2, lam_shift=31),
               dict(horizon=8, lam_shift=4), dict(err=None)):
        assert _step(lib, s, st, **kw) != N.G2048_EINVAL, kw


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmeantc, ntstage, ntuple, stagedelay

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stagedelay.DelayedLambdaState(net, 4)
    assert (st.horizon, st.lam_shift, st.n) == (3, 1, 4)
    for t in (st.acc, st.ea):
        assert t.shape == (3, 2, 65536, 2) and t.dtype == torch.int64 and not t.any()
        assert t.data_ptr() % 16 == 0
    assert st.hist.shape == (3, 4, 16) and st.hist.dtype == torch.uint8
    assert st.head.shape == st.depth.shape == (4,) and st.head.dtype == st.depth.dtype == torch.uint8
    assert st.g.shape == (3, 4) and st.g.dtype == torch.int64
    assert not any(bool(t.any()) for t in (st.hist, st.head, st.depth, st.g))
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros((3, 4), dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        st.step(boards, 1, 6, u8, i32)
    with pytest.raises(g2048.NativeError):
        stagedelay.DelayedLambdaTrainer(net, 256)
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for bad in (None, plain):  # staged networks only; the message points to from_network
        with pytest.raises(TypeError, match="from_network"):
            stagedelay.DelayedLambdaState(bad, 4)
        with pytest.raises(TypeError, match="from_network"):
            stagedelay.DelayedLambdaTrainer(bad, 256)
    for kw in (dict(n_boards=0), dict(horizon=0), dict(horizon=9), dict(lam_shift=0),
               dict(lam_shift=32), dict(horizon=3, lam_shift=16), dict(horizon=8, lam_shift=5)):
        with pytest.raises(ValueError):
            stagedelay.DelayedLambdaState(net, **{"n_boards": 4, **kw})
        with pytest.raises(ValueError):  # before the env is made, so without a GPU
            stagedelay.DelayedLambdaTrainer(net, **{"n_boards": 4, **kw})
    stagedelay.DelayedLambdaState(net, 4, 2, 31), stagedelay.DelayedLambdaState(net, 4, 8, 4)
    assert stagedelay.default_meantc_lr_shift is ntmeantc.default_meantc_lr_shift
    assert "lr_shift = default_meantc_lr_shift(net.spec)" in open(stagedelay.__file__).read()
    assert g2048.stagedelay is stagedelay
    assert g2048.DelayedLambdaState is stagedelay.DelayedLambdaState
    assert g2048.DelayedLambdaTrainer is stagedelay.DelayedLambdaTrainer
    assert issubclass(stagedelay.DelayedLambdaTrainer, ntuple.NTupleTrainer)
    assert {"stagedelay", "DelayedLambdaState", "DelayedLambdaTrainer"} <= set(g2048.__all__)


def _fill(st, seed):
    g = torch.Generator().manual_seed(seed)
    st.ea[..., 1] = torch.randint(0, 1 << 50, st.ea.shape[:-1], generator=g)
    st.ea[..., 0] = st.ea[..., 1] // 3 - 5
    st.hist.copy_(torch.randint(0, 12, st.hist.shape, generator=g).to(torch.uint8))
    st.head.copy_(torch.randint(0, st.horizon, st.head.shape, generator=g).to(torch.uint8))
    st.depth.copy_(torch.randint(0, st.horizon + 1, st.depth.shape, generator=g).to(torch.uint8))
    st.g.copy_(torch.randint(-(1 << 40), 1 << 40, st.g.shape, generator=g))


RING = ("hist", "head", "depth", "g")


def test_the_state_round_trips_through_a_file_and_reset_keeps_ea(tmp_path):
    from g2048 import ntstage, ntuple, stagedelay, stagemeantc

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stagedelay.DelayedLambdaState(net, 9, 4, 2)
    _fill(st, 9)
    keys = {"tuples", "bounds", "ea", "lam_shift", *RING}
    assert set(st.state_dict()) == keys
    st.save(tmp_path / "own.pt")
    back = stagedelay.DelayedLambdaState.load(tmp_path / "own.pt", net)
    assert (back.n, back.horizon, back.lam_shift) == (9, 4, 2) and not back.acc.any()
    for name in ("ea", *RING):
        assert torch.equal(getattr(back, name), getattr(st, name)), name
        assert getattr(back, name) is not getattr(st, name)
    assert set(torch.load(tmp_path / "own.pt", weights_only=True)) == keys
    # ea under StagedMeanTCState's keys: the thirteenth library's state reads the file
    tc = stagemeantc.StagedMeanTCState.load(tmp_path / "own.pt", net)
    assert torch.equal(tc.ea, st.ea)
    for other in (ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu"),
                  ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 9), device="cpu")):
        with pytest.raises(ValueError):
            stagedelay.DelayedLambdaState.load(tmp_path / "own.pt", other)
    good = st.state_dict()
    for bad in (dict(good, ea=st.ea.to(torch.int32)), dict(good, g=st.g[:2]),
                dict(good, hist=st.hist[:, :4]), dict(good, lam_shift=torch.tensor(1)),
                dict(good, depth=st.depth.to(torch.int64))):
        with pytest.raises(ValueError):
            st.load_state_dict(bad)
    ea = st.ea.clone()
    st.reset()
    assert torch.equal(st.ea, ea) and not any(bool(getattr(st, k).any()) for k in RING)


def test_from_state_carries_over_a_staged_or_a_single_tables_ea():
    from g2048 import ntmeantc, ntstage, ntuple, stagedelay, stagemeantc

    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    one = ntmeantc.MeanTCState(plain)
    one.ea[..., 1] = torch.arange(one.ea[..., 1].numel()).reshape(one.ea.shape[:-1]) + 7
    one.ea[..., 0] = 3
    staged = ntstage.StagedNTupleNetwork.from_network(plain, (5, 8))
    st = stagedelay.DelayedLambdaState.from_state(one, staged, 6, 2, 3)
    assert st.net is staged and (st.n, st.horizon, st.lam_shift) == (6, 2, 3)
    assert torch.equal(st.ea[0], one.ea) and not st.ea[1:].any() and not st.acc.any()
    assert not any(bool(getattr(st, k).any()) for k in RING)
    tc = stagemeantc.StagedMeanTCState.from_state(one, staged)
    tc.ea[2] += 11
    st = stagedelay.DelayedLambdaState.from_state(tc, staged, 6)
    assert torch.equal(st.ea, tc.ea) and st.ea.data_ptr() != tc.ea.data_ptr()
    assert (st.horizon, st.lam_shift) == (3, 1)
    other = ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu")
    with pytest.raises(ValueError):
        stagedelay.DelayedLambdaState.from_state(one, other, 6)
    with pytest.raises(ValueError):  # the staged state's bounds must be the network's
        stagedelay.DelayedLambdaState.from_state(
            tc, ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5,), device="cpu"), 6)
    with pytest.raises(TypeError):
        stagedelay.DelayedLambdaState.from_state(st, staged, 6)
    with pytest.raises(TypeError):
        stagedelay.DelayedLambdaState.from_state(one, plain, 6)
