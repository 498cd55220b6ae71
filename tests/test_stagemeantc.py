"""CPU-side checks of temporal-coherence learning on the batch-mean rule for the multi-stage
network: the Python restatement (tests/stagemeantc_ref.py) reproduces its hand-computed anchors and
has the header's nine consequences next to stagemean_ref, ntmeantc_ref and StagedNet.td_step, and
the boundary of libg2048_stagemeantc.so (header == exports == SIGNATURES, build stamps, the
host-only rate, argument validation without a GPU, the Python side's refusals, its save / load and
from_state)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest
import torch

import ntmean_ref as MR
import ntmeantc_ref as MTR
import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR
import stagemean_ref as SMR
import stagemeantc_ref as R
from g2048 import stagemeantc as _library

_library.load()  # every test of this file belongs to the library: without it the file fails here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_stagemeantc.h")
NAMES = ["g2048_stagemeantc_acc_bytes", "g2048_stagemeantc_last_error", "g2048_stagemeantc_rate",
         "g2048_stagemeantc_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
P1 = [1, 0, 0, 0, 0, 2] + [0] * 10
P2 = [1, 0, 0, 0, 0, 3] + [0] * 10
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15
ONE = 1 << 16


def corner(bounds, base_ea=None):
    """Spec ((0,),), lut0[i] = 1024 i, the upper stages UNSET."""
    net = SR.StagedNet(((0,),), bounds, base=lambda s, t, i: 1024 * i if s == 0 else None)
    return R.StagedMeanTC(net, base_ea=base_ea)


def table(net):
    """{(s, t, i): value} of everything the steps have written."""
    return {(s, t, i): v for s, d in enumerate(net.stages) for (t, i), v in d.items()}


def ea_of(mt):
    return {k: (mt.E[k], mt.A[k]) for k in mt.A}


# ------------------------------------------------------------------ the reference's anchors
def test_anchor_1_the_stage_split_three_times():
    mt = corner((3,))
    boards = [A, CHECKER, CHECKER]

    def call():
        prev, has_prev = [list(Q2), list(Q3), list(Q3)], [1, 1, 1]
        out = mt.step(boards, prev, has_prev, 1, 1)
        assert has_prev == [1, 0, 0] and prev == [Q2, Q3, Q3]
        return out

    acts, _err, delta = call()
    assert (acts, delta) == ([2, 0, 0], [2048, -3072, -3072])
    assert mt.last_hits == {(0, 0, 2): (4096, 2), (0, 0, 0): (12288, 6), (1, 0, 3): (-12288, 4),
                            (1, 0, 0): (-36864, 12)} == SMR_split_hits()
    assert mt.net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(mt.net) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    assert ea_of(mt) == {(0, 0, 2): (2048, 2048), (0, 0, 0): (2048, 2048),
                         (1, 0, 3): (-3072, 3072), (1, 0, 0): (-3072, 3072)}
    rates = {k: TR.rate(*mt.get_ea(*k)) for k in mt.A}
    acts, _err, delta = call()
    assert delta == [2048, 9216, 9216] and not mt.net.promoted
    assert set(rates.values()) == {ONE}
    assert table(mt.net) == {(0, 0, 2): 6144, (0, 0, 0): 4096, (1, 0, 3): 9216, (1, 0, 0): 6144}
    assert ea_of(mt) == {(0, 0, 2): (4096, 4096), (0, 0, 0): (4096, 4096),
                         (1, 0, 3): (6144, 12288), (1, 0, 0): (6144, 12288)}
    assert TR.rate(6144, 12288) == 32768 and TR.rate(4096, 4096) == ONE
    acts, _err, delta = call()
    assert delta == [2048, -27648, -27648]
    assert TR.step_of(-27648, 32768) == -13824
    assert table(mt.net) == {(0, 0, 2): 8192, (0, 0, 0): 6144, (1, 0, 3): -4608,
                             (1, 0, 0): -7680}
    assert ea_of(mt) == {(0, 0, 2): (6144, 6144), (0, 0, 0): (6144, 6144),
                         (1, 0, 3): (-21504, 39936), (1, 0, 0): (-21504, 39936)}
    # index 0 runs at two rates in two stages
    assert TR.rate(*mt.get_ea(0, 0, 0)) == ONE and TR.rate(*mt.get_ea(1, 0, 0)) == 35288


def SMR_split_hits():
    """The hits of stagemean_ref's split anchor."""
    net = SR.StagedNet(((0,),), (3,), base=lambda s, t, i: 1024 * i if s == 0 else None)
    SMR.step(net, [A, CHECKER, CHECKER], [list(Q2), list(Q3), list(Q3)], [1, 1, 1], 1, 1)
    assert net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    return dict(SMR.last_hits)


def test_anchor_2_a_cancelled_entry_in_one_stage_only():
    mt = corner((3,), base_ea=lambda s, t, i: (0, 7) if (s, t, i) == (1, 0, 0) else (0, 0))
    mt.step([A, CHECKER, CHECKER], [list(Q2), list(Q3), list(Q3)], [1, 1, 1], 1, 1)
    assert mt.net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(mt.net) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): 0}
    assert ea_of(mt) == {(0, 0, 2): (2048, 2048), (0, 0, 0): (2048, 2048),
                         (1, 0, 3): (-3072, 3072), (1, 0, 0): (-3072, 3079)}


def test_anchor_3_m_equal_to_zero():
    mt = corner((2,), base_ea=lambda s, t, i: (5, 9) if (s, t, i) == (1, 0, 0) else (0, 0))
    prev, has_prev = [list(Q2), list(Q2), list(Q3)], [1, 1, 1]
    _acts, _err, delta = mt.step([A, A, CHECKER], prev, has_prev, 1, 12)
    assert delta == [1, 1, -2]
    assert mt.last_hits == {(1, 0, 2): (4, 4), (1, 0, 0): (0, 18), (1, 0, 3): (-4, 2)}
    assert mt.last_m == {(1, 0, 2): 1, (1, 0, 0): 0, (1, 0, 3): -2}
    assert mt.net.promoted == {(1, 0, 2): 2048, (1, 0, 0): 0, (1, 0, 3): 3072}
    assert table(mt.net) == {(1, 0, 2): 2049, (1, 0, 0): 0, (1, 0, 3): 3070}
    assert ea_of(mt) == {(1, 0, 2): (1, 1), (1, 0, 3): (-2, 2)}
    assert mt.get_ea(1, 0, 0) == (5, 9)
    assert has_prev == [1, 1, 0]


def test_anchor_4_two_stages_promoted_and_moved_in_one_call():
    mt = corner((2, 3))
    prev, has_prev = [list(P1), list(P2)], [1, 1]
    acts, err, delta = mt.step([CHECKER, A], prev, has_prev, 1, 1)
    assert (acts, err, delta) == ([0, 2], [-2048, 6144], [-1024, 3072])
    assert mt.net.promoted == {(1, 0, 1): 1024, (2, 0, 1): 1024, (1, 0, 0): 0, (2, 0, 0): 0}
    assert table(mt.net) == {(1, 0, 1): 0, (1, 0, 0): -1024, (2, 0, 1): 4096, (2, 0, 0): 3072}
    assert ea_of(mt) == {(1, 0, 1): (-1024, 1024), (1, 0, 0): (-1024, 1024),
                         (2, 0, 1): (3072, 3072), (2, 0, 0): (3072, 3072)}
    assert has_prev == [0, 1] and prev == [P1, Q2]


def test_anchor_5_the_two_floors_and_a_41_bit_a_at_stage_0_of_a_two_stage_net():
    base = [0] * 256
    base[33] = base[5] = 1
    net = SR.StagedNet(((0, 1),), (12,), base=lambda s, t, i: base[i] if s == 0 else None)
    X1 = [1, 2] + [0] * 14
    X2 = list(X1)
    X2[11], X2[15] = 6, 5
    mt = R.StagedMeanTC(net, base_ea=lambda s, t, i: (1, 2) if (s, i) == (0, 33) else (0, 0))
    prev, has_prev = [list(X1), list(X2)], [1, 1]
    assert mt.step([CHECKER, CHECKER], prev, has_prev, 1, 0) == ([0, 0], [-1, -2], [-1, -2])
    assert mt.last_hits[(0, 0, 33)] == (-3, 2) and mt.last_m[(0, 0, 33)] == -2
    assert net.stages[0][(0, 33)] == 0 and ea_of(mt)[(0, 0, 33)] == (-1, 4)
    assert mt.last_hits[(0, 0, 1)] == (-3, 2) and net.stages[0][(0, 1)] == -2
    assert mt.last_hits[(0, 0, 0)] == (-14, 10) and mt.last_m[(0, 0, 0)] == -2
    assert not net.stages[1] and not net.promoted
    # an A of 41 bits
    big = (-3 << 38, (1 << 40) + 12345)
    mt = corner((12,), base_ea=lambda s, t, i: big if (s, i) == (0, 0) else (0, 0))
    mt.step([A], [list(Q2)], [1], 1, 1)
    assert table(mt.net) == {(0, 0, 2): 4096, (0, 0, 0): 1536}
    assert ea_of(mt)[(0, 0, 0)] == (big[0] + 2048, big[1] + 2048)


# ------------------------------------------------------------------ consequences, on the reference
T3 = ((0, 1), (1, 5), (2, 7))
BOUNDS = {1: (), 2: (5,), 3: (5, 8)}


def _boards(rng, n, hi=10, fill=0.6):
    return [[rng.randrange(1, hi) if rng.random() < fill else 0 for _ in range(16)]
            for _ in range(n)]


def _staged(rng, n, fill=0.6):
    """Boards whose largest exponents lie below 5, 8 and 11 in turn: with the bounds (5, 8) every
    stage occurs."""
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
    """(s, t, idx) -> a random (E, A) with |E| <= A, every branch of the rate among them."""
    def ea(s, t, i):
        r = random.Random(seed * 1000003 + s * 7919 + t * 65537 + i)
        a = (0, r.randrange(1, 1 << 16), (1 << 16) + r.randrange(-2, 3),
             r.randrange(1 << 40, 1 << 50))[r.randrange(4)]
        e = (0, a, -a, r.randrange(-a, a + 1))[r.randrange(4)]
        return e, a
    return ea


def _unset_pattern(net):
    """The entries a step has set: with one base, two nets have one UNSET pattern iff these agree."""
    return {(s, t, i) for s in range(net.S) for (t, i) in net.stages[s]}


@pytest.mark.parametrize("S", [1, 2, 3])
def test_consequence_1_and_9_a_zero_ea_is_the_staged_batch_mean_step(S):
    rng = random.Random(20 + S)
    base = _base(30 + S, S, 3, 2, upper=0.5)
    mt = R.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base))
    sd = R.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base), base_ea=seeded_ea(40 + S))
    mean = SR.StagedNet(T3, BOUNDS[S], base=base)
    boards, prev, has = _staged(rng, 40), _staged(rng, 40), [1] * 32 + [0] * 8
    a = mt.step(boards, [list(p) for p in prev], list(has), 3, 5)
    b = SMR.step(mean, boards, [list(p) for p in prev], list(has), 3, 5)
    c = sd.step(boards, [list(p) for p in prev], list(has), 3, 5)
    assert a == b == c and mt.last_hits == SMR.last_hits == sd.last_hits
    assert mt.net.stages == mean.stages and mt.net.promoted == mean.promoted
    assert ea_of(mt) == {k: (m, abs(m)) for k, m in mt.last_m.items() if m}
    assert any(c > 8 and d % c for d, c in mt.last_hits.values())
    # 9: the set entries after the call are the same from any ea
    assert _unset_pattern(sd.net) == _unset_pattern(mt.net) and sd.net.promoted == mean.promoted
    assert sd.net.stages != mt.net.stages
    if S > 1:
        assert mean.promoted and {k[0] for k in mt.last_hits} == set(range(S))


def test_consequence_2_s1_without_unset_is_the_single_table_rule_from_the_same_ea():
    rng = random.Random(11)
    base = _base(12, 1, 3, 2)
    one = seeded_ea(13)
    staged = R.StagedMeanTC(SR.StagedNet(T3, (), base=base), base_ea=one)
    plain = MTR.MeanTC(NR.Net(T3, base=base[0]), base_ea=lambda t, i: one(0, t, i))
    p1, h1 = _boards(rng, 40), [1] * 30 + [0] * 10
    p2, h2 = [list(p) for p in p1], list(h1)
    for _ in range(3):
        boards = _boards(rng, 40)
        boards[3] = list(CHECKER)
        assert staged.step(boards, p1, h1, 3, 5) == plain.step(boards, p2, h2, 3, 5)
        assert staged.last_hits == {(0, *k): v for k, v in plain.last_hits.items()}
        assert staged.last_m == {(0, *k): v for k, v in plain.last_m.items()}
        assert staged.net.stages[0] == plain.net.touched and not staged.net.promoted
        assert ea_of(staged) == {(0, *k): v for k, v in
                                 {k: (plain.E[k], plain.A[k]) for k in plain.A}.items()}
        assert (p1, h1) == (p2, h2)
    assert any(TR.rate(*one(*k)) not in (0, ONE) for k in staged.A)


def test_consequence_3_pairwise_distinct_staged_hits_are_the_staged_td_step():
    rng = random.Random(13)
    bounds = (9, 11)
    base = _base(14, 3, 3, 2, upper=0.5)
    ref = SR.StagedNet(T3, bounds, base=base)
    seen, prev = set(), []
    for _try in range(20000):
        hi = (9, 11, 12)[len(prev) % 3]  # exponents below hi: every stage occurs
        p = _boards(rng, 1, hi=hi, fill=0.9)[0]
        keys = [(ref.stage(p), *k) for k in ref.indices(p)]
        if len(set(keys)) == len(keys) and seen.isdisjoint(keys):
            seen.update(keys)
            prev.append(p)
            if len(prev) == 9:
                break
    assert len(prev) == 9 and {ref.stage(p) for p in prev} == {0, 1, 2}
    n = len(prev)
    boards = _boards(rng, n)
    a, b = R.StagedMeanTC(SR.StagedNet(T3, bounds, base=base)), SR.StagedNet(T3, bounds, base=base)
    pa, pb, ha, hb = [list(p) for p in prev], [list(p) for p in prev], [1] * n, [1] * n
    assert a.step(boards, pa, ha, 3, 5) == b.td_step(boards, pb, hb, 3, 5)
    assert a.net.stages == b.stages and a.net.promoted == b.promoted and a.net.promoted
    assert all(c == 1 for _d, c in a.last_hits.values()) and a.last_hits


@pytest.mark.parametrize("S", [1, 2, 3])
def test_consequences_4_and_5_repetition_and_a_zero_rate(S):
    rng = random.Random(15 + S)
    base = _base(16, S, 3, 2, upper=0.5)
    boards, prev, has = _staged(rng, 30), _staged(rng, 30), [1] * 25 + [0] * 5
    out = []
    for k in (1, 3):
        mt = R.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base), base_ea=seeded_ea(17))
        mt.step(boards * k, [list(p) for p in prev] * k, has * k, 3, 5)
        out.append((mt.net.stages, mt.net.promoted, dict(mt.last_hits), ea_of(mt)))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1] and out[0][3] == out[1][3]
    assert all(out[1][2][key] == (3 * d, 3 * c) for key, (d, c) in out[0][2].items())
    assert any(c > 8 for _d, c in out[0][2].values()) and out[0][3]
    # lr_num = 0: promotes, moves nothing, ea as it is
    still = R.StagedMeanTC(SR.StagedNet(T3, BOUNDS[S], base=base), base_ea=seeded_ea(17))
    td = SR.StagedNet(T3, BOUNDS[S], base=base)
    p, h = [list(x) for x in prev], list(has)
    _a, errs, deltas = still.step(boards, p, h, 0, 5)
    td.td_step(boards, [list(x) for x in prev], list(has), 0, 5)
    assert any(errs) and not any(deltas)
    assert still.last_hits == {} and ea_of(still) == {}
    assert still.net.stages == td.stages and still.net.promoted == td.promoted == out[0][1]
    assert table(still.net) == dict(still.net.promoted)
    assert bool(still.net.promoted) == (S > 1)
    assert p != prev  # prev and has_prev are still committed


def test_consequence_6_two_stages_of_one_index_keep_separate_d_c_and_e_a():
    """Anchor 1's third call says it with numbers; here on random batches: a (t, i) hit at two
    stages in one call has two (D, C), two m and, afterwards, two (E, A)."""
    rng = random.Random(18)
    base = _base(19, 3, 3, 2, upper=0.5)
    mt = R.StagedMeanTC(SR.StagedNet(T3, (5, 8), base=base))
    prev, has = _staged(rng, 40), [1] * 40
    for _ in range(3):
        mt.step(_staged(rng, 40), prev, has, 3, 5)
        has = [1] * 40
    shared = [(t, i) for (s, t, i) in mt.A if s == 0 and ((1, t, i) in mt.A or (2, t, i) in mt.A)]
    assert shared
    assert any(mt.get_ea(0, t, i) != mt.get_ea(s, t, i) for t, i in shared for s in (1, 2)
               if (s, t, i) in mt.A)
    both = [(t, i) for (s, t, i) in mt.last_hits if s == 0 and (1, t, i) in mt.last_hits]
    assert both and any(mt.last_hits[(0, *k)] != mt.last_hits[(1, *k)] for k in both)


def test_consequences_7_and_8_over_ten_steps():
    """|E| <= A stays, no A grows by more than the largest |delta| of the call (<= 2^31), which
    8 n hits of a sum rule would exceed, and the hits of a call are that call's alone (the
    reference keeps no workspace: acc all zero between calls)."""
    rng = random.Random(6)
    base = _base(7, 3, 3, 2, upper=0.5)
    mt = R.StagedMeanTC(SR.StagedNet(T3, (5, 8), base=base), base_ea=seeded_ea(8))
    boards, prev, has = _staged(rng, 32), _staged(rng, 32), [1] * 32
    for _k in range(10):
        keys = {(mt.net.stage(p), *k) for p, h in zip(prev, has) if h for k in mt.net.indices(p)}
        before = {k: mt.get_ea(*k) for k in set(mt.A) | keys}
        _a, _e, deltas = mt.step(boards, prev, has, 3, 5)
        top = max(abs(d) for d in deltas)
        for k, (e, a) in ea_of(mt).items():
            assert abs(e) <= a
            assert 0 <= a - before[k][1] <= top <= 1 << 31
        assert set(mt.last_hits) <= keys
        boards = _staged(rng, 32)
    assert any(c > 8 for _d, c in mt.last_hits.values())
    assert {k[0] for k in mt.A} == {0, 1, 2}
    mt.step(boards, prev, has, 0, 5)
    assert mt.last_hits == {}
    # the extreme: every delta INT32_MIN
    assert MR.floor_div(-(1 << 31) * 40, 40) == -(1 << 31)
    assert TR.step_of(-(1 << 31), ONE) == -(1 << 31)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (ntlambda, ntmean, ntmeantc, ntrestart, ntsearch, ntstage, nttc, ntuple,
                       search, stagemean, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean, ntmeantc)


def test_header_equals_exports_equals_signatures():
    from g2048 import stagemeantc

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = stagemeantc.load()
    assert set(names) == set(stagemeantc.SIGNATURES)
    assert _exported(stagemeantc.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_stagemeantc_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(stagemeantc.SIGNATURES["g2048_stagemeantc_step"][1]) == 16
    # g2048_stagemean_step's arguments with ea_dev after acc_dev
    args = [a.split()[-1].lstrip("*") for a in proto.split(",")]
    mean = open(os.path.join(ROOT, "include", "g2048_stagemean.h")).read()
    mean_args = [a.split()[-1].lstrip("*") for a in
                 re.search(r"g2048_stagemean_step\((.*?)\);", mean, re.S).group(1).split(",")]
    k = mean_args.index("acc_dev") + 1
    assert args == mean_args[:k] + ["ea_dev"] + mean_args[k:]
    proto = re.search(r"g2048_stagemeantc_acc_bytes\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == 2 == len(stagemeantc.SIGNATURES["g2048_stagemeantc_acc_bytes"][1])
    # the other twelve libraries keep their ABI: none of the new symbols
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_stagemeantc")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import stagemeantc

    out = subprocess.run(["readelf", "-d", stagemeantc.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other twelve stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS, G.STAGEMEAN_SRCS,
                  G.NTMEANTC_SRCS):
        assert set(G.STAGEMEANTC_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.STAGEMEANTC_SRCS[0]))
    assert open(G.STAGEMEANTC_STAMP).read().strip() == G.stagemeantc_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.STAGEMEAN_STAMP).read().strip() == G.stagemean_source_hash()
    assert open(G.NTMEANTC_STAMP).read().strip() == G.ntmeantc_source_hash()
    assert len(set(_hashes(G))) == 13


def test_stamp_follows_its_source_the_shared_headers_and_the_four_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp -- source_hash() included, which
    lists the file among the sources with stamps of their own; a change to the batch-mean header
    changes exactly the four batch-mean stamps; a change to either other shared csrc header
    changes the new stamp too; a change to each of g2048.h, g2048_ntuple.h, g2048_ntstage.h and
    g2048_stagemeantc.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.STAGEMEANTC_SRCS[0])).read()
    includes = re.findall(r'#include\s+"([^"]+)"', src)
    assert includes == ["../../include/g2048_stagemeantc.h", "g2048_board.hpp", G.NTUPLE_SHARED[0],
                        G.NTSTAGE_SHARED[0], G.NTMEAN_SHARED[0]]
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.STAGEMEANTC_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:12] == before[:12] and after[12] != before[12]
    with open(os.path.join(copy, G.NTMEAN_SHARED[0]), "a") as f:
        f.write("// changed\n")
    last = _hashes(G)
    assert last[:9] == before[:9] and all(last[k] != after[k] for k in (9, 10, 11, 12))
    for shared, also in ((G.NTUPLE_SHARED[0], 2), (G.NTSTAGE_SHARED[0], 6),
                         ("g2048_board.hpp", 1)):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
        now = _hashes(G)
        assert now[12] != last[12] and now[also] != last[also], shared
        if shared != "g2048_board.hpp":  # that one the main library includes too
            assert now[0] == before[0]
        last = now
    shared, include = last, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntstage.h",
                                "g2048_stagemeantc.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[12] != shared[12] and now[12] != last[12], header
        if header == "g2048_stagemeantc.h":
            assert now[:12] == shared[:12]
        last = now


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


def test_acc_bytes():
    import g2048._native as N
    from g2048 import stagemean, stagemeantc

    lib = stagemeantc.load()
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6, T8):
        for bounds in ((), (11,), (5, 8), tuple(range(1, 8))):
            want = 16 * (len(bounds) + 1) * len(tuples) * 16 ** len(tuples[0])
            assert lib.g2048_stagemeantc_acc_bytes(C.byref(_spec(tuples)),
                                                   C.byref(_stages(bounds))) == want
            assert stagemeantc.acc_bytes(tuples, bounds) == want
            assert stagemean.acc_bytes(tuples, bounds) == want
    assert stagemeantc.acc_bytes(NR.TUPLES_4x6, (11,)) == 2 << 30
    full = _spec(tuple(tuple(range(k, k + 6)) for k in range(8)))
    assert lib.g2048_stagemeantc_acc_bytes(C.byref(full),
                                           C.byref(_stages(tuple(range(1, 8))))) == 16 << 30
    assert lib.g2048_stagemeantc_acc_bytes(None, C.byref(_stages(()))) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_stagemeantc_last_error()
    assert lib.g2048_stagemeantc_acc_bytes(C.byref(_spec(NR.TUPLES_2x4)), None) == N.G2048_EINVAL
    assert b"stages" in lib.g2048_stagemeantc_last_error()
    with pytest.raises(ValueError):
        stagemeantc.acc_bytes(NR.TUPLES_2x4, (8, 5))


RATE_GRID_A = [0, 1, 2, 3, 7, 255, (1 << 15), (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 17) - 1,
               1 << 17, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) + 12345, (1 << 47) - 1,
               1 << 61, (1 << 62) - 1]


def test_rate_equals_the_reference_and_the_single_table_library_on_a_grid():
    import g2048._native as N
    from g2048 import ntmeantc, stagemeantc

    lib, one = stagemeantc.load(), ntmeantc.load()
    assert stagemeantc.RATE_BITS == ntmeantc.RATE_BITS == TR.RATE_BITS == 16
    assert stagemeantc.MAX_A == ntmeantc.MAX_A == TR.MAX_A == (1 << 62) - 1
    rng = random.Random(8)
    seen = set()
    for a in RATE_GRID_A:
        es = {0, a, -a, a // 2, -(a // 2), a // 3, a - 1 if a else 0, 1 if a else 0}
        es |= {rng.randrange(-a, a + 1) for _ in range(8)}
        for e in es:
            want = TR.rate(e, a)
            assert lib.g2048_stagemeantc_rate(e, a) == want == one.g2048_ntmeantc_rate(e, a), \
                (e, a)
            assert stagemeantc.rate(e, a) == want == stagemeantc.StagedMeanTCState.rate(e, a)
            seen.add(want)
        assert lib.g2048_stagemeantc_rate(a, a) == ONE == lib.g2048_stagemeantc_rate(-a, a)
    assert {0, ONE, 1 << 15} <= seen and len(seen) > 40
    # nttc_ref's anchors, and the rates of this reference's anchor 1
    for e, a, want in ((1, 3, 21845), (32768, 65535, 32768), (32769, 65536, 32768),
                       (3, 65537, 2), (-3 << 38, (1 << 40) + 12345, 49152),
                       (6144, 12288, 32768), (-21504, 39936, 35288), (0, 7, 0)):
        assert lib.g2048_stagemeantc_rate(e, a) == want
    # the domain errors, those of g2048_ntmeantc_rate
    for e, a, word in ((0, -1, b"A ="), (0, 1 << 62, b"A ="), (2, 1, b"exceeds"),
                       (-2, 1, b"exceeds"), (1, 0, b"exceeds"), (-(1 << 63), 5, b"exceeds")):
        assert lib.g2048_stagemeantc_rate(e, a) == N.G2048_EINVAL == one.g2048_ntmeantc_rate(e, a)
        assert word in lib.g2048_stagemeantc_last_error()
        assert b"stagemeantc_rate" in lib.g2048_stagemeantc_last_error()
        with pytest.raises(ValueError):
            stagemeantc.rate(e, a)
        with pytest.raises(ValueError):
            TR.rate(e, a)


FAKE, FAKE_EA = 1 << 20, 1 << 30  # aligned addresses that stand in for device memory


def _every_entry_point(lib, s, st):
    """Each entry point's message on a call that must be refused."""
    import g2048._native as N

    calls = [lambda: lib.g2048_stagemeantc_acc_bytes(C.byref(s), C.byref(st)),
             lambda: lib.g2048_stagemeantc_step(C.byref(s), C.byref(st), FAKE, FAKE, FAKE_EA, FAKE,
                                                4, FAKE, FAKE, 1, 10, FAKE, FAKE, FAKE, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        yield lib.g2048_stagemeantc_last_error()


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
    (dict(bounds=(), n_stages=-1), b"n_stages"),
    (dict(bounds=(1, 2, 3, 4, 5, 6, 7), n_stages=9), b"n_stages"),
    (dict(bounds=(0,)), b"outside [1, 27]"),
    (dict(bounds=(28,)), b"outside [1, 27]"),
    (dict(bounds=(5, 200)), b"outside [1, 27]"),
    (dict(bounds=(5, 5)), b"strictly increasing"),
    (dict(bounds=(8, 5)), b"strictly increasing"),
    (dict(bounds=(5, 8, 7)), b"strictly increasing"),
    (dict(bounds=(5, 8), n_stages=2), b"unused bound"),
    (dict(bounds=(5,), n_stages=1), b"unused bound"),
    (dict(bounds=(0, 0, 0, 0, 0, 0, 3), n_stages=3), b"outside [1, 27]"),
]


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused_by_every_entry_point(kw, word):
    from g2048 import stagemeantc

    for msg in _every_entry_point(stagemeantc.load(), _spec(**kw), _stages((5, 8))):
        assert word in msg, msg


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused_by_every_entry_point(kw, word):
    from g2048 import stagemeantc

    for msg in _every_entry_point(stagemeantc.load(), _spec(NR.TUPLES_2x4), _stages(**kw)):
        assert word in msg, msg


def test_bad_arguments_are_refused_before_any_device_work():
    """Argument checks run before any device work: G2048_EINVAL with a message, on a machine
    without a GPU, for a device id that does not exist.  The pointers are never dereferenced (fake
    aligned addresses stand in for device memory).  g2048_stagemean_step's checks plus ea's."""
    import g2048._native as N
    from g2048 import stagemeantc

    lib = stagemeantc.load()
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))
    size = stagemeantc.acc_bytes(NR.TUPLES_2x4, (5, 8))
    assert size == 3 * 16 * 2 * 65536

    def step(spec=s, stages=st, lut=FAKE, acc=FAKE, ea=FAKE_EA, boards=FAKE, n=4, prev=FAKE,
             has_prev=FAKE, lr_num=1, lr_shift=10, action=FAKE, delta=FAKE, err=FAKE):
        return lib.g2048_stagemeantc_step(C.byref(spec) if spec is not None else None,
                                          C.byref(stages) if stages is not None else None, lut,
                                          acc, ea, boards, n, prev, has_prev, lr_num, lr_shift,
                                          action, delta, err, 1 << 20, None)

    cases = [(dict(spec=None), b"spec"), (dict(stages=None), b"stages"),
             (dict(lut=None), b"NULL"), (dict(acc=None), b"acc_dev is NULL"),
             (dict(ea=None), b"ea_dev is NULL"), (dict(boards=None), b"NULL"),
             (dict(prev=None), b"NULL"), (dict(has_prev=None), b"NULL"),
             (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=FAKE + 2), b"aligned"), (dict(acc=FAKE + 8), b"acc_dev must be 16-byte"),
             (dict(ea=FAKE_EA + 8), b"ea_dev must be 16-byte"),
             # ea == acc, and ea overlapping acc by one entry from either side: the size is that
             # of all S stages, not of one
             (dict(ea=FAKE), b"overlaps"), (dict(ea=FAKE + size - 16), b"overlaps"),
             (dict(acc=FAKE_EA + size - 16), b"overlaps"),
             (dict(ea=FAKE + size // 3), b"overlaps"),
             (dict(boards=FAKE + 4), b"aligned"), (dict(prev=FAKE + 8), b"aligned"),
             (dict(delta=FAKE + 2), b"aligned"), (dict(err=FAKE + 4), b"aligned")]
    for kw, word in cases:
        assert step(**kw) == N.G2048_EINVAL, kw
        msg = lib.g2048_stagemeantc_last_error()
        assert word in msg and b"stagemeantc_step" in msg, (kw, msg)


# ------------------------------------------------------------------ the Python side
def test_the_default_rate_is_the_single_table_rules():
    from g2048 import ntmeantc, ntstage, ntuple, stagemeantc

    assert stagemeantc.default_meantc_lr_shift is ntmeantc.default_meantc_lr_shift
    src = open(stagemeantc.__file__).read()
    assert "lr_shift = default_meantc_lr_shift(net.spec)" in src
    assert not hasattr(ntstage.StagedNTupleNetwork, "meantc_step")
    assert ntmeantc.default_meantc_lr_shift(ntuple.TUPLES_2x4) == 4


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmeantc, ntstage, ntuple, stagemeantc

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stagemeantc.StagedMeanTCState(net)
    for t in (st.acc, st.ea):
        assert t.shape == (3, 2, 65536, 2) and t.dtype == torch.int64 and not t.any()
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert t.numel() * 8 == stagemeantc.acc_bytes(ntuple.TUPLES_2x4, (5, 8))
    assert st.acc.data_ptr() != st.ea.data_ptr()
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        st.meantc_step(boards, boards.clone(), u8, 1, 6, u8.clone(), i32)
    with pytest.raises(g2048.NativeError):
        stagemeantc.StagedMeanTCTrainer(net, 256)
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for bad in (None, plain):  # staged networks only; the message points to the single-table class
        with pytest.raises(TypeError, match="MeanTCState"):
            stagemeantc.StagedMeanTCState(bad)
        with pytest.raises(TypeError, match="MeanTCTrainer"):
            stagemeantc.StagedMeanTCTrainer(bad, 256)
    # the single-table classes keep refusing staged networks, with their present message
    for cls, args in ((ntmeantc.MeanTCState, ()), (ntmeantc.MeanTCTrainer, (256,))):
        with pytest.raises(TypeError, match="staged tables are not supported"):
            cls(net, *args)
    assert g2048.stagemeantc is stagemeantc
    assert g2048.StagedMeanTCState is stagemeantc.StagedMeanTCState
    assert g2048.StagedMeanTCTrainer is stagemeantc.StagedMeanTCTrainer
    assert issubclass(stagemeantc.StagedMeanTCTrainer, ntuple.NTupleTrainer)
    assert {"stagemeantc", "StagedMeanTCState", "StagedMeanTCTrainer"} <= set(g2048.__all__)


def _fill(ea, seed):
    g = torch.Generator().manual_seed(seed)
    ea[..., 1] = torch.randint(0, 1 << 50, ea.shape[:-1], generator=g)
    ea[..., 0] = ea[..., 1] // 3 - 5


def test_ea_round_trips_through_a_file(tmp_path):
    from g2048 import ntstage, ntuple, stagemeantc

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    st = stagemeantc.StagedMeanTCState(net)
    _fill(st.ea, 9)
    assert set(st.state_dict()) == {"tuples", "bounds", "ea"}
    st.save(tmp_path / "own.pt")
    back = stagemeantc.StagedMeanTCState.load(tmp_path / "own.pt", net)
    assert torch.equal(back.ea, st.ea) and not back.acc.any() and back.ea is not st.ea
    loaded = torch.load(tmp_path / "own.pt", weights_only=True)
    assert set(loaded) == {"tuples", "bounds", "ea"}
    assert loaded["bounds"].tolist() == [5, 8]
    for other in (ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu"),
                  ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 9), device="cpu"),
                  ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5,), device="cpu")):
        with pytest.raises(ValueError):
            stagemeantc.StagedMeanTCState.load(tmp_path / "own.pt", other)
    good = st.state_dict()
    with pytest.raises(ValueError):
        st.load_state_dict(dict(good, ea=st.ea.to(torch.int32)))
    with pytest.raises(ValueError):
        st.load_state_dict(dict(good, ea=st.ea[:2]))


def test_from_state_puts_a_single_tables_ea_into_stage_0():
    from g2048 import ntmeantc, ntstage, ntuple, stagemeantc

    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    one = ntmeantc.MeanTCState(plain)
    _fill(one.ea, 10)
    staged = ntstage.StagedNTupleNetwork.from_network(plain, (5, 8))
    st = stagemeantc.StagedMeanTCState.from_state(one, staged)
    assert st.net is staged and st.ea.shape == (3, 2, 65536, 2)
    assert torch.equal(st.ea[0], one.ea) and not st.ea[1:].any() and not st.acc.any()
    assert st.ea.data_ptr() != one.ea.data_ptr()
    other = ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), (5, 8), device="cpu")
    with pytest.raises(ValueError):
        stagemeantc.StagedMeanTCState.from_state(one, other)
    with pytest.raises(TypeError):
        stagemeantc.StagedMeanTCState.from_state(st, staged)
    with pytest.raises(TypeError):
        stagemeantc.StagedMeanTCState.from_state(one, plain)
