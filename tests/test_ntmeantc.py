"""CPU-side checks of temporal-coherence learning on the batch-mean rule: the Python restatement
(tests/ntmeantc_ref.py) reproduces its hand-computed anchors and has the header's consequences, and
the boundary of libg2048_ntmeantc.so (header == exports == SIGNATURES, build stamps, the host-only
rate, argument validation without a GPU, the Python side's refusals and its save / load)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest
import torch

import ntmean_ref as MR
import ntmeantc_ref as R
import nttc_ref as TR
import ntuple_ref as NR
from g2048 import ntmeantc as _library

_library.load()  # every test of this file belongs to the library: without it the file fails here

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntmeantc.h")
NAMES = ["g2048_ntmeantc_acc_bytes", "g2048_ntmeantc_last_error", "g2048_ntmeantc_rate",
         "g2048_ntmeantc_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
P2, P3 = [2] + [0] * 15, [3] + [0] * 15
ONE = 1 << 16


def corner():
    return NR.Net(((0,),), base=[[1024 * i for i in range(16)]])


def ea_of(mt):
    return {k: (mt.E[k], mt.A[k]) for k in mt.A}


# ------------------------------------------------------------------ the reference's anchors
def test_anchor_1_three_boards_from_a_zero_ea():
    mt = R.MeanTC(corner())
    prev, has_prev = [list(P2), list(P3), list(P3)], [1, 1, 1]
    out = mt.step([A, CHECKER, CHECKER], prev, has_prev, 1, 1)
    assert out == ([2, 0, 0], [4096, -6144, -6144], [2048, -3072, -3072])
    assert mt.last_hits == {(0, 2): (4096, 2), (0, 3): (-12288, 4), (0, 0): (-24576, 18)}
    assert mt.last_m == {(0, 2): 2048, (0, 3): -3072, (0, 0): -1366}
    assert mt.net.touched == {(0, 2): 4096, (0, 3): 0, (0, 0): -1366}
    assert ea_of(mt) == {(0, 2): (2048, 2048), (0, 3): (-3072, 3072), (0, 0): (-1366, 1366)}
    assert has_prev == [1, 0, 0] and prev == [P2, P3, P3]
    # the batch-mean reference leaves the same table
    mean = corner()
    MR.step(mean, [A, CHECKER, CHECKER], [list(P2), list(P3), list(P3)], [1, 1, 1], 1, 1)
    assert mean.touched == mt.net.touched


def test_anchor_2_the_batch_again_and_a_third_time():
    mt = R.MeanTC(corner())
    boards = [A, CHECKER, CHECKER]
    mt.step(boards, [list(P2), list(P3), list(P3)], [1, 1, 1], 1, 1)
    out = mt.step(boards, [list(P2), list(P3), list(P3)], [1, 1, 1], 1, 1)
    assert out == ([2, 0, 0], [4096, 8196, 8196], [2048, 4098, 4098])
    assert mt.last_hits == {(0, 2): (4096, 2), (0, 3): (16392, 4), (0, 0): (61464, 18)}
    assert mt.last_m == {(0, 2): 2048, (0, 3): 4098, (0, 0): 3414}
    assert mt.net.touched == {(0, 2): 6144, (0, 3): 4098, (0, 0): 2048}
    assert ea_of(mt) == {(0, 2): (4096, 4096), (0, 3): (1026, 7170), (0, 0): (2048, 4780)}
    # the rates the entries hold now: entry 0 and entry 3 below 2^16
    assert TR.rate(2048, 4780) == 28079 and 4780 * 28079 == 134217620 < 2048 << 16
    assert TR.rate(1026, 7170) == 9377 and TR.rate(4096, 4096) == ONE
    out = mt.step(boards, [list(P2), list(P3), list(P3)], [1, 1, 1], 1, 1)
    assert out == ([2, 0, 0], [4096, -20484, -20484], [2048, -10242, -10242])
    assert mt.last_m == {(0, 2): 2048, (0, 3): -10242, (0, 0): -6146}
    assert TR.step_of(-10242, 9377) == -1466 and TR.step_of(-6146, 28079) == -2634
    assert mt.net.touched == {(0, 2): 8192, (0, 3): 2632, (0, 0): -586}
    assert ea_of(mt) == {(0, 2): (6144, 6144), (0, 3): (-9216, 17412), (0, 0): (-4098, 10926)}
    # batch-mean without the rate moves entry 0 by the whole m
    assert 2048 - 6146 != -586


def test_anchor_3_an_entry_at_rate_zero_does_not_move_and_still_accumulates():
    mt = R.MeanTC(corner(), base_ea=lambda t, i: (0, 7) if i == 0 else (0, 0))
    assert TR.rate(0, 7) == 0
    assert mt.step([A], [list(P2)], [1], 1, 1) == ([2], [4096], [2048])
    assert mt.last_m == {(0, 2): 2048, (0, 0): 2048}
    assert mt.net.touched == {(0, 2): 4096, (0, 0): 0}
    assert ea_of(mt) == {(0, 2): (2048, 2048), (0, 0): (2048, 2055)}


def test_anchor_4_the_two_floors_compose():
    base = [0] * 256
    base[33] = base[5] = 1
    net = NR.Net(((0, 1),), base=[base])
    X1 = [1, 2] + [0] * 14
    X2 = list(X1)
    X2[11], X2[15] = 6, 5
    assert [i for _t, i in net.indices(X1)] == [33, 0, 0, 0, 1, 0, 0, 0]
    assert [i for _t, i in net.indices(X2)] == [33, 0, 0, 5, 1, 0, 0, 101]
    assert (net.V(X1), net.V(X2)) == (1, 2)
    mt = R.MeanTC(net, base_ea=lambda t, i: (1, 2) if i == 33 else (0, 0))
    prev, has_prev = [list(X1), list(X2)], [1, 1]
    assert mt.step([CHECKER, CHECKER], prev, has_prev, 1, 0) == ([0, 0], [-1, -2], [-1, -2])
    assert mt.last_hits[(0, 33)] == (-3, 2) and mt.last_m[(0, 33)] == -2
    assert MR.floor_div(-3, 2) == -2 and TR.rate(1, 2) == 1 << 15
    assert TR.step_of(-2, 1 << 15) == -1
    assert net.touched[(0, 33)] == 0 and ea_of(mt)[(0, 33)] == (-1, 4)
    assert mt.last_hits[(0, 1)] == (-3, 2) and net.touched[(0, 1)] == -2
    assert mt.last_hits[(0, 0)] == (-14, 10) and mt.last_m[(0, 0)] == -2
    assert has_prev == [0, 0] and prev == [X1, X2]


def test_anchor_5_an_a_of_41_bits_shifts_both_operands():
    big = (-3 << 38, (1 << 40) + 12345)
    assert TR.shift_of(big[1]) == 25 and TR.rate(*big) == 49152
    mt = R.MeanTC(corner(), base_ea=lambda t, i: big if i == 0 else (0, 0))
    mt.step([A], [list(P2)], [1], 1, 1)
    assert mt.net.touched == {(0, 2): 4096, (0, 0): 1536}
    assert ea_of(mt)[(0, 0)] == (big[0] + 2048, big[1] + 2048)


# ------------------------------------------------------------------ the header's consequences
def small_batch(rng, n, hi=6):
    """Boards and previous afterstates of small exponents on few cells, so entries are shared."""
    def board():
        return [rng.randrange(hi) if rng.random() < 0.6 else 0 for _ in range(16)]
    return [board() for _ in range(n)], [board() for _ in range(n)], \
        [int(rng.random() < 0.85) for _ in range(n)]


def random_base(rng, tuples):
    return [[rng.randrange(-(1 << 20), 1 << 20) for _ in range(16 ** len(tuples[0]))]
            for _ in tuples]


def seeded_ea(seed):
    """(t, idx) -> a random (E, A) with |E| <= A, every branch of the rate among them."""
    def ea(t, i):
        r = random.Random(seed * 1000003 + t * 65537 + i)
        a = (0, r.randrange(1, 1 << 16), (1 << 16) + r.randrange(-2, 3),
             r.randrange(1 << 40, 1 << 50))[r.randrange(4)]
        e = (0, a, -a, r.randrange(-a, a + 1))[r.randrange(4)]
        return e, a
    return ea


T2M2 = ((0, 1), (1, 5))


def test_consequence_1_zero_ea_is_the_batch_mean_step():
    rng = random.Random(1)
    base = random_base(rng, T2M2)
    boards, prev, has = small_batch(rng, 24)
    mt, mean = R.MeanTC(NR.Net(T2M2, base=base)), NR.Net(T2M2, base=base)
    a = mt.step(boards, [list(p) for p in prev], list(has), 3, 6)
    b = MR.step(mean, boards, [list(p) for p in prev], list(has), 3, 6)
    assert a == b and mt.last_hits == MR.last_hits
    assert {k: v for k, v in mean.touched.items() if mt.last_m[k]} == mt.net.touched
    assert all(mean.touched[k] == mean.base(*k) for k, m in mt.last_m.items() if m == 0)
    assert ea_of(mt) == {k: (m, abs(m)) for k, m in mt.last_m.items() if m}
    assert any(c > 1 and d % c for d, c in mt.last_hits.values())


def test_consequence_2_pairwise_distinct_hits_are_the_tc_step():
    rng = random.Random(2)
    tuples = NR.TUPLES_2x4
    ref, seen, prev = NR.Net(tuples), set(), []
    while len(prev) < 12:
        p = [rng.randrange(1, 12) for _ in range(16)]
        keys = ref.indices(p)
        if len(set(keys)) == len(keys) and seen.isdisjoint(keys):
            seen.update(keys)
            prev.append(p)
    boards = [[rng.randrange(0, 8) for _ in range(16)] for _ in prev]
    base = {}

    def lut(t, i):
        return base.setdefault((t, i), random.Random(t * 70001 + i).randrange(-(1 << 20), 1 << 20))

    mt = R.MeanTC(NR.Net(tuples, base=lut), base_ea=seeded_ea(3))
    tc = TR.TC(NR.Net(tuples, base=lut), base_ea=seeded_ea(3))
    a = mt.step(boards, [list(p) for p in prev], [1] * 12, 3, 6)
    b = tc.step(boards, [list(p) for p in prev], [1] * 12, 3, 6)
    assert a == b and any(a[2])
    assert all(c == 1 for _d, c in mt.last_hits.values())
    assert mt.net.touched == tc.net.touched and ea_of(mt) == {k: (tc.E[k], tc.A[k]) for k in tc.A}
    assert any(TR.rate(*seeded_ea(3)(*k)) not in (0, ONE) for k in mt.A)


def test_consequences_3_and_4_repetition_and_a_zero_rate():
    rng = random.Random(4)
    base = random_base(rng, T2M2)
    boards, prev, has = small_batch(rng, 20)
    once = R.MeanTC(NR.Net(T2M2, base=base), base_ea=seeded_ea(5))
    once.step(boards, [list(p) for p in prev], list(has), 3, 6)
    thrice = R.MeanTC(NR.Net(T2M2, base=base), base_ea=seeded_ea(5))
    thrice.step(boards * 3, [list(p) for p in prev] * 3, list(has) * 3, 3, 6)
    assert thrice.last_hits == {k: (3 * d, 3 * c) for k, (d, c) in once.last_hits.items()}
    assert thrice.net.touched == once.net.touched and once.net.touched
    assert ea_of(thrice) == ea_of(once)
    still = R.MeanTC(NR.Net(T2M2, base=base), base_ea=seeded_ea(5))
    p, h = [list(x) for x in prev], list(has)
    _a, errs, deltas = still.step(boards, p, h, 0, 6)
    assert any(errs) and not any(deltas)
    assert still.last_hits == {} and still.net.touched == {} and ea_of(still) == {}
    assert p != prev  # prev and has_prev are still committed


def test_consequences_5_6_and_7_over_ten_steps():
    """|E| <= A stays, no A grows by more than 2^31 in a call -- here by no more than the largest
    |delta| of the call, which 8 n hits of the sum rule would exceed -- and the hits of a call are
    that call's alone (the reference keeps no workspace: acc all zero between calls)."""
    rng = random.Random(6)
    base = random_base(rng, T2M2)
    mt = R.MeanTC(NR.Net(T2M2, base=base), base_ea=seeded_ea(7))
    boards, prev, has = small_batch(rng, 32)
    for _k in range(10):
        before = {k: mt.get_ea(*k) for k in set(mt.A) | {key for p in prev
                                                         for key in mt.net.indices(p)}}
        _a, _e, deltas = mt.step(boards, prev, has, 3, 6)
        top = max(abs(d) for d in deltas)
        for k, (e, a) in ea_of(mt).items():
            assert abs(e) <= a
            grown = a - before.get(k, (0, 0))[1]
            assert 0 <= grown <= top <= 1 << 31
        assert set(mt.last_hits) <= {key for p in before for key in [p]}
        boards = [[rng.randrange(6) if rng.random() < 0.6 else 0 for _ in range(16)]
                  for _ in boards]
    assert any(c > 8 for _d, c in mt.last_hits.values())
    mt.step(boards, prev, has, 0, 6)
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
    from g2048 import (ntlambda, ntmean, ntrestart, ntsearch, ntstage, nttc, ntuple, search,
                       stagemean, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean)


def test_header_equals_exports_equals_signatures():
    from g2048 import ntmeantc

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntmeantc.load()
    assert set(names) == set(ntmeantc.SIGNATURES)
    assert _exported(ntmeantc.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_ntmeantc_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(ntmeantc.SIGNATURES["g2048_ntmeantc_step"][1]) == 15
    # the other eleven libraries keep their ABI: none of the new symbols
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_ntmeantc")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntmeantc

    out = subprocess.run(["readelf", "-d", ntmeantc.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other eleven stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS, G.STAGEMEAN_SRCS):
        assert set(G.NTMEANTC_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTMEANTC_SRCS[0]))
    assert open(G.NTMEANTC_STAMP).read().strip() == G.ntmeantc_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.NTMEAN_STAMP).read().strip() == G.ntmean_source_hash()
    assert open(G.NTTC_STAMP).read().strip() == G.nttc_source_hash()
    assert len(set(_hashes(G))) == 12


def test_stamp_follows_its_source_the_shared_header_and_the_three_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp; a change to the batch-mean header
    changes the three batch-mean stamps and none of the other nine; a change to the shared csrc
    header changes the new stamp too; a change to each of g2048.h, g2048_ntuple.h and
    g2048_ntmeantc.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.NTMEANTC_SRCS[0])).read()
    assert f'#include "{G.NTUPLE_SHARED[0]}"' in src
    # the batch-mean step and the rate come from the shared headers, not from another source
    assert f'#include "{G.NTMEAN_SHARED[0]}"' in src
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTMEANTC_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:11] == before[:11] and after[11] != before[11]
    with open(os.path.join(copy, G.NTMEAN_SHARED[0]), "a") as f:
        f.write("// changed\n")
    mean = _hashes(G)
    assert mean[:9] == before[:9] and all(mean[k] != after[k] for k in (9, 10, 11))
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    shared = _hashes(G)
    assert shared[0] == before[0] and shared[11] != mean[11] and shared[2] != before[2]
    last, include = shared, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntmeantc.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[11] != shared[11] and now[11] != last[11], header
        if header == "g2048_ntmeantc.h":
            assert now[:11] == shared[:11]
        last = now


def _spec(tuples, n_tuples=None, n_cells=None):
    from g2048 import ntuple

    s = ntuple._Spec(len(tuples) if n_tuples is None else n_tuples,
                     len(tuples[0]) if n_cells is None else n_cells)
    for t, cells in enumerate(tuples):
        for k, c in enumerate(cells):
            s.cells[t][k] = c
    return s


def test_acc_bytes():
    import g2048._native as N
    from g2048 import ntmean, ntmeantc

    lib = ntmeantc.load()
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6, T8):
        want = 16 * len(tuples) * 16 ** len(tuples[0])
        assert lib.g2048_ntmeantc_acc_bytes(C.byref(_spec(tuples))) == want
        assert ntmeantc.acc_bytes(tuples) == want == ntmean.acc_bytes(tuples)
    assert lib.g2048_ntmeantc_acc_bytes(None) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_ntmeantc_last_error()


RATE_GRID_A = [0, 1, 2, 3, 7, 255, (1 << 15), (1 << 16) - 1, 1 << 16, (1 << 16) + 1, (1 << 17) - 1,
               1 << 17, (1 << 31) - 1, 1 << 31, (1 << 32) + 5, (1 << 40) + 12345, (1 << 47) - 1,
               1 << 61, (1 << 62) - 1]


def test_rate_equals_the_reference_and_the_tc_library_on_a_grid():
    import g2048._native as N
    from g2048 import ntmeantc, nttc

    lib, tc = ntmeantc.load(), nttc.load()
    assert ntmeantc.RATE_BITS == nttc.RATE_BITS == TR.RATE_BITS == 16
    assert ntmeantc.MAX_A == nttc.MAX_A == TR.MAX_A == (1 << 62) - 1
    rng = random.Random(8)
    seen = set()
    for a in RATE_GRID_A:
        es = {0, a, -a, a // 2, -(a // 2), a // 3, a - 1 if a else 0, 1 if a else 0}
        es |= {rng.randrange(-a, a + 1) for _ in range(8)}
        for e in es:
            want = TR.rate(e, a)
            assert lib.g2048_ntmeantc_rate(e, a) == want == tc.g2048_nttc_rate(e, a), (e, a)
            assert ntmeantc.rate(e, a) == want == ntmeantc.MeanTCState.rate(e, a)
            seen.add(want)
        assert lib.g2048_ntmeantc_rate(a, a) == ONE == lib.g2048_ntmeantc_rate(-a, a)
    assert {0, ONE, 1 << 15} <= seen and len(seen) > 40
    # nttc_ref's anchors
    for e, a, want in ((1, 3, 21845), (32768, 65535, 32768), (32769, 65536, 32768),
                       (3, 65537, 2), (-3 << 38, (1 << 40) + 12345, 49152)):
        assert lib.g2048_ntmeantc_rate(e, a) == want
    # the domain errors, those of g2048_nttc_rate
    for e, a, word in ((0, -1, b"A ="), (0, 1 << 62, b"A ="), (2, 1, b"exceeds"),
                       (-2, 1, b"exceeds"), (1, 0, b"exceeds"), (-(1 << 63), 5, b"exceeds")):
        assert lib.g2048_ntmeantc_rate(e, a) == N.G2048_EINVAL == tc.g2048_nttc_rate(e, a)
        assert word in lib.g2048_ntmeantc_last_error()
        assert b"ntmeantc_rate" in lib.g2048_ntmeantc_last_error()
        with pytest.raises(ValueError):
            ntmeantc.rate(e, a)
        with pytest.raises(ValueError):
            TR.rate(e, a)


BAD_SPECS = [
    (dict(tuples=((0,),), n_tuples=0), b"n_tuples"),
    (dict(tuples=((0,),), n_tuples=9), b"n_tuples"),
    (dict(tuples=((0,),), n_cells=0), b"n_cells"),
    (dict(tuples=((0,),), n_cells=7), b"n_cells"),
    (dict(tuples=((0, 1), (2, 16))), b"not a board cell"),
    (dict(tuples=((0, 1, 2), (3, 4, 3))), b"twice"),
]
FAKE, FAKE_EA = 1 << 20, 1 << 30  # aligned addresses that stand in for device memory


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused_by_every_entry_point(kw, word):
    import g2048._native as N
    from g2048 import ntmeantc

    lib = ntmeantc.load()
    s = _spec(**kw)
    calls = [lambda: lib.g2048_ntmeantc_acc_bytes(C.byref(s)),
             lambda: lib.g2048_ntmeantc_step(C.byref(s), FAKE, FAKE, FAKE_EA, FAKE, 4, FAKE, FAKE,
                                             1, 10, FAKE, FAKE, FAKE, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_ntmeantc_last_error(), lib.g2048_ntmeantc_last_error()


def test_bad_arguments_are_refused_before_any_device_work():
    """Argument checks run before any device work: G2048_EINVAL with a message, on a machine
    without a GPU, for a device id that does not exist.  The pointers are never dereferenced (fake
    aligned addresses stand in for device memory)."""
    import g2048._native as N
    from g2048 import ntmeantc

    lib = ntmeantc.load()
    s = _spec(NR.TUPLES_2x4)
    size = ntmeantc.acc_bytes(NR.TUPLES_2x4)

    def step(spec=s, lut=FAKE, acc=FAKE, ea=FAKE_EA, boards=FAKE, n=4, prev=FAKE, has_prev=FAKE,
             lr_num=1, lr_shift=10, action=FAKE, delta=FAKE, err=FAKE):
        return lib.g2048_ntmeantc_step(C.byref(spec) if spec is not None else None, lut, acc, ea,
                                       boards, n, prev, has_prev, lr_num, lr_shift, action, delta,
                                       err, 1 << 20, None)

    cases = [(dict(spec=None), b"spec"), (dict(lut=None), b"NULL"), (dict(acc=None), b"acc_dev"),
             (dict(ea=None), b"ea_dev is NULL"), (dict(boards=None), b"NULL"),
             (dict(prev=None), b"NULL"), (dict(has_prev=None), b"NULL"),
             (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=FAKE + 2), b"aligned"), (dict(acc=FAKE + 8), b"acc_dev must be 16-byte"),
             (dict(ea=FAKE_EA + 8), b"ea_dev must be 16-byte"),
             (dict(ea=FAKE), b"overlaps"), (dict(ea=FAKE + size - 16), b"overlaps"),
             (dict(acc=FAKE_EA + size - 16), b"overlaps"),
             (dict(boards=FAKE + 4), b"aligned"), (dict(prev=FAKE + 8), b"aligned"),
             (dict(delta=FAKE + 2), b"aligned"), (dict(err=FAKE + 4), b"aligned")]
    for kw, word in cases:
        assert step(**kw) == N.G2048_EINVAL, kw
        msg = lib.g2048_ntmeantc_last_error()
        assert word in msg and b"ntmeantc_step" in msg, (kw, msg)


# ------------------------------------------------------------------ the Python side
def test_the_default_rate_reuses_default_mean_lr_shift():
    """8 T * lr = 1, two bits above the batch-mean rule's 1/4, at any batch width."""
    from g2048 import ntmean, ntmeantc, ntuple

    assert ntmeantc.default_mean_lr_shift is ntmean.default_mean_lr_shift
    assert ntmeantc.default_meantc_lr_shift(ntuple.TUPLES_2x4) == 4
    assert ntmeantc.default_meantc_lr_shift(ntuple.TUPLES_4x6) == 5
    assert ntmeantc.default_meantc_lr_shift(ntuple.NTupleSpec(ntuple.TUPLES_4x6)) == 5
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for T in range(1, 9):
        assert ntmeantc.default_meantc_lr_shift(T8[:T]) == ntmean.default_mean_lr_shift(T8[:T]) - 2
        assert 8 * T <= 1 << ntmeantc.default_meantc_lr_shift(T8[:T]) < 16 * T
    src = open(ntmeantc.__file__).read()
    assert "lr_shift = default_meantc_lr_shift(net.spec)" in src


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmeantc, ntstage, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    st = ntmeantc.MeanTCState(net)
    for t in (st.acc, st.ea):
        assert t.shape == (2, 65536, 2) and t.dtype == torch.int64 and not t.any()
        assert t.is_contiguous() and t.data_ptr() % 16 == 0
        assert t.numel() * 8 == ntmeantc.acc_bytes(ntuple.TUPLES_2x4)
    assert st.acc.data_ptr() != st.ea.data_ptr()
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        st.meantc_step(boards, boards.clone(), u8, 1, 6, u8.clone(), i32)
    with pytest.raises(g2048.NativeError):
        ntmeantc.MeanTCTrainer(net, 256)
    for bad in (None, ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (11,), device="cpu")):
        with pytest.raises(TypeError):  # plain single tables only
            ntmeantc.MeanTCState(bad)
        with pytest.raises(TypeError):
            ntmeantc.MeanTCTrainer(bad, 256)
    assert g2048.ntmeantc is ntmeantc and g2048.MeanTCState is ntmeantc.MeanTCState
    assert g2048.MeanTCTrainer is ntmeantc.MeanTCTrainer
    assert issubclass(ntmeantc.MeanTCTrainer, ntuple.NTupleTrainer)
    assert g2048.default_meantc_lr_shift is ntmeantc.default_meantc_lr_shift
    assert {"ntmeantc", "MeanTCState", "MeanTCTrainer",
            "default_meantc_lr_shift"} <= set(g2048.__all__)


def test_ea_round_trips_through_a_file_and_through_a_tcstate_file(tmp_path):
    from g2048 import ntmeantc, nttc, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    st = ntmeantc.MeanTCState(net)
    g = torch.Generator().manual_seed(9)
    st.ea[..., 1] = torch.randint(0, 1 << 50, st.ea.shape[:-1], generator=g)
    st.ea[..., 0] = st.ea[..., 1] // 3 - 5
    assert set(st.state_dict()) == {"tuples", "ea"} == set(nttc.TCState(net).state_dict())
    st.save(tmp_path / "own.pt")
    back = ntmeantc.MeanTCState.load(tmp_path / "own.pt", net)
    assert torch.equal(back.ea, st.ea) and not back.acc.any() and back.ea is not st.ea
    # this state's file into a TCState, and a TCState's file into this state
    tc = nttc.TCState.load(tmp_path / "own.pt", net)
    assert torch.equal(tc.ea, st.ea)
    tc.ea += 1
    tc.save(tmp_path / "tc.pt")
    again = ntmeantc.MeanTCState.load(tmp_path / "tc.pt", net)
    assert torch.equal(again.ea, st.ea + 1)
    assert set(torch.load(tmp_path / "own.pt", weights_only=True)) == {"tuples", "ea"}
    other = ntuple.NTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), device="cpu")
    with pytest.raises(ValueError):
        ntmeantc.MeanTCState.load(tmp_path / "own.pt", other)
    with pytest.raises(ValueError):
        st.load_state_dict({"tuples": st.state_dict()["tuples"], "ea": st.ea.to(torch.int32)})
