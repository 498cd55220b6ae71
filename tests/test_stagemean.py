"""CPU-side checks of batch-mean TD learning on the multi-stage network: the Python restatement
(tests/stagemean_ref.py) reproduces its hand-computed anchors and the consequences the header
states, and the boundary of libg2048_stagemean.so (header == exports == SIGNATURES, build stamps,
argument validation without a GPU, the Python side's refusals)."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest
import torch

import ntmean_ref as MR
import ntstage_ref as SR
import ntuple_ref as NR
import stagemean_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_stagemean.h")
NAMES = ["g2048_stagemean_acc_bytes", "g2048_stagemean_last_error", "g2048_stagemean_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
P1 = [1, 0, 0, 0, 0, 2] + [0] * 10
P2 = [1, 0, 0, 0, 0, 3] + [0] * 10
Q2, Q3 = [2] + [0] * 15, [3] + [0] * 15


def corner(bounds):
    """Spec ((0,),), lut0[i] = 1024 i, the upper stages UNSET."""
    return SR.StagedNet(((0,),), bounds, base=lambda s, t, i: 1024 * i if s == 0 else None)


def table(net):
    """{(s, t, i): value} of everything the steps have written."""
    return {(s, t, i): v for s, d in enumerate(net.stages) for (t, i), v in d.items()}


# ------------------------------------------------------------------ the reference's anchors
def test_floor_div_anchors():
    assert [R.floor_div(*x) for x in ((-3, 2), (3, 2), (-4, 2), (-1, 18), (0, 5), (7, 1))] == \
        [-2, 1, -2, -1, 0, 7]
    assert R.floor_div(-24576, 18) == -1366 and R.floor_div(6144, 18) == 341
    for bad in (0, -1):
        with pytest.raises(ValueError):
            R.floor_div(5, bad)


def test_two_stages_promoted_and_moved_in_one_call():
    net = corner((2, 3))
    prev, has_prev = [list(P1), list(P2)], [1, 1]
    acts, err, delta = R.step(net, [CHECKER, A], prev, has_prev, 1, 1)
    assert (acts, err, delta) == ([0, 2], [-2048, 6144], [-1024, 3072])
    assert net.promoted == {(1, 0, 1): 1024, (2, 0, 1): 1024, (1, 0, 0): 0, (2, 0, 0): 0}
    assert R.last_hits == {(1, 0, 1): (-2048, 2), (1, 0, 0): (-6144, 6), (2, 0, 1): (6144, 2),
                           (2, 0, 0): (18432, 6)}
    assert table(net) == {(1, 0, 1): 0, (1, 0, 0): -1024, (2, 0, 1): 4096, (2, 0, 0): 3072}
    assert not net.stages[0]
    assert has_prev == [0, 1] and prev == [P1, Q2]
    td = corner((2, 3))  # the sum rule on the same call
    td.td_step([CHECKER, A], [list(P1), list(P2)], [1, 1], 1, 1)
    assert table(td) == {(1, 0, 1): -1024, (1, 0, 0): -6144, (2, 0, 1): 7168, (2, 0, 0): 18432}


def test_two_deltas_on_one_staged_entry_negative_and_not_divisible():
    net = corner((2,))
    prev, has_prev = [list(Q2), list(Q3), list(Q3)], [1, 1, 1]
    acts, err, delta = R.step(net, [A, CHECKER, CHECKER], prev, has_prev, 1, 1)
    assert (acts, err, delta) == ([2, 0, 0], [4096, -6144, -6144], [2048, -3072, -3072])
    assert R.last_hits == {(1, 0, 2): (4096, 2), (1, 0, 3): (-12288, 4), (1, 0, 0): (-24576, 18)}
    assert net.promoted == {(1, 0, 2): 2048, (1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(net) == {(1, 0, 2): 4096, (1, 0, 3): 0, (1, 0, 0): -1366}
    assert has_prev == [1, 0, 0] and prev == [Q2, Q3, Q3]


def test_two_deltas_on_one_staged_entry_positive_and_not_divisible():
    net = corner((2,))
    prev, has_prev = [list(Q2), list(Q2), list(Q3)], [1, 1, 1]
    R.step(net, [A, A, CHECKER], prev, has_prev, 1, 1)
    assert R.last_hits == {(1, 0, 2): (8192, 4), (1, 0, 3): (-6144, 2), (1, 0, 0): (6144, 18)}
    assert table(net) == {(1, 0, 0): 341, (1, 0, 2): 4096, (1, 0, 3): 0}


def test_a_hot_index_is_split_by_stage():
    """Index 0 is hit by a stage-0 and by two stage-1 boards: two (D, C), two quotients, each
    entry from the pre-call val.  One table gives the one quotient -1366."""
    net = corner((3,))
    prev, has_prev = [list(Q2), list(Q3), list(Q3)], [1, 1, 1]
    acts, err, delta = R.step(net, [A, CHECKER, CHECKER], prev, has_prev, 1, 1)
    assert (acts, delta) == ([2, 0, 0], [2048, -3072, -3072])
    assert R.last_hits == {(0, 0, 2): (4096, 2), (0, 0, 0): (12288, 6), (1, 0, 3): (-12288, 4),
                           (1, 0, 0): (-36864, 12)}
    assert net.promoted == {(1, 0, 3): 3072, (1, 0, 0): 0}
    assert table(net) == {(0, 0, 2): 4096, (0, 0, 0): 2048, (1, 0, 3): 0, (1, 0, 0): -3072}
    one = NR.Net(((0,),), base=[[1024 * i for i in range(16)]])
    MR.step(one, [A, CHECKER, CHECKER], [list(Q2), list(Q3), list(Q3)], [1, 1, 1], 1, 1)
    assert one.touched[(0, 0)] == -1366


def test_lr_num_0_promotes_and_moves_nothing():
    net = corner((2,))
    probe = [A, P1, Q2, Q3, CHECKER]
    before = [net.V(b) for b in probe]
    prev, has_prev = [list(P1), list(Q3)], [1, 0]
    acts, err, delta = R.step(net, [A, A], prev, has_prev, 0, 1)
    assert delta == [0, 0] and err == [8192 - 2048, 0] and acts == [2, 2]
    assert R.last_hits == {}
    assert net.promoted == {(1, 0, 1): 1024, (1, 0, 0): 0} == table(net)
    assert [net.V(b) for b in probe] == before
    assert prev == [Q2, Q2] and has_prev == [1, 1]


# ------------------------------------------------------------------ consequences, on the reference
T3 = ((0, 1), (1, 5), (2, 7))


def _boards(rng, n, hi=10, fill=0.6):
    return [[rng.randrange(1, hi) if rng.random() < fill else 0 for _ in range(16)]
            for _ in range(n)]


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


def test_s1_without_unset_is_the_single_table_rule():
    rng = random.Random(11)
    base = _base(12, 1, 3, 2)
    staged, plain = SR.StagedNet(T3, (), base=base), NR.Net(T3, base=base[0])
    p1, p2, h1, h2 = _boards(rng, 40), None, [1] * 30 + [0] * 10, None
    p2, h2 = [list(p) for p in p1], list(h1)
    for _ in range(3):
        boards = _boards(rng, 40)
        boards[3] = list(CHECKER)
        assert R.step(staged, boards, p1, h1, 3, 5) == MR.step(plain, boards, p2, h2, 3, 5)
        assert R.last_hits == {(0, *k): v for k, v in MR.last_hits.items()}
        assert staged.stages[0] == plain.touched and not staged.promoted
        assert (p1, h1) == (p2, h2)
    assert any(d % c for d, c in R.last_hits.values())


def test_a_batch_of_pairwise_distinct_staged_hits_is_the_staged_td_step():
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
    a, b = SR.StagedNet(T3, bounds, base=base), SR.StagedNet(T3, bounds, base=base)
    pa, pb, ha, hb = [list(p) for p in prev], [list(p) for p in prev], [1] * n, [1] * n
    assert R.step(a, boards, pa, ha, 3, 5) == b.td_step(boards, pb, hb, 3, 5)
    assert a.stages == b.stages and a.promoted == b.promoted and a.promoted
    assert all(c == 1 for _d, c in R.last_hits.values()) and R.last_hits


def test_a_batch_repeated_three_times_leaves_the_same_table():
    rng = random.Random(15)
    base = _base(16, 3, 3, 2, upper=0.5)
    boards, prev, has = _boards(rng, 30), _boards(rng, 30), [1] * 25 + [0] * 5
    out = []
    for k in (1, 3):
        net = SR.StagedNet(T3, (5, 8), base=base)
        R.step(net, boards * k, [list(p) for p in prev] * k, has * k, 3, 5)
        out.append((net.stages, net.promoted, dict(R.last_hits)))
    assert out[0][0] == out[1][0] and out[0][1] == out[1][1]
    assert all(out[1][2][key] == (3 * d, 3 * c) for key, (d, c) in out[0][2].items())
    assert any(c > 8 for _d, c in out[0][2].values())
    td = SR.StagedNet(T3, (5, 8), base=base)  # the sum rule does not have the property
    td.td_step(boards * 3, [list(p) for p in prev] * 3, has * 3, 3, 5)
    assert td.stages != out[0][0]


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (ntlambda, ntmean, ntrestart, ntsearch, ntstage, nttc, ntuple, search,
                       stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean)


def test_header_equals_exports_equals_signatures():
    from g2048 import stagemean

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = stagemean.load()
    assert set(names) == set(stagemean.SIGNATURES)
    assert _exported(stagemean.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_stagemean_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(stagemean.SIGNATURES["g2048_stagemean_step"][1]) == 15
    proto = re.search(r"g2048_stagemean_acc_bytes\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(stagemean.SIGNATURES["g2048_stagemean_acc_bytes"][1]) == 2
    # the other ten libraries keep their ABI: none of the new symbols
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_stagemean")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import stagemean

    out = subprocess.run(["readelf", "-d", stagemean.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other ten stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS):
        assert set(G.STAGEMEAN_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.STAGEMEAN_SRCS[0]))
    assert open(G.STAGEMEAN_STAMP).read().strip() == G.stagemean_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.NTSTAGE_STAMP).read().strip() == G.ntstage_source_hash()
    assert open(G.NTMEAN_STAMP).read().strip() == G.ntmean_source_hash()
    assert len(set(_hashes(G))) == 11


def test_stamp_follows_its_source_the_shared_headers_and_the_four_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp; a change to the batch-mean header
    changes the two batch-mean stamps and none of the other nine; a change to either other shared
    csrc header changes the new stamp too; a change to each of g2048.h, g2048_ntuple.h,
    g2048_ntstage.h and g2048_stagemean.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.STAGEMEAN_SRCS[0])).read()
    for shared in (G.NTUPLE_SHARED[0], G.NTSTAGE_SHARED[0], G.NTMEAN_SHARED[0]):
        assert f'#include "{shared}"' in src
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.STAGEMEAN_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:10] == before[:10] and after[10] != before[10]
    with open(os.path.join(copy, G.NTMEAN_SHARED[0]), "a") as f:
        f.write("// changed\n")
    last = _hashes(G)
    assert last[:9] == before[:9] and last[9] != after[9] and last[10] != after[10]
    for shared, also in ((G.NTUPLE_SHARED[0], 2), (G.NTSTAGE_SHARED[0], 6)):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
        now = _hashes(G)
        assert now[0] == before[0] and now[10] != last[10] and now[also] != last[also], shared
        last = now
    shared, include = last, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntstage.h",
                                "g2048_stagemean.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[10] != shared[10] and now[10] != last[10], header
        if header == "g2048_stagemean.h":
            assert now[:10] == shared[:10]
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
    from g2048 import stagemean

    lib = stagemean.load()
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6, T8):
        for bounds in ((), (11,), (5, 8), tuple(range(1, 8))):
            want = 16 * (len(bounds) + 1) * len(tuples) * 16 ** len(tuples[0])
            assert lib.g2048_stagemean_acc_bytes(C.byref(_spec(tuples)),
                                                 C.byref(_stages(bounds))) == want
            assert stagemean.acc_bytes(tuples, bounds) == want
    assert stagemean.acc_bytes(NR.TUPLES_4x6, (11,)) == 2 << 30
    full = _spec(tuple(tuple(range(k, k + 6)) for k in range(8)))
    assert lib.g2048_stagemean_acc_bytes(C.byref(full),
                                         C.byref(_stages(tuple(range(1, 8))))) == 16 << 30
    assert lib.g2048_stagemean_acc_bytes(None, C.byref(_stages(()))) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_stagemean_last_error()
    assert lib.g2048_stagemean_acc_bytes(C.byref(_spec(NR.TUPLES_2x4)), None) == N.G2048_EINVAL
    assert b"stages" in lib.g2048_stagemean_last_error()
    with pytest.raises(ValueError):
        stagemean.acc_bytes(NR.TUPLES_2x4, (8, 5))


def _every_entry_point(lib, s, st):
    """Each entry point's message on a call that must be refused."""
    import g2048._native as N

    fake = 1 << 20
    calls = [lambda: lib.g2048_stagemean_acc_bytes(C.byref(s), C.byref(st)),
             lambda: lib.g2048_stagemean_step(C.byref(s), C.byref(st), fake, fake, fake, 4, fake,
                                              fake, 1, 10, fake, fake, fake, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        yield lib.g2048_stagemean_last_error()


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
    from g2048 import stagemean

    for msg in _every_entry_point(stagemean.load(), _spec(**kw), _stages((5, 8))):
        assert word in msg, msg


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused_by_every_entry_point(kw, word):
    from g2048 import stagemean

    for msg in _every_entry_point(stagemean.load(), _spec(NR.TUPLES_2x4), _stages(**kw)):
        assert word in msg, msg


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory).  ntstage's
    checks plus ntmean's acc checks."""
    import g2048._native as N
    from g2048 import stagemean

    lib = stagemean.load()
    fake = 1 << 20
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))

    def step(spec=s, stages=st, lut=fake, acc=fake, boards=fake, n=4, prev=fake, has_prev=fake,
             lr_num=1, lr_shift=10, action=fake, delta=fake, err=fake):
        return lib.g2048_stagemean_step(C.byref(spec) if spec is not None else None,
                                        C.byref(stages) if stages is not None else None, lut,
                                        acc, boards, n, prev, has_prev, lr_num, lr_shift, action,
                                        delta, err, 0, None)

    cases = [(dict(spec=None), b"spec"), (dict(stages=None), b"stages"),
             (dict(lut=None), b"NULL"), (dict(acc=None), b"NULL"),
             (dict(boards=None), b"NULL"), (dict(prev=None), b"NULL"),
             (dict(has_prev=None), b"NULL"), (dict(action=None), b"NULL"),
             (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=fake + 2), b"aligned"), (dict(acc=fake + 8), b"aligned"),
             (dict(boards=fake + 4), b"aligned"), (dict(prev=fake + 8), b"aligned"),
             (dict(delta=fake + 2), b"aligned"), (dict(err=fake + 4), b"aligned")]
    for kw, word in cases:
        assert step(**kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_stagemean_last_error(), (kw, lib.g2048_stagemean_last_error())
        assert b"stagemean_step" in lib.g2048_stagemean_last_error()


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmean, ntstage, ntuple, stagemean

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    ms = stagemean.StagedMeanState(net)
    assert ms.acc.shape == (3, 2, 65536, 2) and ms.acc.dtype == torch.int64 and not ms.acc.any()
    assert ms.acc.is_contiguous() and ms.acc.data_ptr() % 16 == 0
    assert ms.acc.numel() * 8 == stagemean.acc_bytes(ntuple.TUPLES_2x4, (5, 8))
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        ms.mean_step(boards, boards.clone(), u8, 1, 6, u8.clone(), i32)
    with pytest.raises(g2048.NativeError):
        stagemean.StagedMeanTrainer(net, 256)
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for bad in (None, plain):  # staged networks only
        with pytest.raises(TypeError):
            stagemean.StagedMeanState(bad)
        with pytest.raises(TypeError):
            stagemean.StagedMeanTrainer(bad, 256)
    # the single-table classes keep refusing staged networks, with their present message
    for cls, args in ((ntmean.MeanState, ()), (ntmean.MeanTrainer, (256,))):
        with pytest.raises(TypeError, match="staged tables are not supported"):
            cls(net, *args)
    assert not hasattr(ms, "save") and not hasattr(ms, "state_dict")
    assert g2048.stagemean is stagemean and g2048.StagedMeanState is stagemean.StagedMeanState
    assert g2048.StagedMeanTrainer is stagemean.StagedMeanTrainer
    assert stagemean.default_mean_lr_shift is ntmean.default_mean_lr_shift
    assert issubclass(stagemean.StagedMeanTrainer, ntuple.NTupleTrainer)
    assert {"stagemean", "StagedMeanState", "StagedMeanTrainer"} <= set(g2048.__all__)
