"""CPU-side checks of batch-mean TD learning: the Python restatement (tests/ntmean_ref.py)
reproduces its hand-computed anchors, and the boundary of libg2048_ntmean.so (header == exports ==
SIGNATURES, build stamps, argument validation without a GPU, the Python side's refusals)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import ntmean_ref as R
import ntuple_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntmean.h")
NAMES = ["g2048_ntmean_acc_bytes", "g2048_ntmean_last_error", "g2048_ntmean_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
P2, P3 = [2] + [0] * 15, [3] + [0] * 15


def corner():
    return NR.Net(((0,),), base=[[1024 * i for i in range(16)]])


# ------------------------------------------------------------------ the reference's anchors
def test_floor_div_anchors():
    assert [R.floor_div(*x) for x in ((-3, 2), (3, 2), (-4, 2), (-1, 18), (0, 5), (7, 1))] == \
        [-2, 1, -2, -1, 0, 7]
    assert R.floor_div(-(8 << 31), 8) == -(1 << 31) and R.floor_div(-24576, 18) == -1366
    for bad in (0, -1):
        with pytest.raises(ValueError):
            R.floor_div(5, bad)


def test_worked_step_moves_both_entries_by_the_one_delta():
    net = corner()
    prev, has_prev = [list(P2)], [1]
    assert R.step(net, [A], prev, has_prev, 1, 1) == ([2], [4096], [2048])
    assert R.last_hits == {(0, 2): (4096, 2), (0, 0): (12288, 6)}
    assert net.touched == {(0, 2): 4096, (0, 0): 2048}
    assert prev == [P2] and has_prev == [1]
    td = corner()
    td.td_step([A], [list(P2)], [1], 1, 1)
    assert td.touched == {(0, 2): 6144, (0, 0): 12288}


def test_worked_step_with_the_board_given_three_times_is_the_same_step():
    net = corner()
    prev, has_prev = [list(P2) for _ in range(3)], [1, 1, 1]
    assert R.step(net, [A, A, A], prev, has_prev, 1, 1) == ([2] * 3, [4096] * 3, [2048] * 3)
    assert R.last_hits == {(0, 2): (12288, 6), (0, 0): (36864, 18)}
    assert net.touched == {(0, 2): 4096, (0, 0): 2048}


def test_worked_step_with_two_deltas_on_one_entry_negative_and_not_divisible():
    net = corner()
    prev, has_prev = [list(P2), list(P3), list(P3)], [1, 1, 1]
    acts, err, delta = R.step(net, [A, CHECKER, CHECKER], prev, has_prev, 1, 1)
    assert (acts, err, delta) == ([2, 0, 0], [4096, -6144, -6144], [2048, -3072, -3072])
    assert R.last_hits == {(0, 2): (4096, 2), (0, 3): (-12288, 4), (0, 0): (-24576, 18)}
    assert net.touched == {(0, 2): 4096, (0, 3): 0, (0, 0): -1366}
    assert has_prev == [1, 0, 0] and prev == [P2, P3, P3]
    td = corner()
    td.td_step([A, CHECKER, CHECKER], [list(P2), list(P3), list(P3)], [1, 1, 1], 1, 1)
    assert td.touched[(0, 0)] == -24576


def test_worked_step_with_two_deltas_on_one_entry_positive_and_not_divisible():
    net = corner()
    prev, has_prev = [list(P2), list(P2), list(P3)], [1, 1, 1]
    R.step(net, [A, A, CHECKER], prev, has_prev, 1, 1)
    assert R.last_hits == {(0, 2): (8192, 4), (0, 3): (-6144, 2), (0, 0): (6144, 18)}
    assert net.touched == {(0, 2): 4096, (0, 3): 0, (0, 0): 341}


def test_reference_boards_that_do_not_hit():
    """A board without a previous afterstate, a zero delta and lr_num = 0 hit nothing; prev and
    has_prev are still committed."""
    net = corner()
    prev, has_prev = [list(P2), list(P3)], [0, 1]
    acts, err, delta = R.step(net, [A, A], prev, has_prev, 0, 1)
    assert (acts, err, delta) == ([2, 2], [0, 8192 - 6144], [0, 0])
    assert R.last_hits == {} and net.touched == {}
    assert prev == [P2, P2] and has_prev == [1, 1]
    # err = 4096 at lr = 2^-13: delta 0, no hit.  q[left] = 4096 + 2 * 2047, V(prev) = 2 * 2047
    net = NR.Net(((0,),), base=[[0, 0, 2047] + [0] * 13])
    assert R.step(net, [A], [list(P2)], [1], 1, 13)[1:] == ([4096], [0])
    assert R.last_hits == {}


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (ntlambda, ntrestart, ntsearch, ntstage, nttc, ntuple, search,
                       stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart)


def test_header_equals_exports_equals_signatures():
    from g2048 import ntmean

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntmean.load()
    assert set(names) == set(ntmean.SIGNATURES)
    assert _exported(ntmean.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    proto = re.search(r"g2048_ntmean_step\((.*?)\);", src, re.S).group(1)
    assert len(proto.split(",")) == len(ntmean.SIGNATURES["g2048_ntmean_step"][1]) == 14
    # the other nine libraries keep their ABI: none of the new symbols
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_ntmean")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntmean

    out = subprocess.run(["readelf", "-d", ntmean.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other nine stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTSTAGE_SHARED,
                  G.STAGESEARCH_SRCS, G.NTRESTART_SRCS):
        assert set(G.NTMEAN_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTMEAN_SRCS[0]))
    assert open(G.NTMEAN_STAMP).read().strip() == G.ntmean_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert len(set(_hashes(G))) == 10


def test_stamp_follows_its_source_the_shared_header_and_the_three_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp -- the main library's does not move;
    a change to the batch-mean header changes the new stamp and none of the other nine; a change
    to the shared csrc header changes the new stamp too; a change to each of g2048.h,
    g2048_ntuple.h and g2048_ntmean.h changes the new stamp, the last one no other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.NTMEAN_SRCS[0])).read()
    assert f'#include "{G.NTUPLE_SHARED[0]}"' in src and f'#include "{G.NTMEAN_SHARED[0]}"' in src
    assert not re.search(r'#include\s+"[^"]*\.hip"', src)
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTMEAN_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:9] == before[:9] and after[9] != before[9]
    with open(os.path.join(copy, G.NTMEAN_SHARED[0]), "a") as f:
        f.write("// changed\n")
    mean = _hashes(G)
    assert mean[:9] == before[:9] and mean[9] != after[9]
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    shared = _hashes(G)
    assert shared[0] == before[0] and shared[9] != mean[9] and shared[2] != before[2]
    last, include = shared, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntmean.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[9] != shared[9] and now[9] != last[9], header
        if header == "g2048_ntmean.h":
            assert now[:9] == shared[:9]
        last = now


ONE_DEFINITION = ("resolve", "tc_rate", "floor_div", "add_entry", "slot_bits", "check_staged",
                  "k_mean_gather", "k_mean_apply", "k_policy", "k_stage_policy")


def test_the_shared_device_code_is_defined_in_one_file():
    """The fall-through, the rate, the quotient, the (D, C) add, the slot counts, the staged
    checks and the gather, apply, flat-policy and staged-policy kernel templates each have one
    definition under csrc/: a return type, the name and an opening parameter list, comments
    aside."""
    import __graft_entry__ as G

    texts = {}
    for f in sorted(os.listdir(G.CSRC)):
        with open(os.path.join(G.CSRC, f)) as fh:
            texts[f] = re.sub(r"//[^\n]*", "", fh.read())
    for name in ONE_DEFINITION:
        rx = re.compile(r"\b(?:void|int|int64_t|uint32_t)\s+%s\s*\(" % name)
        found = {f: len(rx.findall(t)) for f, t in texts.items() if rx.search(t)}
        assert len(found) == 1 and list(found.values()) == [1], (name, found)
    where = {name: f for name in ONE_DEFINITION for f, t in texts.items()
             if re.search(r"\b(?:void|int|int64_t|uint32_t)\s+%s\s*\(" % name, t)}
    assert {where[n] for n in ("k_policy", "tc_rate")} == {G.NTUPLE_SHARED[0]}
    assert {where[n] for n in ("resolve", "check_staged", "k_stage_policy")} == \
        {G.NTSTAGE_SHARED[0]}
    assert {where[n] for n in ("floor_div", "add_entry", "slot_bits", "k_mean_gather",
                               "k_mean_apply")} == {G.NTMEAN_SHARED[0]}


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
    from g2048 import ntmean

    lib = ntmean.load()
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for tuples in (((0,),), NR.TUPLES_2x4, NR.TUPLES_4x6, T8):
        want = 16 * len(tuples) * 16 ** len(tuples[0])
        assert lib.g2048_ntmean_acc_bytes(C.byref(_spec(tuples))) == want
        assert ntmean.acc_bytes(tuples) == want
    assert lib.g2048_ntmean_acc_bytes(None) == N.G2048_EINVAL
    assert b"spec" in lib.g2048_ntmean_last_error()


BAD_SPECS = [
    (dict(tuples=((0,),), n_tuples=0), b"n_tuples"),
    (dict(tuples=((0,),), n_tuples=9), b"n_tuples"),
    (dict(tuples=((0,),), n_cells=0), b"n_cells"),
    (dict(tuples=((0,),), n_cells=7), b"n_cells"),
    (dict(tuples=((0, 1), (2, 16))), b"not a board cell"),
    (dict(tuples=((0, 1, 2), (3, 4, 3))), b"twice"),
]


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused_by_every_entry_point(kw, word):
    import g2048._native as N
    from g2048 import ntmean

    lib = ntmean.load()
    fake = 1 << 20
    s = _spec(**kw)
    calls = [lambda: lib.g2048_ntmean_acc_bytes(C.byref(s)),
             lambda: lib.g2048_ntmean_step(C.byref(s), fake, fake, fake, 4, fake, fake, 1, 10,
                                           fake, fake, fake, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_ntmean_last_error(), lib.g2048_ntmean_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntmean

    lib = ntmean.load()
    fake = 1 << 20
    s = _spec(NR.TUPLES_2x4)

    def step(spec=s, lut=fake, acc=fake, boards=fake, n=4, prev=fake, has_prev=fake, lr_num=1,
             lr_shift=10, action=fake, delta=fake, err=fake):
        return lib.g2048_ntmean_step(C.byref(spec) if spec is not None else None, lut, acc,
                                     boards, n, prev, has_prev, lr_num, lr_shift, action, delta,
                                     err, 0, None)

    cases = [(dict(spec=None), b"spec"), (dict(lut=None), b"NULL"), (dict(acc=None), b"NULL"),
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
        assert word in lib.g2048_ntmean_last_error(), (kw, lib.g2048_ntmean_last_error())
        assert b"ntmean_step" in lib.g2048_ntmean_last_error()


# ------------------------------------------------------------------ the Python side
def test_default_mean_lr_shift():
    from g2048 import ntmean, ntuple

    assert ntmean.default_mean_lr_shift(ntuple.TUPLES_2x4) == 6
    assert ntmean.default_mean_lr_shift(ntuple.TUPLES_4x6) == 7
    assert ntmean.default_mean_lr_shift(ntuple.NTupleSpec(ntuple.TUPLES_4x6)) == 7
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    assert [ntmean.default_mean_lr_shift(T8[:T]) for T in range(1, 9)] == [5, 6, 7, 7, 8, 8, 8, 8]


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntmean, ntstage, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    ms = ntmean.MeanState(net)
    assert ms.acc.shape == (2, 65536, 2) and ms.acc.dtype == torch.int64 and not ms.acc.any()
    assert ms.acc.is_contiguous() and ms.acc.data_ptr() % 16 == 0
    assert ms.acc.numel() * 8 == ntmean.acc_bytes(ntuple.TUPLES_2x4)
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        ms.mean_step(boards, boards.clone(), u8, 1, 6, u8.clone(), i32)
    with pytest.raises(g2048.NativeError):
        ntmean.MeanTrainer(net, 256)
    with pytest.raises(TypeError):
        ntmean.MeanState(None)
    with pytest.raises(TypeError):  # single tables only
        ntmean.MeanState(ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (11,), device="cpu"))
    with pytest.raises(TypeError):
        ntmean.MeanTrainer(None, 256)
    assert not hasattr(ms, "save") and not hasattr(ms, "state_dict")
    assert g2048.ntmean is ntmean and g2048.MeanState is ntmean.MeanState
    assert g2048.MeanTrainer is ntmean.MeanTrainer
    assert g2048.default_mean_lr_shift is ntmean.default_mean_lr_shift
    assert issubclass(ntmean.MeanTrainer, ntuple.NTupleTrainer)
    assert {"ntmean", "MeanState", "MeanTrainer", "default_mean_lr_shift"} <= set(g2048.__all__)
