"""CPU-side checks of temporal-coherence learning: the Python restatement (tests/nttc_ref.py)
reproduces its hand-computed anchors, the library's host-only rate equals it, and the boundary of
libg2048_nttc.so (header == exports == SIGNATURES, build stamps, argument validation without a
GPU, persistence of the accumulators)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import nttc_ref as R
import ntuple_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_nttc.h")
NAMES = ["g2048_nttc_last_error", "g2048_nttc_rate", "g2048_nttc_step", "g2048_nttc_work_bytes"]

A = [1, 1] + [0] * 14
# (E, A, rate): the anchors of nttc_ref's docstring
RATE_ANCHORS = [
    (0, 0, 65536), (1, 1, 65536), (-1, 1, 65536), (12345, 12345, 65536), (-(1 << 50), 1 << 50, 65536),
    (R.MAX_A, R.MAX_A, 65536), (-R.MAX_A, R.MAX_A, 65536), (1, 3, 21845), (-1, 3, 21845),
    (0, 7, 0), (0, R.MAX_A, 0),
    (32768, 65535, 32768), (32769, 65536, 32768), (3, 65537, 2), (65537, 65537, 65536),
    (-3 * (1 << 38), (1 << 40) + 12345, 49152),
]


# ------------------------------------------------------------------ the reference's anchors
@pytest.mark.parametrize("E,A_,want", RATE_ANCHORS)
def test_rate_anchors(E, A_, want):
    assert R.rate(E, A_) == want


def test_rate_shift_and_step_anchors():
    assert [R.shift_of(a) for a in (0, 1, 65535, 65536, 65537, (1 << 40) + 12345, R.MAX_A)] == \
        [0, 0, 0, 1, 1, 25, 46]
    assert R.step_of(-3, 21845) == -1 and R.step_of(3, 21845) == 0
    assert R.step_of(-(1 << 31), 65536) == -(1 << 31) and R.step_of(2048, 21845) == 682
    for bad in ((2, 1), (-2, 1), (0, -1), (0, 1 << 62), (1, 0)):
        with pytest.raises(ValueError):
            R.rate(*bad)


def corner():
    return NR.Net(((0,),), base=[[1024 * i for i in range(16)]])


def test_worked_step_with_fresh_ea_equals_td0():
    tc = R.TC(corner())
    prev, has_prev = [[2] + [0] * 15], [1]
    assert tc.step([A], prev, has_prev, 1, 1) == ([2], [4096], [2048])
    assert tc.net.touched == {(0, 2): 6144, (0, 0): 12288}
    assert tc.E == {(0, 2): 4096, (0, 0): 12288} and tc.A == tc.E
    assert prev == [[2] + [0] * 15] and has_prev == [1]
    td = corner()
    prev, has_prev = [[2] + [0] * 15], [1]
    assert td.td_step([A], prev, has_prev, 1, 1) == ([2], [4096], [2048])
    assert td.touched == tc.net.touched


def test_worked_step_with_two_different_rates():
    ea = {(0, 2): (1, 3), (0, 0): (-5, 10)}
    tc = R.TC(corner(), base_ea=lambda t, i: ea.get((t, i), (0, 0)))
    prev, has_prev = [[2] + [0] * 15], [1]
    assert tc.step([A], prev, has_prev, 1, 1) == ([2], [4096], [2048])
    assert tc.net.touched == {(0, 2): 3412, (0, 0): 6144}
    assert tc.E == {(0, 2): 4097, (0, 0): 12283} and tc.A == {(0, 2): 4099, (0, 0): 12298}


def test_reference_reads_see_the_state_before_the_call_and_terminal_boards():
    """Two boards with the same previous afterstate: both use the rate from before the call; a
    board without a previous afterstate adds nothing; a terminal board learns toward 0."""
    checker = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
    ea = {(0, 2): (1, 3)}
    tc = R.TC(corner(), base_ea=lambda t, i: ea.get((t, i), (0, 0)))
    prev = [[2] + [0] * 15, [2] + [0] * 15, [3] + [0] * 15, [3] + [0] * 15]
    has_prev = [1, 1, 0, 1]
    acts, err, delta = tc.step([A, A, A, checker], prev, has_prev, 1, 1)
    assert (acts, err, delta) == ([2, 2, 2, 0], [4096, 4096, 0, -6144], [2048, 2048, 0, -3072])
    # entry 2: four pairs at rate 21845; entry 3: two pairs of the terminal board at full rate
    assert tc.net.touched[(0, 2)] == 2048 + 4 * 682 and tc.net.touched[(0, 3)] == 3072 - 2 * 3072
    assert tc.net.touched[(0, 0)] == 12 * 2048 - 6 * 3072
    assert tc.E[(0, 2)] == 1 + 4 * 2048 and tc.A[(0, 2)] == 3 + 4 * 2048
    assert tc.E[(0, 0)] == 12 * 2048 - 6 * 3072 and tc.A[(0, 0)] == 12 * 2048 + 6 * 3072
    assert tc.E[(0, 3)] == -2 * 3072 and tc.A[(0, 3)] == 2 * 3072
    assert has_prev == [1, 1, 1, 0] and prev[3] == [3] + [0] * 15 and prev[2] == [2] + [0] * 15
    # |E| <= A is kept
    assert all(abs(tc.E[k]) <= tc.A[k] for k in tc.A)


# ------------------------------------------------------------------ the library's rate
def test_library_rate_equals_the_reference():
    from g2048 import nttc

    lib = nttc.load()
    for E, A_, want in RATE_ANCHORS:
        assert lib.g2048_nttc_rate(E, A_) == want == nttc.rate(E, A_)
    rng = np.random.default_rng(71)
    bits = rng.integers(0, 62, 10000)
    seen_shift = set()
    for k in range(10000):
        A_ = int(rng.integers(0, 1 << int(bits[k]), endpoint=True)) if k % 7 else \
            (1 << int(bits[k])) + int(rng.integers(-1, 2))
        A_ = min(max(A_, 0), 1 << 61)
        E = int(rng.integers(-A_, A_, endpoint=True)) if k % 5 else (A_ if k % 2 else -A_)
        assert lib.g2048_nttc_rate(E, A_) == R.rate(E, A_), (E, A_)
        seen_shift.add(R.shift_of(A_))
    assert {0, 1, 20, 45} <= seen_shift


def test_library_rate_refuses_pairs_outside_the_domain():
    import g2048._native as N
    from g2048 import nttc

    lib = nttc.load()
    for E, A_, word in ((0, -1, b"A ="), (0, 1 << 62, b"A ="), (0, -(1 << 63), b"A ="),
                        (2, 1, b"exceeds"), (-2, 1, b"exceeds"), (1, 0, b"exceeds"),
                        (-(1 << 63), 5, b"exceeds"), ((1 << 63) - 1, R.MAX_A, b"exceeds")):
        assert lib.g2048_nttc_rate(E, A_) == N.G2048_EINVAL, (E, A_)
        assert word in lib.g2048_nttc_last_error(), lib.g2048_nttc_last_error()
        with pytest.raises(ValueError):
            nttc.rate(E, A_)
        with pytest.raises(ValueError):
            R.rate(E, A_)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_equals_exports_equals_signatures():
    import g2048._native as N
    from g2048 import ntsearch, nttc, ntuple, search

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = nttc.load()
    assert set(names) == set(nttc.SIGNATURES)
    assert _exported(nttc.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other four libraries keep their ABI: none of the new symbols
    for path in (N.LIB_PATH, search.LIB_PATH, ntuple.LIB_PATH, ntsearch.LIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("g2048_nttc")]
    assert not set(names) & (set(N.SIGNATURES) | set(search.SIGNATURES) | set(ntuple.SIGNATURES)
                             | set(ntsearch.SIGNATURES))
    assert nttc.RATE_BITS == R.RATE_BITS == 16 and "G2048_NTTC_RATE_BITS 16" in src
    assert nttc.MAX_A == R.MAX_A


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import nttc

    out = subprocess.run(["readelf", "-d", nttc.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED):
        assert set(G.NTTC_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTTC_SRCS[0]))
    assert open(G.NTTC_STAMP).read().strip() == G.nttc_source_hash()
    assert open(G.NTSEARCH_STAMP).read().strip() == G.ntsearch_source_hash()
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert len(set(_hashes(G))) == 5


def test_stamp_follows_its_source_the_shared_header_and_its_own_header(tmp_path, monkeypatch):
    """A change to the new source changes only the new stamp; a change to the shared csrc header
    changes the three stamps of the libraries that include it; a change to g2048_nttc.h changes
    only the new stamp."""
    import shutil

    import __graft_entry__ as G

    assert len(G.NTUPLE_SHARED) == 1
    assert f'#include "{G.NTUPLE_SHARED[0]}"' in open(os.path.join(G.CSRC, G.NTTC_SRCS[0])).read()
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTTC_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:4] == before[:4] and after[4] != before[4]
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    shared = _hashes(G)
    assert shared[:2] == before[:2]
    assert shared[2] != before[2] and shared[3] != before[3] and shared[4] != after[4]
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(G.ROOT, "include"), os.path.join(root, "include"))
    with open(os.path.join(root, "include", "g2048_nttc.h"), "a") as f:
        f.write("/* changed */\n")
    monkeypatch.setattr(G, "ROOT", root)
    header = _hashes(G)
    assert header[:4] == shared[:4] and header[4] != shared[4]


def test_kernel_has_no_store_data_hazard(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's
    flags, as tests/test_ntuple.py audits the n-tuple library's."""
    import shutil
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.NTTC_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0


def _spec(tuples, n_tuples=None, n_cells=None):
    from g2048 import ntuple

    s = ntuple._Spec(len(tuples) if n_tuples is None else n_tuples,
                     len(tuples[0]) if n_cells is None else n_cells)
    for t, cells in enumerate(tuples):
        for k, c in enumerate(cells):
            s.cells[t][k] = c
    return s


def test_work_bytes():
    import g2048._native as N
    from g2048 import nttc

    lib = nttc.load()
    T8 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
    for tuples, n in ((((0,),), 1), (NR.TUPLES_2x4, 257), (NR.TUPLES_4x6, 65536), (T8, 1031),
                      (T8, N.MAX_BOARDS)):
        want = 4 * 8 * len(tuples) * n
        assert lib.g2048_nttc_work_bytes(C.byref(_spec(tuples)), n) == want
        assert nttc.work_bytes(tuples, n) == want
    s = _spec(NR.TUPLES_2x4)
    for n in (0, -1, N.MAX_BOARDS + 1):
        assert lib.g2048_nttc_work_bytes(C.byref(s), n) == N.G2048_EINVAL
        assert b"n =" in lib.g2048_nttc_last_error()
        with pytest.raises(ValueError):
            nttc.work_bytes(NR.TUPLES_2x4, n)
    assert lib.g2048_nttc_work_bytes(None, 4) == N.G2048_EINVAL


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
    from g2048 import nttc

    lib = nttc.load()
    fake = 1 << 20
    s = _spec(**kw)
    calls = [lambda: lib.g2048_nttc_work_bytes(C.byref(s), 4),
             lambda: lib.g2048_nttc_step(C.byref(s), fake, fake, fake, 4, fake, fake, 1, 10, fake,
                                         fake, fake, fake, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_nttc_last_error(), lib.g2048_nttc_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import nttc

    lib = nttc.load()
    fake = 1 << 20
    s = _spec(NR.TUPLES_2x4)

    def step(spec=s, lut=fake, ea=fake, boards=fake, n=4, prev=fake, has_prev=fake, lr_num=1,
             lr_shift=10, action=fake, delta=fake, err=fake, work=fake):
        return lib.g2048_nttc_step(C.byref(spec) if spec is not None else None, lut, ea, boards,
                                   n, prev, has_prev, lr_num, lr_shift, action, delta, err, work,
                                   0, None)

    cases = [(dict(spec=None), b"spec"), (dict(lut=None), b"NULL"), (dict(ea=None), b"NULL"),
             (dict(boards=None), b"NULL"), (dict(prev=None), b"NULL"),
             (dict(has_prev=None), b"NULL"), (dict(action=None), b"NULL"),
             (dict(delta=None), b"NULL"), (dict(work=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=fake + 2), b"aligned"), (dict(ea=fake + 8), b"aligned"),
             (dict(boards=fake + 4), b"aligned"), (dict(prev=fake + 8), b"aligned"),
             (dict(delta=fake + 2), b"aligned"), (dict(err=fake + 4), b"aligned"),
             (dict(work=fake + 2), b"aligned")]
    for kw, word in cases:
        assert step(**kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_nttc_last_error(), (kw, lib.g2048_nttc_last_error())


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import nttc, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    tc = nttc.TCState(net)
    assert tc.ea.shape == (2, 65536, 2) and tc.ea.dtype == torch.int64 and not tc.ea.any()
    assert tc.ea.is_contiguous() and tc.ea.data_ptr() % 16 == 0
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        tc.tc_step(boards, boards.clone(), u8, 1, 10, u8.clone(), i32)
    with pytest.raises(g2048.NativeError):
        nttc.TCTrainer(net, 256)
    with pytest.raises(TypeError):
        nttc.TCState(None)
    assert g2048.nttc is nttc and g2048.TCState is nttc.TCState
    assert g2048.TCTrainer is nttc.TCTrainer and issubclass(nttc.TCTrainer, ntuple.NTupleTrainer)
    assert {"nttc", "TCState", "TCTrainer"} <= set(g2048.__all__)


def test_tc_state_save_load_round_trip_on_cpu_tensors(tmp_path):
    from g2048 import nttc, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    tc = nttc.TCState(net)
    g = torch.Generator().manual_seed(5)
    a = torch.randint(0, 1 << 61, net.lut.shape, generator=g, dtype=torch.int64)
    tc.ea[..., 1] = a
    tc.ea[..., 0] = a - torch.randint(0, 1 << 61, net.lut.shape, generator=g,
                                      dtype=torch.int64) % (2 * a + 1)
    assert bool((tc.ea[..., 0].abs() <= tc.ea[..., 1]).all()) and bool((tc.ea[..., 0] < 0).any())
    path = str(tmp_path / "tc.pt")
    tc.save(path)
    back = nttc.TCState.load(path, net)
    assert back.net is net and torch.equal(back.ea, tc.ea)
    # the file is plain tensors: weights-only loading reads it
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ["ea", "tuples"] and raw["tuples"].tolist() == [[0, 1, 2, 3],
                                                                         [0, 1, 4, 5]]
    other = nttc.TCState(ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu"))
    other.load_state_dict(tc.state_dict())
    assert torch.equal(other.ea, tc.ea)
    with pytest.raises(ValueError):  # other tuples
        nttc.TCState.load(path, ntuple.NTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), device="cpu"))
    with pytest.raises(ValueError):
        other.load_state_dict({"tuples": raw["tuples"], "ea": raw["ea"][:, :16]})
    with pytest.raises(ValueError):
        other.load_state_dict({"tuples": raw["tuples"], "ea": raw["ea"].to(torch.int32)})
