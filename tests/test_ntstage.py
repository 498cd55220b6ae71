"""CPU-side checks of the multi-stage n-tuple network: the Python restatement
(tests/ntstage_ref.py) reproduces its hand-computed anchors and, at S = 1, ntuple_ref's TD(0)
step; and the boundary of libg2048_ntstage.so (header == exports == SIGNATURES, build stamps,
argument validation without a GPU, the Python side's refusals, save / load)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ntstage_ref as R
import ntuple_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntstage.h")
NAMES = ["g2048_ntstage_act", "g2048_ntstage_last_error", "g2048_ntstage_lut_entries",
         "g2048_ntstage_td_step", "g2048_ntstage_values"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
P1 = [1, 0, 0, 0, 0, 2] + [0] * 10
P2 = [1, 0, 0, 0, 0, 3] + [0] * 10
TWO = [2] + [0] * 15


def corner(bounds, upper=None):
    """Spec ((0,),), stage 0 lut0[i] = 1024 i, the upper stages UNSET but for `upper`
    {(s, i): value}."""
    upper = upper or {}

    def base(s, t, i):
        return 1024 * i if s == 0 else upper.get((s, i))

    return R.StagedNet(((0,),), bounds, base=base)


# ------------------------------------------------------------------ the reference's anchors
def test_stage_counts_the_bounds_the_largest_tile_reaches():
    net = R.StagedNet(NR.TUPLES_2x4, (5, 8))
    for m, s in ((4, 0), (5, 1), (7, 1), (8, 2), (17, 2)):
        assert net.stage([1, m] + [0] * 14) == s and net.stage([0] * 15 + [m]) == s
    assert R.StagedNet(NR.TUPLES_2x4, ()).stage([17] * 16) == 0
    for bad in ((0,), (28,), (5, 5), (6, 5), tuple(range(1, 9))):
        with pytest.raises(ValueError):
            R.StagedNet(NR.TUPLES_2x4, bad)
    assert R.StagedNet(NR.TUPLES_2x4, tuple(range(1, 8))).S == 8


def test_worked_policy_a_merge_crosses_a_bound():
    net = corner((2,), {(1, 2): 5000})
    assert net.stage(A) == 0 and net.stage(TWO) == 1
    assert net.policy(A) == ([None, 2048, 14096, 14096], 2, TWO)
    assert NR.Net(((0,),), base=[[1024 * i for i in range(16)]]).policy(A)[0][2] == 8192
    assert net.policy(CHECKER) == ([None] * 4, 0, CHECKER)


def test_worked_three_stage_fall_through():
    b = [3] + [0] * 15
    assert corner((2, 3)).stage(b) == 2
    assert corner((2, 3)).V(b) == 6144
    assert corner((2, 3), {(1, 3): 7}).V(b) == 14
    assert corner((2, 3), {(1, 3): 7, (2, 0): 5}).V(b) == 44
    assert R.StagedNet(((0,),), (2, 3)).V(b) == 0  # a fresh network values every board at 0


def test_worked_step_one_entry_promoted_at_two_stages_in_one_call():
    net = corner((2, 3))
    prev, has_prev = [list(P1), list(P2)], [1, 1]
    assert net.V(P1) == net.V(P2) == 2048
    assert net.td_step([CHECKER, A], prev, has_prev, 1, 1) == ([0, 2], [-2048, 6144],
                                                               [-1024, 3072])
    assert net.promoted == {(1, 0, 1): 1024, (1, 0, 0): 0, (2, 0, 1): 1024, (2, 0, 0): 0}
    assert net.stages == [{}, {(0, 1): -1024, (0, 0): -6144}, {(0, 1): 7168, (0, 0): 18432}]
    assert prev == [P1, TWO] and has_prev == [0, 1]
    assert sorted(net.set_entries()) == [(1, 0, 0), (1, 0, 1), (2, 0, 0), (2, 0, 1)]


def test_worked_step_promotion_with_a_zero_delta():
    net = corner((2,))
    before = [net.V(b) for b in (P1, P2, A, TWO)]
    prev, has_prev = [list(P1)], [1]
    assert net.td_step([A], prev, has_prev, 0, 1) == ([2], [6144], [0])
    assert net.promoted == {(1, 0, 1): 1024, (1, 0, 0): 0}
    assert net.stages == [{}, {(0, 1): 1024, (0, 0): 0}]
    assert [net.V(b) for b in (P1, P2, A, TWO)] == before
    assert prev == [TWO] and has_prev == [1]
    net = corner((2,))
    prev, has_prev = [list(P1)], [0]
    assert net.td_step([A], prev, has_prev, 1, 1) == ([2], [0], [0])
    assert net.promoted == {} and net.stages == [{}, {}] and prev == [TWO] and has_prev == [1]


def test_worked_step_terminal_board_on_a_fresh_table():
    net = R.StagedNet(((0,),), (2,))
    prev, has_prev = [[1] + [0] * 15], [1]
    assert net.td_step([CHECKER], prev, has_prev, 1, 1) == ([0], [0], [0])
    assert net.promoted == {(0, 0, 1): 0, (0, 0, 0): 0}
    assert net.stages == [{(0, 1): 0, (0, 0): 0}, {}]
    assert prev == [[1] + [0] * 15] and has_prev == [0]


def test_reference_at_s1_is_ntuple_refs_td_step():
    rng = np.random.default_rng(91)
    n = 24
    base = rng.integers(-(1 << 20), 1 << 20, (2, 65536))
    td, st = NR.Net(NR.TUPLES_2x4, base=base), R.StagedNet(NR.TUPLES_2x4, (), base=[base])
    prev, has_prev = [[0] * 16 for _ in range(n)], [0] * n
    sprev, shas = [[0] * 16 for _ in range(n)], [0] * n
    for t in range(4):
        boards = (rng.integers(1, 12, (n, 16)) * (rng.random((n, 16)) < 0.6)).astype(np.uint8)
        if t >= 2:  # terminal boards: at t = 3 some follow a terminal step, some do not
            boards[t - 2:t + 1] = CHECKER
        assert st.td_step(boards, sprev, shas, 3, 6) == td.td_step(boards, prev, has_prev, 3, 6)
        assert st.stages == [td.touched] and st.promoted == {}
        assert sprev == prev and shas == has_prev
    assert td.touched and 0 in has_prev


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_equals_exports_equals_signatures():
    import g2048._native as N
    from g2048 import ntlambda, ntsearch, ntstage, nttc, ntuple, search

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntstage.load()
    assert set(names) == set(ntstage.SIGNATURES)
    assert _exported(ntstage.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other six libraries keep their ABI: none of the new symbols
    others = (N, search, ntuple, ntsearch, nttc, ntlambda)
    for mod in others:
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_ntstage")]
        assert not set(names) & set(mod.SIGNATURES)
    assert ntstage.MAX_STAGES == R.MAX_STAGES == 8 and ntstage.MAX_BOUND == R.MAX_BOUND == 27
    assert ntstage.UNSET == R.UNSET == torch.iinfo(torch.int32).min
    assert "G2048_NTSTAGE_MAX_STAGES 8" in src and "G2048_NTSTAGE_MAX_BOUND 27" in src
    assert "G2048_NTSTAGE_UNSET INT32_MIN" in src
    assert C.sizeof(ntstage._Stages) == 12


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntstage

    out = subprocess.run(["readelf", "-d", ntstage.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTTC_SRCS,
                  G.NTLAMBDA_SRCS, G.NTUPLE_SHARED):
        assert set(G.NTSTAGE_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTSTAGE_SRCS[0]))
    assert open(G.NTSTAGE_STAMP).read().strip() == G.ntstage_source_hash()
    assert open(G.NTLAMBDA_STAMP).read().strip() == G.ntlambda_source_hash()
    assert open(G.NTTC_STAMP).read().strip() == G.nttc_source_hash()
    assert open(G.NTSEARCH_STAMP).read().strip() == G.ntsearch_source_hash()
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert open(G.SEARCH_STAMP).read().strip() == G.search_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert len(set(_hashes(G))) == 7


def test_stamp_follows_its_source_the_shared_header_and_its_own_header(tmp_path, monkeypatch):
    """Without the new source and header the six existing stamps have the values they have with
    them; a change to the new source changes only the new stamp; a change to the shared csrc
    header changes the five stamps of the libraries that include it; a change to
    g2048_ntstage.h changes only the new stamp."""
    import shutil

    import __graft_entry__ as G

    assert len(G.NTUPLE_SHARED) == 1
    src = open(os.path.join(G.CSRC, G.NTSTAGE_SRCS[0])).read()
    assert f'#include "{G.NTUPLE_SHARED[0]}"' in src
    before = _hashes(G)
    real_csrc, real_root = G.CSRC, G.ROOT
    copy = str(tmp_path / "csrc")
    shutil.copytree(real_csrc, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTSTAGE_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:6] == before[:6] and after[6] != before[6]
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    shared = _hashes(G)
    assert shared[:2] == before[:2]
    assert all(shared[k] != before[k] for k in (2, 3, 4, 5)) and shared[6] != after[6]
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(G.ROOT, "include"), os.path.join(root, "include"))
    with open(os.path.join(root, "include", "g2048_ntstage.h"), "a") as f:
        f.write("/* changed */\n")
    monkeypatch.setattr(G, "ROOT", root)
    header = _hashes(G)
    assert header[:6] == shared[:6] and header[6] != shared[6]
    # a tree without the seventh library: the six existing stamps are what they are with it
    bare, bare_root = str(tmp_path / "bare"), str(tmp_path / "bare_root")
    shutil.copytree(real_csrc, bare)
    os.remove(os.path.join(bare, G.NTSTAGE_SRCS[0]))
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(bare_root, "include"))
    os.remove(os.path.join(bare_root, "include", "g2048_ntstage.h"))
    monkeypatch.setattr(G, "CSRC", bare)
    monkeypatch.setattr(G, "ROOT", bare_root)
    assert (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(),
            G.ntlambda_source_hash()) == before[:6]
    with pytest.raises(FileNotFoundError):
        G.ntstage_source_hash()


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

    for f in G.NTSTAGE_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0
        asm = open(out).read()
        # no scratch, in any of the 32 kernels (8 values, 16 policy, 8 update)
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert len(sizes) == 32 and set(sizes) == {"0"}


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


FAKE = 1 << 20


def _ref(x):
    return C.byref(x) if x is not None else None


def _values(lib, spec, stages, lut=FAKE, boards=FAKE, n=4, out=FAKE):
    return lib.g2048_ntstage_values(_ref(spec), _ref(stages), lut, boards, n, out, 0, None)


def _act(lib, spec, stages, lut=FAKE, boards=FAKE, n=4, q=FAKE, action=FAKE, after=FAKE):
    return lib.g2048_ntstage_act(_ref(spec), _ref(stages), lut, boards, n, q, action, after, 0,
                                 None)


def _step(lib, spec, stages, lut=FAKE, boards=FAKE, n=4, prev=FAKE, has_prev=FAKE, lr_num=1,
          lr_shift=10, action=FAKE, delta=FAKE, err=FAKE):
    return lib.g2048_ntstage_td_step(_ref(spec), _ref(stages), lut, boards, n, prev, has_prev,
                                     lr_num, lr_shift, action, delta, err, 0, None)


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


def _every_entry_point(lib, spec, stages):
    import g2048._native as N

    for call in (_values, _act, _step):
        assert call(lib, spec, stages) == N.G2048_EINVAL
        yield lib.g2048_ntstage_last_error()
    assert lib.g2048_ntstage_lut_entries(_ref(spec), _ref(stages)) == N.G2048_EINVAL
    yield lib.g2048_ntstage_last_error()


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused(kw, word):
    from g2048 import ntstage

    for msg in _every_entry_point(ntstage.load(), _spec(**kw), _stages((5, 8))):
        assert word in msg, msg


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused(kw, word):
    from g2048 import ntstage

    for msg in _every_entry_point(ntstage.load(), _spec(NR.TUPLES_2x4), _stages(**kw)):
        assert word in msg, msg


def test_lut_entries_counts_every_stage():
    from g2048 import ntstage

    lib = ntstage.load()
    s2, s4 = _spec(NR.TUPLES_2x4), _spec(NR.TUPLES_4x6)
    assert lib.g2048_ntstage_lut_entries(C.byref(s2), C.byref(_stages(()))) == 2 * 65536
    assert lib.g2048_ntstage_lut_entries(C.byref(s2), C.byref(_stages((5, 8)))) == 6 * 65536
    assert lib.g2048_ntstage_lut_entries(C.byref(s4), C.byref(_stages((11,)))) == 2 * 4 * 16 ** 6
    full = _spec(tuple(tuple(range(k, k + 6)) for k in range(8)))
    assert lib.g2048_ntstage_lut_entries(
        C.byref(full), C.byref(_stages(tuple(range(1, 8))))) == 1 << 30
    assert lib.g2048_ntstage_lut_entries(C.byref(s2), C.byref(_stages((1, 27)))) == 6 * 65536


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntstage

    lib = ntstage.load()
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))
    err = lib.g2048_ntstage_last_error
    common = [(dict(lut=None), b"NULL"), (dict(boards=None), b"NULL"), (dict(n=0), b"n ="),
              (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
              (dict(lut=FAKE + 2), b"aligned"), (dict(boards=FAKE + 4), b"aligned")]
    cases = {
        _values: common + [(dict(out=None), b"NULL"), (dict(out=FAKE + 4), b"aligned")],
        _act: common + [(dict(q=None, action=None, after=None), b"NULL"),
                        (dict(q=FAKE + 4), b"aligned"), (dict(after=FAKE + 8), b"aligned")],
        _step: common + [(dict(prev=None), b"NULL"), (dict(has_prev=None), b"NULL"),
                         (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
                         (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
                         (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
                         (dict(prev=FAKE + 8), b"aligned"), (dict(delta=FAKE + 2), b"aligned"),
                         (dict(err=FAKE + 4), b"aligned")],
    }
    for call, rows in cases.items():
        for kw, word in rows:
            assert call(lib, s, st, **kw) == N.G2048_EINVAL, kw
            assert word in err(), (kw, err())
        assert call(lib, None, st) == N.G2048_EINVAL and b"spec" in err()
        assert call(lib, s, None) == N.G2048_EINVAL and b"stages" in err()


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntstage, ntuple

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    assert net.n_stages == 3 and net.bounds == (5, 8)
    assert net.lut.shape == (3, 2, 65536) and net.lut.dtype == torch.int32
    assert bool((net.lut == ntstage.UNSET).all()) and net.set_counts() == [0, 0, 0]
    assert ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (), device="cpu").n_stages == 1
    for bad in ((0,), (28,), (5, 5), (8, 5), (300,), (-1,), tuple(range(1, 9))):
        with pytest.raises(ValueError):
            ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, bad, device="cpu")
    with pytest.raises(ValueError):
        ntstage.StagedNTupleNetwork(((0, 0),), (5,), device="cpu")
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    u8, i32 = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.int32)
    for call in (lambda: net.values(boards), lambda: net.act(boards),
                 lambda: net.td_step(boards, boards.clone(), u8, 1, 10, u8.clone(), i32)):
        with pytest.raises(g2048.NativeError):  # CPU tensors: there is no CPU path
            call()
    with pytest.raises(g2048.NativeError):
        ntuple.NTupleTrainer(net, 256)
    # shapes and dtypes are checked before the device
    for bad in (torch.zeros((4, 15), dtype=torch.uint8), torch.zeros((4, 16), dtype=torch.int32),
                torch.zeros(16, dtype=torch.uint8), torch.zeros((0, 16), dtype=torch.uint8),
                np.zeros((4, 16), dtype=np.uint8)):
        with pytest.raises((ValueError, TypeError)):
            net.stage_of(bad)
    # it is not an NTupleNetwork: the search, TC and lambda refuse it
    assert not isinstance(net, ntuple.NTupleNetwork)
    with pytest.raises(TypeError):
        net.search(boards)
    with pytest.raises(TypeError):
        g2048.ntsearch.expectimax(net, boards)
    with pytest.raises(TypeError):
        g2048.TCState(net)
    with pytest.raises(TypeError):
        g2048.TDLambdaState(net, 256)
    with pytest.raises(TypeError):
        ntstage.StagedNTupleNetwork.from_network(net, (5,))
    with pytest.raises(ValueError):
        net.resolved(3)
    assert g2048.ntstage is ntstage and g2048.StagedNTupleNetwork is ntstage.StagedNTupleNetwork
    assert {"ntstage", "StagedNTupleNetwork"} <= set(g2048.__all__)


def test_stage_of_resolved_and_from_network_on_the_cpu():
    """The plain-torch parts need no GPU: they agree with the reference."""
    from g2048 import ntstage, ntuple

    rng = np.random.default_rng(92)
    boards = (rng.integers(1, 12, (64, 16)) * (rng.random((64, 16)) < 0.6)).astype(np.uint8)
    # a cap per board, so that every stage of the bounds (5, 8) occurs
    boards = np.minimum(boards, rng.choice([4, 7, 11], (64, 1))).astype(np.uint8)
    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    ref = R.StagedNet(NR.TUPLES_2x4, (5, 8))
    got = net.stage_of(torch.from_numpy(boards))
    assert got.dtype == torch.int64 and got.tolist() == [ref.stage(b) for b in boards]
    assert set(got.tolist()) == {0, 1, 2}
    lut = rng.integers(-(1 << 20), 1 << 20, (3, 2, 65536)).astype(np.int32)
    lut[1:][rng.random((2, 2, 65536)) < 0.5] = ntstage.UNSET
    lut[0][rng.random((2, 65536)) < 0.25] = ntstage.UNSET
    net.lut.copy_(torch.from_numpy(lut))
    ref = R.StagedNet(NR.TUPLES_2x4, (5, 8), base=lut)
    assert net.set_counts() == [int((lut[s] != ntstage.UNSET).sum()) for s in range(3)]
    probe = rng.integers(0, 65536, 200)
    for s in range(3):
        plain = net.resolved(s)
        assert isinstance(plain, ntuple.NTupleNetwork) and plain.lut.shape == (2, 65536)
        assert not bool((plain.lut == ntstage.UNSET).any())
        for t in range(2):
            assert plain.lut[t][probe].tolist() == [ref.val(s, t, int(i)) for i in probe]
    single = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    single.lut.copy_(torch.from_numpy(rng.integers(-(1 << 20), 1 << 20, (2, 65536))))
    staged = ntstage.StagedNTupleNetwork.from_network(single, (5, 8))
    assert staged.bounds == (5, 8) and torch.equal(staged.lut[0], single.lut)
    assert staged.lut[0].data_ptr() != single.lut.data_ptr()
    assert bool((staged.lut[1:] == ntstage.UNSET).all())
    assert torch.equal(staged.resolved(2).lut, single.lut)


def test_save_load_round_trips_a_table_with_unset(tmp_path):
    from g2048 import ntstage, ntuple

    rng = np.random.default_rng(93)
    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (7,), device="cpu")
    lut = rng.integers(-(1 << 31) + 1, 1 << 31, (2, 2, 65536)).astype(np.int32)
    lut[rng.random(lut.shape) < 0.5] = ntstage.UNSET
    net.lut.copy_(torch.from_numpy(lut))
    path = str(tmp_path / "staged.pt")
    net.save(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(state) == ["bounds", "lut", "tuples"] and state["bounds"].tolist() == [7]
    back = ntstage.StagedNTupleNetwork.load(path, device="cpu")
    assert back.spec == net.spec and back.bounds == (7,) and torch.equal(back.lut, net.lut)
    assert back.set_counts() == net.set_counts() and 0 < back.set_counts()[1] < 2 * 65536
    with pytest.raises(ValueError):
        ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (8,), device="cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        ntstage.StagedNTupleNetwork(((0, 1, 2, 3), (4, 5, 6, 7)), (7,),
                                    device="cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (7, 9),
                                    device="cpu").load_state_dict(state)
    single = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (), device="cpu")
    single.save(path)
    assert ntstage.StagedNTupleNetwork.load(path, device="cpu").bounds == ()
