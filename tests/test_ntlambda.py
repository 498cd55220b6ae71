"""CPU-side checks of truncated TD(lambda) learning: the Python restatement
(tests/ntlambda_ref.py) reproduces its hand-computed anchors and, at H = 1, ntuple_ref's TD(0)
step; and the boundary of libg2048_ntlambda.so (header == exports == SIGNATURES, build stamps,
argument validation without a GPU, the Python side's refusals)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ntlambda_ref as R
import ntuple_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntlambda.h")
NAMES = ["g2048_ntlambda_last_error", "g2048_ntlambda_step"]

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]


# ------------------------------------------------------------------ the reference's anchors
def test_shifted_rounds_toward_zero():
    assert R.shifted(-7, 1, 1) == -3 and R.shifted(7, 1, 1) == 3
    assert R.shifted(-7, 2, 1) == -1 and R.shifted(-7, 3, 1) == 0
    assert R.shifted(-7, 0, 5) == -7 and R.shifted(-(1 << 31), 1, 31) == -1
    assert R.shifted(-(1 << 31), 0, 1) == -(1 << 31) and R.shifted((1 << 31) - 1, 7, 4) == 7


def corner(four=4096):
    base = [1024 * i for i in range(16)]
    base[4] = four
    return NR.Net(((0,),), base=[base])


def two_deep(net):
    lam = R.Lam(net, 1, 2, 1)
    lam.hist[1][0] = [4] + [0] * 15  # 0 steps back
    lam.hist[0][0] = [2] + [0] * 15  # 1 step back
    lam.head, lam.depth = [1], [2]
    return lam


def test_worked_step_two_deep_history_with_a_negative_odd_delta():
    lam = two_deep(corner())
    assert lam.step([A], 7, 2) == ([2], [0], [0]) and not lam.net.touched
    lam = two_deep(corner(4099))
    assert lam.back(0, 0) == [4] + [0] * 15 and lam.back(0, 1) == [2] + [0] * 15
    assert lam.step([A], 7, 2) == ([2], [-6], [-11])
    # delta_1 = -5: rounded toward zero (a floor would add 2 * -6 and 6 * -6)
    assert lam.net.touched == {(0, 4): 4077, (0, 2): 2038, (0, 0): -96}
    assert lam.head == [0] and lam.depth == [2]
    assert lam.hist[0][0] == [2] + [0] * 15 and lam.hist[1][0] == [4] + [0] * 15


def test_worked_step_terminal_board_drops_the_depth_and_keeps_the_head():
    lam = two_deep(corner())
    hist0 = [[list(r) for r in plane] for plane in lam.hist]
    # no legal move: target 0, err = -V(P0) = -8192, lr = 1 / 2: delta_0 = -4096, delta_1 = -2048
    assert lam.step([CHECKER], 1, 1) == ([0], [-8192], [-4096])
    assert lam.net.touched == {(0, 4): 4096 - 2 * 4096, (0, 2): 2048 - 2 * 2048,
                               (0, 0): -6 * 4096 - 6 * 2048}
    assert lam.depth == [0] and lam.head == [1] and lam.hist == hist0
    # the next step has no previous afterstate: nothing is added, and the ring goes on from head.
    # On the table as it is now, q[down] = 2 lut[1] + 6 lut[0] = 2048 + 6 lut[0] beats
    # q[left] = q[right] = 4096 + 2 lut[2] + 6 lut[0] = 6 lut[0].
    touched = dict(lam.net.touched)
    assert lam.step([A], 1, 1) == ([1], [0], [0]) and lam.net.touched == touched
    assert lam.head == [0] and lam.depth == [1]
    assert lam.hist[0][0] == [0] * 12 + [1, 1, 0, 0] and lam.hist[1] == hist0[1]


def test_depth_ramps_after_a_reset_and_the_ring_wraps():
    lam = R.Lam(NR.Net(NR.TUPLES_2x4), 1, 3, 1)
    board = [1, 1] + [0] * 14
    seen = []
    for _t in range(5):
        _acts, _errs, _deltas = lam.step([board], 1, 1)
        seen.append((lam.head[0], lam.depth[0]))
    assert seen == [(1, 1), (2, 2), (0, 3), (1, 3), (2, 3)]
    assert all(lam.hist[p][0] == [2] + [0] * 15 for p in range(3))
    for bad in ((0, 1), (9, 1), (3, 0), (2, 32), (3, 16), (8, 5)):
        with pytest.raises(ValueError):
            R.Lam(NR.Net(NR.TUPLES_2x4), 1, *bad)
    R.Lam(NR.Net(NR.TUPLES_2x4), 1, 2, 31)
    R.Lam(NR.Net(NR.TUPLES_2x4), 1, 1, 31)


def test_reference_at_h1_is_ntuple_refs_td_step():
    rng = np.random.default_rng(81)
    n = 24
    base = rng.integers(-(1 << 20), 1 << 20, (2, 65536))
    td, lam = NR.Net(NR.TUPLES_2x4, base=base), R.Lam(NR.Net(NR.TUPLES_2x4, base=base), n, 1, 3)
    prev, has_prev = [[0] * 16 for _ in range(n)], [0] * n
    for t in range(4):
        boards = (rng.integers(1, 12, (n, 16)) * (rng.random((n, 16)) < 0.6)).astype(np.uint8)
        if t >= 2:  # terminal boards: at t = 3 some follow a terminal step, some do not
            boards[t - 2:t + 1] = CHECKER
        assert lam.step(boards, 3, 6) == td.td_step(boards, prev, has_prev, 3, 6)
        assert lam.net.touched == td.touched and lam.hist[0] == prev
        assert lam.depth == has_prev and lam.head == [0] * n
    assert td.touched and 0 in has_prev


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_equals_exports_equals_signatures():
    import g2048._native as N
    from g2048 import ntlambda, ntsearch, nttc, ntuple, search

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntlambda.load()
    assert set(names) == set(ntlambda.SIGNATURES)
    assert _exported(ntlambda.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other five libraries keep their ABI: none of the new symbols
    for path in (N.LIB_PATH, search.LIB_PATH, ntuple.LIB_PATH, ntsearch.LIB_PATH, nttc.LIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("g2048_ntlambda")]
    assert not set(names) & (set(N.SIGNATURES) | set(search.SIGNATURES) | set(ntuple.SIGNATURES)
                             | set(ntsearch.SIGNATURES) | set(nttc.SIGNATURES))
    assert ntlambda.MAX_HORIZON == R.MAX_HORIZON == 8
    assert "G2048_NTLAMBDA_MAX_HORIZON 8" in src and "G2048_NTLAMBDA_MAX_LAM_SHIFT 31" in src
    assert ntlambda.MAX_LAM_SHIFT == 31


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntlambda

    out = subprocess.run(["readelf", "-d", ntlambda.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTTC_SRCS,
                  G.NTUPLE_SHARED):
        assert set(G.NTLAMBDA_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTLAMBDA_SRCS[0]))
    assert open(G.NTLAMBDA_STAMP).read().strip() == G.ntlambda_source_hash()
    assert open(G.NTTC_STAMP).read().strip() == G.nttc_source_hash()
    assert open(G.NTSEARCH_STAMP).read().strip() == G.ntsearch_source_hash()
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert open(G.SEARCH_STAMP).read().strip() == G.search_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert len(set(_hashes(G))) == 6


def test_stamp_follows_its_source_the_shared_header_and_its_own_header(tmp_path, monkeypatch):
    """Without the new source and header the five existing stamps have the values they have
    with them; a change to the new source changes only the new stamp; a change to the shared
    csrc header changes the four stamps of the libraries that include it; a change to
    g2048_ntlambda.h changes only the new stamp."""
    import shutil

    import __graft_entry__ as G

    assert len(G.NTUPLE_SHARED) == 1
    src = open(os.path.join(G.CSRC, G.NTLAMBDA_SRCS[0])).read()
    assert f'#include "{G.NTUPLE_SHARED[0]}"' in src
    before = _hashes(G)
    real_csrc, real_root = G.CSRC, G.ROOT
    copy = str(tmp_path / "csrc")
    shutil.copytree(real_csrc, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTLAMBDA_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:5] == before[:5] and after[5] != before[5]
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    shared = _hashes(G)
    assert shared[:2] == before[:2]
    assert all(shared[k] != before[k] for k in (2, 3, 4)) and shared[5] != after[5]
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(G.ROOT, "include"), os.path.join(root, "include"))
    with open(os.path.join(root, "include", "g2048_ntlambda.h"), "a") as f:
        f.write("/* changed */\n")
    monkeypatch.setattr(G, "ROOT", root)
    header = _hashes(G)
    assert header[:5] == shared[:5] and header[5] != shared[5]
    # a tree without the sixth library: the five existing stamps are what they are with it
    bare = str(tmp_path / "bare")
    shutil.copytree(real_csrc, bare)
    os.remove(os.path.join(bare, G.NTLAMBDA_SRCS[0]))
    monkeypatch.setattr(G, "CSRC", bare)
    monkeypatch.setattr(G, "ROOT", real_root)
    assert (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash()) == before[:5]
    with pytest.raises(FileNotFoundError):
        G.ntlambda_source_hash()


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

    for f in G.NTLAMBDA_SRCS:
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


FAKE = 1 << 20


def _step(lib, spec, lut=FAKE, boards=FAKE, n=4, hist=FAKE, head=FAKE, depth=FAKE, horizon=3,
          lam_shift=1, lr_num=1, lr_shift=10, action=FAKE, delta=FAKE, err=FAKE):
    return lib.g2048_ntlambda_step(C.byref(spec) if spec is not None else None, lut, boards, n,
                                   hist, head, depth, horizon, lam_shift, lr_num, lr_shift,
                                   action, delta, err, 0, None)


BAD_SPECS = [
    (dict(tuples=((0,),), n_tuples=0), b"n_tuples"),
    (dict(tuples=((0,),), n_tuples=9), b"n_tuples"),
    (dict(tuples=((0,),), n_cells=0), b"n_cells"),
    (dict(tuples=((0,),), n_cells=7), b"n_cells"),
    (dict(tuples=((0, 1), (2, 16))), b"not a board cell"),
    (dict(tuples=((0, 1, 2), (3, 4, 3))), b"twice"),
]


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused(kw, word):
    import g2048._native as N
    from g2048 import ntlambda

    lib = ntlambda.load()
    assert _step(lib, _spec(**kw)) == N.G2048_EINVAL
    assert word in lib.g2048_ntlambda_last_error(), lib.g2048_ntlambda_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntlambda

    lib = ntlambda.load()
    s = _spec(NR.TUPLES_2x4)
    cases = [(dict(lut=None), b"NULL"), (dict(boards=None), b"NULL"), (dict(hist=None), b"NULL"),
             (dict(head=None), b"NULL"), (dict(depth=None), b"NULL"),
             (dict(action=None), b"NULL"), (dict(delta=None), b"NULL"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(horizon=0), b"horizon"), (dict(horizon=9), b"horizon"),
             (dict(horizon=-1), b"horizon"),
             (dict(lam_shift=0), b"lam_shift"), (dict(lam_shift=32), b"lam_shift"),
             (dict(lam_shift=-1), b"lam_shift"),
             (dict(horizon=2, lam_shift=32), b"lam_shift"),
             (dict(horizon=3, lam_shift=16), b"exceeds 31"),   # (H - 1) s = 32
             (dict(horizon=5, lam_shift=8), b"exceeds 31"),    # (H - 1) s = 32
             (dict(horizon=8, lam_shift=5), b"exceeds 31"),    # (H - 1) s = 35
             (dict(lr_shift=32), b"lr_shift"), (dict(lr_shift=-1), b"lr_shift"),
             (dict(lr_num=-1), b"lr_num"), (dict(lr_num=(1 << 16) + 1), b"lr_num"),
             (dict(lut=FAKE + 2), b"aligned"), (dict(boards=FAKE + 4), b"aligned"),
             (dict(hist=FAKE + 8), b"aligned"), (dict(delta=FAKE + 2), b"aligned"),
             (dict(err=FAKE + 4), b"aligned")]
    for kw, word in cases:
        assert _step(lib, s, **kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_ntlambda_last_error(), (kw, lib.g2048_ntlambda_last_error())
    assert _step(lib, None) == N.G2048_EINVAL and b"spec" in lib.g2048_ntlambda_last_error()


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntlambda, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for kw in (dict(horizon=0), dict(horizon=9), dict(lam_shift=0), dict(lam_shift=32),
               dict(horizon=3, lam_shift=16), dict(horizon=8, lam_shift=5)):
        with pytest.raises(ValueError):
            ntlambda.TDLambdaState(net, 4, **kw)
    for n in (0, -1, g2048._native.MAX_BOARDS + 1):
        with pytest.raises(ValueError):
            ntlambda.TDLambdaState(net, n)
    with pytest.raises(TypeError):
        ntlambda.TDLambdaState(None, 4)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        ntlambda.TDLambdaState(net, 4)
    with pytest.raises(g2048.NativeError):
        ntlambda.TDLambdaTrainer(net, 256)
    # a state whose tensors live on the CPU steps nowhere
    lam = object.__new__(ntlambda.TDLambdaState)
    lam.net, lam.n, lam.horizon, lam.lam_shift = net, 4, 3, 1
    lam.hist = torch.zeros((3, 4, 16), dtype=torch.uint8)
    lam.head, lam.depth = torch.zeros(4, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(g2048.NativeError):
        lam.step(boards, 1, 10, torch.zeros(4, dtype=torch.uint8),
                 torch.zeros(4, dtype=torch.int32))
    assert g2048.ntlambda is ntlambda and g2048.TDLambdaState is ntlambda.TDLambdaState
    assert g2048.TDLambdaTrainer is ntlambda.TDLambdaTrainer
    assert issubclass(ntlambda.TDLambdaTrainer, ntuple.NTupleTrainer)
    assert {"ntlambda", "TDLambdaState", "TDLambdaTrainer"} <= set(g2048.__all__)
