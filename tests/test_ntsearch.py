"""CPU-side checks of the expectimax over the n-tuple network: the Python restatement
(tests/ntsearch_ref.py) reproduces the anchors the search was specified with, and the boundary of
libg2048_ntsearch.so (header == exports == SIGNATURES, build stamps, argument validation without
a GPU, the Python side's refusals)."""
import ctypes as C
import os
import re
import subprocess

import pytest
import torch

import ntsearch_ref as R
import ntuple_ref as NR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntsearch.h")

A = [1, 1] + [0] * 14
NEAR = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0]  # most of its children are terminal
CHECKER = NEAR[:15] + [1]
_ = None


def corner_up():
    return NR.Net(((0,),), base=lambda t, i: 1024 * i)


def corner_down():
    return NR.Net(((0,),), base=lambda t, i: -1000 * i - 7)


def zero_2x4():
    return NR.Net(NR.TUPLES_2x4)


# (network, board, p4, [values at depth 1, 2, 3] in move order up/down/left/right, action)
ANCHORS = [
    (corner_up, A, 0.5, [[_, 2048, 8192, 8192], [_, 9069, 11400, 11400],
                         [_, 15526, 15865, 15865]], 2),
    (corner_up, A, 0.1, [[_, 2048, 8192, 8192], [_, 8835, 9598, 9598],
                         [_, 11652, 11975, 11975]], 2),
    (corner_down, A, 0.5, [[_, -2056, 40, 40], [_, -256, 1478, 1478], [_, 4161, 4654, 4654]], 2),
    (zero_2x4, A, 0.5, [[_, 0, 4096, 4096], [_, 4096, 5734, 5734], [_, 9006, 9152, 9152]], 2),
    (corner_up, NEAR, 0.5, [[_, 10240, _, 10240], [_, 33792, _, 33792], [_, 53205, _, 53205]], 1),
    (corner_up, CHECKER, 0.1, [[_, _, _, _]] * 3, 0),
]


@pytest.mark.parametrize("make,board,p4,values,action", ANCHORS)
def test_reference_reproduces_the_anchors(make, board, p4, values, action):
    s = R.Search(make(), p4)
    for depth in (1, 2, 3):
        assert s.root(board, depth) == (values[depth - 1], action), depth


def test_zero_table_depth_2_by_hand():
    """left = 4096 + floor(6 * 8192 / 30): of the 15 empty cells next to the merged 4, the six in
    its row and column let a spawned 4 merge with it."""
    s = R.Search(zero_2x4())
    after = bytes([2] + [0] * 15)
    assert s.vafter(after, 1) == (6 * 8192) // 30 == 1638
    assert s.root(A, 2)[0][2] == 4096 + 1638


def test_depth_1_is_the_greedy_afterstate_policy():
    import numpy as np

    rng = np.random.default_rng(3)
    base = rng.integers(-(1 << 20), 1 << 20, (2, 65536))
    net = NR.Net(NR.TUPLES_2x4, base=base)
    s = R.Search(net)
    for _k in range(50):
        b = (rng.integers(1, 12, 16) * (rng.random(16) < 0.7)).astype(np.uint8)
        q, action, _after = net.policy(b)
        assert s.root(b, 1) == (q, action)


def test_the_floor_is_toward_minus_infinity_and_terminal_children_count_zero():
    import numpy as np

    rng = np.random.default_rng(4)
    base = rng.integers(-(1 << 20), 1 << 10, (2, 65536))  # mostly negative: so are the sums
    negative_inexact = 0
    for p4, W in ((0.5, 2), (0.1, 10)):
        s = R.Search(NR.Net(NR.TUPLES_2x4, base=base), p4)
        for _k in range(40):
            key = bytes(int(x) for x in rng.integers(1, 9, 16) * (rng.random(16) < 0.8))
            em = [c for c in range(16) if key[c] == 0]
            if not em:
                continue
            total = sum(k * s.vmax(key[:c] + bytes([e]) + key[c + 1:], 1)
                        for c in em for e, k in ((1, W - 1), (2, 1)))
            q, r = divmod(total, W * len(em))
            assert s.vafter(key, 1) == q and 0 <= r
            negative_inexact += total < 0 and r != 0
    assert negative_inexact >= 20
    assert R.Search(corner_up()).vmax(bytes(CHECKER), 2) == 0
    with pytest.raises(ValueError):
        R.Search(corner_up()).root(A, 4)
    with pytest.raises(ValueError):
        R.Search(corner_up(), 0.3)


def test_leaf_count_of_the_reference():
    s = R.Search(zero_2x4())
    assert [len(s.leaf_boards(A, d)) for d in (1, 2)] == [3, 318]
    assert len(s.leaf_boards(CHECKER, 2)) == 0


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_equals_exports_equals_signatures():
    import g2048._native as N
    from g2048 import ntsearch, ntuple, search

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == ["g2048_ntsearch_expectimax", "g2048_ntsearch_last_error"]
    lib = ntsearch.load()
    assert set(names) == set(ntsearch.SIGNATURES)
    assert _exported(ntsearch.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other three libraries keep their ABI: none of the new symbols
    for path in (N.LIB_PATH, search.LIB_PATH, ntuple.LIB_PATH):
        assert not [s for s in _exported(path) if s.startswith("g2048_ntsearch")]
    assert not set(names) & (set(N.SIGNATURES) | set(search.SIGNATURES) | set(ntuple.SIGNATURES))
    assert ntsearch.MAX_DEPTH == R.MAX_DEPTH == 3 and "G2048_NTSEARCH_MAX_DEPTH 3" in src


def test_library_does_not_link_against_the_ntuple_library():
    from g2048 import ntsearch

    out = subprocess.run(["readelf", "-d", ntsearch.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS):
        assert set(G.NTSEARCH_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTSEARCH_SRCS[0]))
    assert open(G.NTSEARCH_STAMP).read().strip() == G.ntsearch_source_hash()
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    hashes = [G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
              G.ntsearch_source_hash()]
    assert len(set(hashes)) == 4


def test_shared_header_is_in_both_stamps_and_not_in_the_main_one(tmp_path, monkeypatch):
    """The helpers both libraries use live in one csrc header: a change to it changes the stamps
    of libg2048_ntuple.so and libg2048_ntsearch.so and neither of the other two."""
    import shutil

    import __graft_entry__ as G

    assert len(G.NTUPLE_SHARED) == 1
    for src in G.NTUPLE_SRCS + G.NTSEARCH_SRCS:
        assert f'#include "{G.NTUPLE_SHARED[0]}"' in open(os.path.join(G.CSRC, src)).read()
    before = (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
              G.ntsearch_source_hash())
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    with open(os.path.join(copy, G.NTUPLE_SHARED[0]), "a") as f:
        f.write("// changed\n")
    monkeypatch.setattr(G, "CSRC", copy)
    after = (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
             G.ntsearch_source_hash())
    assert after[:2] == before[:2] and after[2] != before[2] and after[3] != before[3]


def _all_hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash())


def test_tree_walk_header_is_in_the_two_search_stamps_and_in_no_other(tmp_path, monkeypatch):
    """The expectimax tree lives in one csrc header that both search sources include: a change to
    it changes the stamps of libg2048_ntsearch.so and libg2048_stagesearch.so and of none of the
    other libraries."""
    import shutil

    import __graft_entry__ as G

    assert G.NTSEARCH_SHARED == ("g2048_ntsearch_dev.hpp",)
    for src in G.NTSEARCH_SRCS + G.STAGESEARCH_SRCS:
        assert f'#include "{G.NTSEARCH_SHARED[0]}"' in open(os.path.join(G.CSRC, src)).read()
    shared = open(os.path.join(G.CSRC, G.NTSEARCH_SHARED[0])).read()
    assert G.NTSTAGE_SHARED[0] not in re.sub(r"//[^\n]*", "", shared)
    before = _all_hashes(G)
    assert len(set(before)) == 13
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _all_hashes(G) == before
    with open(os.path.join(copy, G.NTSEARCH_SHARED[0]), "a") as f:
        f.write("// changed\n")
    after = _all_hashes(G)
    assert {k for k in range(13) if after[k] != before[k]} == {3, 7}


def test_both_sources_include_the_one_copy_of_the_tree_walk():
    """The tree (vmax, vafter, leaf_value), its helpers and the kernel are defined once, in the
    shared header, and in neither search source; the sources define no kernel at all."""
    import __graft_entry__ as G

    shared = open(os.path.join(G.CSRC, G.NTSEARCH_SHARED[0])).read()
    for src in G.NTSEARCH_SRCS + G.STAGESEARCH_SRCS:
        text = open(os.path.join(G.CSRC, src)).read()
        assert f'#include "{G.NTSEARCH_SHARED[0]}"' in text
        for name in ("int64_t vmax(", "int64_t vafter(", "int64_t leaf_value(",
                     "int64_t floor_quot(", "uint32_t empties(", "uint64_t flip_rows(",
                     "uint64_t flip_cols(", "int64_t row_sum(", "void k_search("):
            assert name in shared and name not in text, (src, name)
        assert "__global__" not in text, src


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

    for f in G.NTSEARCH_SRCS:
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
    from g2048 import ntsearch

    lib = ntsearch.load()
    fake = 1 << 20
    rc = lib.g2048_ntsearch_expectimax(C.byref(_spec(**kw)), fake, fake, 4, 2, 0, fake, fake, 0,
                                       None)
    assert rc == N.G2048_EINVAL
    assert word in lib.g2048_ntsearch_last_error(), lib.g2048_ntsearch_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntsearch

    lib = ntsearch.load()
    fake = 1 << 20
    s = _spec(NR.TUPLES_2x4)

    def call(spec=s, lut=fake, boards=fake, n=4, depth=2, flags=0, values=fake, action=fake):
        return lib.g2048_ntsearch_expectimax(C.byref(spec) if spec is not None else None, lut,
                                             boards, n, depth, flags, values, action, 0, None)

    for kw, word in ((dict(spec=None), b"spec"), (dict(lut=None), b"NULL"),
                     (dict(boards=None), b"NULL"), (dict(values=None, action=None), b"NULL"),
                     (dict(n=0), b"n ="), (dict(n=-3), b"n ="),
                     (dict(n=N.MAX_BOARDS + 1), b"n ="),
                     (dict(depth=0), b"depth"), (dict(depth=4), b"depth"),
                     (dict(depth=-1), b"depth"),
                     (dict(flags=N.EGREEDY_FIXED), b"flags"), (dict(flags=8), b"flags"),
                     (dict(flags=N.P4_10 | 8), b"flags"),
                     (dict(lut=fake + 2), b"aligned"), (dict(boards=fake + 4), b"aligned"),
                     (dict(values=fake + 4), b"aligned")):
        assert call(**kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_ntsearch_last_error(), (kw, lib.g2048_ntsearch_last_error())


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntsearch, ntuple, player

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        ntsearch.expectimax(net, boards)
    with pytest.raises(g2048.NativeError):
        net.search(boards, depth=1)
    with pytest.raises(ValueError, match="p4"):
        ntsearch.expectimax(net, boards, p4=0.3)
    for depth in (0, 4):
        with pytest.raises(ValueError, match="depth"):
            ntsearch.expectimax(net, boards, depth=depth)
    with pytest.raises(TypeError):
        ntsearch.expectimax(None, boards)
    with pytest.raises(ValueError, match="network"):
        player.BatchedPlayer(4).play("ntuple_search")
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=net, search_depth=4).play("ntuple_search")
    with pytest.raises(ValueError, match="ntuple_search"):  # the message lists the new policy
        player.BatchedPlayer(4).play("minimax")
    assert g2048.ntsearch is ntsearch and "ntsearch" in g2048.__all__
