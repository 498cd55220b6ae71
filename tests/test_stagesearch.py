"""CPU-side checks of the expectimax over the multi-stage n-tuple network: the reference
(tests/stagesearch_ref.py, the composition of ntsearch_ref's search and ntstage_ref's network)
reproduces the anchors the search was specified with and the three identities of the header; and
the boundary of libg2048_stagesearch.so (header == exports == SIGNATURES, build stamps, argument
validation without a GPU, the Python side's refusals and the player's argument checks)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ntsearch_ref as SR
import ntstage_ref as TR
import ntuple_ref as NR
import stagesearch_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_stagesearch.h")
NAMES = ["g2048_stagesearch_expectimax", "g2048_stagesearch_last_error"]

A = [1, 1] + [0] * 14
NEAR = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0]
CHECKER = NEAR[:15] + [1]
TOP = [24, 24, 23, 23, 22, 22, 0, 0, 1, 2, 1, 2, 0, 0, 1, 1]
_ = None


def table_x(s, t, i):
    """bounds (2,): stage 0 1024 i; stage 1 4096 i + 3 at even i, UNSET at odd i."""
    if s == 0:
        return 1024 * i
    return 4096 * i + 3 if i % 2 == 0 else None


def table_y(s, t, i):
    """bounds (25,): stage 0 1000 i, stage 1 all -77."""
    return 1000 * i if s == 0 else -77


# (bounds, table, board, p4, [values at depth 1, 2, 3], [action at depth 1, 2, 3])
ANCHORS = [
    ((2,), table_x, A, 0.5, [[_, 2048, 20504, 20504], [_, 23136, 24803, 24803],
                             [_, 27020, 28091, 28091]], [2, 2, 2]),
    ((2,), table_x, A, 0.1, [[_, 2048, 20504, 20504], [_, 21497, 22126, 22126],
                             [_, 24087, 25024, 25024]], [2, 2, 2]),
    ((2,), table_x, NEAR, 0.5, [[_, 34834, _, 34834], [_, 51218, _, 51218],
                                [_, 69650, _, 69650]], [1, 1, 1]),
    ((25,), table_y, TOP, 0.5, [[64096, 8096, 60129545624, 60129545624],
                                [60129555044, 42949684632, 60129549464, 60129556632]], [2, 3]),
    ((2,), table_x, CHECKER, 0.1, [[_, _, _, _]] * 3, [0, 0, 0]),
]


# ------------------------------------------------------------------ the reference's anchors
@pytest.mark.parametrize("bounds,table,board,p4,values,actions", ANCHORS)
def test_reference_reproduces_the_anchors(bounds, table, board, p4, values, actions):
    s = R.staged_search(((0,),), bounds, table, p4)
    for depth, (v, a) in enumerate(zip(values, actions), start=1):
        assert s.root(board, depth) == (v, a), depth


def test_anchors_by_hand():
    """The hand computations of the reference's docstring, step by step."""
    s = R.staged_search(((0,),), (2,), table_x)
    net = s.net
    assert [net.val(1, 0, i) for i in range(4)] == [3, 1024, 8195, 3072]
    left = [2] + [0] * 15
    assert net.stage(A) == 0 and net.stage(left) == 1
    assert net.V(left) == 2 * 8195 + 6 * 3 and (4 << 10) + net.V(left) == 20504
    # the single table alone: tests/ntsearch_ref.py's anchor
    single = SR.Search(NR.Net(((0,),), base=lambda t, i: 1024 * i))
    assert single.root(A, 1) == ([_, 2048, 8192, 8192], 2)
    # board N, down, depth 2: one empty cell, two children
    after = bytes([1, 2, 1, 0, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2])
    assert [m for m in s.moves(bytes(NEAR)) if m[0] == 1] == [(1, after, 0)]
    assert net.V(after) == 2 * (1024 + 3 + 8195 + 8195) == 34834
    two, four = after[:3] + b"\x01" + after[4:], after[:3] + b"\x02" + after[4:]
    assert s.vmax(two, 1) == 24576 + 2 * (3 + 8195 + 3 + 3072) == 47122
    assert s.vmax(four, 1) == 20480 + 34834 == 55314
    assert s.vafter(after, 1) == (47122 + 55314) // 2 == 51218
    # table Y: the bound is reached only by the merge
    y = R.staged_search(((0,),), (25,), table_y)
    assert y.net.stage(TOP) == 0
    moved, gain = NR.E.move(TOP, 2)
    assert y.net.stage(moved) == 1 and gain == (1 << 25) + (1 << 24) + (1 << 23) + 4
    assert (gain << 10) + 8 * -77 == 60129545624


def test_leaves_cross_stages_and_one_frozen_stage_is_another_search():
    """What the library is for: with the bounds (5, 8) most depth-2 leaves of a mixed batch lie
    in another stage than their root, and a search over one frozen stage gives other values."""
    rng = np.random.default_rng(301)
    base = rng.integers(-(1 << 20), 1 << 20, (3, 2, 65536))
    base[1:][rng.random((2, 2, 65536)) < 0.5] = TR.UNSET
    s = R.staged_search(NR.TUPLES_2x4, (5, 8), base)
    b = rng.integers(1, 12, (12, 16)) * (rng.random((12, 16)) < 0.6)
    boards = np.minimum(b, rng.choice([4, 7, 11], (12, 1))).astype(np.uint8)
    leaves, crossed = R.crossing(s, boards, 2)
    assert leaves > 1000 and 4 * crossed >= leaves
    depths = R.fall_depths(s, boards, 2)
    assert sum(depths) == 16 * leaves and all(d > 0 for d in depths)
    frozen = SR.Search(NR.Net(NR.TUPLES_2x4, base=base[0]))
    assert sum(frozen.root(x, 2) != s.root(x, 2) for x in boards) >= 10


def test_the_three_identities_hold_in_the_reference():
    rng = np.random.default_rng(302)
    base = rng.integers(-(1 << 20), 1 << 20, (2, 65536))
    boards = (rng.integers(1, 12, (6, 16)) * (rng.random((6, 16)) < 0.7)).astype(np.uint8)
    half = np.stack([base, np.where(rng.random(base.shape) < 0.5, TR.UNSET, base + 5)])
    staged = TR.StagedNet(NR.TUPLES_2x4, (5,), base=half)
    s = SR.Search(staged)
    plain = SR.Search(NR.Net(NR.TUPLES_2x4, base=base))
    one = R.staged_search(NR.TUPLES_2x4, (), [base])
    lifted = R.staged_search(NR.TUPLES_2x4, (5, 8), lambda st, t, i: int(base[t][i]) if st == 0
                             else None)
    for b in boards:
        q, action, _after = staged.policy(b)
        assert s.root(b, 1) == (q, action)                        # depth 1 is the staged policy
        for depth in (1, 2):
            assert one.root(b, depth) == plain.root(b, depth)     # S = 1 is the plain search
            assert lifted.root(b, depth) == plain.root(b, depth)  # stage 0 alone, the rest UNSET
    with pytest.raises(ValueError):
        one.root(boards[0], 4)
    with pytest.raises(ValueError):
        R.staged_search(NR.TUPLES_2x4, (5,), None, 0.3)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_equals_exports_equals_signatures():
    import g2048._native as N
    from g2048 import ntlambda, ntsearch, ntstage, nttc, ntuple, search, stagesearch

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = stagesearch.load()
    assert set(names) == set(stagesearch.SIGNATURES)
    assert _exported(stagesearch.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other seven libraries keep their ABI: none of the new symbols
    for mod in (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage):
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_stagesearch")]
        assert not set(names) & set(mod.SIGNATURES)
    assert stagesearch.MAX_DEPTH == R.MAX_DEPTH == 3
    assert "G2048_STAGESEARCH_MAX_DEPTH 3" in src and "G2048_STAGESEARCH_MAX_EXPONENT 24" in src
    assert stagesearch.INT64_MIN == R.INT64_MIN == torch.iinfo(torch.int64).min


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import stagesearch

    out = subprocess.run(["readelf", "-d", stagesearch.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash())


def test_build_keeps_the_new_files_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTTC_SRCS,
                  G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.NTUPLE_SHARED):
        assert set(G.STAGESEARCH_SRCS).isdisjoint(other)
        assert set(G.NTSTAGE_SHARED).isdisjoint(other)
    assert G.NTSTAGE_SHARED == ("g2048_ntstage_dev.hpp",) and len(G.NTUPLE_SHARED) == 1
    for f in G.STAGESEARCH_SRCS + G.NTSTAGE_SHARED:
        assert os.path.exists(os.path.join(G.CSRC, f))
    for stamp, want in ((G.STAGESEARCH_STAMP, G.stagesearch_source_hash()),
                        (G.NTSTAGE_STAMP, G.ntstage_source_hash()),
                        (G.NTLAMBDA_STAMP, G.ntlambda_source_hash()),
                        (G.NTTC_STAMP, G.nttc_source_hash()),
                        (G.NTSEARCH_STAMP, G.ntsearch_source_hash()),
                        (G.NTUPLE_STAMP, G.ntuple_source_hash()),
                        (G.SEARCH_STAMP, G.search_source_hash()), (G.STAMP, G.source_hash())):
        assert open(stamp).read().strip() == want, stamp
    assert len(set(_hashes(G))) == 8


def test_both_sources_include_the_one_copy_of_the_stage_rule():
    """StageParams, max_tile, stage_of, make_stage_params and check_stages are defined once, in
    the shared header, and in neither source."""
    import __graft_entry__ as G

    shared = open(os.path.join(G.CSRC, G.NTSTAGE_SHARED[0])).read()
    for src in G.NTSTAGE_SRCS + G.STAGESEARCH_SRCS:
        text = open(os.path.join(G.CSRC, src)).read()
        assert f'#include "{G.NTSTAGE_SHARED[0]}"' in text
        assert f'#include "{G.NTUPLE_SHARED[0]}"' in text
        for name in ("struct StageParams", "uint32_t max_tile(", "uint32_t stage_of(",
                     "make_stage_params(const", "int check_stages("):
            assert name in shared and name not in text, (src, name)


def test_stamps_follow_the_new_files(tmp_path, monkeypatch):
    """The new stamp follows its source, both shared csrc headers and its public headers; the
    stage library's stamp follows the new shared header too; the stamps of the main library and
    of the search, ntuple, ntsearch, nttc and ntlambda libraries follow none of the new files,
    and have the same values in a tree without them."""
    import shutil

    import __graft_entry__ as G

    before = _hashes(G)
    real_csrc, real_root = G.CSRC, G.ROOT
    copy = str(tmp_path / "csrc")
    shutil.copytree(real_csrc, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before

    def touch(path):
        with open(path, "a") as f:
            f.write("// changed\n" if path.endswith(("hip", "hpp")) else "/* changed */\n")
        return _hashes(G)

    own = touch(os.path.join(copy, G.STAGESEARCH_SRCS[0]))
    assert own[:7] == before[:7] and own[7] != before[7]
    rule = touch(os.path.join(copy, G.NTSTAGE_SHARED[0]))
    assert rule[:6] == before[:6] and rule[6] != own[6] and rule[7] != own[7]
    tree = touch(os.path.join(copy, G.NTSEARCH_SHARED[0]))  # the two searches' tree walk
    assert {k for k in range(8) if tree[k] != rule[k]} == {3, 7}
    family = touch(os.path.join(copy, G.NTUPLE_SHARED[0]))
    assert family[:2] == before[:2]
    assert all(family[k] != tree[k] for k in range(2, 8))
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(root, "include"))
    monkeypatch.setattr(G, "ROOT", root)
    assert _hashes(G) == family
    last = family
    for header, moved in (("g2048_stagesearch.h", {7}), ("g2048_ntstage.h", {6, 7}),
                          ("g2048_ntuple.h", {2, 3, 4, 5, 6, 7})):
        now = touch(os.path.join(root, "include", header))
        assert {k for k in range(8) if now[k] != last[k]} == moved, header
        last = now
    # a tree without the eighth library and the shared stage header
    bare, bare_root = str(tmp_path / "bare"), str(tmp_path / "bare_root")
    shutil.copytree(real_csrc, bare)
    for f in G.STAGESEARCH_SRCS + G.NTSTAGE_SHARED:
        os.remove(os.path.join(bare, f))
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(bare_root, "include"))
    os.remove(os.path.join(bare_root, "include", "g2048_stagesearch.h"))
    monkeypatch.setattr(G, "CSRC", bare)
    monkeypatch.setattr(G, "ROOT", bare_root)
    assert (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(),
            G.ntlambda_source_hash()) == before[:6]
    for missing in (G.ntstage_source_hash, G.stagesearch_source_hash):
        with pytest.raises(FileNotFoundError):
            missing()


def test_kernel_has_no_store_data_hazard_and_no_scratch(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's flags,
    as the other libraries' tests audit theirs; and none of the three kernels uses scratch."""
    import shutil
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.STAGESEARCH_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", open(out).read())
        assert len(sizes) == 3 and set(sizes) == {"0"}


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
UNGIVEN = object()


def _call(lib, spec=UNGIVEN, stages=UNGIVEN, lut=FAKE, boards=FAKE, n=4, depth=2, flags=0,
          values=FAKE, action=FAKE):
    spec = _spec(NR.TUPLES_2x4) if spec is UNGIVEN else spec
    stages = _stages((5, 8)) if stages is UNGIVEN else stages
    return lib.g2048_stagesearch_expectimax(
        C.byref(spec) if spec is not None else None,
        C.byref(stages) if stages is not None else None, lut, boards, n, depth, flags, values,
        action, 0, None)


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
def test_bad_specs_are_refused(kw, word):
    import g2048._native as N
    from g2048 import stagesearch

    lib = stagesearch.load()
    assert _call(lib, spec=_spec(**kw)) == N.G2048_EINVAL
    assert word in lib.g2048_stagesearch_last_error(), lib.g2048_stagesearch_last_error()


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused(kw, word):
    import g2048._native as N
    from g2048 import stagesearch

    lib = stagesearch.load()
    assert _call(lib, stages=_stages(**kw)) == N.G2048_EINVAL
    assert word in lib.g2048_stagesearch_last_error(), lib.g2048_stagesearch_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import stagesearch

    lib = stagesearch.load()
    err = lib.g2048_stagesearch_last_error
    for kw, word in ((dict(spec=None), b"spec"), (dict(stages=None), b"stages"),
                     (dict(lut=None), b"NULL"), (dict(boards=None), b"NULL"),
                     (dict(values=None, action=None), b"NULL"),
                     (dict(n=0), b"n ="), (dict(n=-3), b"n ="),
                     (dict(n=N.MAX_BOARDS + 1), b"n ="),
                     (dict(depth=0), b"depth"), (dict(depth=4), b"depth"),
                     (dict(depth=-1), b"depth"),
                     (dict(flags=N.EGREEDY_FIXED), b"flags"), (dict(flags=8), b"flags"),
                     (dict(flags=N.P4_10 | 8), b"flags"),
                     (dict(lut=FAKE + 2), b"aligned"), (dict(boards=FAKE + 4), b"aligned"),
                     (dict(values=FAKE + 4), b"aligned")):
        assert _call(lib, **kw) == N.G2048_EINVAL, kw
        assert word in err(), (kw, err())
        assert b"stagesearch_expectimax" in err()


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntsearch, ntstage, ntuple, stagesearch

    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
        stagesearch.expectimax(net, boards)
    with pytest.raises(g2048.NativeError):
        net.expectimax(boards, depth=1)
    with pytest.raises(ValueError, match="p4"):
        stagesearch.expectimax(net, boards, p4=0.3)
    for depth in (0, 4):
        with pytest.raises(ValueError, match="depth"):
            net.expectimax(boards, depth=depth)
    for other in (None, plain, net.lut):  # it takes a staged network and nothing else
        with pytest.raises(TypeError, match="StagedNTupleNetwork"):
            stagesearch.expectimax(other, boards)
    # the refusals that stay: the single-table search does not take a staged network
    with pytest.raises(TypeError, match="expectimax"):  # the message names the new method
        net.search(boards)
    with pytest.raises(TypeError):
        ntsearch.expectimax(net, boards)
    assert g2048.stagesearch is stagesearch and "stagesearch" in g2048.__all__
    assert stagesearch.LIB_PATH.endswith("libg2048_stagesearch.so")


def test_player_checks_the_ntstage_search_arguments():
    from g2048 import ntstage, ntuple, player

    staged = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (7,), device="cpu")
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    with pytest.raises(ValueError, match="network"):
        player.BatchedPlayer(4).play("ntstage_search")
    with pytest.raises(TypeError, match="StagedNTupleNetwork"):
        player.BatchedPlayer(4, ntuple=plain).play("ntstage_search")
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=staged, search_depth=4).play("ntstage_search")
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=staged, search_depth=0)
    with pytest.raises(ValueError, match="ntstage_search"):  # the message lists the new policy
        player.BatchedPlayer(4).play("minimax")
