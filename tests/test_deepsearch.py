"""CPU-side checks of the wide expectimax (include/g2048_deepsearch.h): the level-wise reference
(tests/deepsearch_ref.py: slots, sentinels, sub-search, backups) equals the plain recursion at
every depth and every split, on one table and on staged ones; depths 4 and 5 are pinned as
literals; and the boundary of libg2048_deepsearch.so (header == exports == SIGNATURES, the
fourteen build stamps, the workspace formula, argument validation without a GPU, the Python
side's refusals and chunking, the player's argument checks)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import deepsearch_ref as R
import ntsearch_ref as SR
import ntstage_ref as TR
import ntuple_ref as NR
import stagesearch_ref as SSR
from boards import mask_boards

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_deepsearch.h")
NAMES = ["g2048_deepsearch_expectimax", "g2048_deepsearch_last_error",
         "g2048_deepsearch_staged_expectimax", "g2048_deepsearch_workspace_bytes"]
_ = None

A = [1, 1] + [0] * 14                                       # a tie between left and right
ONE = [1] + [0] * 15                                        # one tile, 15 empty cells
NEAR = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 0]     # afterstates with one empty cell
CHECKER = NEAR[:15] + [1]                                   # no legal move
B1 = [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 0, 1]  # right: every child is terminal
B2 = [3, 7, 2, 9, 1, 5, 8, 4, 6, 10, 0, 11, 12, 0, 13, 14]
B3 = [2, 5, 1, 6, 0, 9, 3, 7, 4, 0, 8, 10, 11, 12, 0, 13]
ONE_MOVE = [0, 1, 2, 3, 0, 2, 3, 4, 0, 3, 4, 5, 0, 4, 5, 6]  # only left is legal
BOARDS = {"A": A, "ONE": ONE, "NEAR": NEAR, "B1": B1, "B2": B2, "B3": B3}


def table_1x1(t, i):
    return 1024 * i


def table_2x4(t, i):
    """A fixed table in +-2^20 (about half negative, so the floors matter)."""
    return ((i * 2654435761 + t * 40503 + 12345) % (1 << 21)) - (1 << 20)


NETS = {"1x1": (((0,),), table_1x1), "2x4": (NR.TUPLES_2x4, table_2x4)}
_deeps = {}


def deep(name, p4=0.5):
    """One memoising reference per (table, p4), shared by every test."""
    if (name, p4) not in _deeps:
        tuples, base = NETS[name]
        _deeps[(name, p4)] = R.Deep(SR.Search(NR.Net(tuples, base=base), p4))
    return _deeps[(name, p4)]


# (table, p4, board) -> {depth: (values, action)}: the plain recursion, written down
DEEP_ANCHORS = {
    ("1x1", 0.5, "A"): {4: ([_, 19897, 20050, 20050], 2), 5: ([_, 24895, 24928, 24928], 2)},
    ("1x1", 0.5, "ONE"): {4: ([_, 15021, _, 15021], 1), 5: ([_, 19807, _, 19807], 1)},
    ("1x1", 0.5, "NEAR"): {4: ([_, 90142, _, 90142], 1), 5: ([_, 128053, _, 128053], 1)},
    ("1x1", 0.5, "B1"): {4: ([_, 48128, 4096, 0], 1), 5: ([_, 51818, 4096, 0], 1)},
    ("1x1", 0.5, "B2"): {4: ([33536, 57152, 14720, 26624], 1),
                         5: ([28160, 60672, 10560, 27840], 1)},
    ("1x1", 0.5, "B3"): {4: ([59221, 71106, 34154, 48426], 1),
                         5: ([49205, 75035, 35808, 40483], 1)},
    ("1x1", 0.1, "NEAR"): {4: ([_, 98153, _, 98153], 1), 5: ([_, 140700, _, 140700], 1)},
    ("1x1", 0.1, "B1"): {4: ([_, 9625, 4423, 0], 1), 5: ([_, 11564, 4423, 0], 1)},
    ("1x1", 0.1, "B2"): {4: ([7575, 18674, 6274, 31817], 3), 5: ([5598, 19207, 4371, 35101], 3)},
    ("1x1", 0.1, "B3"): {4: ([60791, 68987, 40908, 50014], 1),
                         5: ([61843, 78347, 36272, 54531], 1)},
    ("2x4", 0.5, "NEAR"): {4: ([_, 3703313, _, 3703313], 1), 5: ([_, 4236715, _, 4236715], 1)},
    ("2x4", 0.5, "B1"): {4: ([_, 794144, 4096, 0], 1), 5: ([_, 1971441, 4096, 0], 1)},
    ("2x4", 0.5, "B2"): {4: ([842880, 646156, 444016, 4500], 0),
                         5: ([368931, 1128945, 180044, 219992], 1)},
    ("2x4", 0.5, "B3"): {4: ([2831672, 2662285, 4304100, 1948333], 2),
                         5: ([1977298, 2468506, 3172210, 1745366], 2)},
    ("2x4", 0.1, "NEAR"): {4: ([_, 3785435, _, 3785435], 1), 5: ([_, 3261991, _, 3261991], 1)},
    ("2x4", 0.1, "B1"): {4: ([_, 231268, 4423, 0], 1), 5: ([_, 505952, 4423, 0], 1)},
    ("2x4", 0.1, "B2"): {4: ([256037, 179958, 188242, 56114], 0),
                         5: ([120010, 616622, 58575, 205012], 1)},
    ("2x4", 0.1, "B3"): {4: ([2233499, 3130636, 6179746, 2891657], 2),
                         5: ([1509027, 2120452, 4954504, 2810491], 2)},
}


# ------------------------------------------------------------------ the reference
def small_boards():
    """tests/boards.py's boards, one per legal mask, and the named ones."""
    by_mask = {}
    for b in mask_boards():
        moves = SR.Search(NR.Net(((0,),))).moves(bytes(b))
        by_mask.setdefault(sum(1 << a for a, _s, _g in moves), b)
    assert len(by_mask) == 16
    return [list(map(int, by_mask[m])) for m in range(16)] + [A, ONE, NEAR, CHECKER, B1, B2, B3,
                                                              ONE_MOVE]


@pytest.mark.parametrize("p4", [0.5, 0.1])
@pytest.mark.parametrize("name", ["1x1", "2x4"])
def test_level_wise_equals_the_recursive_root_at_depths_1_to_3(name, p4):
    d = deep(name, p4)
    for depth in (1, 2, 3):
        assert R.legal_tops(depth) == tuple(range(depth))
        for b in small_boards():
            want = d.s.root(b, depth)
            for top in R.legal_tops(depth):
                assert d.root(b, depth, top) == want, (depth, top, b)


def test_the_anchors_of_ntsearch_ref_at_every_split():
    """The hand-checked numbers of tests/ntsearch_ref.py's docstring, level-wise."""
    want = {(1, 0.5): [_, 2048, 8192, 8192], (2, 0.5): [_, 9069, 11400, 11400],
            (3, 0.5): [_, 15526, 15865, 15865], (2, 0.1): [_, 8835, 9598, 9598],
            (3, 0.1): [_, 11652, 11975, 11975]}
    near = {1: [_, 10240, _, 10240], 2: [_, 33792, _, 33792], 3: [_, 53205, _, 53205]}
    for (depth, p4), v in want.items():
        for top in R.legal_tops(depth):
            assert deep("1x1", p4).root(A, depth, top) == (v, 2)
            if p4 == 0.5:
                assert deep("1x1").root(NEAR, depth, top) == (near[depth], 1)
    neg = R.Deep(SR.Search(NR.Net(((0,),), base=lambda t, i: -1000 * i - 7)))
    for depth, v in ((1, [_, -2056, 40, 40]), (2, [_, -256, 1478, 1478]),
                     (3, [_, 4161, 4654, 4654])):
        for top in R.legal_tops(depth):
            assert neg.root(A, depth, top) == (v, 2)
    zero = R.Deep(SR.Search(NR.Net(NR.TUPLES_2x4)))
    for depth, v in ((1, [_, 0, 4096, 4096]), (2, [_, 4096, 5734, 5734]),
                     (3, [_, 9006, 9152, 9152])):
        for top in R.legal_tops(depth):
            assert zero.root(A, depth, top) == (v, 2)


def staged(S, kind, p4=0.5):
    """S stages over the 2x4 set; the top stage fresh (no UNSET), half UNSET or all UNSET."""
    bounds = {1: (), 2: (3,), 3: (3, 6)}[S]

    def base(s, t, i):
        if s == S - 1 and S > 1:
            if kind == "unset" or (kind == "half" and (i + t) % 2):
                return None
        return table_2x4(t, i + 977 * s)

    return R.Deep(SSR.staged_search(NR.TUPLES_2x4, bounds, base, p4))


@pytest.mark.parametrize("kind", ["fresh", "half", "unset"])
@pytest.mark.parametrize("S", [1, 2, 3])
def test_level_wise_equals_the_recursive_root_on_staged_tables(S, kind):
    boards = [A, NEAR, B2, B3, [5, 6, 0, 0, 2, 2, 1, 0, 0, 1, 3, 0, 0, 0, 0, 1], CHECKER]
    for p4 in (0.5, 0.1):
        d = staged(S, kind, p4)
        for depth in (1, 2, 3):
            for b in boards:
                want = d.s.root(b, depth)
                for top in R.legal_tops(depth):
                    assert d.root(b, depth, top) == want, (depth, top, b)
    # a leaf in a later stage than its root: the merge of the two 4s reaches the bound 3
    if S > 1:
        d = staged(S, kind)
        root = [2, 2, 1, 0] + [0] * 12
        assert d.s.net.stage(root) == 0
        assert any(d.s.net.stage(s) == 1 for _a, s, _g in d.s.moves(bytes(root)))
        assert d.root(root, 4, 1) == d.root(root, 4, 2) == d.plain(root, 4)


@pytest.mark.parametrize("key", list(DEEP_ANCHORS), ids=lambda k: f"{k[0]}-{k[1]}-{k[2]}")
def test_depths_4_and_5_against_the_plain_recursion_and_the_literals(key):
    name, p4, board = key
    d = deep(name, p4)
    assert R.legal_tops(4) == (1, 2) and R.legal_tops(5) == (2,)
    for depth, want in DEEP_ANCHORS[key].items():
        assert d.plain(BOARDS[board], depth) == want, depth
        for top in R.legal_tops(depth):
            assert d.root(BOARDS[board], depth, top) == want, (depth, top)


def test_the_named_cases():
    d = deep("1x1")
    m = d.s.moves
    # a root with no legal move: every slot is a sentinel, action 0 and four illegal values
    assert m(bytes(CHECKER)) == [] and set(d.levels(CHECKER, 2)[1]) == {None}
    for depth in (2, 3, 4, 5):
        for top in R.legal_tops(depth):
            assert d.root(CHECKER, depth, top) == ([_, _, _, _], 0)
    # a root with one legal move
    assert [a for a, _s, _g in m(bytes(ONE_MOVE))] == [2]
    for depth, top in ((4, 1), (4, 2), (5, 2)):
        v, a = d.root(ONE_MOVE, depth, top)
        assert a == 2 and [x is None for x in v] == [True, True, False, True]
        assert (v, a) == d.plain(ONE_MOVE, depth)
    # a level-1 board with no legal move after its spawn: Vmax 0, and every slot below it a
    # sentinel; B1's move right gains nothing and all its children are terminal
    l1, l2 = d.levels(B1, 2)
    right = [q for q in range(R.slot(0, 3, 0, 0), R.slot(0, 3, 0, 0) + 32) if l1[q] is not None]
    assert len(right) == 2 and all(m(l1[q]) == [] for q in right)
    assert all(set(l2[q * 128:(q + 1) * 128]) == {None} for q in right)
    assert d.root(B1, 4, 2)[0][3] == 0
    # an afterstate with exactly one empty cell: two slots of the 32 of its move
    after = [s for a, s, _g in m(bytes(NEAR)) if a == 1][0]
    assert sum(c == 0 for c in after) == 1
    l1 = d.levels(NEAR, 1)[0]
    assert sum(b is not None for b in l1[32:64]) == 2 and sum(b is not None for b in l1) == 4
    # a one-tile root: 15 empty cells after either legal move, 30 slots each
    l1 = d.levels(ONE, 1)[0]
    assert [sum(b is not None for b in l1[32 * a:32 * a + 32]) for a in range(4)] == [0, 30, 0, 30]
    # a slot holds after(b, a) with the tile at `cell`
    s = R.slot(0, 1, 1, 5)
    assert l1[s][5] == 2 and l1[s][12] == 1 and sum(l1[s]) == 3
    # a tie between two moves goes to the smaller one
    for depth, top in ((4, 1), (4, 2), (5, 2)):
        v, a = d.root(A, depth, top)
        assert v[2] == v[3] > v[1] and a == 2


def test_the_no_overflow_bound_of_the_header():
    src = open(HEADER).read()
    assert 5 * 2 ** 41 + 2 ** 37 < 2 ** 44 and 160 * 2 ** 44 < 2 ** 52
    assert "5 * 2^41 + 2^37 < 2^44" in src and "160 * 2^44" in src and "2^52" in src
    assert R.MAX_EXPONENT + R.MAX_DEPTH == 27  # the largest bound a stage spec may hold


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _modules():
    import g2048._native as N
    from g2048 import (ntlambda, ntmean, ntmeantc, ntrestart, ntsearch, ntstage, nttc, ntuple,
                       search, stagemean, stagemeantc, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean, ntmeantc, stagemeantc)


def test_header_equals_exports_equals_signatures():
    from g2048 import deepsearch

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = deepsearch.load()
    assert set(names) == set(deepsearch.SIGNATURES)
    assert _exported(deepsearch.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other thirteen libraries keep their ABI: none of the new symbols
    for mod in _modules():
        mod.load()
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_deepsearch")]
        assert not set(names) & set(mod.SIGNATURES)
    assert deepsearch.MAX_DEPTH == R.MAX_DEPTH == 5
    assert (deepsearch.MAX_TOP, deepsearch.MAX_SUB) == (R.MAX_TOP, R.MAX_SUB) == (2, 3)
    for word in ("G2048_DEEPSEARCH_MAX_DEPTH 5", "G2048_DEEPSEARCH_MAX_EXPONENT 22",
                 "G2048_DEEPSEARCH_MAX_TOP_PLIES 2", "G2048_DEEPSEARCH_MAX_SUB_DEPTH 3"):
        assert word in src
    assert deepsearch.INT64_MIN == R.INT64_MIN == torch.iinfo(torch.int64).min


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import deepsearch

    out = subprocess.run(["readelf", "-d", deepsearch.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other thirteen stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash(), G.deepsearch_source_hash())


def test_build_keeps_the_new_files_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTSEARCH_SHARED, G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS,
                  G.NTSTAGE_SHARED, G.STAGESEARCH_SRCS, G.NTRESTART_SRCS, G.NTMEAN_SRCS,
                  G.NTMEAN_SHARED, G.STAGEMEAN_SRCS, G.NTMEANTC_SRCS, G.STAGEMEANTC_SRCS):
        assert set(G.DEEPSEARCH_SRCS).isdisjoint(other)
        assert set(G.STAGELEAF_SHARED).isdisjoint(other)
    for f in G.DEEPSEARCH_SRCS + G.STAGELEAF_SHARED:
        assert os.path.exists(os.path.join(G.CSRC, f))
    assert open(G.DEEPSEARCH_STAMP).read().strip() == G.deepsearch_source_hash()
    assert open(G.STAGESEARCH_STAMP).read().strip() == G.stagesearch_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert len(set(_hashes(G))) == 14


def test_both_sources_include_the_one_copy_of_the_staged_leaf():
    import __graft_entry__ as G

    shared = open(os.path.join(G.CSRC, G.STAGELEAF_SHARED[0])).read()
    assert "struct StagedLeaf {" in shared
    for src in G.STAGESEARCH_SRCS + G.DEEPSEARCH_SRCS:
        text = open(os.path.join(G.CSRC, src)).read()
        assert f'#include "{G.STAGELEAF_SHARED[0]}"' in text
        assert f'#include "{G.NTSEARCH_SHARED[0]}"' in text
        assert "struct StagedLeaf" not in text and "struct FlatLeaf" not in text


def test_stamps_follow_the_new_files(tmp_path, monkeypatch):
    """The new stamp follows its source, the four shared csrc headers and its public headers and
    nothing else; the new source moves no other stamp; the staged leaf's header moves the two
    libraries that search a staged table; and the main library's stamp has the same value in a
    tree without the new files."""
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

    def moved(now, last):
        return {k for k in range(14) if now[k] != last[k]}

    last = touch(os.path.join(copy, G.DEEPSEARCH_SRCS[0]))
    assert moved(last, before) == {13}
    for f, want in ((G.STAGELEAF_SHARED[0], {7, 13}), (G.NTSEARCH_SHARED[0], {3, 7, 13}),
                    (G.NTSTAGE_SHARED[0], {6, 7, 10, 12, 13}),
                    (G.STAGESEARCH_SRCS[0], {7}), (G.NTSEARCH_SRCS[0], {3}),
                    ("g2048_search.hip", {1}), ("g2048_qnet.hip", {0})):
        now = touch(os.path.join(copy, f))
        assert moved(now, last) == want, f
        last = now
    now = touch(os.path.join(copy, G.NTUPLE_SHARED[0]))
    assert 13 in moved(now, last) and not {0, 1, 8} & moved(now, last)
    last = now
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(root, "include"))
    monkeypatch.setattr(G, "ROOT", root)
    assert _hashes(G) == last
    for header, want in (("g2048_deepsearch.h", {13}), ("g2048_stagesearch.h", {7}),
                         ("g2048_ntsearch.h", {3})):
        now = touch(os.path.join(root, "include", header))
        assert moved(now, last) == want, header
        last = now
    for header in ("g2048_ntstage.h", "g2048_ntuple.h", "g2048.h"):
        now = touch(os.path.join(root, "include", header))
        assert 13 in moved(now, last), header
        last = now
    # a tree without the fourteenth library and the staged leaf's header: the main stamp and
    # those of the libraries that include neither keep their values
    bare, bare_root = str(tmp_path / "bare"), str(tmp_path / "bare_root")
    shutil.copytree(real_csrc, bare)
    for f in G.DEEPSEARCH_SRCS + G.STAGELEAF_SHARED:
        os.remove(os.path.join(bare, f))
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(bare_root, "include"))
    os.remove(os.path.join(bare_root, "include", "g2048_deepsearch.h"))
    monkeypatch.setattr(G, "CSRC", bare)
    monkeypatch.setattr(G, "ROOT", bare_root)
    assert (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash()) == before[:7]
    assert (G.ntrestart_source_hash(), G.ntmean_source_hash(), G.stagemean_source_hash(),
            G.ntmeantc_source_hash(), G.stagemeantc_source_hash()) == before[8:13]
    for missing in (G.stagesearch_source_hash, G.deepsearch_source_hash):
        with pytest.raises(FileNotFoundError):
            missing()


def test_kernels_have_no_store_data_hazard_and_no_scratch(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's flags,
    as the other libraries' tests audit theirs; and none of the kernels uses scratch: expand,
    two backups, and per leaf three sub-searches and the three k_search of top_plies = 0."""
    import sys

    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.DEEPSEARCH_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", open(out).read())
        assert len(sizes) == 1 + 2 + 2 * (3 + 3) and set(sizes) == {"0"}


def test_workspace_bytes_follows_its_formula_and_refuses():
    import g2048._native as N
    from g2048 import deepsearch

    lib = deepsearch.load()
    for n in (1, 2, 129, 677, 65536, N.MAX_BOARDS):
        assert deepsearch.workspace_bytes(n, 0) == R.workspace_bytes(n, 0) == 0
        assert deepsearch.workspace_bytes(n, 1) == R.workspace_bytes(n, 1) == 3072 * n
        assert deepsearch.workspace_bytes(n, 2) == R.workspace_bytes(n, 2) == 396288 * n
    assert 396288 == (128 + 16384) * 24
    for n, top, word in ((0, 1, b"n ="), (-1, 0, b"n ="), (N.MAX_BOARDS + 1, 2, b"n ="),
                         (4, -1, b"top_plies"), (4, 3, b"top_plies")):
        assert lib.g2048_deepsearch_workspace_bytes(n, top) == N.G2048_EINVAL
        assert word in lib.g2048_deepsearch_last_error()
        with pytest.raises(ValueError):
            deepsearch.workspace_bytes(n, top)


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


def _call(lib, entry, spec=UNGIVEN, stages=UNGIVEN, lut=FAKE, boards=FAKE, n=4, depth=4, top=2,
          flags=0, values=FAKE, action=FAKE, ws=FAKE, ws_bytes=None):
    spec = _spec(NR.TUPLES_2x4) if spec is UNGIVEN else spec
    stages = _stages((5, 8)) if stages is UNGIVEN else stages
    if ws_bytes is None:
        ws_bytes = R.workspace_bytes(max(n, 1), top) if top in (0, 1, 2) else 0
    tail = (lut, boards, n, depth, top, flags, values, action, ws, ws_bytes, 0, None)
    sp = C.byref(spec) if spec is not None else None
    if entry == "flat":
        return lib.g2048_deepsearch_expectimax(sp, *tail)
    return lib.g2048_deepsearch_staged_expectimax(
        sp, C.byref(stages) if stages is not None else None, *tail)


@pytest.mark.parametrize("entry", ["flat", "staged"])
def test_bad_arguments_are_refused_without_a_gpu(entry):
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import deepsearch

    lib = deepsearch.load()
    err = lib.g2048_deepsearch_last_error
    who = b"deepsearch_expectimax" if entry == "flat" else b"deepsearch_staged_expectimax"
    cases = [(dict(spec=None), b"spec"), (dict(lut=None), b"NULL"), (dict(boards=None), b"NULL"),
             (dict(spec=_spec(((0,),), n_tuples=9)), b"n_tuples"),
             (dict(spec=_spec(((0, 1), (2, 16)))), b"not a board cell"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(lut=FAKE + 2), b"aligned"), (dict(boards=FAKE + 4), b"aligned"),
             (dict(depth=0, top=0), b"depth"), (dict(depth=6, top=2), b"depth"),
             (dict(depth=-1, top=0), b"depth"),
             (dict(top=-1), b"top_plies"), (dict(top=3), b"top_plies"),
             # sub = depth - top_plies outside 1..3
             (dict(depth=4, top=0), b"sub"), (dict(depth=5, top=1), b"sub"),
             (dict(depth=5, top=0), b"sub"), (dict(depth=2, top=2), b"sub"),
             (dict(depth=1, top=1), b"sub"), (dict(depth=1, top=2), b"sub"),
             (dict(flags=N.EGREEDY_FIXED), b"flags"), (dict(flags=8), b"flags"),
             (dict(flags=N.P4_10 | 8), b"flags"),
             (dict(values=None, action=None), b"NULL"), (dict(values=FAKE + 4), b"aligned"),
             (dict(ws=None), b"workspace_dev is NULL"), (dict(ws=FAKE + 8), b"16-byte aligned"),
             (dict(ws_bytes=R.workspace_bytes(4, 2) - 1), b"smaller"),
             (dict(top=1, ws_bytes=R.workspace_bytes(4, 1) - 1), b"smaller"),
             (dict(top=1, ws_bytes=0), b"smaller"), (dict(ws_bytes=-1), b"smaller")]
    if entry == "staged":
        cases += [(dict(stages=None), b"stages"), (dict(stages=_stages((5, 5))), b"increasing"),
                  (dict(stages=_stages((28,))), b"outside [1, 27]")]
    for kw, word in cases:
        assert _call(lib, entry, **kw) == N.G2048_EINVAL, kw
        assert word in err(), (kw, err())
        assert who in err()


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import deepsearch, ntsearch, ntstage, ntuple, stagesearch

    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    for x in (plain, net):
        with pytest.raises(g2048.NativeError):  # a network on the CPU: there is no CPU path
            deepsearch.expectimax(x, boards, 4)
        with pytest.raises(g2048.NativeError):
            x.deep_search(boards, depth=5)
        with pytest.raises(ValueError, match="p4"):
            deepsearch.expectimax(x, boards, 4, p4=0.3)
        for depth in (0, 6):
            with pytest.raises(ValueError, match="depth"):
                x.deep_search(boards, depth=depth)
        for depth, top in ((4, 0), (5, 1), (1, 1), (2, 2), (3, 3), (3, -1)):
            with pytest.raises(ValueError, match="top"):
                deepsearch.expectimax(x, boards, depth, top=top)
    for other in (None, plain.lut, "net"):
        with pytest.raises(TypeError, match="NTupleNetwork"):
            deepsearch.expectimax(other, boards, 4)
    # the existing searches keep their depth
    assert ntsearch.MAX_DEPTH == stagesearch.MAX_DEPTH == 3
    with pytest.raises(ValueError, match="depth"):
        plain.search(boards, depth=4)
    with pytest.raises(ValueError, match="depth"):
        net.expectimax(boards, depth=4)
    assert g2048.deepsearch is deepsearch and "deepsearch" in g2048.__all__
    assert deepsearch.LIB_PATH.endswith("libg2048_deepsearch.so")


def test_chunking_and_default_top():
    from g2048 import deepsearch as D

    assert [D.legal_tops(d) for d in range(1, 6)] == [(0,), (0, 1), (0, 1, 2), (1, 2), (2,)]
    assert D.legal_tops(4) == R.legal_tops(4)
    cap = D.WORKSPACE_CAP
    assert D.chunk_boards(1) == cap // 3072 and D.chunk_boards(2) == cap // 396288 == 677
    assert D.chunks(5, 2) == [(0, 5)] and D.chunks(677, 2) == [(0, 677)]
    assert D.chunks(678, 2) == [(0, 677), (677, 678)]
    assert D.chunks(1031, 2, cap=3 * 396288 + 5) == [(i, min(i + 3, 1031))
                                                    for i in range(0, 1031, 3)]
    assert D.chunks(7, 1, cap=1) == [(i, i + 1) for i in range(7)]  # never less than one board
    assert D.chunks(1 << 20, 0) == [(0, 1 << 20)]                   # top 0 has no workspace
    for lo, hi in D.chunks(100000, 1):
        assert D.workspace_bytes(hi - lo, 1) <= cap
    for depth in range(1, 6):
        for n in (1, 2, 15, 16, 17, 255, 256, 4095, 4096, 65536, 1 << 20):
            assert D.default_top(depth, n) in D.legal_tops(depth)
    with pytest.raises(ValueError):
        D.default_top(6, 4)
    with pytest.raises(ValueError):
        D.default_top(3, 0)


def test_player_checks_the_deep_policies_arguments():
    import g2048
    from g2048 import ntstage, ntuple, player

    staged_net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (7,), device="cpu")
    plain = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for policy in ("ntuple_deep", "ntstage_deep"):
        with pytest.raises(ValueError, match="network"):
            player.BatchedPlayer(4).play(policy)
    with pytest.raises(TypeError, match="StagedNTupleNetwork"):
        player.BatchedPlayer(4, ntuple=plain).play("ntstage_deep")
    with pytest.raises(TypeError, match="NTupleNetwork"):
        player.BatchedPlayer(4, ntuple=staged_net).play("ntuple_deep")
    # the constructor's bound stays: the player reaches depth 4, the module function 5
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=plain, search_depth=5)
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=plain, search_depth=4).play("ntuple_search")
    with pytest.raises(ValueError, match="search_depth"):
        player.BatchedPlayer(4, ntuple=staged_net, search_depth=4).play("ntstage_search")
    with pytest.raises(ValueError, match="ntuple_deep"):  # the message lists the new policies
        player.BatchedPlayer(4).play("minimax")
    if not torch.cuda.is_available():
        # depth 4 passes the deep policies' checks and stops only at the missing GPU
        with pytest.raises(g2048.NativeError):
            player.BatchedPlayer(4, ntuple=plain, search_depth=4).play("ntuple_deep")
