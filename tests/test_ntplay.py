"""The on-device n-tuple player (include/g2048_ntplay.h, csrc/g2048_ntplay.hip ->
libg2048_ntplay.so) without a GPU: the closed form of a terminal board against the stepwise rule
(tests/ntplay_ref.py) on hand-made cases, and the library's boundary -- its header, exports and
signatures, its stamp, every refused argument of both entry points and of the Python wrapper,
and the kernels' resource usage from the build's metadata."""
import ctypes as C
import os
import re
import subprocess
import types

import numpy as np
import pytest
import torch

import ntplay_ref as R
import ntsearch_ref as S
import ntuple_ref as NR
import stagesearch_ref as SSR
from g2048 import ntplay as _library  # noqa: F401  (every test of this file needs the library)
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntplay.h")
NAMES = ["g2048_ntplay_last_error", "g2048_ntplay_staged_steps", "g2048_ntplay_steps"]
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
NEAR = CHECKER[:15] + [0]  # one empty cell: most of its moves end the game
KEYS = ("board", "meta", "ep", "clock", "fin", "result")


def table(seed, tuples=NR.TUPLES_2x4):
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 20), 1 << 20, (len(tuples), 16 ** len(tuples[0])))


def search(seed=3, p4=0.5):
    return S.Search(NR.Net(NR.TUPLES_2x4, base=table(seed)), p4)


def same(a, b, what=""):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), (what, k, a[k], b[k])


def pair(n, flags, setup, **kw):
    """Two players in the same state: one takes the closed form, one steps every move."""
    out = []
    for _ in range(2):
        p = R.Play(search(), n, flags=flags, **kw)
        setup(p)
        out.append(p)
    return out


def game(flags=O.NO_AUTORESET, seed=0x2048, depth=1):
    """One game from the deal to its terminal board: [(board, score, moves)] before every move,
    the terminal board last."""
    p = R.Play(search(), 1, seed=seed, flags=flags)
    e, out = p.envs[0], []
    while True:
        out.append((e.board[0].copy(), int(e.meta[0, 0]), int(e.meta[0, 1])))
        if O.legal_mask(e.board[0]) == 0:
            return out
        p.steps(1, depth)


# ------------------------------------------------------------------ the closed form
def test_terminal_tail_by_hand():
    """A terminal board with 7 finished episodes, score 100, 30 moves made: the next step ends
    episode 8 at 31 moves; 5 steps leave 12 episodes and 35 moves.  The words wrap at 2^32."""
    ep, first = R.terminal_tail([7, 1, 2, 3], 100, 30, 9, 5)
    assert first == (8, 100, 31, 9) and ep == (12, 100, 35, 9)
    ep, first = R.terminal_tail([R.M32, 0, 0, 0], 5, R.M32 - 1, 4, 3)
    assert first == (0, 5, R.M32, 4) and ep == (2, 5, 1, 4)


@pytest.mark.parametrize("K", [1, 2, 7, 33])
def test_a_board_terminal_on_entry(K):
    def setup(p):
        p.set_board(0, CHECKER, score=1234, moves=77)
        p.set_clock(500)

    a, b = pair(1, O.NO_AUTORESET, setup)
    a.steps(K, 1, closed=True)
    b.steps(K, 1, closed=False)
    same(a.state(), b.state())
    st = a.state()
    assert st["ep"][0].tolist() == [K, 1234, 77 + K, 2] and st["clock"][0] == 500 + K
    assert st["result"][0].tolist() == [1, 1234, 78, 2] and st["fin"][0] == 1
    assert st["meta"][:, 0].tolist() == [1234, 500 - 77]  # score and start as they were
    assert st["board"][0].tolist() == CHECKER


def test_a_window_whose_terminal_step_is_its_first_second_and_last_move():
    """A recorded game: a window of K moves that starts j boards before the terminal one ends the
    episode at its move j + 1, for j = 0 (terminal on entry), 1, K - 2 and K - 1."""
    g = game()
    assert len(g) > 12
    K, end = 9, len(g) - 1
    for j in (0, 1, K - 2, K - 1):
        board, score, moves = g[end - j]

        def setup(p):
            p.set_board(0, board, score, moves)
            p.set_clock(moves)

        a, b = pair(1, O.NO_AUTORESET, setup)
        a.steps(K, 1, closed=True)
        b.steps(K, 1, closed=False)
        same(a.state(), b.state(), j)
        st = a.state()
        assert st["board"][0].tolist() == g[end][0].tolist(), j
        assert st["result"][0].tolist() == [1, g[end][1], end + 1, int(g[end][0].max())], j
        assert st["ep"][0].tolist() == [K - j, g[end][1], moves + K, int(g[end][0].max())], j


def test_an_autoreset_board_is_dealt_again_inside_the_window_and_plays_on():
    """With auto-reset the closed form never applies: both players re-deal the board at the
    terminal step and play the new game; the latch keeps the first game's row."""
    g = game(flags=0)
    end, K = len(g) - 1, 12
    board, score, moves = g[end - 4]

    def setup(p):
        p.set_board(0, board, score, moves)
        p.set_clock(moves)

    a, b = pair(1, 0, setup)
    a.steps(K, 1, closed=True)
    b.steps(K, 1, closed=False)
    same(a.state(), b.state())
    st = a.state()
    assert st["ep"][0].tolist() == [1, g[end][1], end + 1, int(g[end][0].max())]
    assert st["result"][0].tolist() == st["ep"][0].tolist() and st["fin"][0] == 1
    assert st["meta"][1, 0] == end + 1            # the new game began after the terminal step
    assert 0 < np.count_nonzero(st["board"][0]) <= 2 + (K - 5)
    assert st["clock"][0] == moves + K


def test_a_row_with_fin_set_keeps_its_result():
    def setup(p):
        p.set_board(0, CHECKER, 10, 5)
        p.set_board(1, CHECKER, 20, 6)
        p.set_clock(40)
        p.fin[1] = 1
        p.result[1] = (9, 9, 9, 9)

    a, b = pair(2, O.NO_AUTORESET, setup)
    a.steps(4, 1, closed=True)
    b.steps(4, 1, closed=False)
    same(a.state(), b.state())
    st = a.state()
    assert st["result"].tolist() == [[1, 10, 6, 2], [9, 9, 9, 9]] and st["fin"].tolist() == [1, 1]
    assert st["ep"].tolist() == [[4, 10, 9, 2], [4, 20, 10, 2]]


@pytest.mark.parametrize("flags", [O.NO_AUTORESET, 0])
def test_a_clock_window_that_crosses_2_to_the_32(flags):
    """The clock is 64 bits wide, start and moves 32: a window from 2^32 - 3 over a terminal
    board, a board about to end and a live one."""
    t0 = (1 << 32) - 3
    live = [1, 1] + [0] * 14

    def setup(p):
        p.set_board(0, CHECKER, 7, 100)
        p.set_board(1, NEAR, 3, 50)
        p.set_board(2, live, 0, 0)
        p.set_clock(t0)

    a, b = pair(3, flags, setup)
    a.steps(7, 1, closed=True)
    b.steps(7, 1, closed=False)
    same(a.state(), b.state())
    st = a.state()
    assert st["clock"][0] == t0 + 7 and st["clock"][0] > 1 << 32
    assert st["result"][0].tolist() == [1, 7, 101, 2]
    if flags:
        assert st["ep"][0].tolist() == [7, 7, 107, 2]
        assert st["meta"][1, 0] == (t0 - 100) & R.M32
    else:
        assert st["meta"][1, 0] == (t0 + 1) & R.M32   # dealt again after the first step


def test_depth_2_and_the_staged_table_go_through_the_same_player():
    """The player reads its network only through Search.root: a staged search plays as well."""
    base = np.stack([table(5), table(6)])
    base[1][base[1] % 2 == 0] = -(1 << 31)  # half of stage 1 UNSET
    s = SSR.staged_search(NR.TUPLES_2x4, (3,), base)
    a, b = R.Play(s, 2, flags=O.NO_AUTORESET), R.Play(s, 2, flags=O.NO_AUTORESET)
    for p in (a, b):
        p.set_board(1, NEAR, 0, 0)
    a.steps(6, 2, closed=True)
    b.steps(6, 2, closed=False)
    same(a.state(), b.state())
    with pytest.raises(ValueError):
        a.steps(0)
    with pytest.raises(ValueError):
        a.steps(1, 4)
    with pytest.raises(ValueError):
        a.steps((1 << 20) + 1)


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import (deepsearch, ntlambda, ntmean, ntmeantc, ntrestart, ntsearch, ntstage, nttc,
                       ntuple, search, stageback, stagedelay, stagemean, stagemeantc, stagesearch)

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch, ntrestart, ntmean,
            stagemean, ntmeantc, stagemeantc, deepsearch, stagedelay, stageback)


def test_header_equals_exports_equals_signatures():
    from g2048 import ntplay

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntplay.load()
    assert set(names) == set(ntplay.SIGNATURES)
    assert _exported(ntplay.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    flat = re.search(r"g2048_ntplay_steps\((.*?)\);", src, re.S).group(1)
    staged = re.search(r"g2048_ntplay_staged_steps\((.*?)\);", src, re.S).group(1)
    assert len(flat.split(",")) == len(ntplay.SIGNATURES["g2048_ntplay_steps"][1]) == 16
    assert len(staged.split(",")) == len(ntplay.SIGNATURES["g2048_ntplay_staged_steps"][1]) == 17
    args = [a.split()[-1].lstrip("*") for a in flat.split(",")]
    sargs = [a.split()[-1].lstrip("*") for a in staged.split(",")]
    assert sargs == args[:1] + ["stages"] + args[1:]
    for name, value in (("MAX_DEPTH", "3"), ("MAX_STEPS", "(1 << 20)")):
        assert f"#define G2048_NTPLAY_{name} {value}" in src
        assert getattr(ntplay, name) == eval(value)
    # the other sixteen libraries keep their ABI: none of the new symbols
    assert len(_others()) == 16
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_ntplay")]
        assert not set(names) & set(mod.SIGNATURES)


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntplay

    out = subprocess.run(["readelf", "-d", ntplay.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def _hashes(G):
    """The other sixteen stamps, then the new one."""
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash(),
            G.ntmean_source_hash(), G.stagemean_source_hash(), G.ntmeantc_source_hash(),
            G.stagemeantc_source_hash(), G.deepsearch_source_hash(), G.stagedelay_source_hash(),
            G.stageback_source_hash(), G.ntplay_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTSEARCH_SHARED, G.NTTC_SRCS, G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS,
                  G.NTSTAGE_SHARED, G.STAGESEARCH_SRCS, G.STAGELEAF_SHARED, G.NTRESTART_SRCS,
                  G.NTMEAN_SRCS, G.NTMEAN_SHARED, G.STAGEMEAN_SRCS, G.NTMEANTC_SRCS,
                  G.STAGEMEANTC_SRCS, G.DEEPSEARCH_SRCS, G.STAGEDELAY_SRCS, G.STAGEBACK_SRCS):
        assert set(G.NTPLAY_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTPLAY_SRCS[0]))
    assert open(G.NTPLAY_STAMP).read().strip() == G.ntplay_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert open(G.DEEPSEARCH_STAMP).read().strip() == G.deepsearch_source_hash()
    assert len(set(_hashes(G))) == 17


def test_stamp_follows_its_source_the_shared_headers_and_the_four_public_headers(tmp_path,
                                                                                 monkeypatch):
    """A change to the new source changes only the new stamp (source_hash() lists the file among
    the sources with stamps of their own); a change to each csrc header it includes changes the
    new stamp and the deep search's, which includes the same ones; a change to each of g2048.h,
    g2048_ntuple.h, g2048_ntstage.h and g2048_ntplay.h changes the new stamp, the last one no
    other."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.NTPLAY_SRCS[0])).read()
    includes = re.findall(r'#include\s+"([^"]+)"', src)
    assert includes == ["../../include/g2048_ntplay.h", "g2048_board.hpp", G.NTUPLE_SHARED[0],
                        G.NTSTAGE_SHARED[0], G.NTSEARCH_SHARED[0], G.STAGELEAF_SHARED[0]]
    before = _hashes(G)
    copy = str(tmp_path / "csrc")
    shutil.copytree(G.CSRC, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTPLAY_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:16] == before[:16] and after[16] != before[16]
    last = after
    for shared in (G.STAGELEAF_SHARED[0], G.NTSEARCH_SHARED[0], G.NTSTAGE_SHARED[0],
                   G.NTUPLE_SHARED[0], "g2048_board.hpp"):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
        now = _hashes(G)
        assert now[16] != last[16] and now[13] != last[13], shared  # the fourteenth follows too
        if shared != "g2048_board.hpp":  # that one the main library includes too
            assert now[0] == before[0]
        last = now
    shared, include = last, os.path.join(G.ROOT, "include")
    for k, header in enumerate(("g2048.h", "g2048_ntuple.h", "g2048_ntstage.h",
                                "g2048_ntplay.h")):
        root = str(tmp_path / f"root{k}")
        shutil.copytree(include, os.path.join(root, "include"))
        with open(os.path.join(root, "include", header), "a") as f:
            f.write("/* changed */\n")
        monkeypatch.setattr(G, "ROOT", root)
        now = _hashes(G)
        assert now[16] != shared[16] and now[16] != last[16], header
        if header == "g2048_ntplay.h":
            assert now[:16] == shared[:16]
        last = now


def test_kernels_use_no_scratch_and_no_lds(tmp_path):
    """The library's source compiled with the library's flags: seven kernels (k_play at depths
    1..3 for the flat and the staged leaf, k_tick), none with scratch, LDS or a spilled VGPR
    (the figures of this build are recorded in profiles/ntplay/resource_usage.txt)."""
    import __graft_entry__ as G

    for f in G.NTPLAY_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
        for key in ("private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count"):
            sizes = re.findall(rf"\.{key}:\s*(\d+)", text)
            assert len(sizes) == 7 and set(sizes) == {"0"}, key
        assert len(re.findall(r"\.name:\s+\S*k_play", text)) == 6
        assert len(re.findall(r"\.name:\s+\S*k_tick", text)) == 1
    assert os.path.exists(os.path.join(ROOT, "profiles", "ntplay", "resource_usage.txt"))


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


FAKE = 1 << 20  # an aligned address that stands in for device memory


def _flat(lib, spec, stages=None, lut=FAKE, board=FAKE, meta=FAKE, ep=FAKE, clock=FAKE, n=4,
          seed=1, offset=0, flags=0, k=3, depth=1, fin=FAKE, result=FAKE):
    return lib.g2048_ntplay_steps(C.byref(spec) if spec is not None else None, lut, board, meta,
                                  ep, clock, n, seed, offset, flags, k, depth, fin, result,
                                  1 << 20, None)


def _staged(lib, spec, stages, lut=FAKE, board=FAKE, meta=FAKE, ep=FAKE, clock=FAKE, n=4, seed=1,
            offset=0, flags=0, k=3, depth=1, fin=FAKE, result=FAKE):
    return lib.g2048_ntplay_staged_steps(C.byref(spec) if spec is not None else None,
                                         C.byref(stages) if stages is not None else None, lut,
                                         board, meta, ep, clock, n, seed, offset, flags, k, depth,
                                         fin, result, 1 << 20, None)


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
    (dict(bounds=(1, 2, 3, 4, 5, 6, 7), n_stages=9), b"n_stages"),
    (dict(bounds=(0,)), b"outside [1, 27]"),
    (dict(bounds=(28,)), b"outside [1, 27]"),
    (dict(bounds=(5, 5)), b"strictly increasing"),
    (dict(bounds=(8, 5)), b"strictly increasing"),
    (dict(bounds=(5, 8), n_stages=2), b"unused bound"),
]


@pytest.mark.parametrize("kw,word", BAD_SPECS)
def test_bad_specs_are_refused_by_both_entry_points(kw, word):
    import g2048._native as N
    from g2048 import ntplay

    lib, s, st = ntplay.load(), _spec(**kw), _stages((5, 8))
    for call in (lambda: _flat(lib, s), lambda: _staged(lib, s, st)):
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_ntplay_last_error()


@pytest.mark.parametrize("kw,word", BAD_STAGES)
def test_bad_stage_specs_are_refused(kw, word):
    import g2048._native as N
    from g2048 import ntplay

    lib = ntplay.load()
    assert _staged(lib, _spec(NR.TUPLES_2x4), _stages(**kw)) == N.G2048_EINVAL
    msg = lib.g2048_ntplay_last_error()
    assert word in msg and b"ntplay_staged_steps" in msg


def test_bad_arguments_are_refused_before_any_device_work():
    """Argument checks run before any device work: G2048_EINVAL with a message, on a machine
    without a GPU, for a device id that does not exist.  The pointers are never dereferenced (fake
    aligned addresses stand in for device memory)."""
    import g2048._native as N
    from g2048 import ntplay

    lib = ntplay.load()
    s, st = _spec(NR.TUPLES_2x4), _stages((5, 8))
    cases = [(dict(spec=None), b"spec"), (dict(lut=None), b"NULL"), (dict(lut=FAKE + 2), b"aligned"),
             (dict(board=None), b"NULL"), (dict(board=FAKE + 4), b"aligned"),
             (dict(meta=None), b"meta_dev is NULL"), (dict(meta=FAKE + 2), b"meta_dev must be"),
             (dict(ep=None), b"ep_dev is NULL"), (dict(ep=FAKE + 8), b"ep_dev must be 16-byte"),
             (dict(clock=None), b"clock_dev is NULL"),
             (dict(clock=FAKE + 4), b"clock_dev must be 8-byte"),
             (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
             (dict(flags=8), b"env_flags"), (dict(flags=1 << 31), b"env_flags"),
             (dict(k=0), b"k_steps"), (dict(k=-1), b"k_steps"), (dict(k=(1 << 20) + 1), b"k_steps"),
             (dict(depth=0), b"depth"), (dict(depth=4), b"depth"), (dict(depth=-1), b"depth"),
             (dict(fin=None), b"together"), (dict(result=None), b"together"),
             (dict(result=FAKE + 8), b"result_dev must be 16-byte")]
    for call, who in ((_flat, b"ntplay_steps"), (_staged, b"ntplay_staged_steps")):
        for kw, word in cases:
            assert call(lib, **{"spec": s, "stages": st, **kw}) == N.G2048_EINVAL, kw
            msg = lib.g2048_ntplay_last_error()
            assert word in msg and who in msg, (kw, msg)
        # the edges of the domain pass the checks and fail only at the device that does not exist
        for kw in (dict(k=1), dict(k=1 << 20), dict(depth=3), dict(n=1), dict(n=N.MAX_BOARDS),
                   dict(flags=7), dict(fin=None, result=None), dict(fin=FAKE + 1),
                   dict(seed=(1 << 64) - 1, offset=(1 << 64) - 1)):
            assert call(lib, s, st, **kw) != N.G2048_EINVAL, kw
    assert _staged(lib, s, None) == N.G2048_EINVAL
    assert b"stages" in lib.g2048_ntplay_last_error()


# ------------------------------------------------------------------ the Python side
def _fake_env(n=4, **kw):
    env = types.SimpleNamespace(
        n=n, seed=1, board_offset=0, flags=4, episode_log=None,
        board=torch.zeros((n, 16), dtype=torch.uint8), meta=torch.zeros((2, n), dtype=torch.int32),
        ep=torch.zeros((n, 4), dtype=torch.int32),
        clock=torch.zeros(((n + 63) // 64,), dtype=torch.int64))
    for k, v in kw.items():
        setattr(env, k, v)
    return env


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntplay, ntstage, ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    staged = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5, 8), device="cpu")
    env = _fake_env()
    fin, result = torch.zeros(4, dtype=torch.uint8), torch.zeros((4, 4), dtype=torch.int32)
    for bad in (None, "net", torch.zeros(3)):
        with pytest.raises(TypeError, match="NTupleNetwork"):
            ntplay.steps(bad, env, 1)
    for kw in (dict(k=0), dict(k=-1), dict(k=(1 << 20) + 1), dict(depth=0), dict(depth=4),
               dict(fin=fin), dict(result=result)):
        with pytest.raises(ValueError):
            ntplay.steps(net, env, **{"k": 1, **kw})
    with pytest.raises(TypeError, match="VecEnv2048"):
        ntplay.steps(net, object(), 1)
    with pytest.raises(ValueError, match="episode log"):
        ntplay.steps(net, _fake_env(episode_log=object()), 1)
    for n_ in (net, staged):  # a network on the CPU: there is no CPU path
        with pytest.raises(g2048.NativeError):
            ntplay.steps(n_, env, 1)
        with pytest.raises(g2048.NativeError):
            n_.play_steps(env, 1, depth=2, fin=fin, result=result)
    # the buffers are checked against the env's n before anything is launched
    dev = torch.device("cpu")
    ntplay._buffer(env.meta, "env.meta", torch.int32, (2, 4), dev)
    for t, dt, shape in ((env.meta, torch.int32, (2, 5)), (env.meta, torch.int64, (2, 4)),
                         (env.ep.t(), torch.int32, (4, 4)), (fin, torch.uint8, (5,))):
        with pytest.raises(ValueError):
            ntplay._buffer(t, "x", dt, shape, dev)
    with pytest.raises(ValueError):
        ntplay._buffer(env.meta, "x", torch.int32, (2, 4), torch.device("meta"))
    with pytest.raises(TypeError):
        ntplay._buffer(None, "x", torch.int32, (2, 4), dev)
    assert g2048.ntplay is ntplay and "ntplay" in g2048.__all__


def test_the_player_knows_the_fused_policies():
    """Class, depth and record_games checks of the two new policies, before any env is made;
    the unknown-policy message names every policy, old and new."""
    from g2048 import ntstage, ntuple
    from g2048.player import BatchedPlayer

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    staged = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, (5,), device="cpu")
    for policy, good, bad in (("ntuple_fused", net, staged), ("ntstage_fused", staged, net)):
        with pytest.raises(ValueError, match="needs a network"):
            BatchedPlayer(4, device="cpu").play(policy)
        with pytest.raises(TypeError, match="takes a"):
            BatchedPlayer(4, device="cpu", ntuple=bad).play(policy)
        with pytest.raises(ValueError, match="1..3"):
            BatchedPlayer(4, device="cpu", ntuple=good, search_depth=4).play(policy)
        with pytest.raises(ValueError, match="record_games"):
            BatchedPlayer(4, device="cpu", ntuple=good, record_games=1).play(policy)
    with pytest.raises(ValueError) as e:
        BatchedPlayer(4, device="cpu").play("nope")
    for name in ("random", "upleft", "greedy", "expectimax", "ntuple", "ntuple_search",
                 "ntstage_search", "ntuple_deep", "ntstage_deep", "ntuple_fused",
                 "ntstage_fused"):
        assert f"'{name}'" in str(e.value)
