"""CPU-side checks of the per-board restart pool: the Python restatement (tests/ntrestart_ref.py)
reproduces its hand-computed anchors; and the boundary of libg2048_ntrestart.so (header == exports
== SIGNATURES, build stamps, argument validation without a GPU, the Python side's refusals,
save / load)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ntrestart_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntrestart.h")
NAMES = ["g2048_ntrestart_apply", "g2048_ntrestart_last_error", "g2048_ntrestart_state_bytes"]

B2 = [1, 2] + [0] * 14
B2X = [2, 2, 1] + [0] * 13
B3 = [3, 1] + [0] * 14
B4 = [4] + [0] * 15
FRESH = [1, 0, 0, 1] + [0] * 12
WRAP = (1 << 32) + 2


# ------------------------------------------------------------------ the reference's anchors
def climbed():
    """The state after the docstring's capture, no re-capture and climb, checked on the way."""
    st = R.fresh(1)
    assert st == {"snap": [{}], "valid": [0], "top": [0], "turn": [0]}
    st, board, meta, back = R.apply((0, 3), st, [B2], [[4], [10]], [13], [0])
    assert st == {"snap": [{2: (tuple(B2), 4, 3)}], "valid": [0b100], "top": [2], "turn": [0]}
    assert (board, meta, back) == ([B2], [[4], [10]], [0])  # slot 1 stays unset
    again, board, meta, back = R.apply((0, 3), st, [B2X], [[8], [10]], [14], [0])
    assert again == st and (board, meta, back) == ([B2X], [[8], [10]], [0])
    st, board, meta, back = R.apply((0, 3), st, [B3], [[12], [10]], [15], [0])
    assert st == {"snap": [{2: (tuple(B2), 4, 3), 3: (tuple(B3), 12, 5)}], "valid": [0b1100],
                  "top": [3], "turn": [0]}
    assert (board, meta, back) == ([B3], [[12], [10]], [0])
    return st


def test_worked_capture_at_every_crossing_and_no_recapture():
    climbed()


def test_worked_restore_folds_the_moves_into_a_start_that_wraps():
    st = climbed() | {"turn": [1]}
    new, board, meta, back = R.apply((0, 3), st, [FRESH], [[0], [2]], [WRAP], [1])
    assert board == [B3] and meta == [[12], [4294967293]] and back == [3]
    assert (2 - meta[1][0]) % (1 << 32) == 5  # the env's moves = now - start
    assert new == st | {"turn": [2]}  # top was 3 already, the slot is kept
    assert st["turn"] == [1]  # apply is pure


def test_worked_unset_level_falls_back_and_still_advances_turn():
    st = climbed() | {"turn": [1]}
    new, board, meta, back = R.apply((0, 7), st, [FRESH], [[0], [2]], [WRAP], [1])
    assert (board, meta, back) == ([FRESH], [[0], [2]], [0])
    assert new == st | {"turn": [2], "top": [1]}
    st = climbed()
    new, board, meta, back = R.apply((0, 3), st, [FRESH], [[0], [2]], [WRAP], [1])  # e = 0
    assert (board, meta, back) == ([FRESH], [[0], [2]], [0])
    assert new == st | {"turn": [1], "top": [1]}


def test_worked_rotation_of_one_fresh_level_changes_only_top_and_turn():
    st = climbed() | {"turn": [4294967295]}
    new, board, meta, back = R.apply((0,), st, [B2], [[0], [2]], [WRAP], [1])
    assert (board, meta, back) == ([B2], [[0], [2]], [0])
    assert new == st | {"turn": [0], "top": [2]}  # turn counts modulo 2^32


def test_worked_restore_then_climb_overwrites_the_higher_slot():
    st = climbed() | {"turn": [1]}
    st["snap"][0][4] = (tuple(B4[::-1]), 99, 40)
    st["valid"] = [0b11100]
    st, board, meta, back = R.apply((0, 3), st, [FRESH], [[0], [2]], [WRAP], [1])
    assert board == [B3] and st["top"] == [3]
    st, board, meta, back = R.apply((0, 3), st, [B4], [[28], meta[1]], [WRAP + 2], [0])
    assert st["snap"][0][4] == (tuple(B4), 28, 7) and st["snap"][0][3] == (tuple(B3), 12, 5)
    assert st["valid"] == [0b11100] and st["top"] == [4] and back == [0]
    assert (board, meta) == ([B4], [[28], [4294967293]])


def test_out_of_domain_board_is_never_captured_and_bad_rotations_are_refused():
    st, *_ = R.apply((0,), R.fresh(1), [[16, 1] + [0] * 14], [[0], [0]], [5], [0])
    assert st == R.fresh(1)
    st, *_ = R.apply((0,), R.fresh(1), [[15, 1] + [0] * 14], [[7], [1]], [5], [0])
    assert st["snap"] == [{15: ((15, 1) + (0,) * 14, 7, 4)}] and st["valid"] == [1 << 15]
    for bad in ((), (16,), (0, -1), tuple(range(9))):
        with pytest.raises(ValueError):
            R.check_levels(bad)
    assert R.check_levels(range(8)) == tuple(range(8))


def test_stagger_and_the_group_clock():
    """Board 64 reads clock word 1; staggered boards sit at different turns."""
    st = R.fresh(65, stagger=True)
    assert st["turn"] == list(range(65))
    boards = [list(B3) for _ in range(65)]
    st, *_ = R.apply((0, 3), st, boards, [[0] * 65, [0] * 65], [7, 9], [0] * 65)
    assert st["snap"][63][3][2] == 7 and st["snap"][64][3][2] == 9
    fresh = [list(FRESH) for _ in range(65)]
    st, board, meta, back = R.apply((0, 3), st, fresh, [[0] * 65, [20] * 65], [20, 20], [1] * 65)
    assert back == [3 * (i % 2) for i in range(65)]
    assert board[0] == FRESH and board[1] == B3 and meta[1][:2] == [20, 13]
    assert st["turn"] == list(range(1, 66))


def test_dense_and_sparse_are_inverse():
    st = climbed()
    arrays = R.dense(st)
    assert arrays["snap"].shape == (1, 16, 32) and arrays["snap"][0, 3].tolist() == (
        B3 + [12, 0, 0, 0, 5, 0, 0, 0] + [0] * 8)
    assert not arrays["snap"][0, [0, 1, 4]].any()
    assert R.sparse(arrays) == st


# ------------------------------------------------------------------ the library's boundary
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def _others():
    import g2048._native as N
    from g2048 import ntlambda, ntsearch, ntstage, nttc, ntuple, search, stagesearch

    return (N, search, ntuple, ntsearch, nttc, ntlambda, ntstage, stagesearch)


def test_header_equals_exports_equals_signatures():
    from g2048 import ntrestart

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == NAMES
    lib = ntrestart.load()
    assert set(names) == set(ntrestart.SIGNATURES)
    assert _exported(ntrestart.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other eight libraries keep their ABI: none of the new symbols
    for mod in _others():
        assert not [s for s in _exported(mod.LIB_PATH) if s.startswith("g2048_ntrestart")]
        assert not set(names) & set(mod.SIGNATURES)
    assert ntrestart.LEVELS == R.LEVELS == 16 and ntrestart.MAX_ROTATION == R.MAX_ROTATION == 8
    assert ntrestart.SLOT_BYTES == R.SLOT_BYTES == 32
    for line in ("G2048_NTRESTART_LEVELS 16", "G2048_NTRESTART_MAX_ROTATION 8",
                 "G2048_NTRESTART_SLOT_BYTES 32"):
        assert line in src
    # one argument per parameter of the header's prototype
    proto = re.search(r"g2048_ntrestart_apply\(([^)]*)\)", src).group(1)
    assert len(proto.split(",")) == len(ntrestart.SIGNATURES["g2048_ntrestart_apply"][1]) == 14


def test_library_does_not_link_against_another_g2048_library():
    from g2048 import ntrestart

    out = subprocess.run(["readelf", "-d", ntrestart.LIB_PATH], capture_output=True, text=True,
                         check=True).stdout
    needed = re.findall(r"\(NEEDED\).*\[(.*)\]", out)
    assert needed and not [n for n in needed if "g2048" in n]


def test_header_compiles_as_c(tmp_path):
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)
    # and the slot is the 32 bytes the kernel and the Python side assume
    prog = tmp_path / "slot.c"
    prog.write_text('#include "g2048_ntrestart.h"\n#include <stddef.h>\n'
                    "_Static_assert(sizeof(g2048_ntrestart_slot) == 32, \"size\");\n"
                    "_Static_assert(offsetof(g2048_ntrestart_slot, score) == 16, \"score\");\n"
                    "_Static_assert(offsetof(g2048_ntrestart_slot, moves) == 20, \"moves\");\n")
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I",
                    os.path.join(ROOT, "include"), str(prog)], check=True)


def _hashes(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash(), G.ntrestart_source_hash())


def test_build_keeps_the_new_source_out_of_the_other_stamps():
    import __graft_entry__ as G

    for other in (G.SRCS, G.SEARCH_SRCS, G.NTUPLE_SRCS, G.NTSEARCH_SRCS, G.NTTC_SRCS,
                  G.NTLAMBDA_SRCS, G.NTSTAGE_SRCS, G.STAGESEARCH_SRCS, G.NTUPLE_SHARED,
                  G.NTSTAGE_SHARED):
        assert set(G.NTRESTART_SRCS).isdisjoint(other)
    assert os.path.exists(os.path.join(G.CSRC, G.NTRESTART_SRCS[0]))
    for stamp, want in ((G.NTRESTART_STAMP, G.ntrestart_source_hash()),
                        (G.STAGESEARCH_STAMP, G.stagesearch_source_hash()),
                        (G.NTSTAGE_STAMP, G.ntstage_source_hash()),
                        (G.NTLAMBDA_STAMP, G.ntlambda_source_hash()),
                        (G.NTTC_STAMP, G.nttc_source_hash()),
                        (G.NTSEARCH_STAMP, G.ntsearch_source_hash()),
                        (G.NTUPLE_STAMP, G.ntuple_source_hash()),
                        (G.SEARCH_STAMP, G.search_source_hash()), (G.STAMP, G.source_hash())):
        assert open(stamp).read().strip() == want
    assert len(set(_hashes(G))) == 9


def test_stamp_follows_its_own_source_and_header_only(tmp_path, monkeypatch):
    """A change to the new source or to g2048_ntrestart.h changes only the new stamp; a change to
    either internal header the other libraries share leaves it alone (the source includes no
    csrc header); and without the new source and header the eight existing stamps have the
    values they have with them."""
    import shutil

    import __graft_entry__ as G

    src = open(os.path.join(G.CSRC, G.NTRESTART_SRCS[0])).read()
    assert re.findall(r'#include "([^"]+)"', src) == ["../../include/g2048_ntrestart.h"]
    before = _hashes(G)
    real_csrc, real_root = G.CSRC, G.ROOT
    copy = str(tmp_path / "csrc")
    shutil.copytree(real_csrc, copy)
    monkeypatch.setattr(G, "CSRC", copy)
    assert _hashes(G) == before
    with open(os.path.join(copy, G.NTRESTART_SRCS[0]), "a") as f:
        f.write("// changed\n")
    after = _hashes(G)
    assert after[:8] == before[:8] and after[8] != before[8]
    for shared in (G.NTUPLE_SHARED[0], G.NTSTAGE_SHARED[0], "g2048_board.hpp"):
        with open(os.path.join(copy, shared), "a") as f:
            f.write("// changed\n")
    assert _hashes(G)[8] == after[8]
    root = str(tmp_path / "root")
    shutil.copytree(os.path.join(G.ROOT, "include"), os.path.join(root, "include"))
    with open(os.path.join(root, "include", "g2048_ntrestart.h"), "a") as f:
        f.write("/* changed */\n")
    monkeypatch.setattr(G, "CSRC", real_csrc)
    monkeypatch.setattr(G, "ROOT", root)
    header = _hashes(G)
    assert header[:8] == before[:8] and header[8] != before[8]
    # a tree without the ninth library: the eight existing stamps are what they are with it
    bare, bare_root = str(tmp_path / "bare"), str(tmp_path / "bare_root")
    shutil.copytree(real_csrc, bare)
    os.remove(os.path.join(bare, G.NTRESTART_SRCS[0]))
    shutil.copytree(os.path.join(real_root, "include"), os.path.join(bare_root, "include"))
    os.remove(os.path.join(bare_root, "include", "g2048_ntrestart.h"))
    monkeypatch.setattr(G, "CSRC", bare)
    monkeypatch.setattr(G, "ROOT", bare_root)
    assert _hashes_without_the_new(G) == before[:8]
    with pytest.raises(FileNotFoundError):
        G.ntrestart_source_hash()


def _hashes_without_the_new(G):
    return (G.source_hash(), G.search_source_hash(), G.ntuple_source_hash(),
            G.ntsearch_source_hash(), G.nttc_source_hash(), G.ntlambda_source_hash(),
            G.ntstage_source_hash(), G.stagesearch_source_hash())


def test_kernel_has_no_store_data_hazard(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's
    flags, as tests/test_ntstage.py audits its library's: the snapshot and the restore are
    16-byte stores.  One kernel, no scratch."""
    import shutil
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.NTRESTART_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0
        asm = open(out).read()
        sizes = re.findall(r"\.private_segment_fixed_size:\s*(\d+)", asm)
        assert sizes == ["0"]
        # the capture's two slot stores and the restore's board store; the slot loads
        assert len(re.findall(r"global_store_dwordx4", asm)) == 3
        assert len(re.findall(r"global_load_dwordx4", asm)) >= 2


FAKE = 1 << 20


def _apply(lib, levels=(0, 5), n_levels=None, board=FAKE, meta=FAKE, clock=FAKE, done=FAKE,
           snap=FAKE, valid=FAKE, top=FAKE, turn=FAKE, restored=FAKE, n=4):
    arr = (C.c_uint8 * max(len(levels), 1))(*levels) if levels is not None else None
    return lib.g2048_ntrestart_apply(arr, len(levels) if n_levels is None else n_levels, board,
                                     meta, clock, done, snap, valid, top, turn, restored, n, 0,
                                     None)


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntrestart

    lib = ntrestart.load()
    err = lib.g2048_ntrestart_last_error
    rows = [(dict(levels=None, n_levels=2), b"levels is NULL"),
            (dict(levels=(), n_levels=0), b"n_levels"), (dict(n_levels=-1), b"n_levels"),
            (dict(levels=tuple(range(9))), b"n_levels"),
            (dict(levels=(0, 16)), b"level 1 = 16"), (dict(levels=(255,)), b"level 0 = 255"),
            (dict(levels=(0, 1, 2, 3, 4, 5, 6, 99)), b"level 7 = 99"),
            (dict(n=0), b"n ="), (dict(n=-3), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
            (dict(board=None), b"NULL"), (dict(meta=None), b"NULL"), (dict(clock=None), b"NULL"),
            (dict(done=None), b"NULL"), (dict(snap=None), b"NULL"), (dict(valid=None), b"NULL"),
            (dict(top=None), b"NULL"), (dict(turn=None), b"NULL"),
            (dict(snap=FAKE + 8), b"snap_dev must be 16-byte aligned"),
            (dict(snap=FAKE + 1), b"snap_dev must be 16-byte aligned"),
            (dict(board=FAKE + 4), b"board_dev must be 16-byte aligned"),
            (dict(clock=FAKE + 4), b"clock_dev must be 8-byte aligned"),
            (dict(meta=FAKE + 2), b"meta_dev must be 4-byte aligned"),
            (dict(turn=FAKE + 2), b"turn_dev must be 4-byte aligned"),
            (dict(valid=FAKE + 1), b"valid_dev must be 2-byte aligned")]
    for kw, word in rows:
        assert _apply(lib, **kw) == N.G2048_EINVAL, kw
        assert word in err(), (kw, err())
    assert lib.g2048_ntrestart_state_bytes(0) == N.G2048_EINVAL and b"n =" in err()
    assert lib.g2048_ntrestart_state_bytes(N.MAX_BOARDS + 1) == N.G2048_EINVAL
    assert lib.g2048_ntrestart_state_bytes(1) == 16 * 32 + 2 + 1 + 4
    assert lib.g2048_ntrestart_state_bytes(4096) == 4096 * 519
    assert ntrestart.state_bytes(65536) == 65536 * 519
    with pytest.raises(ValueError):
        ntrestart.state_bytes(0)


# ------------------------------------------------------------------ the Python side
class FakeEnv:
    def __init__(self, n, **kw):
        self.board = torch.zeros((n, 16), dtype=torch.uint8)
        self.meta = torch.zeros((2, n), dtype=torch.int32)
        self.clock = torch.zeros(((n + 63) // 64,), dtype=torch.int64)
        for k, v in kw.items():
            setattr(self, k, v)


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntrestart, ntuple

    pool = ntrestart.RestartPool(65, (0, 5, 6), device="cpu")
    assert pool.n == 65 and pool.levels == (0, 5, 6) and not pool.stagger
    assert pool.snap.shape == (65, 16, 32) and pool.snap.dtype == torch.uint8
    assert pool.valid.shape == pool.top.shape == pool.turn.shape == (65,)
    assert (pool.valid.dtype, pool.top.dtype, pool.turn.dtype) == (torch.int16, torch.uint8,
                                                                    torch.int32)
    assert sum(t.numel() * t.element_size() for t in (pool.snap, pool.valid, pool.top,
                                                      pool.turn)) == ntrestart.state_bytes(65)
    assert not pool.snap.any() and not pool.turn.any() and pool.counts() == [0] * 16
    staggered = ntrestart.RestartPool(65, (0, 5), device="cpu", stagger=True)
    assert staggered.turn.tolist() == list(range(65))
    staggered.turn.zero_()
    staggered.valid[:3] = torch.tensor([0b100000, 0b1100000, -32768], dtype=torch.int16)
    assert staggered.counts() == [0] * 5 + [2, 1] + [0] * 8 + [1]
    staggered.reset()
    assert staggered.turn.tolist() == list(range(65)) and staggered.counts() == [0] * 16
    for bad in ((), (16,), (0, -1), (300,), tuple(range(9))):
        with pytest.raises(ValueError):
            ntrestart.RestartPool(8, bad, device="cpu")
    for bad_n in (0, -1, g2048._native.MAX_BOARDS + 1):
        with pytest.raises(ValueError):
            ntrestart.RestartPool(bad_n, (0,), device="cpu")
    done = torch.zeros(65, dtype=torch.uint8)
    with pytest.raises(g2048.NativeError):  # CPU tensors: there is no CPU path
        pool.apply(FakeEnv(65), done)
    # shapes, dtypes and contiguity are checked before the device
    gpu_like = ntrestart.RestartPool(65, (0, 5), device="cpu")
    gpu_like._gpu = lambda: torch.device("cpu")
    with pytest.raises(TypeError):
        gpu_like.apply(object(), done)
    with pytest.raises(TypeError):
        gpu_like.apply(FakeEnv(65), np.zeros(65, np.uint8))
    for bad_env in (FakeEnv(64), FakeEnv(65, board=torch.zeros((65, 16), dtype=torch.int32)),
                    FakeEnv(65, meta=torch.zeros((65, 2), dtype=torch.int32)),
                    FakeEnv(65, meta=torch.zeros((2, 65), dtype=torch.int64)),
                    FakeEnv(65, clock=torch.zeros(1, dtype=torch.int64)),
                    FakeEnv(65, board=torch.zeros((65, 32), dtype=torch.uint8)[:, ::2])):
        with pytest.raises(ValueError):
            gpu_like.apply(bad_env, done)
    for bad_done in (torch.zeros(64, dtype=torch.uint8), torch.zeros(65, dtype=torch.bool),
                     torch.zeros(130, dtype=torch.uint8)[::2]):
        with pytest.raises(ValueError):
            gpu_like.apply(FakeEnv(65), bad_done)
    with pytest.raises(ValueError):
        gpu_like.apply(FakeEnv(65), done, restored_out=torch.zeros(65, dtype=torch.int32))
    # the trainers check the pool in the constructor, before any device work
    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    for cls in (g2048.NTupleTrainer, g2048.TCTrainer, g2048.TDLambdaTrainer):
        with pytest.raises(ValueError):
            cls(net, 64, restart=pool)  # 65 boards
        with pytest.raises(TypeError):
            cls(net, 65, restart="pool")
        with pytest.raises(g2048.NativeError):
            cls(net, 65, restart=pool)  # the pool fits; the CPU network has no GPU path
    assert g2048.ntrestart is ntrestart and g2048.RestartPool is ntrestart.RestartPool
    assert {"ntrestart", "RestartPool"} <= set(g2048.__all__)


def test_save_load_round_trips(tmp_path):
    from g2048 import ntrestart

    rng = np.random.default_rng(94)
    pool = ntrestart.RestartPool(33, (0, 11, 12), device="cpu", stagger=True)
    pool.snap.copy_(torch.from_numpy(rng.integers(0, 256, (33, 16, 32)).astype(np.uint8)))
    pool.valid.copy_(torch.from_numpy(rng.integers(-(1 << 15), 1 << 15, 33).astype(np.int16)))
    pool.top.copy_(torch.from_numpy(rng.integers(0, 16, 33).astype(np.uint8)))
    pool.turn.copy_(torch.from_numpy(rng.integers(-(1 << 31), 1 << 31, 33).astype(np.int32)))
    path = str(tmp_path / "pool.pt")
    pool.save(path)
    state = torch.load(path, map_location="cpu", weights_only=True)
    assert sorted(state) == ["levels", "snap", "top", "turn", "valid"]
    assert state["levels"].tolist() == [0, 11, 12]
    back = ntrestart.RestartPool.load(path, device="cpu")
    assert back.n == 33 and back.levels == (0, 11, 12)
    for name in ("snap", "valid", "top", "turn"):
        assert torch.equal(getattr(back, name), getattr(pool, name)), name
    assert back.counts() == pool.counts()
    with pytest.raises(ValueError):
        ntrestart.RestartPool(33, (0, 11), device="cpu").load_state_dict(state)
    with pytest.raises(ValueError):
        ntrestart.RestartPool(34, (0, 11, 12), device="cpu").load_state_dict(state)
    other = ntrestart.RestartPool(33, (0, 11, 12), device="cpu")
    other.load_state_dict(pool.state_dict())
    assert torch.equal(other.snap, pool.snap) and torch.equal(other.turn, pool.turn)
