"""CPU-side checks of the n-tuple network: the Python restatement (tests/ntuple_ref.py) reproduces
its hand-computed anchors, the library's host-only symmetry expansion equals it, and the boundary
of libg2048_ntuple.so (header == exports, argument validation without a GPU, persistence)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import ntuple_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_ntuple.h")

A = [1, 1] + [0] * 14
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
D = [11, 10, 9, 8, 4, 5, 6, 7, 3, 2, 1, 1, 0, 0, 0, 0]
SPECS = [((0,),), R.TUPLES_2x4, R.TUPLES_4x6,
         tuple((t, t + 5, (t + 11) % 16) for t in range(8))]


# ------------------------------------------------------------------ the reference's anchors
def test_symmetry_anchors():
    assert [R.source_cell(0, g) for g in range(8)] == [0, 12, 3, 15, 0, 3, 12, 15]
    ex = R.expand(((0, 1, 2, 3),))
    assert ex[0][0] == [0, 1, 2, 3] and ex[1][0] == [12, 13, 14, 15] and ex[2][0] == [3, 2, 1, 0]
    assert ex[4][0] == [0, 4, 8, 12] and ex[7][0] == [15, 11, 7, 3]


def test_index_and_value_anchors():
    assert R.index(A, (0, 1, 2, 3)) == 17
    assert R.index([17, 16, 15, 3] + [0] * 12, (0, 1, 2, 3)) == 16383
    net = R.Net(((0,),), base=lambda t, i: i)
    assert net.V(D) == 38
    assert net.V([17] + D[1:]) == 46
    assert len(net.indices(D)) == 8 and len(R.Net(R.TUPLES_4x6).indices(D)) == 32


def test_policy_anchors():
    net = R.Net(R.TUPLES_2x4)
    q, action, after = net.policy(A)
    assert q == [None, 0, 4 << 10, 4 << 10] and action == 2 and after == [2] + [0] * 15
    q, action, after = net.policy(CHECKER)
    assert q == [None] * 4 and action == 0 and after == CHECKER


def test_td_step_anchor():
    net = R.Net(((0,),), base=[[1024 * i for i in range(16)]])
    prev, has_prev = [[2] + [0] * 15], [1]
    assert net.policy(A)[0] == [None, 2048, 8192, 8192]
    actions, err, delta = net.td_step([A], prev, has_prev, 1, 1)
    assert (actions, err, delta) == ([2], [4096], [2048])
    assert net.touched == {(0, 2): 6144, (0, 0): 12288}
    assert prev == [[2] + [0] * 15] and has_prev == [1]
    # without a previous afterstate nothing is learned; a terminal board clears has_prev and
    # learns toward 0
    net = R.Net(((0,),), base=[[1024 * i for i in range(16)]])
    prev, has_prev = [[2] + [0] * 15, [3] + [0] * 15], [0, 1]
    actions, err, delta = net.td_step([A, CHECKER], prev, has_prev, 1, 0)
    assert (actions, err, delta) == ([2, 0], [0, -6144], [0, -6144])
    assert prev == [[2] + [0] * 15, [3] + [0] * 15] and has_prev == [1, 0]
    assert net.touched == {(0, 3): 3072 - 2 * 6144, (0, 0): -6 * 6144}


def test_delta_floors_and_wraps():
    assert R.delta_of(-3, 1, 1) == -2 and R.delta_of(3, 1, 1) == 1
    assert R.delta_of(-1, 1, 31) == -1 and R.delta_of(5, 0, 0) == 0
    assert R.wrap32((1 << 31) + 5) == -(1 << 31) + 5 and R.wrap32(-(1 << 31) - 1) == (1 << 31) - 1


def test_the_eight_symmetries_are_distinct_and_closed():
    """On a 16-cell identity board: 8 different maps, and composing any two gives one of them."""
    ident = list(range(16))
    maps = [tuple(R.transform(ident, g)) for g in range(8)]
    assert len(set(maps)) == 8 and maps[0] == tuple(ident)
    for g in range(8):
        for h in range(8):
            assert tuple(R.transform(maps[g], h)) in maps


# ------------------------------------------------------------------ the library's boundary
def _spec(tuples, n_tuples=None, n_cells=None):
    from g2048 import ntuple

    s = ntuple._Spec(len(tuples) if n_tuples is None else n_tuples,
                     len(tuples[0]) if n_cells is None else n_cells)
    for t, cells in enumerate(tuples):
        for k, c in enumerate(cells):
            s.cells[t][k] = c
    return s


def test_library_loads_without_a_gpu_and_header_equals_exports():
    import g2048._native as N
    from g2048 import ntuple, search

    src = open(HEADER).read()
    names = sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))
    assert names == ["g2048_ntuple_act", "g2048_ntuple_expand", "g2048_ntuple_last_error",
                     "g2048_ntuple_lut_entries", "g2048_ntuple_td_step", "g2048_ntuple_values"]
    lib = ntuple.load()
    assert set(names) == set(ntuple.SIGNATURES)

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True,
                             text=True, check=True).stdout
        return sorted(set(re.findall(r" T (g2048_\w+)", out)))

    assert exported(ntuple.LIB_PATH) == names
    assert all(hasattr(lib, name) for name in names)
    # the other two libraries keep their ABI: none of the new symbols
    for path in (N.LIB_PATH, search.LIB_PATH):
        assert not [s for s in exported(path) if s.startswith("g2048_ntuple")]
    assert not set(names) & (set(N.SIGNATURES) | set(search.SIGNATURES))
    assert C.sizeof(ntuple._Spec) == 56


def test_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def test_build_keeps_the_new_source_out_of_the_main_stamp():
    import __graft_entry__ as G

    assert set(G.NTUPLE_SRCS).isdisjoint(G.SRCS) and set(G.NTUPLE_SRCS).isdisjoint(G.SEARCH_SRCS)
    assert os.path.exists(os.path.join(G.CSRC, G.NTUPLE_SRCS[0]))
    assert open(G.NTUPLE_STAMP).read().strip() == G.ntuple_source_hash()
    assert open(G.STAMP).read().strip() == G.source_hash()
    assert G.ntuple_source_hash() not in (G.source_hash(), G.search_source_hash())


def test_kernel_has_no_store_data_hazard(tmp_path):
    """tools/store_hazard_audit.py over the library's source, compiled with the library's
    flags, as tests/test_store_hazard.py audits the main library's sources."""
    import shutil
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.NTUPLE_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0


@pytest.mark.parametrize("tuples", SPECS)
def test_lut_entries_and_expand_equal_the_reference(tuples):
    from g2048 import ntuple

    spec = ntuple.NTupleSpec(tuples)
    T, m = len(tuples), len(tuples[0])
    assert spec.lut_entries == T * 16 ** m == ntuple.load().g2048_ntuple_lut_entries(
        C.byref(_spec(tuples)))
    assert spec.expand() == R.expand(tuples)
    # the raw output: entries past T or m are zero
    out = ntuple._EXPANDED()
    for g in range(8):
        for t in range(8):
            for k in range(6):
                out[g][t][k] = 0xEE
    assert ntuple.load().g2048_ntuple_expand(C.byref(_spec(tuples)), C.byref(out)) == 0
    for g in range(8):
        for t in range(8):
            for k in range(6):
                want = R.expand(tuples)[g][t][k] if t < T and k < m else 0
                assert out[g][t][k] == want


def test_named_sets_and_sizes():
    from g2048 import ntuple

    assert ntuple.TUPLES_4x6 == R.TUPLES_4x6 and ntuple.TUPLES_2x4 == R.TUPLES_2x4
    assert ntuple.NTupleSpec(ntuple.TUPLES_4x6).lut_entries * 4 == 256 << 20
    assert ntuple.NTupleSpec(ntuple.TUPLES_2x4).lut_entries * 4 == 512 << 10
    assert ntuple.FRAC_BITS == R.F == 10


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
    from g2048 import ntuple

    lib = ntuple.load()
    fake = 1 << 20
    s = _spec(**kw)
    out = ntuple._EXPANDED()
    calls = [lambda: lib.g2048_ntuple_lut_entries(C.byref(s)),
             lambda: lib.g2048_ntuple_expand(C.byref(s), C.byref(out)),
             lambda: lib.g2048_ntuple_values(C.byref(s), fake, fake, 4, fake, 0, None),
             lambda: lib.g2048_ntuple_act(C.byref(s), fake, fake, 4, fake, fake, fake, 0, None),
             lambda: lib.g2048_ntuple_td_step(C.byref(s), fake, fake, 4, fake, fake, 1, 10, fake,
                                              fake, fake, 0, None)]
    for call in calls:
        assert call() == N.G2048_EINVAL
        assert word in lib.g2048_ntuple_last_error(), lib.g2048_ntuple_last_error()


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import ntuple

    lib = ntuple.load()
    fake = 1 << 20
    s = _spec(R.TUPLES_2x4)

    def values(spec=s, lut=fake, boards=fake, n=4, out=fake):
        return lib.g2048_ntuple_values(C.byref(spec) if spec is not None else None, lut, boards,
                                       n, out, 0, None)

    def act(lut=fake, boards=fake, n=4, q=fake, action=fake, after=fake):
        return lib.g2048_ntuple_act(C.byref(s), lut, boards, n, q, action, after, 0, None)

    def td(lut=fake, boards=fake, n=4, prev=fake, has_prev=fake, lr_num=1, lr_shift=10,
           action=fake, delta=fake, err=fake):
        return lib.g2048_ntuple_td_step(C.byref(s), lut, boards, n, prev, has_prev, lr_num,
                                        lr_shift, action, delta, err, 0, None)

    cases = [(values, dict(spec=None), b"spec"), (values, dict(lut=None), b"NULL"),
             (values, dict(boards=None), b"NULL"), (values, dict(out=None), b"NULL"),
             (values, dict(n=0), b"n ="), (values, dict(n=N.MAX_BOARDS + 1), b"n ="),
             (values, dict(boards=fake + 4), b"aligned"), (values, dict(out=fake + 4), b"aligned"),
             (values, dict(lut=fake + 2), b"aligned"),
             (act, dict(q=None, action=None, after=None), b"NULL"), (act, dict(n=0), b"n ="),
             (act, dict(n=-3), b"n ="), (act, dict(q=fake + 4), b"aligned"),
             (act, dict(after=fake + 8), b"aligned"), (act, dict(boards=None), b"NULL"),
             (td, dict(n=0), b"n ="), (td, dict(lr_shift=32), b"lr_shift"),
             (td, dict(lr_shift=-1), b"lr_shift"), (td, dict(lr_num=-1), b"lr_num"),
             (td, dict(lr_num=(1 << 16) + 1), b"lr_num"), (td, dict(prev=None), b"NULL"),
             (td, dict(has_prev=None), b"NULL"), (td, dict(action=None), b"NULL"),
             (td, dict(delta=None), b"NULL"), (td, dict(prev=fake + 8), b"aligned"),
             (td, dict(delta=fake + 2), b"aligned"), (td, dict(err=fake + 4), b"aligned")]
    for fn, kw, word in cases:
        assert fn(**kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_ntuple_last_error(), (kw, lib.g2048_ntuple_last_error())
    assert lib.g2048_ntuple_lut_entries(None) == N.G2048_EINVAL


# ------------------------------------------------------------------ the Python side
def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import g2048
    from g2048 import ntuple, player

    for bad in ((), ((0, 1), (2,)), ((0, 16),), ((1, 1),), tuple((c,) for c in range(9)),
                ((0, 1, 2, 3, 4, 5, 6),)):
        with pytest.raises(ValueError):
            ntuple.NTupleSpec(bad)
    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    boards = torch.zeros((4, 16), dtype=torch.uint8)
    with pytest.raises(g2048.NativeError):
        net.values(boards)
    with pytest.raises(g2048.NativeError):
        net.act(boards)
    with pytest.raises(g2048.NativeError):
        ntuple.NTupleTrainer(net, 256)
    with pytest.raises(ValueError, match="network"):
        player.BatchedPlayer(4).play("ntuple")
    assert g2048.NTupleNetwork is ntuple.NTupleNetwork and g2048.TUPLES_4x6 == R.TUPLES_4x6
    assert g2048.NTupleSpec is ntuple.NTupleSpec and g2048.NTupleTrainer is ntuple.NTupleTrainer
    assert g2048.TUPLES_2x4 == R.TUPLES_2x4


def test_trainer_default_lr_shift():
    """ceil(log2(n_boards)) + 2: 1 / 2^10 at 256 boards, the rate the prototype learned with."""
    from g2048 import ntuple

    for n, want in ((1, 2), (2, 3), (3, 4), (255, 10), (256, 10), (257, 11), (65536, 18)):
        assert ntuple.default_lr_shift(n) == want, n


def test_state_dict_save_load_round_trip_on_cpu_tensors(tmp_path):
    from g2048 import ntuple

    net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    assert net.lut.shape == (2, 65536) and net.lut.dtype == torch.int32 and not net.lut.any()
    g = torch.Generator().manual_seed(3)
    net.lut.copy_(torch.randint(-(1 << 31), (1 << 31) - 1, net.lut.shape, generator=g,
                                dtype=torch.int64).to(torch.int32))
    path = str(tmp_path / "net.pt")
    net.save(path)
    back = ntuple.NTupleNetwork.load(path, device="cpu")
    assert back.spec == net.spec and torch.equal(back.lut, net.lut)
    # the file is plain tensors: weights-only loading reads it
    raw = torch.load(path, weights_only=True)
    assert sorted(raw) == ["lut", "tuples"] and raw["tuples"].tolist() == [[0, 1, 2, 3],
                                                                          [0, 1, 4, 5]]
    other = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cpu")
    other.load_state_dict(net.state_dict())
    assert torch.equal(other.lut, net.lut)
    with pytest.raises(ValueError):
        ntuple.NTupleNetwork(((0, 1, 2, 3), (0, 1, 4, 6)), device="cpu").load_state_dict(raw)
    with pytest.raises(ValueError):
        other.load_state_dict({"tuples": raw["tuples"], "lut": raw["lut"][:, :16]})


def test_reference_table_arithmetic_against_numpy():
    """The reference's sparse table against a dense numpy int32 table under the same adds."""
    rng = np.random.default_rng(2)
    base = rng.integers(-(1 << 20), 1 << 20, (2, 65536)).astype(np.int32)
    net = R.Net(R.TUPLES_2x4, base=base)
    boards = (rng.integers(1, 8, (6, 16)) * (rng.random((6, 16)) < 0.7)).astype(np.uint8)
    prev = [list(map(int, b)) for b in (rng.integers(0, 5, (6, 16))).astype(np.uint8)]
    has_prev = [1, 1, 0, 1, 1, 1]
    old_prev = [list(p) for p in prev]
    _, err, delta = net.td_step(boards, prev, has_prev, 3, 4)
    dense = base.astype(np.int64)
    for i in range(6):
        if i != 2:
            want_err = max(q for q in R.Net(R.TUPLES_2x4, base=base).policy(boards[i])[0]
                           if q is not None) - R.Net(R.TUPLES_2x4, base=base).V(old_prev[i])
            assert err[i] == want_err and delta[i] == (want_err * 3) >> 4
            for t, idx in net.indices(old_prev[i]):
                dense[t, idx] += delta[i]
    for (t, idx), v in net.touched.items():
        assert v == dense[t, idx]
    assert err[2] == 0 and delta[2] == 0
