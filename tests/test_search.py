"""CPU-side checks of the expectimax search: the Python restatement (tests/expectimax_ref.py)
reproduces the anchor numbers the search was specified with, the heuristic on hand-built boards,
and the boundary of libg2048_search.so (header == exports, argument validation without a GPU)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import expectimax_ref as R
from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "g2048_search.h")

A = [1, 1] + [0] * 14
B = [1, 2, 3, 4, 8, 7, 6, 5, 1, 2, 3, 4, 2, 1, 2, 0]
CHECKER = [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 1]
D = [11, 10, 9, 8, 4, 5, 6, 7, 3, 2, 1, 1, 0, 0, 0, 0]
_ = None
# (board, p4, depth, values up/down/left/right, action)
ANCHORS = [
    (A, 0.5, 1, [_, 23506, 26982, 26982], 2),
    (A, 0.5, 2, [_, 23570, 24987, 24987], 2),
    (A, 0.1, 1, [_, 24376, 27706, 27706], 2),
    (A, 0.1, 2, [_, 24771, 25225, 25225], 2),
    (B, 0.5, 1, [_, -1000000, _, -29696], 3),
    (B, 0.5, 2, [_, -1000000, _, -26144], 3),
    (B, 0.1, 2, [_, -1000000, _, -24619], 3),
    (CHECKER, 0.5, 1, [_, _, _, _], 0),
    (CHECKER, 0.1, 3, [_, _, _, _], 0),
    (D, 0.5, 1, [_, -46016, 1664, 384], 2),
    (D, 0.5, 2, [_, -27990, 3122, 3046], 2),
    (D, 0.5, 3, [_, -25619, 7231, 7231], 2),
    (D, 0.1, 1, [_, -45965, 1971, 691], 2),
    (D, 0.1, 2, [_, -28212, 3560, 3549], 2),
]


@pytest.mark.parametrize("board,p4,depth,values,action", ANCHORS)
def test_reference_reproduces_the_anchors(board, p4, depth, values, action):
    got, act = R.expectimax(board, depth, p4=p4)
    assert got == values and act == action


def test_heuristic_anchors():
    assert R.H(A) == 28416 and R.H(B) == -28672 and R.H(D) == 2048


def test_heuristic_terms_on_hand_built_boards():
    # empty board: 16 empties, nothing else
    assert R.terms([0] * 16) == (16, 0, 0, 0)
    # one 2^5 tile in a corner: the two pairs next to it differ by 5
    b = [0] * 16
    b[0] = 5
    assert R.terms(b) == (15, 10, 0, 5)
    # the same tile in the middle: four pairs, a 0-5-0-0 bump in its row and in its column
    # (inc = dec = 5), and no corner holds the maximum
    b = [0] * 16
    b[5] = 5
    assert R.terms(b) == (15, 20, 10, 0)
    # rows that rise, columns that are flat: monotone, smoothness 3 per row
    b = [1, 2, 3, 4] * 4
    assert R.terms(b) == (0, 12, 0, 4)
    # a zig-zag row 1 3 1 3 over empties: inc = 4, dec = 2 in that row, columns fall to 0
    b = [1, 3, 1, 3] + [0] * 12
    assert R.terms(b) == (12, 6 + 8, 2, 3)
    # the snake D: every line monotone (rows differ by 8, columns by 38); the 2^11 sits in a corner
    assert R.terms(D) == (4, 8 + 38, 0, 11)
    # weights enter linearly, a zero weight drops its term
    w = R.Weights(gain=7, empty=3, smooth=5, mono=11, corner=0, lost=9)
    E, Sm, Mo, Cn = R.terms(B)
    assert R.H(B, w) == 3 * E - 5 * Sm - 11 * Mo


def test_reference_slide_equals_the_oracle():
    rng = np.random.default_rng(11)
    for _k in range(300):
        b = rng.integers(0, 6, 16).astype(np.uint8) * (rng.random(16) < 0.7)
        mask = O.legal_mask(b)
        for a in range(4):
            after, gain = R.move(b, a)
            o_after, o_gain = O.move(b, a)
            assert after == list(o_after) and gain == o_gain
            assert (after != list(b)) == bool((mask >> a) & 1)
        assert R.has_move(bytes(b)) == (mask != 0)
    for b in ([0] * 16, CHECKER, B, [1, 2, 1, 2, 2, 1, 2, 1, 1, 2, 1, 2, 2, 1, 2, 2]):
        assert R.has_move(bytes(b)) == (O.legal_mask(np.array(b, np.uint8)) != 0)


def test_floor_division_is_toward_minus_infinity():
    """The chance node floors like Python's //, also where the numerator is negative and the
    division inexact (a truncating division would be one too high there)."""
    import math
    from fractions import Fraction

    rng = np.random.default_rng(5)
    negative_inexact = 0
    for p4, (W, w4) in ((0.5, (2, 1)), (0.1, (10, 1))):
        s = R.Search(p4=p4)
        for _k in range(60):
            b = bytes(int(x) for x in rng.integers(1, 9, 16) * (rng.random(16) < 0.8))
            em = [c for c in range(16) if b[c] == 0]
            if not em:
                continue
            total = sum(k * s.vmax(b[:c] + bytes([e]) + b[c + 1:], 0)
                        for c in em for e, k in ((1, W - w4), (2, w4)))
            den = W * len(em)
            assert s.vchance(b, 0) == math.floor(Fraction(total, den))
            negative_inexact += total < 0 and total % den != 0
    assert negative_inexact >= 10


# ------------------------------------------------------------------ the library's boundary
def _declared():
    src = open(HEADER).read()
    return sorted(set(re.findall(r"G2048_API\s+[\w\s\*]+?\b(g2048_\w+)\s*\(", src)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True,
                         check=True).stdout
    return sorted(set(re.findall(r" T (g2048_\w+)", out)))


def test_header_declarations_equal_the_exports():
    import g2048._native as N
    from g2048 import search

    names = _declared()
    assert names == ["g2048_search_default_weights", "g2048_search_expectimax",
                     "g2048_search_last_error"]
    lib = search.load()
    for name in names:
        assert hasattr(lib, name), name
    assert set(names) == set(search.SIGNATURES)
    assert _exported(search.LIB_PATH) == names
    # the main library keeps its ABI: none of the search symbols
    assert not [s for s in _exported(N.LIB_PATH) if s.startswith("g2048_search")]
    assert not set(names) & set(N.SIGNATURES)


def test_search_header_compiles_as_c():
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                   check=True)


def test_search_kernel_has_no_store_data_hazard(tmp_path):
    """tools/store_hazard_audit.py over the search library's source, compiled with the library's
    flags, as tests/test_store_hazard.py audits the main library's sources."""
    import shutil
    import sys

    if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not in this image")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as G
    import store_hazard_audit

    for f in G.SEARCH_SRCS:
        src, out = os.path.join(G.CSRC, f), str(tmp_path / (f + ".s"))
        flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        assert store_hazard_audit.audit(out) == 0


def test_default_weights():
    from g2048 import search

    assert search.default_weights() == search.SearchWeights()
    assert tuple(R.DEFAULT) == (256, 2048, 256, 1024, 512, 1000000)
    w = search.SearchWeights()
    assert (w.gain, w.empty, w.smooth, w.mono, w.corner, w.lost) == tuple(R.DEFAULT)


def test_bad_arguments_are_refused_without_a_gpu():
    """Argument checks run before any device work: G2048_EINVAL with a message.  The pointers
    are never dereferenced (a fake aligned address stands in for device memory)."""
    import g2048._native as N
    from g2048 import search

    lib = search.load()
    fake = 1 << 20
    w = search.SearchWeights()._c()

    def call(boards=fake, n=4, depth=2, flags=0, weights=w, values=fake, action=fake):
        return lib.g2048_search_expectimax(boards, n, depth, flags,
                                           C.byref(weights) if weights is not None else None,
                                           values, action, 0, None)

    for kw, word in ((dict(depth=0), b"depth"), (dict(depth=5), b"depth"),
                     (dict(values=None, action=None), b"NULL"), (dict(boards=None), b"NULL"),
                     (dict(n=0), b"n ="), (dict(n=N.MAX_BOARDS + 1), b"n ="),
                     (dict(flags=N.EGREEDY_FIXED), b"flags"), (dict(flags=8), b"flags"),
                     (dict(boards=fake + 4), b"aligned"), (dict(values=fake + 4), b"aligned"),
                     (dict(weights=search.SearchWeights(mono=-1)._c()), b"mono"),
                     (dict(weights=search.SearchWeights(gain=(1 << 24) + 1)._c()), b"gain"),
                     (dict(weights=search.SearchWeights(lost=(1 << 30) + 1)._c()), b"lost")):
        assert call(**kw) == N.G2048_EINVAL, kw
        assert word in lib.g2048_search_last_error(), (kw, lib.g2048_search_last_error())


def test_python_side_refuses_bad_input_and_has_no_cpu_path():
    import torch

    import g2048
    from g2048 import player, search

    with pytest.raises(g2048.NativeError):
        search.expectimax(torch.zeros((4, 16), dtype=torch.uint8))  # a CPU tensor
    with pytest.raises(ValueError):
        search.expectimax(torch.zeros((4, 16), dtype=torch.uint8), p4=0.3)
    with pytest.raises(ValueError):
        player.BatchedPlayer(4, search_depth=5)
    with pytest.raises(ValueError):
        player.BatchedPlayer(4).play("minimax")
    with pytest.raises(ValueError, match="multiple"):  # the ring takes whole steps of n rows
        search.generate_replay_buffer_using_expectimax(64, 8, 500)
    assert g2048.expectimax is search.expectimax
