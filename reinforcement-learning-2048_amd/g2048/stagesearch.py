"""Expectimax search over a multi-stage n-tuple network (libg2048_stagesearch.so, C ABI in
include/g2048_stagesearch.h).

`g2048.ntsearch` searches with one table at the leaves; `g2048.ntstage` gives every stage of the
game a table of its own.  `expectimax(staged, boards, depth)` is the search of the first over the
value function of the second: every leaf is valued at its own stage -- a merge inside the tree can
raise the largest tile, so a leaf can lie in a later stage than its root -- and UNSET entries fall
through to the stage below.  One launch for every board of a device tensor (one wavefront per
board, csrc/g2048_stagesearch.hip); `StagedNTupleNetwork.expectimax` is a method over it and
`BatchedPlayer(..., ntuple=staged, search_depth=d).play("ntstage_search")` plays whole games with
it.  Depth 1 is exactly `StagedNTupleNetwork.act`; with one stage and no UNSET entry the search is
`g2048.ntsearch.expectimax`.  The table is only read: the search promotes nothing.  Values and
actions are checked bit for bit against tests/stagesearch_ref.py.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntstage as NS
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_stagesearch.so")
MAX_DEPTH = 3           # include/g2048_stagesearch.h G2048_STAGESEARCH_MAX_DEPTH
INT64_MIN = -(1 << 63)  # the value of an illegal move

SIGNATURES = {
    "g2048_stagesearch_expectimax": (C.c_int, [C.POINTER(NT._Spec), C.POINTER(NS._Stages),
                                               C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                               C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]),
    "g2048_stagesearch_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_stagesearch.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_stagesearch") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_stagesearch_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def expectimax(net, boards: torch.Tensor, depth: int = 2, p4: float = 0.5, values=True,
               actions=True, values_out: torch.Tensor | None = None,
               actions_out: torch.Tensor | None = None):
    """Expectimax over a u8 [n, 16] device tensor of log2 exponents (such as env.board) with the
    tables of `net` (a StagedNTupleNetwork on the same GPU) at the leaves, each leaf at its own
    stage: `depth` player moves deep (1..3), chance nodes weighted by p(4) = p4.  Returns
    (actions u8 [n], values i64 [n, 4]), None for an output not asked for (a given *_out tensor
    asks for it); an illegal move's value is INT64_MIN.  Stream-ordered on the current stream of
    the network's device, no host sync, so a call with preallocated outputs can be captured into
    a graph."""
    if p4 not in (0.5, 0.1):
        raise ValueError("p4 must be 0.5 (reference, src/board.py:12) or 0.1")
    if not isinstance(net, NS.StagedNTupleNetwork):
        raise TypeError("net must be a StagedNTupleNetwork (g2048.ntsearch searches an "
                        "NTupleNetwork)")
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
    dev = net._gpu()
    n = NT._boards(boards, dev)
    vals = (NT._out(values_out, torch.int64, (n, 4), dev)
            if (values or values_out is not None) else None)
    acts = (NT._out(actions_out, torch.uint8, (n,), dev)
            if (actions or actions_out is not None) else None)
    if vals is None and acts is None:
        raise ValueError("ask for the values, the actions or both")
    with torch.cuda.device(dev):
        check(load().g2048_stagesearch_expectimax(
            C.byref(net._c), C.byref(net._cs), N.ptr(net.lut), N.ptr(boards), n, int(depth),
            N.P4_10 if p4 == 0.1 else 0, N.ptr(vals), N.ptr(acts), dev.index, N.stream_of(dev)),
            "g2048_stagesearch_expectimax")
    return acts, vals
