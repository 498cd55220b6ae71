"""Expectimax search over an n-tuple value network (libg2048_ntsearch.so, C ABI in
include/g2048_ntsearch.h): the two strong players of this package combined.

`g2048.search` looks 1-4 moves ahead and scores its leaves with a fixed heuristic; `g2048.ntuple`
learns a value function and plays one move deep.  Strong 2048 programs run the expectimax with the
learned afterstate values at the leaves (Szubert and Jaskowski 2014; Yeh et al. 2016; Jaskowski
2017).  `expectimax(net, boards, depth)` is that search for every board of a device tensor in one
launch (one wavefront per board, csrc/g2048_ntsearch.hip); `NTupleNetwork.search` is a method over
it and `BatchedPlayer(..., ntuple=net, search_depth=d).play("ntuple_search")` plays whole games
with it.  Depth 1 is exactly `NTupleNetwork.act`.  The search is defined in integer arithmetic
(see the header), so values and actions are checked bit for bit against tests/ntsearch_ref.py.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntsearch.so")
MAX_DEPTH = 3           # include/g2048_ntsearch.h G2048_NTSEARCH_MAX_DEPTH
INT64_MIN = -(1 << 63)  # the value of an illegal move

SIGNATURES = {
    "g2048_ntsearch_expectimax": (C.c_int, [C.POINTER(NT._Spec), C.c_void_p, C.c_void_p, C.c_int64,
                                            C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_void_p]),
    "g2048_ntsearch_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntsearch.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntsearch") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntsearch_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def expectimax(net, boards: torch.Tensor, depth: int = 2, p4: float = 0.5, values=True,
               actions=True, values_out: torch.Tensor | None = None,
               actions_out: torch.Tensor | None = None):
    """Expectimax over a u8 [n, 16] device tensor of log2 exponents (such as env.board) with the
    table of `net` (an NTupleNetwork on the same GPU) at the leaves: `depth` player moves deep
    (1..3), chance nodes weighted by p(4) = p4.  Returns (actions u8 [n], values i64 [n, 4]), None
    for an output not asked for (a given *_out tensor asks for it); an illegal move's value is
    INT64_MIN.  Stream-ordered on the current stream of the network's device, no host sync, so a
    call with preallocated outputs can be captured into a graph."""
    if p4 not in (0.5, 0.1):
        raise ValueError("p4 must be 0.5 (reference, src/board.py:12) or 0.1")
    if not isinstance(net, NT.NTupleNetwork):
        raise TypeError("net must be an NTupleNetwork")
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
        check(load().g2048_ntsearch_expectimax(
            C.byref(net._c), N.ptr(net.lut), N.ptr(boards), n, int(depth),
            N.P4_10 if p4 == 0.1 else 0, N.ptr(vals), N.ptr(acts), dev.index, N.stream_of(dev)),
            "g2048_ntsearch_expectimax")
    return acts, vals
