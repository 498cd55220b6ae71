"""The on-device n-tuple player (libg2048_ntplay.so, C ABI in include/g2048_ntplay.h): K moves of
the greedy or expectimax policy of an n-tuple network, played on an env's own buffers in one
launch.

`net.act` / `ntsearch.expectimax` / `stagesearch.expectimax` choose a move and `env.step` plays
it: two launches and a host round trip per move.  `steps(net, env, k, depth)` plays k moves of the
same policy inside one kernel (csrc/g2048_ntplay.hip: the boards stay in registers, the table is
only read) and leaves `env.board`, `env.meta`, `env.ep` and `env.clock` byte for byte as k
iterations of that loop leave them, for an env with or without auto-reset and for both p(4).
`net` is an `NTupleNetwork` or a `StagedNTupleNetwork`; `net.play_steps(env, k, depth)` is a method
over it and `BatchedPlayer(..., ntuple=net, search_depth=d).play("ntuple_fused" | "ntstage_fused")`
plays whole games with it.

`fin` u8 [n] and `result` i32 [n, 4] are the player's latch, given together: at the first
terminal step of board i at which fin[i] == 0, result[i] receives what that step writes to
env.ep[i] (episodes, score, moves, largest exponent) and fin[i] becomes 1; a row with fin[i] != 0
is never written.  The replay ring and the episode log are not served: an env with a log attached
is refused.

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

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntplay.so")
MAX_DEPTH = 3        # include/g2048_ntplay.h G2048_NTPLAY_MAX_DEPTH
MAX_STEPS = 1 << 20  # G2048_NTPLAY_MAX_STEPS

_COMMON = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64,
           C.c_uint64, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
SIGNATURES = {
    "g2048_ntplay_steps": (C.c_int, [C.POINTER(NT._Spec), *_COMMON]),
    "g2048_ntplay_staged_steps": (C.c_int, [C.POINTER(NT._Spec), C.POINTER(NS._Stages),
                                            *_COMMON]),
    "g2048_ntplay_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntplay.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntplay") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntplay_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def _buffer(t, name, dtype, shape, dev):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor on the GPU")
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} {list(shape)} tensor")
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}")


def steps(net, env, k: int, depth: int = 1, fin: torch.Tensor | None = None,
          result: torch.Tensor | None = None) -> None:
    """k moves (1..2^20) of the depth-`depth` policy (1..3; 1 is net.act, 2..3 the expectimax of
    g2048.ntsearch / g2048.stagesearch with the env's p(4) at the chance nodes) of `net` on every
    board of `env` (a VecEnv2048 on the network's GPU), in one launch, plus one for the clocks.
    `fin` u8 [n] and `result` i32 [n, 4] are the latch of the module docstring, both or neither.
    Stream-ordered on the current stream of the network's device, no host sync and no allocation,
    so the call may be captured into a graph."""
    if not isinstance(net, (NT.NTupleNetwork, NS.StagedNTupleNetwork)):
        raise TypeError("net must be an NTupleNetwork or a StagedNTupleNetwork")
    if not 1 <= int(k) <= MAX_STEPS:
        raise ValueError(f"k must be in [1, {MAX_STEPS}]")
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
    if (fin is None) != (result is None):
        raise ValueError("fin and result are given together or not at all")
    for name in ("board", "meta", "ep", "clock", "seed", "board_offset", "flags", "n"):
        if not hasattr(env, name):
            raise TypeError(f"env must be a VecEnv2048 (it has no `{name}`)")
    if getattr(env, "episode_log", None) is not None:
        raise ValueError("the env has an episode log attached: the on-device player writes no "
                         "episode records (detach the log, or step the env move by move)")
    dev = net._gpu()
    n = int(env.n)
    NT._boards(env.board, dev)
    _buffer(env.board, "env.board", torch.uint8, (n, 16), dev)
    _buffer(env.meta, "env.meta", torch.int32, (2, n), dev)
    _buffer(env.ep, "env.ep", torch.int32, (n, 4), dev)
    _buffer(env.clock, "env.clock", torch.int64, ((n + 63) // 64,), dev)
    if fin is not None:
        _buffer(fin, "fin", torch.uint8, (n,), dev)
        _buffer(result, "result", torch.int32, (n, 4), dev)
    tail = (N.ptr(net.lut), N.ptr(env.board), N.ptr(env.meta), N.ptr(env.ep), N.ptr(env.clock), n,
            int(env.seed), int(env.board_offset), int(env.flags), int(k), int(depth), N.ptr(fin),
            N.ptr(result), dev.index, N.stream_of(dev))
    with torch.cuda.device(dev):
        if isinstance(net, NS.StagedNTupleNetwork):
            check(load().g2048_ntplay_staged_steps(C.byref(net._c), C.byref(net._cs), *tail),
                  "g2048_ntplay_staged_steps")
        else:
            check(load().g2048_ntplay_steps(C.byref(net._c), *tail), "g2048_ntplay_steps")
