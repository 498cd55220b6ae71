"""Batched expectimax search player (libg2048_search.so, C ABI in include/g2048_search.h).

The reference reserves Player.play_state_space_search_game(sss_algo) (src/player.py:87-88) and
leaves it empty; this module fills the slot: `expectimax` searches every board of a device
tensor in one launch (one wavefront per board, csrc/g2048_search.hip),
`BatchedPlayer.play("expectimax")` plays whole games with it, and
`generate_replay_buffer_using_expectimax` is the search-teacher counterpart of
generate_replay_buffer_using_A_star: it fills a device replay ring with the search policy's
transitions.  The search is defined in integer arithmetic (see the header), so its values and
actions are checked bit for bit against tests/expectimax_ref.py.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import astuple, dataclass

import torch

from . import _native as N

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_search.so")
MAX_DEPTH = 4  # include/g2048_search.h G2048_SEARCH_MAX_DEPTH
INT64_MIN = -(1 << 63)  # the value of an illegal move


class _Weights(C.Structure):
    """g2048_search_weights."""
    _fields_ = [(n, C.c_int32) for n in ("gain", "empty", "smooth", "mono", "corner", "lost")]


@dataclass(frozen=True)
class SearchWeights:
    """The six int32 weights of the search (defaults as g2048_search_default_weights)."""
    gain: int = 256
    empty: int = 2048
    smooth: int = 256
    mono: int = 1024
    corner: int = 512
    lost: int = 1000000

    def _c(self) -> _Weights:
        return _Weights(*(int(x) for x in astuple(self)))


SIGNATURES = {
    "g2048_search_default_weights": (None, [C.POINTER(_Weights)]),
    "g2048_search_expectimax": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_uint32,
                                          C.POINTER(_Weights), C.c_void_p, C.c_void_p, C.c_int,
                                          C.c_void_p]),
    "g2048_search_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_search.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_search") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_search_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def default_weights() -> SearchWeights:
    """The library's defaults, read through g2048_search_default_weights."""
    w = _Weights()
    load().g2048_search_default_weights(C.byref(w))
    return SearchWeights(w.gain, w.empty, w.smooth, w.mono, w.corner, w.lost)


def expectimax(boards: torch.Tensor, depth: int = 2, weights: SearchWeights | None = None,
               p4: float = 0.5, values=True, actions_out: torch.Tensor | None = None,
               values_out: torch.Tensor | None = None):
    """Expectimax over a u8 [n, 16] device tensor of log2 exponents (such as env.board):
    `depth` player moves deep, chance nodes weighted by p(4) = p4.  Returns
    (actions u8 [n], values i64 [n, 4] or None with values=False); an illegal move's value is
    INT64_MIN.  Stream-ordered on the current stream of the boards' device, no host sync, so a
    call with preallocated `actions_out` / `values_out` can be captured into a graph."""
    if p4 not in (0.5, 0.1):
        raise ValueError("p4 must be 0.5 (reference, src/board.py:12) or 0.1")
    if not isinstance(boards, torch.Tensor):
        raise TypeError("boards must be a torch tensor on the GPU")
    dev = N.require_gpu(boards.device)
    if boards.dtype != torch.uint8 or boards.dim() != 2 or boards.shape[1] != 16:
        raise ValueError("boards must be uint8 [n, 16]")
    if not boards.is_contiguous():
        raise ValueError("boards must be contiguous")
    n = boards.shape[0]
    if n < 1:
        raise ValueError("boards is empty")
    acts = actions_out if actions_out is not None else torch.empty(n, dtype=torch.uint8, device=dev)
    vals = None
    if values:
        vals = (values_out if values_out is not None
                else torch.empty((n, 4), dtype=torch.int64, device=dev))
    for t, dt, shape in ((acts, torch.uint8, (n,)), (vals, torch.int64, (n, 4))):
        if t is not None and (t.dtype != dt or tuple(t.shape) != shape or t.device != dev
                              or not t.is_contiguous()):
            raise ValueError(f"output must be a contiguous {dt} {shape} tensor on {dev}")
    w = (weights if weights is not None else SearchWeights())._c()
    with torch.cuda.device(dev):
        check(load().g2048_search_expectimax(
            N.ptr(boards), n, int(depth), N.P4_10 if p4 == 0.1 else 0, C.byref(w), N.ptr(vals),
            N.ptr(acts), dev.index, N.stream_of(dev)), "g2048_search_expectimax")
    return acts, vals


def generate_replay_buffer_using_expectimax(n_boards: int, steps: int, maxlen: int, depth: int = 1,
                                            device="cuda", seed: int = 0x2048, p4: float = 0.5,
                                            weights: SearchWeights | None = None):
    """The search-teacher counterpart of generate_replay_buffer_using_A_star
    (src/state_space_search.py:103-131): `steps` env steps of `n_boards` auto-resetting boards
    under the expectimax policy, each step appended to a device ring of `maxlen` rows by the
    step kernel itself (env.step(actions, replay=rb)).  Returns the ReplayBuffer."""
    from .env import ReplayBuffer, VecEnv2048

    if int(n_boards) < 1 or int(maxlen) < 1 or int(maxlen) % int(n_boards) != 0:
        # the env appends one block of n_boards rows per step (include/g2048.h, replay ring)
        raise ValueError(f"maxlen = {maxlen} must be a positive multiple of n_boards = {n_boards}")
    env = VecEnv2048(int(n_boards), seed=seed, device=device, p4=p4)
    rb = ReplayBuffer(int(maxlen), device=device)
    acts = torch.empty(env.n, dtype=torch.uint8, device=env.device)
    out = tuple(torch.empty(env.n, dtype=dt, device=env.device)
                for dt in (torch.int32, torch.uint8, torch.uint8))
    for _ in range(int(steps)):
        expectimax(env.board, depth, weights, p4, values=False, actions_out=acts)
        env.step(acts, replay=rb, reward=out[0], done=out[1], legal=out[2])
    env.check_errors()
    torch.cuda.synchronize(env.device)
    return rb
