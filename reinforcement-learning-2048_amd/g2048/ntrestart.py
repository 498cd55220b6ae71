"""Per-board restart pool (carousel) for n-tuple self-play (libg2048_ntrestart.so, C ABI in
include/g2048_ntrestart.h).

Every self-play trainer starts every episode from a freshly dealt board, so boards with a large
tile are rare and the late stages of a staged network see a fraction of the updates.  Carousel
shaping (Jaskowski 2017) and the restart strategy (Matsuzaki 2017) start some episodes from a
position an earlier game reached.  Here each board keeps a pool of snapshots of its own games on
the device, one per largest-tile level; one call after `env.step` records a snapshot when a board
first reaches a level, and replaces a freshly re-dealt board with a snapshot according to a fixed
rotation of levels (0 = start fresh).  Everything is per board and in integer arithmetic (see the
header): no atomics, reproducible, and checked bit for bit against tests/ntrestart_ref.py.

  RestartPool(n_boards, levels, device, stagger=False)   owns snap / valid / top / turn:
                    apply(env, done), reset(), counts(), state_dict() / load_state_dict(),
                    save() / load()
  NTupleTrainer / TCTrainer / TDLambdaTrainer(..., restart=pool)   each iteration of step(k)
                    becomes (learner step, env.step, pool.apply); restart=None is the plain loop

The score and move count of a restarted episode continue from the snapshot, so the env's episode
log records the whole virtual game.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntrestart.so")
LEVELS = 16        # include/g2048_ntrestart.h G2048_NTRESTART_LEVELS
MAX_ROTATION = 8   # G2048_NTRESTART_MAX_ROTATION
SLOT_BYTES = 32    # G2048_NTRESTART_SLOT_BYTES: u8 board[16], u32 score, u32 moves, u32 pad[2]

SIGNATURES = {
    "g2048_ntrestart_state_bytes": (C.c_int64, [C.c_int64]),
    "g2048_ntrestart_apply": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int,
                                        C.c_void_p]),
    "g2048_ntrestart_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntrestart.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntrestart") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntrestart_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def state_bytes(n_boards: int) -> int:
    """The bytes of the four state buffers of `n_boards` boards (host only)."""
    n = int(load().g2048_ntrestart_state_bytes(int(n_boards)))
    if n < 0:
        raise ValueError(load().g2048_ntrestart_last_error().decode(errors="replace"))
    return n


def _typed(t, dtype, shape, dev, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch tensor on the GPU")
    if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous {dtype} {shape} tensor")
    if t.device != dev:
        raise ValueError(f"{name} must be on {dev}")
    return t


class RestartPool:
    """The pool of `n_boards` boards on `device`:

      snap   uint8 [n, 16, 32]  slot e of board i: board (16 bytes), score, moves (u32 each), pad
      valid  int16 [n]          bit e set iff slot e of board i holds a snapshot (u16 bits)
      top    uint8 [n]          the largest level the running episode has been captured at
      turn   int32 [n]          episodes finished (+ the board index with stagger=True), u32 bits

    `levels` is the rotation: 1..8 levels in 0..15, 0 = start fresh.  With `stagger` the boards
    sit at different points of the rotation.  On the CPU the pool only holds, saves and loads."""

    def __init__(self, n_boards: int, levels, device="cuda", stagger: bool = False):
        self.n = int(n_boards)
        if not 1 <= self.n <= N.MAX_BOARDS:
            raise ValueError(f"n_boards must be in [1, {N.MAX_BOARDS}]")
        levels = tuple(int(e) for e in levels)
        if not 1 <= len(levels) <= MAX_ROTATION:
            raise ValueError(f"a rotation holds 1..{MAX_ROTATION} levels")
        if any(not 0 <= e < LEVELS for e in levels):
            raise ValueError(f"levels must be in 0..{LEVELS - 1}")
        self.levels = levels
        self._c = (C.c_uint8 * len(levels))(*levels)
        self.stagger = bool(stagger)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.device = N.require_gpu(self.device)
        kw = dict(device=self.device)
        self.snap = torch.zeros((self.n, LEVELS, SLOT_BYTES), dtype=torch.uint8, **kw)
        self.valid = torch.zeros(self.n, dtype=torch.int16, **kw)
        self.top = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.turn = torch.zeros(self.n, dtype=torch.int32, **kw)
        self.reset()

    def _gpu(self) -> torch.device:
        return N.require_gpu(self.device)

    def reset(self) -> None:
        """Forget every snapshot and start the rotation over (stream-ordered)."""
        self.snap.zero_()
        self.valid.zero_()
        self.top.zero_()
        if self.stagger:
            # board i starts at turn i (the u32 pattern; n <= G2048_MAX_BOARDS < 2^31)
            torch.arange(self.n, out=self.turn)
        else:
            self.turn.zero_()

    def apply(self, env, done: torch.Tensor, restored_out: torch.Tensor | None = None):
        """The call of the header on `env.board / env.meta / env.clock`, after an `env.step` that
        wrote `done` (uint8 [n]).  `restored_out` (uint8 [n]) receives the level each board was
        restored at, 0 for none.  Stream-ordered, one launch, no allocation."""
        dev = self._gpu()
        n = self.n
        for name in ("board", "meta", "clock"):
            if not hasattr(env, name):
                raise TypeError("env must be a VecEnv2048 (board, meta, clock)")
        _typed(env.board, torch.uint8, (n, 16), dev, "env.board")
        _typed(env.meta, torch.int32, (2, n), dev, "env.meta")
        _typed(env.clock, torch.int64, ((n + 63) // 64,), dev, "env.clock")
        _typed(done, torch.uint8, (n,), dev, "done")
        if restored_out is not None:
            _typed(restored_out, torch.uint8, (n,), dev, "restored_out")
        with torch.cuda.device(dev):
            check(load().g2048_ntrestart_apply(
                self._c, len(self.levels), N.ptr(env.board), N.ptr(env.meta), N.ptr(env.clock),
                N.ptr(done), N.ptr(self.snap), N.ptr(self.valid), N.ptr(self.top),
                N.ptr(self.turn), N.ptr(restored_out), n, dev.index, N.stream_of(dev)),
                "g2048_ntrestart_apply")
        return restored_out

    def counts(self) -> list:
        """The number of boards whose slot e is set, for e = 0..15 (host sync; for reports)."""
        v = self.valid.to(torch.int64) & 0xFFFF
        return [int(x) for x in ((v[:, None] >> torch.arange(LEVELS, device=v.device)) & 1)
                .sum(dim=0).tolist()]

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back."""
        return {"levels": torch.tensor(self.levels, dtype=torch.int64), "snap": self.snap,
                "valid": self.valid, "top": self.top, "turn": self.turn}

    def load_state_dict(self, state: dict) -> None:
        levels = tuple(int(e) for e in state["levels"].tolist())
        if levels != self.levels:
            raise ValueError(f"the file's levels {levels} are not this pool's {self.levels}")
        for name in ("snap", "valid", "top", "turn"):
            mine, t = getattr(self, name), state[name]
            if t.dtype != mine.dtype or t.shape != mine.shape:
                raise ValueError(f"{name} must be {mine.dtype} {tuple(mine.shape)}")
        for name in ("snap", "valid", "top", "turn"):
            getattr(self, name).copy_(state[name])

    def save(self, path) -> None:
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, device="cuda") -> "RestartPool":
        state = torch.load(path, map_location="cpu", weights_only=True)
        pool = cls(state["turn"].shape[0], tuple(int(e) for e in state["levels"].tolist()),
                   device)
        pool.load_state_dict(state)
        return pool
