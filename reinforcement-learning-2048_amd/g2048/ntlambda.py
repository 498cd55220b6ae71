"""Truncated TD(lambda) learning for the n-tuple value network (libg2048_ntlambda.so, C ABI in
include/g2048_ntlambda.h).

`NTupleTrainer`'s TD(0) step moves, with the error a board observes, only its previous afterstate.
TD(lambda) with eligibility traces truncated to a horizon H (Jaskowski 2017: lambda = 0.5, H = 3)
also moves the afterstates 2, 3, ... H steps back, the one k steps back by delta * lambda^k.  Here
lambda = 2^-lam_shift, so the weights are shifts: like the TD(0) step the rule is defined in
integer arithmetic (see the header) and its updates are 32-bit integer atomic adds, which commute:
a whole run is reproducible bit for bit and is checked bit for bit against tests/ntlambda_ref.py.

  TDLambdaState(net, n_boards, horizon=3, lam_shift=1)
                    owns the boards' ring of afterstates (`hist` u8 [H, n, 16], `head` u8 [n],
                    `depth` u8 [n]): step(), reset().  The ring is transient, as
                    NTupleTrainer.prev is: it is not saved.
  TDLambdaTrainer   NTupleTrainer with the lambda step: k x (step, env.step), no host sync

The table the rule trains is the network's own `net.lut`: `NTupleNetwork.act` / `search` and
`BatchedPlayer(..., ntuple=net)` play from it as before.  With horizon = 1 the step is
`NTupleNetwork.td_step` exactly.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntlambda.so")
MAX_HORIZON = 8      # include/g2048_ntlambda.h G2048_NTLAMBDA_MAX_HORIZON
MAX_LAM_SHIFT = 31   # G2048_NTLAMBDA_MAX_LAM_SHIFT; also the bound of (horizon - 1) * lam_shift

SIGNATURES = {
    "g2048_ntlambda_step": (C.c_int, [C.POINTER(NT._Spec), C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                      C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_int, C.c_void_p]),
    "g2048_ntlambda_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntlambda.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntlambda") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntlambda_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


class TDLambdaState:
    """The ring of the last `horizon` afterstates of each of `n_boards` boards, on the network's
    device: `hist` u8 [H, n, 16], `head` u8 [n] (the plane of the latest one) and `depth` u8 [n]
    (how many the running episode has), all zero when fresh.  lambda = 2^-lam_shift."""

    def __init__(self, net: NT.NTupleNetwork, n_boards: int, horizon: int = 3,
                 lam_shift: int = 1):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be an NTupleNetwork")
        self.net = net
        self.n, self.horizon, self.lam_shift = int(n_boards), int(horizon), int(lam_shift)
        if not 1 <= self.n <= N.MAX_BOARDS:
            raise ValueError(f"n_boards must be in [1, {N.MAX_BOARDS}]")
        if not 1 <= self.horizon <= MAX_HORIZON:
            raise ValueError(f"horizon must be in [1, {MAX_HORIZON}]")
        if not 1 <= self.lam_shift <= MAX_LAM_SHIFT:
            raise ValueError(f"lam_shift must be in [1, {MAX_LAM_SHIFT}]")
        if (self.horizon - 1) * self.lam_shift > MAX_LAM_SHIFT:
            raise ValueError(f"(horizon - 1) * lam_shift must not exceed {MAX_LAM_SHIFT}")
        dev = net._gpu()
        self.hist = torch.zeros((self.horizon, self.n, 16), dtype=torch.uint8, device=dev)
        self.head = torch.zeros(self.n, dtype=torch.uint8, device=dev)
        self.depth = torch.zeros(self.n, dtype=torch.uint8, device=dev)

    def reset(self) -> None:
        """Forget every board's afterstates (stream-ordered): the fresh state."""
        self.hist.zero_()
        self.head.zero_()
        self.depth.zero_()

    def step(self, boards, lr_num, lr_shift, actions_out, delta_out, err_out=None):
        """One TD(lambda) step of the header on this state and caller-owned outputs (no
        allocation)."""
        net = self.net
        dev = net._gpu()
        n = NT._boards(boards, dev)
        if n != self.n:
            raise ValueError(f"boards must be uint8 [{self.n}, 16]")
        if actions_out is None or delta_out is None:
            raise ValueError("step needs actions_out and delta_out")
        NT._out(actions_out, torch.uint8, (n,), dev)
        NT._out(delta_out, torch.int32, (n,), dev)
        if err_out is not None:
            NT._out(err_out, torch.int64, (n,), dev)
        if not 0 <= int(lr_num) <= NT.MAX_LR_NUM or not 0 <= int(lr_shift) <= NT.MAX_LR_SHIFT:
            raise ValueError(f"lr_num must be in [0, {NT.MAX_LR_NUM}] and lr_shift in "
                             f"[0, {NT.MAX_LR_SHIFT}]")
        with torch.cuda.device(dev):
            check(load().g2048_ntlambda_step(
                C.byref(net._c), N.ptr(net.lut), N.ptr(boards), n, N.ptr(self.hist),
                N.ptr(self.head), N.ptr(self.depth), self.horizon, self.lam_shift, int(lr_num),
                int(lr_shift), N.ptr(actions_out), N.ptr(delta_out), N.ptr(err_out), dev.index,
                N.stream_of(dev)), "g2048_ntlambda_step")
        return actions_out, delta_out, err_out


class TDLambdaTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the truncated TD(lambda) step: the same self-play loop, env, episode
    log and default rate, the table moved by TDLambdaState.step.  `step(k)` enqueues
    k x (lambda step, env.step) on the current stream with no host sync and no allocation.  The
    base class's `prev` / `has_prev` are not used: the afterstates live in `self.lam`."""

    def __init__(self, net: NT.NTupleNetwork, n_boards: int, horizon: int = 3,
                 lam_shift: int = 1, **kw):
        super().__init__(net, n_boards, **kw)
        self.lam = TDLambdaState(net, self.n, horizon, lam_shift)

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.lam.step(self.env.board, self.lr_num, self.lr_shift, self.actions, self.delta,
                          self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
