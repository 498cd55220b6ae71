"""Delayed TD(lambda) on the staged batch-mean temporal-coherence rule for the multi-stage n-tuple
value network (libg2048_stagedelay.so, C ABI in include/g2048_stagedelay.h).

`TDLambdaTrainer` runs the eager truncated lambda-return: every step walks a board's ring of H
afterstates and adds H sets of updates, on a single table under the summed rule.
`StagedMeanTCTrainer` runs the family's strongest rule -- staged table, batch mean, a rate per
entry -- with no lambda.  This module is the delayed lambda-return (Jaskowski 2017) on that rule:
an afterstate is updated once, when it leaves a window of `horizon` steps (or when its episode
ends), by the sum of the errors seen while it sat in the window, the one k steps later weighted
lambda^k = 2^(-k lam_shift).  A board makes about one set of table hits per step, and every hit
stays one sample of the batch mean.  Like the other learners the rule is defined in integer
arithmetic (see the header), its result does not depend on any order, a whole run is reproducible
bit for bit and is checked bit for bit against tests/stagedelay_ref.py.  With horizon = 1 the step
is `StagedMeanTCState.meantc_step` exactly.

  DelayedLambdaState(net, n_boards, horizon=3, lam_shift=1)
                        owns `acc` and `ea` (as StagedMeanTCState) and the ring: `hist` u8
                        [H, n, 16], `head` u8 [n], `depth` u8 [n] and the collected error sums `g`
                        int64 [H, n]: step(), reset(), rate(), save() / load() of `ea` and the
                        ring, from_state() of a StagedMeanTCState or a single table's MeanTCState
  DelayedLambdaTrainer  NTupleTrainer with this step: k x (step, env.step[, restart.apply]), no
                        host sync; the default rate is
                        g2048.ntmeantc.default_meantc_lr_shift(spec)

`StagedNTupleNetwork` only; a single `NTupleNetwork` goes through
`StagedNTupleNetwork.from_network(net, ())`.  The players need nothing new: `play("ntuple")` and
`play("ntstage_search")` read the same table.  The binding is this module's own (not in
_native.SIGNATURES).  There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntstage as NS
from . import ntuple as NT
from .ntmeantc import MeanTCState, default_meantc_lr_shift
from .stagemeantc import StagedMeanTCState, StagedTCState, bound_rate_and_acc_bytes

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_stagedelay.so")
MAX_HORIZON = 8           # include/g2048_stagedelay.h G2048_STAGEDELAY_MAX_HORIZON
MAX_LAM_SHIFT = 31        # G2048_STAGEDELAY_MAX_LAM_SHIFT; also bounds (horizon - 1) * lam_shift
RATE_BITS = 16            # G2048_STAGEDELAY_RATE_BITS
MAX_A = (1 << 62) - 1     # G2048_STAGEDELAY_MAX_A

_HEAD = [C.POINTER(NT._Spec), C.POINTER(NS._Stages)]

SIGNATURES = {
    "g2048_stagedelay_rate": (C.c_int32, [C.c_int64, C.c_int64]),
    "g2048_stagedelay_acc_bytes": (C.c_int64, list(_HEAD)),
    "g2048_stagedelay_step": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                                C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                C.c_int, C.c_void_p]),
    "g2048_stagedelay_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_stagedelay.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_stagedelay") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_stagedelay_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


rate, acc_bytes = bound_rate_and_acc_bytes(load, "stagedelay")

_RING = ("hist", "head", "depth", "g")


class DelayedLambdaState(StagedTCState):
    """The state of the rule for one StagedNTupleNetwork and `n_boards` boards, on the network's
    device: the workspace `acc` and the accumulators `ea` of StagedTCState, and the ring of each
    board's last `horizon` afterstates: `hist` u8 [H, n, 16], `head` u8 [n] (the plane of the
    latest one), `depth` u8 [n] (how many the running episode has) and `g` int64 [H, n] (the error
    sum each has collected), all zero when fresh.  lambda = 2^-lam_shift.  The ring holds errors
    not yet applied, so it is saved with `ea`, and a file's lam_shift must be the state's.  On a
    GPU device it steps through the library; on the CPU it only holds, saves and loads."""

    _TENSORS, _SCALARS = _RING, ("lam_shift",)
    rate = staticmethod(rate)

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int, horizon: int = 3,
                 lam_shift: int = 1):
        super().__init__(net)
        self.n, self.horizon, self.lam_shift = int(n_boards), int(horizon), int(lam_shift)
        if not 1 <= self.n <= N.MAX_BOARDS:
            raise ValueError(f"n_boards must be in [1, {N.MAX_BOARDS}]")
        if not 1 <= self.horizon <= MAX_HORIZON:
            raise ValueError(f"horizon must be in [1, {MAX_HORIZON}]")
        if not 1 <= self.lam_shift <= MAX_LAM_SHIFT:
            raise ValueError(f"lam_shift must be in [1, {MAX_LAM_SHIFT}]")
        if (self.horizon - 1) * self.lam_shift > MAX_LAM_SHIFT:
            raise ValueError(f"(horizon - 1) * lam_shift must not exceed {MAX_LAM_SHIFT}")
        kw = dict(device=net.device)
        self.hist = torch.zeros((self.horizon, self.n, 16), dtype=torch.uint8, **kw)
        self.head = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.depth = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.g = torch.zeros((self.horizon, self.n), dtype=torch.int64, **kw)

    @classmethod
    def from_state(cls, state, net: NS.StagedNTupleNetwork, n_boards: int, horizon: int = 3,
                   lam_shift: int = 1) -> "DelayedLambdaState":
        """A fresh ring over the accumulators of a run under another rule: a StagedMeanTCState's
        `ea` as it is (`net` must have its tuples and bounds), or a single table's MeanTCState's
        in stage 0 with zeros above (`net` must have its tuples).  `ea` is copied to `net`'s
        device."""
        if not isinstance(state, (StagedMeanTCState, MeanTCState)):
            raise TypeError("state must be a StagedMeanTCState or a g2048.ntmeantc.MeanTCState")
        st = cls(net, n_boards, horizon, lam_shift)
        st._adopt(state)
        return st

    def reset(self) -> None:
        """Forget every board's afterstates and their collected errors (stream-ordered): the fresh
        ring.  `ea` is kept.  A caller that replaces the table calls this."""
        for name in _RING:
            getattr(self, name).zero_()

    def step(self, boards, lr_num, lr_shift, actions_out, delta_out, err_out=None):
        """One step of the header on this state and caller-owned outputs (no allocation):
        actions_out u8 [n], delta_out i32 [H, n], err_out i64 [n] or None."""
        net = self.net
        dev = net._gpu()
        n = NT._boards(boards, dev)
        if n != self.n:
            raise ValueError(f"boards must be uint8 [{self.n}, 16]")
        if actions_out is None or delta_out is None:
            raise ValueError("step needs actions_out and delta_out")
        NT._out(actions_out, torch.uint8, (n,), dev)
        NT._out(delta_out, torch.int32, (self.horizon, n), dev)
        if err_out is not None:
            NT._out(err_out, torch.int64, (n,), dev)
        if not 0 <= int(lr_num) <= NT.MAX_LR_NUM or not 0 <= int(lr_shift) <= NT.MAX_LR_SHIFT:
            raise ValueError(f"lr_num must be in [0, {NT.MAX_LR_NUM}] and lr_shift in "
                             f"[0, {NT.MAX_LR_SHIFT}]")
        if any(getattr(self, name).device != dev for name in ("acc", "ea", *_RING)):
            raise ValueError(f"acc, ea and the ring must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_stagedelay_step(
                C.byref(net._c), C.byref(net._cs), N.ptr(net.lut), N.ptr(self.acc),
                N.ptr(self.ea), N.ptr(boards), n, N.ptr(self.hist), N.ptr(self.head),
                N.ptr(self.depth), N.ptr(self.g), self.horizon, self.lam_shift, int(lr_num),
                int(lr_shift), N.ptr(actions_out), N.ptr(delta_out), N.ptr(err_out), dev.index,
                N.stream_of(dev)), "g2048_stagedelay_step")
        return actions_out, delta_out, err_out

    @classmethod
    def load(cls, path, net: NS.StagedNTupleNetwork) -> "DelayedLambdaState":
        """The state saved at `path`, for `net` (whose tuples and bounds must be the file's); the
        board count, the horizon and lam_shift are the file's."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        H, n = state["g"].shape
        st = cls(net, n, H, int(state["lam_shift"]))
        st.load_state_dict(state)
        return st


class DelayedLambdaTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the step of this module: the same self-play loop, env, episode log and
    `restart=` keyword, the table moved by DelayedLambdaState.step.  `lr_shift=None` picks
    default_meantc_lr_shift(net.spec).  `step(k)` enqueues k x (step, env.step[, restart.apply])
    on the current stream with no host sync and no allocation.  The base class's `prev` /
    `has_prev` are not used: the afterstates live in `self.state`; `self.delta` is int32 [H, n]."""

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int, horizon: int = 3,
                 lam_shift: int = 1, state: DelayedLambdaState | None = None,
                 lr_shift: int | None = None, **kw):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes through "
                            "StagedNTupleNetwork.from_network(net, ()))")
        if state is None:  # validates n_boards, horizon and lam_shift before the env exists
            state = DelayedLambdaState(net, n_boards, horizon, lam_shift)
        elif not isinstance(state, DelayedLambdaState) or state.net is not net:
            raise ValueError("state must be the DelayedLambdaState of this network")
        elif state.n != int(n_boards):
            raise ValueError(f"state must hold {int(n_boards)} boards")
        if lr_shift is None:
            lr_shift = default_meantc_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.state = state
        self.delta = torch.zeros((state.horizon, self.n), dtype=torch.int32, device=net.device)

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.state.step(self.env.board, self.lr_num, self.lr_shift, self.actions, self.delta,
                            self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
