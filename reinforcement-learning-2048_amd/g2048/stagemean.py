"""Batch-mean TD learning for the multi-stage n-tuple value network (libg2048_stagemean.so, C ABI
in include/g2048_stagemean.h).

`NTupleTrainer(staged, ...)` moves a staged table by the sum rule, whose rate is sized for the hot
early-game entries (n * lr = 1/4): the late stages' tables, which a handful of boards touch per
step, barely move.  `MeanTrainer` removes that dependence on the batch, but takes a single table
only.  This module is the composition: the batch-mean rule on a `StagedNTupleNetwork`, weight
promotion included.  Every staged entry hit in a step moves by floor(D / C), the mean of the deltas
that hit it at its own stage; two boards of different stages that address the same (t, i) move two
different entries.  Like the other learners the rule is defined in integer arithmetic (see the
header), its accumulation is integer atomic adds, which commute, and it is checked bit for bit
against tests/stagemean_ref.py.

  StagedMeanState(net)    owns `acc`, int64 [S, T, 16^m, 2] ((D, C) per staged entry; a workspace
                          that is all zero between steps, 16 bytes per table entry): mean_step()
  StagedMeanTrainer       NTupleTrainer with the staged batch-mean step: k x (mean_step, env.step
                          [, restart.apply]), no host sync; the default rate is
                          g2048.ntmean.default_mean_lr_shift(spec)

`StagedNTupleNetwork` only; a single `NTupleNetwork` goes to g2048.ntmean.  The players need
nothing new: `play("ntuple")` and `play("ntstage_search")` read the same table.  The binding is
this module's own (not in _native.SIGNATURES).  There is no CPU fallback: a missing library or a
non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntstage as NS
from . import ntuple as NT
from .ntmean import default_mean_lr_shift

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_stagemean.so")

_HEAD = [C.POINTER(NT._Spec), C.POINTER(NS._Stages)]

SIGNATURES = {
    "g2048_stagemean_acc_bytes": (C.c_int64, list(_HEAD)),
    "g2048_stagemean_step": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64,
                                               C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]),
    "g2048_stagemean_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_stagemean.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_stagemean") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_stagemean_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def acc_bytes(spec, bounds=()) -> int:
    """Bytes of the (D, C) workspace of a spec with len(bounds) + 1 stages: 16 per staged entry."""
    bounds = tuple(int(b) for b in bounds)
    if len(bounds) > NS.MAX_STAGES - 1 or any(not 1 <= b <= NS.MAX_BOUND for b in bounds):
        raise ValueError(f"a staged network holds 1..{NS.MAX_STAGES} stages with bounds in "
                         f"1..{NS.MAX_BOUND}")
    r = load().g2048_stagemean_acc_bytes(C.byref(NT._as_spec(spec)._c()),
                                         C.byref(NS._c_stages(bounds)))
    if r < 0:
        raise ValueError(load().g2048_stagemean_last_error().decode(errors="replace"))
    return int(r)


class StagedMeanState:
    """The batch-mean workspace of one StagedNTupleNetwork: `acc` int64 [S, T, 16^m, 2] on the
    network's device, zeroed here and left all zero by every step.  It carries nothing across
    steps, so there is nothing to save."""

    def __init__(self, net: NS.StagedNTupleNetwork):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes to "
                            "g2048.ntmean.MeanState)")
        self.net = net
        self.acc = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)

    def mean_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                  err_out=None):
        """One staged batch-mean step of the header, promotion included, on caller-owned state and
        outputs (no allocation); the arguments of StagedNTupleNetwork.td_step."""
        net = self.net
        dev = net._gpu()
        n = NT._step_args("mean_step", boards, prev, has_prev, actions_out, delta_out, err_out,
                          dev)
        if self.acc.device != dev:
            raise ValueError(f"acc must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_stagemean_step(
                C.byref(net._c), C.byref(net._cs), N.ptr(net.lut), N.ptr(self.acc), N.ptr(boards),
                n, N.ptr(prev), N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_stagemean_step")
        return actions_out, delta_out, err_out


class StagedMeanTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the staged batch-mean step: the same self-play loop, env, episode log
    and `restart=` keyword, the table moved by StagedMeanState.mean_step.  `lr_shift=None` picks
    default_mean_lr_shift(net.spec), which depends neither on n_boards nor on the stages.
    `step(k)` enqueues k x (mean_step, env.step[, restart.apply]) on the current stream with no
    host sync and no allocation."""

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int,
                 mean: StagedMeanState | None = None, lr_shift: int | None = None, **kw):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes to "
                            "g2048.ntmean.MeanTrainer)")
        if lr_shift is None:
            lr_shift = default_mean_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.mean = StagedMeanState(net) if mean is None else mean
        if self.mean.net is not net:
            raise ValueError("mean must be the StagedMeanState of this network")

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.mean.mean_step(self.env.board, self.prev, self.has_prev, self.lr_num,
                                self.lr_shift, self.actions, self.delta, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
