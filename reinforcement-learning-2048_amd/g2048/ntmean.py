"""Batch-mean TD learning for the n-tuple value network (libg2048_ntmean.so, C ABI in
include/g2048_ntmean.h).

`NTupleTrainer` adds into every table entry the sum of the deltas a lock-step batch sends it, so
its rate has to shrink with the batch (`default_lr_shift(n)` keeps n * lr = 1/4) and an entry only
one board touches moves n times more slowly than it could.  The batch-mean rule moves every touched
entry by the mean of the deltas that hit it in this step, floor(D / C): a hot entry moves by the
batch's mean error, a rare one by its own, and the rate depends on the number of entries that make
up a value (8 T), not on the batch.  Like the TD(0) step the rule is defined in integer arithmetic
(see the header) and its accumulation is integer atomic adds, which commute: a whole run is
reproducible bit for bit and is checked bit for bit against tests/ntmean_ref.py.

  MeanState(net)              owns `acc`, int64 [T, 16^m, 2] ((D, C) per entry; a workspace that
                              is all zero between steps, 16 bytes per table entry): mean_step()
  default_mean_lr_shift(spec) ceil(log2(8 T)) + 2: 6 for TUPLES_2x4, 7 for TUPLES_4x6
  MeanTrainer                 NTupleTrainer with the batch-mean step: k x (mean_step, env.step),
                              no host sync

Single `NTupleNetwork` tables only; staged tables and combinations with TC or TD(lambda) are not
offered.  The binding is this module's own (not in _native.SIGNATURES).  There is no CPU
fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntmean.so")

SIGNATURES = {
    "g2048_ntmean_acc_bytes": (C.c_int64, [C.POINTER(NT._Spec)]),
    "g2048_ntmean_step": (C.c_int, [C.POINTER(NT._Spec), C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                    C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntmean_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntmean.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntmean") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntmean_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def acc_bytes(spec) -> int:
    """Bytes of the (D, C) workspace of a spec: 16 per table entry."""
    r = load().g2048_ntmean_acc_bytes(C.byref(NT._as_spec(spec)._c()))
    if r < 0:
        raise ValueError(load().g2048_ntmean_last_error().decode(errors="replace"))
    return int(r)


def default_mean_lr_shift(spec) -> int:
    """ceil(log2(8 T)) + 2.  A value is the sum of 8 T entries, and under the batch-mean rule each
    of them moves by (the mean of) delta, so V(prev) moves by about 8 T * lr * err.  Keeping
    8 T * lr_num / 2^lr_shift at 1/4, as default_lr_shift keeps n * lr, makes that a contraction
    at any batch width: 2^-6 on TUPLES_2x4, 2^-7 on TUPLES_4x6."""
    return (8 * NT._as_spec(spec).n_tuples - 1).bit_length() + 2


class MeanState:
    """The batch-mean workspace of one NTupleNetwork: `acc` int64 [T, 16^m, 2] on the network's
    device, zeroed here and left all zero by every step.  It carries nothing across steps, so
    there is nothing to save."""

    def __init__(self, net: NT.NTupleNetwork):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be an NTupleNetwork (staged tables are not supported)")
        self.net = net
        self.acc = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)

    def mean_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                  err_out=None):
        """One batch-mean step of the header on caller-owned state and outputs (no allocation);
        the arguments of NTupleNetwork.td_step."""
        net = self.net
        dev = net._gpu()
        n = NT._step_args("mean_step", boards, prev, has_prev, actions_out, delta_out, err_out,
                          dev)
        if self.acc.device != dev:
            raise ValueError(f"acc must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_ntmean_step(
                C.byref(net._c), N.ptr(net.lut), N.ptr(self.acc), N.ptr(boards), n, N.ptr(prev),
                N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_ntmean_step")
        return actions_out, delta_out, err_out


class MeanTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the batch-mean step: the same self-play loop, env, episode log and
    `restart=` keyword, the table moved by MeanState.mean_step.  `lr_shift=None` picks
    default_mean_lr_shift(net.spec), which does not depend on n_boards.  `step(k)` enqueues
    k x (mean_step, env.step[, restart.apply]) on the current stream with no host sync and no
    allocation."""

    def __init__(self, net: NT.NTupleNetwork, n_boards: int, mean: MeanState | None = None,
                 lr_shift: int | None = None, **kw):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be an NTupleNetwork (staged tables are not supported)")
        if lr_shift is None:
            lr_shift = default_mean_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.mean = MeanState(net) if mean is None else mean
        if self.mean.net is not net:
            raise ValueError("mean must be the MeanState of this network")

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.mean.mean_step(self.env.board, self.prev, self.has_prev, self.lr_num,
                                self.lr_shift, self.actions, self.delta, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
