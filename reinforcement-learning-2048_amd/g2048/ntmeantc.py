"""Temporal-coherence learning on the batch-mean rule for the n-tuple value network
(libg2048_ntmeantc.so, C ABI in include/g2048_ntmeantc.h).

`TCTrainer` gives every entry a rate of its own, |E| / A, but in a lock-step batch a hot entry
receives thousands of deltas of both signs in one step and its rate collapses at once.
`MeanTrainer` moves every touched entry once per step, by the mean floor(D / C) of its hits, but at
one fixed rate.  Here an entry hit in a step receives that one mean m scaled by rate(E, A), and E
and A accumulate m and |m|: the accumulators see one error per entry per step.  Like the other
rules it is defined in integer arithmetic (see the header), its result does not depend on any
order, a whole run is reproducible bit for bit and is checked bit for bit against
tests/ntmeantc_ref.py.

  MeanTCState(net)   owns `acc`, int64 [T, 16^m, 2] ((D, C) per entry; a workspace that is all
                     zero between steps) and `ea`, int64 [T, 16^m, 2] (E and A interleaved; it
                     carries across steps): meantc_step(), rate(), save() / load() of `ea` with
                     TCState's keys, so a file written by either loads into the other
  default_meantc_lr_shift(spec)
                     default_mean_lr_shift(spec) - 2: 4 for TUPLES_2x4, 5 for TUPLES_4x6
  MeanTCTrainer      NTupleTrainer with this step: k x (meantc_step, env.step), no host sync

Single `NTupleNetwork` tables only.  The binding is this module's own (not in
_native.SIGNATURES).  There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT
from .ntmean import default_mean_lr_shift

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntmeantc.so")
RATE_BITS = 16            # include/g2048_ntmeantc.h G2048_NTMEANTC_RATE_BITS: a rate of 2^16 is 1
MAX_A = (1 << 62) - 1     # G2048_NTMEANTC_MAX_A

SIGNATURES = {
    "g2048_ntmeantc_rate": (C.c_int32, [C.c_int64, C.c_int64]),
    "g2048_ntmeantc_acc_bytes": (C.c_int64, [C.POINTER(NT._Spec)]),
    "g2048_ntmeantc_step": (C.c_int, [C.POINTER(NT._Spec), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                      C.c_void_p]),
    "g2048_ntmeantc_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntmeantc.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntmeantc") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntmeantc_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def rate(E: int, A: int) -> int:
    """rate(E, A) of the header, in [0, 2^16] (host code of the library)."""
    r = load().g2048_ntmeantc_rate(int(E), int(A))
    if r < 0:
        raise ValueError(load().g2048_ntmeantc_last_error().decode(errors="replace"))
    return int(r)


def acc_bytes(spec) -> int:
    """Bytes of the (D, C) workspace of a spec, and of `ea`: 16 per table entry each."""
    r = load().g2048_ntmeantc_acc_bytes(C.byref(NT._as_spec(spec)._c()))
    if r < 0:
        raise ValueError(load().g2048_ntmeantc_last_error().decode(errors="replace"))
    return int(r)


def default_meantc_lr_shift(spec) -> int:
    """default_mean_lr_shift(spec) - 2: the base rate 8 T * lr_num / 2^lr_shift = 1 that the
    literature runs temporal coherence at.  The batch-mean rule alone needs 1/4 there and diverges
    at 1; with the per-entry rate on top an entry slows itself down once its errors
    cancel, and on the 60-second 4x6 protocol a base rate of 1 beat 1/4 on both players by more
    than a seed moves them, on two seeds: 2^-4 on TUPLES_2x4, 2^-5 on TUPLES_4x6."""
    return default_mean_lr_shift(spec) - 2


class MeanTCState:
    """The state of the rule for one NTupleNetwork, on the network's device: the workspace `acc`
    int64 [T, 16^m, 2], zeroed here and left all zero by every step, and the accumulators `ea`
    int64 [T, 16^m, 2], ea[t, i, 0] = E and ea[t, i, 1] = A of net.lut[t, i], zero-initialised.
    On a GPU device it steps through the library; on the CPU it only holds, saves and loads."""

    def __init__(self, net: NT.NTupleNetwork):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be a plain NTupleNetwork (staged tables are not supported)")
        self.net = net
        self.acc = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)
        self.ea = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)

    rate = staticmethod(rate)

    def meantc_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                    err_out=None):
        """One step of the header on caller-owned state and outputs (no allocation); the
        arguments of NTupleNetwork.td_step."""
        net = self.net
        dev = net._gpu()
        n = NT._step_args("meantc_step", boards, prev, has_prev, actions_out, delta_out, err_out,
                          dev)
        if self.acc.device != dev or self.ea.device != dev:
            raise ValueError(f"acc and ea must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_ntmeantc_step(
                C.byref(net._c), N.ptr(net.lut), N.ptr(self.acc), N.ptr(self.ea), N.ptr(boards),
                n, N.ptr(prev), N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_ntmeantc_step")
        return actions_out, delta_out, err_out

    # ------------------------------------------------------------------ persistence (TCState's)
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back.  `acc` holds
        nothing between steps and is not saved."""
        return {"tuples": torch.tensor(self.net.spec.tuples, dtype=torch.int64), "ea": self.ea}

    def load_state_dict(self, state: dict) -> None:
        tuples = tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist())
        if tuples != self.net.spec.tuples:
            raise ValueError(f"the file's tuples {tuples} are not this network's "
                             f"{self.net.spec.tuples}")
        ea = state["ea"]
        if ea.dtype != torch.int64 or ea.shape != self.ea.shape:
            raise ValueError(f"ea must be int64 {tuple(self.ea.shape)}")
        self.ea.copy_(ea)

    def save(self, path) -> None:
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, net: NT.NTupleNetwork) -> "MeanTCState":
        """The accumulators saved at `path`, for `net` (whose tuples must be the file's)."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        st = cls(net)
        st.load_state_dict(state)
        return st


class MeanTCTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the step of this module: the same self-play loop, env, episode log and
    `restart=` keyword, the table moved by MeanTCState.meantc_step.  `lr_shift=None` picks
    default_meantc_lr_shift(net.spec), which does not depend on n_boards.  `step(k)` enqueues
    k x (meantc_step, env.step[, restart.apply]) on the current stream with no host sync and no
    allocation."""

    def __init__(self, net: NT.NTupleNetwork, n_boards: int, state: MeanTCState | None = None,
                 lr_shift: int | None = None, **kw):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be a plain NTupleNetwork (staged tables are not supported)")
        if lr_shift is None:
            lr_shift = default_meantc_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.state = MeanTCState(net) if state is None else state
        if self.state.net is not net:
            raise ValueError("state must be the MeanTCState of this network")

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.state.meantc_step(self.env.board, self.prev, self.has_prev, self.lr_num,
                                   self.lr_shift, self.actions, self.delta, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
