"""Temporal-coherence (TC) learning for the n-tuple value network (libg2048_nttc.so, C ABI in
include/g2048_nttc.h).

`NTupleTrainer` moves every table entry at one global, fixed rate.  TC learning (Beal and Smith
1999; for 2048: Jaskowski 2017) gives each entry a rate of its own: next to the table, every entry
keeps the running sum E of the deltas it received and the running sum A of their magnitudes, and
moves by delta * |E| / A -- at full speed while its errors agree in sign, slower once they start
to cancel.  Like the TD(0) step the rule is defined in integer arithmetic (see the header) and its
updates are integer atomic adds, which commute: a whole run is reproducible bit for bit and is
checked bit for bit against tests/nttc_ref.py.

  TCState(net)      owns `ea`, int64 [T, 16^m, 2] (E and A interleaved; 16 bytes per table entry,
                    1 GiB for TUPLES_4x6): tc_step(), save() / load()
  TCTrainer         NTupleTrainer with the TC step: k x (tc_step, env.step), no host sync

The table the rule trains is the network's own `net.lut`: `NTupleNetwork.act` / `search` and
`BatchedPlayer(..., ntuple=net)` play from it as before.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_nttc.so")
RATE_BITS = 16            # include/g2048_nttc.h G2048_NTTC_RATE_BITS: a rate of 2^16 is 1
MAX_A = (1 << 62) - 1     # G2048_NTTC_MAX_A

SIGNATURES = {
    "g2048_nttc_rate": (C.c_int32, [C.c_int64, C.c_int64]),
    "g2048_nttc_work_bytes": (C.c_int64, [C.POINTER(NT._Spec), C.c_int64]),
    "g2048_nttc_step": (C.c_int, [C.POINTER(NT._Spec), C.c_void_p, C.c_void_p, C.c_void_p,
                                  C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                  C.c_void_p]),
    "g2048_nttc_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_nttc.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_nttc") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_nttc_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def rate(E: int, A: int) -> int:
    """rate(E, A) of the header, in [0, 2^16] (host code of the library)."""
    r = load().g2048_nttc_rate(int(E), int(A))
    if r < 0:
        raise ValueError(load().g2048_nttc_last_error().decode(errors="replace"))
    return int(r)


def work_bytes(spec, n_boards: int) -> int:
    """Bytes of scratch one tc_step over n_boards boards needs."""
    r = load().g2048_nttc_work_bytes(C.byref(NT._as_spec(spec)._c()), int(n_boards))
    if r < 0:
        raise ValueError(load().g2048_nttc_last_error().decode(errors="replace"))
    return int(r)


class TCState:
    """The temporal-coherence accumulators of one NTupleNetwork: `ea` int64 [T, 16^m, 2] on the
    network's device, ea[t, i, 0] = E and ea[t, i, 1] = A of net.lut[t, i], zero-initialised.  On
    a GPU device it steps through the library; on the CPU it only holds, saves and loads."""

    def __init__(self, net: NT.NTupleNetwork):
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be an NTupleNetwork")
        self.net = net
        self.ea = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)

    def tc_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                err_out=None, work=None):
        """One TC step of the header on caller-owned state and outputs.  `work` is a uint8
        device tensor of at least work_bytes(spec, n); without one it is allocated here."""
        net = self.net
        dev = net._gpu()
        n = NT._step_args("tc_step", boards, prev, has_prev, actions_out, delta_out, err_out, dev)
        need = work_bytes(net.spec, n)
        if work is None:
            work = torch.empty(need, dtype=torch.uint8, device=dev)
        elif (work.dtype != torch.uint8 or work.dim() != 1 or work.numel() < need
              or work.device != dev or not work.is_contiguous()):
            raise ValueError(f"work must be a contiguous uint8 [>= {need}] tensor on {dev}")
        if self.ea.device != dev:
            raise ValueError(f"ea must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_nttc_step(
                C.byref(net._c), N.ptr(net.lut), N.ptr(self.ea), N.ptr(boards), n, N.ptr(prev),
                N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), N.ptr(work), dev.index, N.stream_of(dev)),
                "g2048_nttc_step")
        return actions_out, delta_out, err_out

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back."""
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
    def load(cls, path, net: NT.NTupleNetwork) -> "TCState":
        """The accumulators saved at `path`, for `net` (whose tuples must be the file's)."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        tc = cls(net)
        tc.load_state_dict(state)
        return tc


class TCTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the temporal-coherence step: the same self-play loop, env, episode log
    and default rate, the table moved by TCState.tc_step.  `step(k)` enqueues
    k x (tc_step, env.step) on the current stream with no host sync and no allocation."""

    def __init__(self, net: NT.NTupleNetwork, n_boards: int, tc: TCState | None = None, **kw):
        super().__init__(net, n_boards, **kw)
        self.tc = TCState(net) if tc is None else tc
        if self.tc.net is not net:
            raise ValueError("tc must be the TCState of this network")
        self.work = torch.empty(work_bytes(net.spec, self.n), dtype=torch.uint8,
                                device=net._gpu())

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.tc.tc_step(self.env.board, self.prev, self.has_prev, self.lr_num, self.lr_shift,
                            self.actions, self.delta, self.err, self.work)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
