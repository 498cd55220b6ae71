"""Temporal-coherence learning on the batch-mean rule for the multi-stage n-tuple value network
(libg2048_stagemeantc.so, C ABI in include/g2048_stagemeantc.h).

`MeanTCTrainer` scales the one mean update an entry receives per step by a rate of the entry's
own, |E| / A, but takes a single table only; `StagedMeanTrainer` runs the batch-mean rule on a
`StagedNTupleNetwork`, but at one fixed rate.  This module is the composition: every staged entry
hit in a step moves by floor(D / C), the mean of the deltas that hit it at its own stage, scaled
by rate(E, A) of (E, A) that belong to that STAGED entry; two boards of different stages that
address the same (t, i) move two different entries at two different rates.  Promotion copies the
weight only: a promoted entry starts from its own (E, A), zeros if it never moved.  Like the other
learners the rule is defined in integer arithmetic (see the header), its result does not depend on
any order, a whole run is reproducible bit for bit and is checked bit for bit against
tests/stagemeantc_ref.py.

  StagedTCState(net)      the base of this state and of g2048.stagedelay's and g2048.stageback's,
                          the same rule on other schedules: `acc`, `ea`, the adoption of another
                          state's `ea`, state_dict() / load_state_dict() / save()
  StagedMeanTCState(net)  owns `acc`, int64 [S, T, 16^m, 2] ((D, C) per staged entry; a workspace
                          that is all zero between steps) and `ea`, int64 [S, T, 16^m, 2] (E and A
                          interleaved; it carries across steps): meantc_step(), rate(), save() /
                          load() of `ea`, from_state() of a single table's MeanTCState
  StagedMeanTCTrainer     NTupleTrainer with this step: k x (meantc_step, env.step
                          [, restart.apply]), no host sync; the default rate is
                          g2048.ntmeantc.default_meantc_lr_shift(spec)

`StagedNTupleNetwork` only; a single `NTupleNetwork` goes to g2048.ntmeantc.  The players need
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
from .ntmeantc import MeanTCState, default_meantc_lr_shift

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_stagemeantc.so")
RATE_BITS = 16            # include/g2048_stagemeantc.h G2048_STAGEMEANTC_RATE_BITS
MAX_A = (1 << 62) - 1     # G2048_STAGEMEANTC_MAX_A

_HEAD = [C.POINTER(NT._Spec), C.POINTER(NS._Stages)]

SIGNATURES = {
    "g2048_stagemeantc_rate": (C.c_int32, [C.c_int64, C.c_int64]),
    "g2048_stagemeantc_acc_bytes": (C.c_int64, list(_HEAD)),
    "g2048_stagemeantc_step": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int64, C.c_void_p, C.c_void_p, C.c_int32,
                                                 C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_int, C.c_void_p]),
    "g2048_stagemeantc_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_stagemeantc.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_stagemeantc") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_stagemeantc_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def bound_rate_and_acc_bytes(load, name: str):
    """`rate` and `acc_bytes` of the staged mean-TC library that `load()` binds and whose symbols
    start with g2048_`name`_: the three libraries of the rule export the same two host calls."""
    def call(symbol, *args):
        r = getattr(load(), f"g2048_{name}_{symbol}")(*args)
        if r < 0:
            raise ValueError(getattr(load(), f"g2048_{name}_last_error")().decode(
                errors="replace"))
        return int(r)

    def rate(E: int, A: int) -> int:
        """rate(E, A) of the header, in [0, 2^16] (host code of the library)."""
        return call("rate", int(E), int(A))

    def acc_bytes(spec, bounds=()) -> int:
        """Bytes of the (D, C) workspace of a spec with len(bounds) + 1 stages, and of `ea`: 16
        per staged entry each."""
        bounds = tuple(int(b) for b in bounds)
        if len(bounds) > NS.MAX_STAGES - 1 or any(not 1 <= b <= NS.MAX_BOUND for b in bounds):
            raise ValueError(f"a staged network holds 1..{NS.MAX_STAGES} stages with bounds in "
                             f"1..{NS.MAX_BOUND}")
        return call("acc_bytes", C.byref(NT._as_spec(spec)._c()), C.byref(NS._c_stages(bounds)))

    return rate, acc_bytes


rate, acc_bytes = bound_rate_and_acc_bytes(load, "stagemeantc")


class StagedTCState:
    """What the states of the staged mean-TC rule share, whatever the schedule: the workspace
    `acc` int64 [S, T, 16^m, 2], zeroed here and left all zero by every step, and the accumulators
    `ea` int64 [S, T, 16^m, 2], ea[s, t, i, 0] = E and ea[s, t, i, 1] = A of net.lut[s, t, i],
    zero-initialised, on the network's device; the adoption of another state's `ea`; state_dict(),
    load_state_dict() and save().  A subclass names what it carries beside `ea`: its tensors in
    `_TENSORS` and its int attributes, which a file must match, in `_SCALARS`."""

    _TENSORS: tuple = ()
    _SCALARS: tuple = ()

    def __init__(self, net: NS.StagedNTupleNetwork):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes through "
                            "StagedNTupleNetwork.from_network(net, ()))")
        self.net = net
        self.acc = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)
        self.ea = torch.zeros((*net.lut.shape, 2), dtype=torch.int64, device=net.device)

    def _adopt(self, state) -> None:
        """`ea` of a run under another rule, copied to this state's device: a StagedTCState's as
        it is (its network must have this one's tuples and bounds), or a single table's
        MeanTCState's in stage 0 with zeros above (its network must have this one's tuples)."""
        net = self.net
        if state.net.spec.tuples != net.spec.tuples:
            raise ValueError(f"the state's tuples {state.net.spec.tuples} are not this network's "
                             f"{net.spec.tuples}")
        if isinstance(state, MeanTCState):
            self.ea[0].copy_(state.ea)
            return
        if state.net.bounds != net.bounds:
            raise ValueError(f"the state's bounds {state.net.bounds} are not this network's "
                             f"{net.bounds}")
        self.ea.copy_(state.ea)

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back: `ea` under
        the same keys in every subclass, then the subclass's own, with which (and the table and
        the env) a run resumes bit for bit.  `acc` holds nothing between steps and is not
        saved."""
        out = {"tuples": torch.tensor(self.net.spec.tuples, dtype=torch.int64),
               "bounds": torch.tensor(self.net.bounds, dtype=torch.int64), "ea": self.ea}
        out.update({k: torch.tensor(getattr(self, k), dtype=torch.int64) for k in self._SCALARS})
        out.update({name: getattr(self, name) for name in self._TENSORS})
        return out

    def load_state_dict(self, state: dict) -> None:
        tuples = tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist())
        if tuples != self.net.spec.tuples:
            raise ValueError(f"the file's tuples {tuples} are not this network's "
                             f"{self.net.spec.tuples}")
        bounds = tuple(int(b) for b in state["bounds"].tolist())
        if bounds != self.net.bounds:
            raise ValueError(f"the file's bounds {bounds} are not this network's "
                             f"{self.net.bounds}")
        for k in self._SCALARS:
            if int(state[k]) != getattr(self, k):
                raise ValueError(f"the file's {k} {int(state[k])} is not this state's "
                                 f"{getattr(self, k)}")
        for name in ("ea", *self._TENSORS):
            own, t = getattr(self, name), state[name]
            if t.dtype != own.dtype or t.shape != own.shape:
                raise ValueError(f"{name} must be {own.dtype} {tuple(own.shape)}")
        for name in ("ea", *self._TENSORS):
            getattr(self, name).copy_(state[name])

    def save(self, path) -> None:
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, path)


class StagedMeanTCState(StagedTCState):
    """The state of the rule for one StagedNTupleNetwork: `acc` and `ea` of StagedTCState and
    nothing else.  On a GPU device it steps through the library; on the CPU it only holds, saves
    and loads."""

    rate = staticmethod(rate)

    def __init__(self, net: NS.StagedNTupleNetwork):
        if not isinstance(net, NS.StagedNTupleNetwork):  # this rule has a single-table library
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes to "
                            "g2048.ntmeantc.MeanTCState)")
        super().__init__(net)

    @classmethod
    def from_state(cls, state: MeanTCState, net: NS.StagedNTupleNetwork) -> "StagedMeanTCState":
        """The accumulators of a single table in stage 0, zeros above: the counterpart of
        StagedNTupleNetwork.from_network, so a single-table run can continue staged.  `net` must
        have the tuples of the state's network; `ea` is copied to `net`'s device."""
        if not isinstance(state, MeanTCState):
            raise TypeError("state must be a g2048.ntmeantc.MeanTCState")
        st = cls(net)
        st._adopt(state)
        return st

    def meantc_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                    err_out=None):
        """One step of the header, promotion included, on caller-owned state and outputs (no
        allocation); the arguments of StagedNTupleNetwork.td_step."""
        net = self.net
        dev = net._gpu()
        n = NT._step_args("meantc_step", boards, prev, has_prev, actions_out, delta_out, err_out,
                          dev)
        if self.acc.device != dev or self.ea.device != dev:
            raise ValueError(f"acc and ea must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_stagemeantc_step(
                C.byref(net._c), C.byref(net._cs), N.ptr(net.lut), N.ptr(self.acc),
                N.ptr(self.ea), N.ptr(boards), n, N.ptr(prev), N.ptr(has_prev), int(lr_num),
                int(lr_shift), N.ptr(actions_out), N.ptr(delta_out), N.ptr(err_out), dev.index,
                N.stream_of(dev)), "g2048_stagemeantc_step")
        return actions_out, delta_out, err_out

    @classmethod
    def load(cls, path, net: NS.StagedNTupleNetwork) -> "StagedMeanTCState":
        """The accumulators saved at `path`, for `net` (whose tuples and bounds must be the
        file's)."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        st = cls(net)
        st.load_state_dict(state)
        return st


class StagedMeanTCTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the step of this module: the same self-play loop, env, episode log and
    `restart=` keyword, the table moved by StagedMeanTCState.meantc_step.  `lr_shift=None` picks
    default_meantc_lr_shift(net.spec), which depends neither on n_boards nor on the stages.
    `step(k)` enqueues k x (meantc_step, env.step[, restart.apply]) on the current stream with no
    host sync and no allocation."""

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int,
                 state: StagedMeanTCState | None = None, lr_shift: int | None = None, **kw):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes to "
                            "g2048.ntmeantc.MeanTCTrainer)")
        if lr_shift is None:
            lr_shift = default_meantc_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.state = StagedMeanTCState(net) if state is None else state
        if self.state.net is not net:
            raise ValueError("state must be the StagedMeanTCState of this network")

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.state.meantc_step(self.env.board, self.prev, self.has_prev, self.lr_num,
                                   self.lr_shift, self.actions, self.delta, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
