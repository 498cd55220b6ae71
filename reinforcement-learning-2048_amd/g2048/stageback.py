"""Backward episode learning on the staged batch-mean temporal-coherence rule for the multi-stage
n-tuple value network (libg2048_stageback.so, C ABI in include/g2048_stageback.h).

Every other learner here is forward and online: an afterstate is updated against its successor in
the step that produces the successor, so what the terminal position teaches moves one step towards
the start of the game per later visit.  This module is backward learning (Matsuzaki 2017, the
paper `RestartPool` takes its restarts from): a board records its episode while it plays it, and
once the episode has ended it is learned from its last afterstate to its first, one afterstate per
step, each against the successor that was updated the step before -- while the board already plays
and records its next episode.  A replaying board makes one set of table hits per step, and every
hit stays one sample of `StagedMeanTCTrainer`'s batch mean.  Like the other learners the rule is
defined in integer arithmetic (see the header), its result does not depend on any order, a whole
run is reproducible bit for bit and is checked bit for bit against tests/stageback_ref.py.

  BackwardState(net, n_boards, horizon=4096)
                        owns `acc` and `ea` (as StagedMeanTCState) and the trajectory: `traj` u8
                        [n, 2, L, 16], `gain` i32 [n, 2, L], `cur` u8 [n] and the counters `rec`,
                        `rep_n`, `rep_k` (u32 [n], held as int32 tensors): step(), reset(),
                        rate(), save() / load() of `ea` and the trajectory, from_state() of a
                        StagedMeanTCState or a single table's MeanTCState
  BackwardTrainer       NTupleTrainer with this step: k x (step, env.step[, restart.apply]), no
                        host sync; the default rate is
                        g2048.ntmeantc.default_meantc_lr_shift(spec)

`horizon` afterstates of an episode are kept, 48 bytes per board each: a longer episode is
learned over its last `horizon`.  `StagedNTupleNetwork` only; a single `NTupleNetwork` goes
through `StagedNTupleNetwork.from_network(net, ())`.  The players need nothing new:
`play("ntuple")` and `play("ntstage_search")` read the same table.  The binding is this module's
own (not in _native.SIGNATURES).  There is no CPU fallback: a missing library or a non-GPU tensor
raises.
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

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_stageback.so")
MAX_HORIZON = 1 << 20     # include/g2048_stageback.h G2048_STAGEBACK_MAX_HORIZON
MAX_SLOTS = 1 << 31       # G2048_STAGEBACK_MAX_SLOTS: the bound of n_boards * horizon
RATE_BITS = 16            # G2048_STAGEBACK_RATE_BITS
MAX_A = (1 << 62) - 1     # G2048_STAGEBACK_MAX_A

_HEAD = [C.POINTER(NT._Spec), C.POINTER(NS._Stages)]

SIGNATURES = {
    "g2048_stageback_rate": (C.c_int32, [C.c_int64, C.c_int64]),
    "g2048_stageback_acc_bytes": (C.c_int64, list(_HEAD)),
    "g2048_stageback_traj_bytes": (C.c_int64, [C.c_int64, C.c_int32]),
    "g2048_stageback_step": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                               C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                               C.c_void_p]),
    "g2048_stageback_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_stageback.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_stageback") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_stageback_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


rate, acc_bytes = bound_rate_and_acc_bytes(load, "stageback")


def _check_horizon(n_boards: int, horizon: int) -> None:
    if not 1 <= n_boards <= N.MAX_BOARDS:
        raise ValueError(f"n_boards must be in [1, {N.MAX_BOARDS}]")
    if not 1 <= horizon <= MAX_HORIZON:
        raise ValueError(f"horizon must be in [1, {MAX_HORIZON}]")
    if n_boards * horizon > MAX_SLOTS:
        raise ValueError(f"n_boards * horizon must not exceed {MAX_SLOTS}")


def traj_bytes(n_boards: int, horizon: int) -> int:
    """Bytes of `traj` for a board count and a horizon, 32 n L; `gain` takes a quarter of it."""
    n_boards, horizon = int(n_boards), int(horizon)
    _check_horizon(n_boards, horizon)
    r = load().g2048_stageback_traj_bytes(n_boards, horizon)
    if r < 0:
        raise ValueError(load().g2048_stageback_last_error().decode(errors="replace"))
    return int(r)


_TRAJ = ("traj", "gain", "cur", "rec", "rep_n", "rep_k")


class BackwardState(StagedTCState):
    """The state of the rule for one StagedNTupleNetwork and `n_boards` boards, on the network's
    device: the workspace `acc` and the accumulators `ea` of StagedTCState, and per board two
    buffers of `horizon` afterstates, `traj` u8 [n, 2, L, 16] with the gains `gain` i32 [n, 2, L],
    the buffer being recorded `cur` u8 [n] and the counters `rec`, `rep_n`, `rep_k` [n] -- the
    header's u32, held in int32 tensors (torch has no arithmetic on uint32; a count above 2^31
    reads as negative) -- all zero when fresh.  The trajectory holds episodes not yet learned, so
    it is saved with `ea`.  On a GPU device it steps through the library; on the CPU it only
    holds, saves and loads."""

    _TENSORS = _TRAJ
    rate = staticmethod(rate)

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int, horizon: int = 4096):
        super().__init__(net)
        self.n, self.horizon = int(n_boards), int(horizon)
        _check_horizon(self.n, self.horizon)
        kw = dict(device=net.device)
        self.traj = torch.zeros((self.n, 2, self.horizon, 16), dtype=torch.uint8, **kw)
        self.gain = torch.zeros((self.n, 2, self.horizon), dtype=torch.int32, **kw)
        self.cur = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.rec = torch.zeros(self.n, dtype=torch.int32, **kw)
        self.rep_n = torch.zeros(self.n, dtype=torch.int32, **kw)
        self.rep_k = torch.zeros(self.n, dtype=torch.int32, **kw)

    @classmethod
    def from_state(cls, state, net: NS.StagedNTupleNetwork, n_boards: int,
                   horizon: int = 4096) -> "BackwardState":
        """A fresh trajectory over the accumulators of a run under another rule: a
        StagedMeanTCState's `ea` as it is (`net` must have its tuples and bounds), or a single
        table's MeanTCState's in stage 0 with zeros above (`net` must have its tuples).  `ea` is
        copied to `net`'s device."""
        if not isinstance(state, (StagedMeanTCState, MeanTCState)):
            raise TypeError("state must be a StagedMeanTCState or a g2048.ntmeantc.MeanTCState")
        st = cls(net, n_boards, horizon)
        st._adopt(state)
        return st

    def reset(self) -> None:
        """Forget every recorded and every replaying episode (stream-ordered): the fresh
        trajectory.  `ea` is kept.  Replacing the table does not require this (consequence 4 of
        the header)."""
        for name in _TRAJ:
            getattr(self, name).zero_()

    def step(self, boards, lr_num, lr_shift, actions_out, delta_out, x_out, replay_out,
             err_out=None):
        """One call of the header on this state and caller-owned outputs (no allocation):
        actions_out u8 [n], delta_out i32 [n], x_out u8 [n, 16], replay_out u8 [n], err_out i64
        [n] or None."""
        net = self.net
        dev = net._gpu()
        n = NT._boards(boards, dev)
        if n != self.n:
            raise ValueError(f"boards must be uint8 [{self.n}, 16]")
        if actions_out is None or delta_out is None or x_out is None or replay_out is None:
            raise ValueError("step needs actions_out, delta_out, x_out and replay_out")
        NT._out(actions_out, torch.uint8, (n,), dev)
        NT._out(delta_out, torch.int32, (n,), dev)
        NT._out(x_out, torch.uint8, (n, 16), dev)
        NT._out(replay_out, torch.uint8, (n,), dev)
        if err_out is not None:
            NT._out(err_out, torch.int64, (n,), dev)
        if not 0 <= int(lr_num) <= NT.MAX_LR_NUM or not 0 <= int(lr_shift) <= NT.MAX_LR_SHIFT:
            raise ValueError(f"lr_num must be in [0, {NT.MAX_LR_NUM}] and lr_shift in "
                             f"[0, {NT.MAX_LR_SHIFT}]")
        if any(getattr(self, name).device != dev for name in ("acc", "ea", *_TRAJ)):
            raise ValueError(f"acc, ea and the trajectory must be on {dev}")
        with torch.cuda.device(dev):
            check(load().g2048_stageback_step(
                C.byref(net._c), C.byref(net._cs), N.ptr(net.lut), N.ptr(self.acc),
                N.ptr(self.ea), N.ptr(boards), n, N.ptr(self.traj), N.ptr(self.gain),
                N.ptr(self.cur), N.ptr(self.rec), N.ptr(self.rep_n), N.ptr(self.rep_k),
                self.horizon, int(lr_num), int(lr_shift), N.ptr(actions_out), N.ptr(delta_out),
                N.ptr(x_out), N.ptr(replay_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_stageback_step")
        return actions_out, delta_out, err_out

    @classmethod
    def load(cls, path, net: NS.StagedNTupleNetwork) -> "BackwardState":
        """The state saved at `path`, for `net` (whose tuples and bounds must be the file's); the
        board count and the horizon are the file's."""
        state = torch.load(path, map_location="cpu", weights_only=True)
        n, _, L = state["gain"].shape
        st = cls(net, n, L)
        st.load_state_dict(state)
        return st


class BackwardTrainer(NT.NTupleTrainer):
    """NTupleTrainer with the step of this module: the same self-play loop, env, episode log and
    `restart=` keyword, the table moved by BackwardState.step.  `lr_shift=None` picks
    default_meantc_lr_shift(net.spec).  `step(k)` enqueues k x (step, env.step[, restart.apply])
    on the current stream with no host sync and no allocation.  The base class's `prev` /
    `has_prev` are not used: the afterstates live in `self.state`; `self.x` u8 [n, 16] and
    `self.replays` u8 [n] hold the afterstate each board learned in the last step and whether it
    learned one."""

    def __init__(self, net: NS.StagedNTupleNetwork, n_boards: int, horizon: int = 4096,
                 state: BackwardState | None = None, lr_shift: int | None = None, **kw):
        if not isinstance(net, NS.StagedNTupleNetwork):
            raise TypeError("net must be a StagedNTupleNetwork (a single table goes through "
                            "StagedNTupleNetwork.from_network(net, ()))")
        if state is None:  # validates n_boards and horizon before the env exists
            state = BackwardState(net, n_boards, horizon)
        elif not isinstance(state, BackwardState) or state.net is not net:
            raise ValueError("state must be the BackwardState of this network")
        elif state.n != int(n_boards):
            raise ValueError(f"state must hold {int(n_boards)} boards")
        if lr_shift is None:
            lr_shift = default_meantc_lr_shift(net.spec)
        super().__init__(net, n_boards, lr_shift=lr_shift, **kw)
        self.state = state
        self.x = torch.zeros((self.n, 16), dtype=torch.uint8, device=net.device)
        self.replays = torch.zeros(self.n, dtype=torch.uint8, device=net.device)

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.state.step(self.env.board, self.lr_num, self.lr_shift, self.actions, self.delta,
                            self.x, self.replays, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)
