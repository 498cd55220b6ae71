"""Multi-stage n-tuple value network with weight promotion (libg2048_ntstage.so, C ABI in
include/g2048_ntstage.h).

One table has to value an opening board and a board with a 4096 tile on it.  A multi-stage
network (Wu et al. 2014; Yeh et al. 2016; Jaskowski 2017) gives every stage of the game, by
largest tile, a table of its own: `bounds` (b_0 < b_1 < ...) are exponents, and a board whose
largest exponent reaches k of them reads stage k.  An entry that was never written holds UNSET
(INT32_MIN) and falls through to the stage below; the TD step *promotes* the entries it is about
to move, writing the value they resolve to, so a later stage starts from what the earlier one
learned.  The rule is integer arithmetic (see the header), its result does not depend on the order
in which boards are processed, and it is checked bit for bit against tests/ntstage_ref.py.

  StagedNTupleNetwork(spec, bounds, device)   owns `lut` int32 [S, T, 16^m], all UNSET when fresh:
                    values(), act(), td_step() with NTupleNetwork's signatures, so
                    NTupleTrainer(staged, ...) and BatchedPlayer(..., ntuple=staged).play("ntuple")
                    work as they are; expectimax(), from_network(), resolved(), stage_of(),
                    set_counts(), save() / load()

A staged network is not an NTupleNetwork: the single-table expectimax search
(`play("ntuple_search")`, g2048.ntsearch), TCTrainer and TDLambdaTrainer refuse it.
`resolved(stage)` gives a plain NTupleNetwork of one fixed stage for them.  The search that values
every leaf at its own stage is `expectimax()` (g2048.stagesearch, `play("ntstage_search")`).

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntstage.so")
MAX_STAGES = 8         # include/g2048_ntstage.h G2048_NTSTAGE_MAX_STAGES
MAX_BOUND = 27         # G2048_NTSTAGE_MAX_BOUND
UNSET = -(1 << 31)     # G2048_NTSTAGE_UNSET: "never written"


class _Stages(C.Structure):
    """g2048_ntstage_spec."""
    _fields_ = [("n_stages", C.c_int32), ("bounds", C.c_uint8 * (MAX_STAGES - 1))]


_HEAD = [C.POINTER(NT._Spec), C.POINTER(_Stages)]

SIGNATURES = {
    "g2048_ntstage_lut_entries": (C.c_int64, list(_HEAD)),
    "g2048_ntstage_values": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                               C.c_int, C.c_void_p]),
    "g2048_ntstage_act": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntstage_td_step": (C.c_int, _HEAD + [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p,
                                                C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntstage_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntstage.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntstage") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntstage_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def _c_stages(bounds) -> _Stages:
    s = _Stages(len(bounds) + 1)
    for k, b in enumerate(bounds):
        s.bounds[k] = b
    return s


class StagedNTupleNetwork:
    """S = len(bounds) + 1 tables of one spec: `lut` int32 [S, T, 16^m], filled with UNSET.  On a
    GPU device it evaluates, acts and learns through the library; on the CPU it only holds, saves
    and loads the table."""

    def __init__(self, spec=NT.TUPLES_4x6, bounds=(), device="cuda"):
        self.spec = NT._as_spec(spec)
        bounds = tuple(int(b) for b in bounds)
        if len(bounds) > MAX_STAGES - 1:
            raise ValueError(f"a staged network holds 1..{MAX_STAGES} stages")
        if any(not 0 <= b <= 255 for b in bounds):
            raise ValueError(f"bounds must be exponents in 1..{MAX_BOUND}")
        self.bounds = bounds
        self._c = self.spec._c()
        self._cs = _c_stages(bounds)
        n = load().g2048_ntstage_lut_entries(C.byref(self._c), C.byref(self._cs))
        if n < 0:
            raise ValueError(load().g2048_ntstage_last_error().decode(errors="replace"))
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.device = N.require_gpu(self.device)
        self.lut = torch.full((self.n_stages, self.spec.n_tuples, 16 ** self.spec.n_cells), UNSET,
                              dtype=torch.int32, device=self.device)

    @property
    def n_stages(self) -> int:
        return len(self.bounds) + 1

    def _gpu(self) -> torch.device:
        return N.require_gpu(self.device)

    @classmethod
    def from_network(cls, net: NT.NTupleNetwork, bounds) -> "StagedNTupleNetwork":
        """Stage 0 is a copy of `net.lut`, the other stages are UNSET: every board is valued as
        `net` values it.  (An entry of `net` that is exactly INT32_MIN reads as 0.)"""
        if not isinstance(net, NT.NTupleNetwork):
            raise TypeError("net must be an NTupleNetwork")
        staged = cls(net.spec, bounds, net.device)
        staged.lut[0].copy_(net.lut)
        return staged

    def resolved(self, stage: int) -> NT.NTupleNetwork:
        """A plain NTupleNetwork holding val(stage, ., .): boards of that stage are valued as
        this network values them.  It is a copy; the route to the search with one fixed stage."""
        stage = int(stage)
        if not 0 <= stage < self.n_stages:
            raise ValueError(f"stage must be in [0, {self.n_stages})")
        net = NT.NTupleNetwork(self.spec, self.device)
        out = self.lut[0].clone()
        for s in range(1, stage + 1):
            out = torch.where(self.lut[s] != UNSET, self.lut[s], out)
        net.lut.copy_(torch.where(out != UNSET, out, torch.zeros_like(out)))
        return net

    def stage_of(self, boards: torch.Tensor) -> torch.Tensor:
        """stage(board) int64 [n] for u8 [n, 16] boards (plain torch, on the boards' device)."""
        NT._boards(boards)
        m = boards.max(dim=1).values.to(torch.int64)
        out = torch.zeros_like(m)
        for b in self.bounds:
            out += (m >= b).to(torch.int64)
        return out

    def set_counts(self) -> list:
        """The number of entries that are not UNSET, per stage (host sync)."""
        return [int(x) for x in (self.lut != UNSET).sum(dim=(1, 2)).tolist()]

    def values(self, boards: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """V(board) int64 [n] for u8 [n, 16] boards on the network's device (stream-ordered)."""
        dev = self._gpu()
        n = NT._boards(boards, dev)
        out = NT._out(out, torch.int64, (n,), dev)
        with torch.cuda.device(dev):
            check(load().g2048_ntstage_values(C.byref(self._c), C.byref(self._cs),
                                              N.ptr(self.lut), N.ptr(boards), n, N.ptr(out),
                                              dev.index, N.stream_of(dev)),
                  "g2048_ntstage_values")
        return out

    def act(self, boards: torch.Tensor, q=True, actions=True, after=False,
            q_out=None, actions_out=None, after_out=None):
        """The greedy afterstate policy, as NTupleNetwork.act: (actions u8 [n], q i64 [n, 4],
        after u8 [n, 16]), None for each output not asked for.  Each afterstate is valued at its
        own stage."""
        dev = self._gpu()
        n = NT._boards(boards, dev)
        qs = NT._out(q_out, torch.int64, (n, 4), dev) if (q or q_out is not None) else None
        acts = (NT._out(actions_out, torch.uint8, (n,), dev)
                if (actions or actions_out is not None) else None)
        aft = (NT._out(after_out, torch.uint8, (n, 16), dev)
               if (after or after_out is not None) else None)
        with torch.cuda.device(dev):
            check(load().g2048_ntstage_act(C.byref(self._c), C.byref(self._cs), N.ptr(self.lut),
                                           N.ptr(boards), n, N.ptr(qs), N.ptr(acts), N.ptr(aft),
                                           dev.index, N.stream_of(dev)), "g2048_ntstage_act")
        return acts, qs, aft

    def search(self, boards: torch.Tensor, depth: int = 2, p4: float = 0.5, values=True,
               actions=True, values_out=None, actions_out=None):
        """Not available: g2048.ntsearch reads one table.  `expectimax(...)` is the search over
        this network, every leaf at its own stage; `resolved(stage).search(...)` searches with
        one fixed stage."""
        raise TypeError("the single-table expectimax search takes an NTupleNetwork, not a staged "
                        "network; use expectimax(...) (every leaf at its own stage) or "
                        "resolved(stage).search(...)")

    def expectimax(self, boards: torch.Tensor, depth: int = 2, p4: float = 0.5, values=True,
                   actions=True, values_out=None, actions_out=None):
        """Expectimax `depth` player moves deep with every leaf valued at its own stage
        (g2048.stagesearch.expectimax): (actions u8 [n], values i64 [n, 4]).  Depth 1 is act().
        The table is only read: nothing is promoted."""
        from . import stagesearch

        return stagesearch.expectimax(self, boards, depth, p4, values, actions, values_out,
                                      actions_out)

    def deep_search(self, boards: torch.Tensor, depth: int = 4, p4: float = 0.5, top=None,
                    values=True, actions=True, values_out=None, actions_out=None):
        """The same search 1..5 moves deep with the top `top` moves spread over many waves
        (g2048.deepsearch.expectimax), every leaf at its own stage: (actions u8 [n], values i64
        [n, 4]).  The table is only read."""
        from . import deepsearch

        return deepsearch.expectimax(self, boards, depth, p4, top, values, actions, values_out,
                                     actions_out)

    def play_steps(self, env, k: int, depth: int = 1, fin=None, result=None) -> None:
        """k moves of the depth-`depth` policy of these tables on every board of `env`, inside
        one launch (g2048.ntplay.steps), every leaf at its own stage.  The table is only read."""
        from . import ntplay

        ntplay.steps(self, env, k, depth, fin, result)

    def td_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                err_out=None):
        """One TD(0) step of the header, promotion included, on caller-owned state and outputs
        (no allocation)."""
        dev = self._gpu()
        n = NT._step_args("td_step", boards, prev, has_prev, actions_out, delta_out, err_out, dev)
        with torch.cuda.device(dev):
            check(load().g2048_ntstage_td_step(
                C.byref(self._c), C.byref(self._cs), N.ptr(self.lut), N.ptr(boards), n,
                N.ptr(prev), N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_ntstage_td_step")
        return actions_out, delta_out, err_out

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back."""
        return {"tuples": torch.tensor(self.spec.tuples, dtype=torch.int64),
                "bounds": torch.tensor(self.bounds, dtype=torch.int64), "lut": self.lut}

    def load_state_dict(self, state: dict) -> None:
        tuples = tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist())
        if tuples != self.spec.tuples:
            raise ValueError(f"the file's tuples {tuples} are not this network's "
                             f"{self.spec.tuples}")
        bounds = tuple(int(b) for b in state["bounds"].tolist())
        if bounds != self.bounds:
            raise ValueError(f"the file's bounds {bounds} are not this network's {self.bounds}")
        lut = state["lut"]
        if lut.dtype != torch.int32 or lut.shape != self.lut.shape:
            raise ValueError(f"lut must be int32 {tuple(self.lut.shape)}")
        self.lut.copy_(lut)

    def save(self, path) -> None:
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, device="cuda") -> "StagedNTupleNetwork":
        state = torch.load(path, map_location="cpu", weights_only=True)
        net = cls(tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist()),
                  tuple(int(b) for b in state["bounds"].tolist()), device)
        net.load_state_dict(state)
        return net
