"""N-tuple value network (libg2048_ntuple.so, C ABI in include/g2048_ntuple.h): the learner that
gets good at 2048 (Szubert and Jaskowski, CIG 2014).

The value of a board is a sum of table lookups over small groups of cells, shared across the 8
board symmetries; it is trained by afterstate TD(0) during self-play.  Everything is defined in
integer arithmetic (see the header) and the table update uses 32-bit integer atomic adds, which
commute: a whole training run is reproducible bit for bit and is checked bit for bit against
tests/ntuple_ref.py.

  NTupleSpec        the tuples (TUPLES_4x6, TUPLES_2x4 or your own)
  NTupleNetwork     owns the int32 table on the device: values(), act(), save() / load()
  NTupleTrainer     self-play: k x (td_step, env.step) with no host sync, episodes from the log
  BatchedPlayer(..., ntuple=net).play("ntuple")   whole games under the greedy afterstate policy
  NTupleNetwork.search / play("ntuple_search")    expectimax with the table at the leaves
                                                  (g2048.ntsearch, a library of its own)
  g2048.ntstage.StagedNTupleNetwork   one table per stage of the game (by largest tile): it takes
                                      NTupleNetwork's place in NTupleTrainer and play("ntuple")
  g2048.ntrestart.RestartPool   per-board snapshots by largest tile; NTupleTrainer(...,
                                restart=pool) restarts some episodes from them (a carousel)

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass

import torch

from . import _native as N

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_ntuple.so")
MAX_TUPLES, MAX_CELLS = 8, 6  # G2048_NTUPLE_MAX_TUPLES / _MAX_CELLS
FRAC_BITS = 10                # G2048_NTUPLE_FRAC_BITS: table values are merge score << 10
MAX_LR_NUM, MAX_LR_SHIFT = 1 << 16, 31
INT64_MIN = -(1 << 63)        # the q of an illegal move

# the 4 x 6-tuple set of Szubert and Jaskowski (256 MiB of int32) and a small 2 x 4-tuple set
# (512 KiB) that learns at about two thirds of its strength
TUPLES_4x6 = ((0, 1, 2, 3, 4, 5), (4, 5, 6, 7, 8, 9), (0, 1, 2, 4, 5, 6), (4, 5, 6, 8, 9, 10))
TUPLES_2x4 = ((0, 1, 2, 3), (0, 1, 4, 5))


class _Spec(C.Structure):
    """g2048_ntuple_spec."""
    _fields_ = [("n_tuples", C.c_int32), ("n_cells", C.c_int32),
                ("cells", (C.c_uint8 * MAX_CELLS) * MAX_TUPLES)]


_EXPANDED = ((C.c_uint8 * MAX_CELLS) * MAX_TUPLES) * 8

SIGNATURES = {
    "g2048_ntuple_lut_entries": (C.c_int64, [C.POINTER(_Spec)]),
    "g2048_ntuple_expand": (C.c_int, [C.POINTER(_Spec), C.POINTER(_EXPANDED)]),
    "g2048_ntuple_values": (C.c_int, [C.POINTER(_Spec), C.c_void_p, C.c_void_p, C.c_int64,
                                      C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntuple_act": (C.c_int, [C.POINTER(_Spec), C.c_void_p, C.c_void_p, C.c_int64,
                                   C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntuple_td_step": (C.c_int, [C.POINTER(_Spec), C.c_void_p, C.c_void_p, C.c_int64,
                                       C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]),
    "g2048_ntuple_last_error": (C.c_char_p, []),
}

_lib = None


def load() -> C.CDLL:
    """Load libg2048_ntuple.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_ntuple") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_ntuple_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


@dataclass(frozen=True)
class NTupleSpec:
    """T tuples of m board cells each (1 <= T <= 8, 1 <= m <= 6, cells 0..15, distinct within a
    tuple); the library validates it."""
    tuples: tuple = TUPLES_4x6

    def __post_init__(self):
        tuples = tuple(tuple(int(c) for c in t) for t in self.tuples)
        object.__setattr__(self, "tuples", tuples)
        if not 1 <= len(tuples) <= MAX_TUPLES:
            raise ValueError(f"a spec holds 1..{MAX_TUPLES} tuples")
        m = len(tuples[0])
        if not 1 <= m <= MAX_CELLS or any(len(t) != m for t in tuples):
            raise ValueError(f"every tuple must have the same 1..{MAX_CELLS} cells")
        if any(not 0 <= c <= 255 for t in tuples for c in t):
            raise ValueError("cells must be 0..15")
        n = load().g2048_ntuple_lut_entries(C.byref(self._c()))
        if n < 0:
            raise ValueError(load().g2048_ntuple_last_error().decode(errors="replace"))

    @property
    def n_tuples(self) -> int:
        return len(self.tuples)

    @property
    def n_cells(self) -> int:
        return len(self.tuples[0])

    @property
    def lut_entries(self) -> int:
        return int(load().g2048_ntuple_lut_entries(C.byref(self._c())))

    def _c(self) -> _Spec:
        s = _Spec(len(self.tuples), len(self.tuples[0]))
        for t, cells in enumerate(self.tuples):
            for k, c in enumerate(cells):
                s.cells[t][k] = c
        return s

    def expand(self):
        """[g][t][k]: the board cell that symmetry g reads for position k of tuple t."""
        out = _EXPANDED()
        check(load().g2048_ntuple_expand(C.byref(self._c()), C.byref(out)), "g2048_ntuple_expand")
        return [[[int(out[g][t][k]) for k in range(self.n_cells)] for t in range(self.n_tuples)]
                for g in range(8)]


def _as_spec(spec) -> NTupleSpec:
    return spec if isinstance(spec, NTupleSpec) else NTupleSpec(tuple(spec))


def _boards(boards, dev=None) -> int:
    if not isinstance(boards, torch.Tensor):
        raise TypeError("boards must be a torch tensor on the GPU")
    if boards.dtype != torch.uint8 or boards.dim() != 2 or boards.shape[1] != 16:
        raise ValueError("boards must be uint8 [n, 16]")
    if not boards.is_contiguous():
        raise ValueError("boards must be contiguous")
    if dev is not None and boards.device != dev:
        raise ValueError(f"boards must be on {dev}")
    if boards.shape[0] < 1:
        raise ValueError("boards is empty")
    return boards.shape[0]


def _out(t, dtype, shape, dev):
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.dtype != dtype or tuple(t.shape) != shape or t.device != dev or not t.is_contiguous():
        raise ValueError(f"output must be a contiguous {dtype} {shape} tensor on {dev}")
    return t


def _step_args(who, boards, prev, has_prev, actions_out, delta_out, err_out, dev) -> int:
    """The tensors td_step and tc_step (`who`) share, validated; returns n."""
    n = _boards(boards, dev)
    _boards(prev, dev)
    for t, dt, shape in ((prev, torch.uint8, (n, 16)), (has_prev, torch.uint8, (n,)),
                         (actions_out, torch.uint8, (n,)), (delta_out, torch.int32, (n,))):
        if t is None:
            raise ValueError(f"{who} needs prev, has_prev, actions_out and delta_out")
        _out(t, dt, shape, dev)
    if err_out is not None:
        _out(err_out, torch.int64, (n,), dev)
    return n


class NTupleNetwork:
    """The table of one spec: `lut` int32 [T, 16^m], zero-initialised.  On a GPU device it
    evaluates and acts through the library; on the CPU it only holds, saves and loads the table."""

    def __init__(self, spec=TUPLES_4x6, device="cuda"):
        self.spec = _as_spec(spec)
        self.device = torch.device(device)
        if self.device.type == "cuda":
            self.device = N.require_gpu(self.device)
        self._c = self.spec._c()
        self.lut = torch.zeros((self.spec.n_tuples, 16 ** self.spec.n_cells), dtype=torch.int32,
                               device=self.device)

    def _gpu(self) -> torch.device:
        return N.require_gpu(self.device)

    def values(self, boards: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
        """V(board) int64 [n] for u8 [n, 16] boards on the network's device (stream-ordered)."""
        dev = self._gpu()
        n = _boards(boards, dev)
        out = _out(out, torch.int64, (n,), dev)
        with torch.cuda.device(dev):
            check(load().g2048_ntuple_values(C.byref(self._c), N.ptr(self.lut), N.ptr(boards), n,
                                             N.ptr(out), dev.index, N.stream_of(dev)),
                  "g2048_ntuple_values")
        return out

    def act(self, boards: torch.Tensor, q=True, actions=True, after=False,
            q_out=None, actions_out=None, after_out=None):
        """The greedy afterstate policy: returns (actions u8 [n], q i64 [n, 4], after u8 [n, 16]),
        None for each output not asked for (a given *_out tensor asks for it).  An illegal
        move's q is INT64_MIN; with no legal move the action is 0 and after = board."""
        dev = self._gpu()
        n = _boards(boards, dev)
        qs = _out(q_out, torch.int64, (n, 4), dev) if (q or q_out is not None) else None
        acts = (_out(actions_out, torch.uint8, (n,), dev)
                if (actions or actions_out is not None) else None)
        aft = (_out(after_out, torch.uint8, (n, 16), dev)
               if (after or after_out is not None) else None)
        with torch.cuda.device(dev):
            check(load().g2048_ntuple_act(C.byref(self._c), N.ptr(self.lut), N.ptr(boards), n,
                                          N.ptr(qs), N.ptr(acts), N.ptr(aft), dev.index,
                                          N.stream_of(dev)), "g2048_ntuple_act")
        return acts, qs, aft

    def search(self, boards: torch.Tensor, depth: int = 2, p4: float = 0.5, values=True,
               actions=True, values_out=None, actions_out=None):
        """Expectimax `depth` player moves deep with this table at the leaves
        (g2048.ntsearch.expectimax): (actions u8 [n], values i64 [n, 4]).  Depth 1 is act()."""
        from . import ntsearch

        return ntsearch.expectimax(self, boards, depth, p4, values, actions, values_out,
                                   actions_out)

    def deep_search(self, boards: torch.Tensor, depth: int = 4, p4: float = 0.5, top=None,
                    values=True, actions=True, values_out=None, actions_out=None):
        """The same search 1..5 moves deep with the top `top` moves spread over many waves
        (g2048.deepsearch.expectimax): (actions u8 [n], values i64 [n, 4])."""
        from . import deepsearch

        return deepsearch.expectimax(self, boards, depth, p4, top, values, actions, values_out,
                                     actions_out)

    def play_steps(self, env, k: int, depth: int = 1, fin=None, result=None) -> None:
        """k moves of the depth-`depth` policy of this table on every board of `env`, inside one
        launch (g2048.ntplay.steps)."""
        from . import ntplay

        ntplay.steps(self, env, k, depth, fin, result)

    def td_step(self, boards, prev, has_prev, lr_num, lr_shift, actions_out, delta_out,
                err_out=None):
        """One TD(0) step of the header on caller-owned state and outputs (no allocation)."""
        dev = self._gpu()
        n = _step_args("td_step", boards, prev, has_prev, actions_out, delta_out, err_out, dev)
        with torch.cuda.device(dev):
            check(load().g2048_ntuple_td_step(
                C.byref(self._c), N.ptr(self.lut), N.ptr(boards), n, N.ptr(prev),
                N.ptr(has_prev), int(lr_num), int(lr_shift), N.ptr(actions_out),
                N.ptr(delta_out), N.ptr(err_out), dev.index, N.stream_of(dev)),
                "g2048_ntuple_td_step")
        return actions_out, delta_out, err_out

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """Plain tensors only, so torch.load(weights_only=True) reads the file back."""
        return {"tuples": torch.tensor(self.spec.tuples, dtype=torch.int64), "lut": self.lut}

    def load_state_dict(self, state: dict) -> None:
        tuples = tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist())
        if tuples != self.spec.tuples:
            raise ValueError(f"the file's tuples {tuples} are not this network's "
                             f"{self.spec.tuples}")
        lut = state["lut"]
        if lut.dtype != torch.int32 or lut.shape != self.lut.shape:
            raise ValueError(f"lut must be int32 {tuple(self.lut.shape)}")
        self.lut.copy_(lut)

    def save(self, path) -> None:
        torch.save({k: v.cpu() for k, v in self.state_dict().items()}, path)

    @classmethod
    def load(cls, path, device="cuda") -> "NTupleNetwork":
        state = torch.load(path, map_location="cpu", weights_only=True)
        net = cls(tuple(tuple(int(c) for c in t) for t in state["tuples"].tolist()), device)
        net.load_state_dict(state)
        return net


def default_lr_shift(n_boards: int) -> int:
    """ceil(log2(n_boards)) + 2.  The boards of a lock-step batch all walk through the same
    early-game afterstates, so one step adds up to n_boards deltas into one entry and the
    effective rate on it is n_boards * lr.  Keeping n_boards * lr_num / 2^lr_shift at 1/4 keeps
    that sum a contraction; the CPU prototype learned with exactly this setting (1 / 2^10 at 256
    boards) and ran its entries to the edge of int32 at 2^-7."""
    return max(int(n_boards) - 1, 0).bit_length() + 2


class NTupleTrainer:
    """Afterstate TD(0) self-play: n_boards auto-resetting boards, every step the greedy move of
    the current table, the table moved toward reward + V(next afterstate).  `step(k)` enqueues
    k x (td_step, env.step) on the current stream with no host sync; `episodes()` reads the
    finished episodes from the env's device log.  With `restart` (a g2048.ntrestart.RestartPool
    of n_boards boards on the network's device) every iteration ends with `restart.apply`, one
    more launch; this class and its subclasses share the keyword."""

    def __init__(self, net: NTupleNetwork, n_boards: int, seed: int = 0x2048, p4: float = 0.5,
                 lr_num: int = 1, lr_shift: int | None = None, log_slots: int = 8, restart=None):
        self.net = net
        self.n = int(n_boards)
        self.lr_num = int(lr_num)
        self.lr_shift = default_lr_shift(self.n) if lr_shift is None else int(lr_shift)
        if not 0 <= self.lr_num <= MAX_LR_NUM or not 0 <= self.lr_shift <= MAX_LR_SHIFT:
            raise ValueError(f"lr_num must be in [0, {MAX_LR_NUM}] and lr_shift in "
                             f"[0, {MAX_LR_SHIFT}]")
        from .env import VecEnv2048

        if restart is not None:
            from .ntrestart import RestartPool

            if not isinstance(restart, RestartPool):
                raise TypeError("restart must be a RestartPool or None")
            if restart.n != self.n or restart.device != net.device:
                raise ValueError(f"restart must hold {self.n} boards on {net.device}")
        self.restart = restart
        dev = net._gpu()
        self.env = VecEnv2048(self.n, seed=seed, device=dev, p4=p4)
        self.log = self.env.attach_episode_log(log_slots)
        kw = dict(device=dev)
        self.prev = torch.zeros((self.n, 16), dtype=torch.uint8, **kw)
        self.has_prev = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.actions = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.delta = torch.zeros(self.n, dtype=torch.int32, **kw)
        self.err = torch.zeros(self.n, dtype=torch.int64, **kw)
        self.reward = torch.zeros(self.n, dtype=torch.int32, **kw)
        self.done = torch.zeros(self.n, dtype=torch.uint8, **kw)
        self.legal = torch.zeros(self.n, dtype=torch.uint8, **kw)

    def step(self, k: int = 1) -> None:
        for _ in range(int(k)):
            self.net.td_step(self.env.board, self.prev, self.has_prev, self.lr_num, self.lr_shift,
                             self.actions, self.delta, self.err)
            self.env.step(self.actions, reward=self.reward, done=self.done, legal=self.legal)
            if self.restart is not None:
                self.restart.apply(self.env, self.done)

    def episodes(self, strict: bool = True) -> dict:
        """Records of the episodes finished since the last call (EpisodeLog.read; host sync)."""
        return self.log.read(strict)
