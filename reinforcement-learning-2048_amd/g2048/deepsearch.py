"""The wide expectimax over an n-tuple value network (libg2048_deepsearch.so, C ABI in
include/g2048_deepsearch.h): depths up to 5, one tree spread over many wavefronts.

`g2048.ntsearch` and `g2048.stagesearch` give one wavefront to one board and stop at three player
moves: right for tens of thousands of boards, wrong for playing one game or evaluating a few
hundred.  `expectimax(net, boards, depth, top=...)` runs the same search with the top `top` player
moves (0, 1 or 2) expanded breadth-first into a workspace, every frontier board searched as a root
of its own by the per-wave walk `depth - top` (1..3) moves deep, and the values backed up level by
level (csrc/g2048_deepsearch.hip).  The result is the same int64 as the recursion, bit for bit,
whatever the split; for depth <= 3 it is `ntsearch.expectimax` / `stagesearch.expectimax`
exactly.  `net` is an `NTupleNetwork` or a `StagedNTupleNetwork` (every leaf at its own stage).
`BatchedPlayer(..., ntuple=net, search_depth=d).play("ntuple_deep" | "ntstage_deep")` plays whole
games with it, up to depth 4; this function reaches depth 5.  Values and actions are checked bit
for bit against tests/deepsearch_ref.py.

The module owns one workspace per device, grown on demand up to WORKSPACE_CAP bytes; more boards
than fit are searched in chunks, one call each.  The workspace is not kept across a change of
size, so a call that is to be captured into a graph is run once before the capture.

The binding is this module's own (not in _native.SIGNATURES: libg2048.so's ABI stays as it is).
There is no CPU fallback: a missing library or a non-GPU tensor raises.
"""
from __future__ import annotations

import ctypes as C
import os

import torch

from . import _native as N
from . import ntstage as NS
from . import ntuple as NT

LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libg2048_deepsearch.so")
MAX_DEPTH = 5           # include/g2048_deepsearch.h G2048_DEEPSEARCH_MAX_DEPTH
MAX_TOP = 2             # G2048_DEEPSEARCH_MAX_TOP_PLIES
MAX_SUB = 3             # G2048_DEEPSEARCH_MAX_SUB_DEPTH
INT64_MIN = -(1 << 63)  # the value of an illegal move
SLOT_BYTES = 24         # a 16-byte board and its 8-byte Vmax
PER_BOARD = (0, 128 * SLOT_BYTES, (128 + 128 * 128) * SLOT_BYTES)  # workspace bytes by top
WORKSPACE_CAP = 256 << 20  # bytes of the module's workspace: 87 381 boards at top 1, 677 at top 2

_COMMON = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_uint32, C.c_void_p,
           C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
SIGNATURES = {
    "g2048_deepsearch_workspace_bytes": (C.c_int64, [C.c_int64, C.c_int]),
    "g2048_deepsearch_expectimax": (C.c_int, [C.POINTER(NT._Spec), *_COMMON]),
    "g2048_deepsearch_staged_expectimax": (C.c_int, [C.POINTER(NT._Spec), C.POINTER(NS._Stages),
                                                     *_COMMON]),
    "g2048_deepsearch_last_error": (C.c_char_p, []),
}

_lib = None
_workspace: dict = {}  # device -> u8 tensor


def load() -> C.CDLL:
    """Load libg2048_deepsearch.so and bind its symbols (no GPU needed for this)."""
    global _lib
    if _lib is None:
        _lib = N.bind(LIB_PATH, SIGNATURES)
    return _lib


def check(rc: int, what: str = "g2048_deepsearch") -> None:
    if rc != N.G2048_OK:
        msg = load().g2048_deepsearch_last_error().decode(errors="replace")
        raise N.NativeError(f"{what} failed ({rc}): {msg}")


def legal_tops(depth: int) -> tuple:
    """The splits a depth may take: top in 0..2 with depth - top in 1..3."""
    if not 1 <= int(depth) <= MAX_DEPTH:
        raise ValueError(f"depth must be in [1, {MAX_DEPTH}]")
    return tuple(t for t in range(MAX_TOP + 1) if 1 <= int(depth) - t <= MAX_SUB)


def workspace_bytes(n: int, top: int) -> int:
    """The bytes a call over n boards with `top` expanded plies needs (the library's answer):
    0, 128 * 24 * n or (128 + 16 384) * 24 * n."""
    got = load().g2048_deepsearch_workspace_bytes(int(n), int(top))
    if got < 0:
        raise ValueError(load().g2048_deepsearch_last_error().decode(errors="replace"))
    return got


def default_top(depth: int, n: int) -> int:
    """The split the module takes when the caller names none: per depth the fastest measured at
    each n on an MI355X, the switch points rounded to a power of two (DESIGN 4.21's cost table)."""
    tops = legal_tops(depth)
    if int(n) < 1:
        raise ValueError("n must be positive")
    want = _DEFAULT_TOP[int(depth)](int(n))
    return min(max(want, tops[0]), tops[-1])


# depth -> n -> top, from DESIGN 4.21's cost table (profiles/deepsearch/cost_*.txt).  Depth 2: one
# expanded ply is ahead up to 16 boards and behind from 4 096 on; at 256 the two tuple sets differ,
# each within its rows' min-max.  Depth 3: two plies are ahead for one board, one ply from 16 to
# 4 096 boards, the per-wave walk at 65 536.  Depth 4: two plies up to 4 096 boards, one ply at
# 65 536.  A switch lies at the power of two in the middle of the two sizes around it.
_DEFAULT_TOP = {
    1: lambda n: 0,
    2: lambda n: 1 if n < 64 else 0,
    3: lambda n: 2 if n < 4 else 1 if n < 16384 else 0,
    4: lambda n: 2 if n < 16384 else 1,
    5: lambda n: 2,
}


def chunk_boards(top: int, cap: int = WORKSPACE_CAP) -> int:
    """The boards one call takes so that its workspace stays within `cap` bytes (at least one;
    no limit at top 0, which has no workspace)."""
    if top == 0:
        return N.MAX_BOARDS
    return max(1, int(cap) // PER_BOARD[top])


def chunks(n: int, top: int, cap: int = WORKSPACE_CAP) -> list:
    """[(start, stop)] of the calls that cover n boards."""
    step = chunk_boards(top, cap)
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def _workspace_for(dev, nbytes: int) -> torch.Tensor | None:
    if nbytes == 0:
        return None
    ws = _workspace.get(dev)
    if ws is None or ws.numel() < nbytes:
        _workspace.pop(dev, None)
        del ws
        ws = _workspace[dev] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    return ws


def release_workspace() -> None:
    """Drop the module's workspaces."""
    _workspace.clear()


def expectimax(net, boards: torch.Tensor, depth: int = 4, p4: float = 0.5, top: int | None = None,
               values=True, actions=True, values_out: torch.Tensor | None = None,
               actions_out: torch.Tensor | None = None, workspace: torch.Tensor | None = None):
    """Expectimax over a u8 [n, 16] device tensor of log2 exponents (such as env.board) with the
    table(s) of `net` (an NTupleNetwork or a StagedNTupleNetwork on the same GPU) at the leaves:
    `depth` player moves deep (1..5), chance nodes weighted by p(4) = p4, the top `top` moves
    expanded over many waves (None: default_top(depth, n)).  Returns (actions u8 [n], values i64
    [n, 4]), None for an output not asked for (a given *_out tensor asks for it); an illegal
    move's value is INT64_MIN.  Stream-ordered on the current stream of the network's device, no
    host sync.  `workspace` (a contiguous u8 device tensor, 16-byte aligned) replaces the
    module's own; the boards are chunked to its size."""
    if p4 not in (0.5, 0.1):
        raise ValueError("p4 must be 0.5 (reference, src/board.py:12) or 0.1")
    if not isinstance(net, (NT.NTupleNetwork, NS.StagedNTupleNetwork)):
        raise TypeError("net must be an NTupleNetwork or a StagedNTupleNetwork")
    tops = legal_tops(depth)
    if top is not None and int(top) not in tops:
        raise ValueError(f"top must be one of {tops} at depth {int(depth)} "
                         f"(depth - top in [1, {MAX_SUB}])")
    dev = net._gpu()
    n = NT._boards(boards, dev)
    top = default_top(depth, n) if top is None else int(top)
    vals = (NT._out(values_out, torch.int64, (n, 4), dev)
            if (values or values_out is not None) else None)
    acts = (NT._out(actions_out, torch.uint8, (n,), dev)
            if (actions or actions_out is not None) else None)
    if vals is None and acts is None:
        raise ValueError("ask for the values, the actions or both")
    cap = WORKSPACE_CAP
    if workspace is not None:
        if (workspace.dtype != torch.uint8 or workspace.device != dev
                or not workspace.is_contiguous()):
            raise ValueError(f"workspace must be a contiguous uint8 tensor on {dev}")
        cap = workspace.numel()
        if cap < PER_BOARD[top]:
            raise ValueError(f"workspace holds {cap} bytes, one board at top {top} needs "
                             f"{PER_BOARD[top]}")
    # one call where the workspace allows it: the tensors go in as they are, without a view
    parts = chunks(n, top, cap) if top and n * PER_BOARD[top] > cap else [(0, n)]
    ws = workspace
    if ws is None:
        ws = _workspace_for(dev, (parts[0][1] - parts[0][0]) * PER_BOARD[top])
    whole = len(parts) == 1
    staged = isinstance(net, NS.StagedNTupleNetwork)
    lib = load()
    flags = N.P4_10 if p4 == 0.1 else 0
    with torch.cuda.device(dev):
        for lo, hi in parts:
            tail = (N.ptr(net.lut), N.ptr(boards if whole else boards[lo:hi]), hi - lo,
                    int(depth), top, flags,
                    N.ptr(vals if whole or vals is None else vals[lo:hi]),
                    N.ptr(acts if whole or acts is None else acts[lo:hi]),
                    N.ptr(ws), ws.numel() if ws is not None else 0, dev.index,
                    N.stream_of(dev))
            if staged:
                check(lib.g2048_deepsearch_staged_expectimax(C.byref(net._c), C.byref(net._cs),
                                                             *tail),
                      "g2048_deepsearch_staged_expectimax")
            else:
                check(lib.g2048_deepsearch_expectimax(C.byref(net._c), *tail),
                      "g2048_deepsearch_expectimax")
    return acts, vals
