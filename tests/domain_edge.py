"""Inputs at the edges of the domains the n-tuple headers declare (include/g2048_ntuple.h and the
headers built on it), shared by tests/test_domain_edge.py (CPU: the premises, on the Python
references alone) and tests/test_domain_edge_gpu.py (the kernels against those references).

    tables      table(name, shape, device, seed): "full", "max", "min", "edge_unset" as torch
                int32; wide_table / wide_staged / flat_table as numpy (the learning cases, so that
                the CPU file proves the very tables the GPU file runs)
    specs       SPECS; SMALL names the ones that may sit beside an ea or acc; STAGE_BOUNDS
    boards      high_boards(rng, n, cap), low_boards(rng, n), distinct_prev(tuples, n, seed)
    caps        CAP_LEARN = 27; SEARCH_CAP[depth] for the two per-wave searches; DEEP_CAP for the
                wide search, whose header declares 22 at every depth
    solved rows solved_rows(tuples, lr, seed): (prev, board, entries) whose delta is known exactly
    InDomain    the guard around a reference step: it fails the test when the *reference* leaves
                the domain (a wrapped delta or entry, a staged entry landing on UNSET, |E| > A,
                A >= 2^62).  No case may trip it: out-of-domain behaviour is not tested.
    cases       learning_cases(): every learning case of the GPU file, as (id, lib, build)

Everything is generated from seeds.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass, field

import numpy as np

import ntlambda_ref as LR
import ntmean_ref as MR
import ntmeantc_ref as MTR
import ntstage_ref as SR
import nttc_ref as TR
import ntuple_ref as NR
import stagemean_ref as SMR
import stagemeantc_ref as SMTR

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1
UNSET = SR.UNSET
F = NR.F
T8M3 = tuple((t, t + 5, (t + 11) % 16) for t in range(8))
# 8 tuples of 4 distinct cells: T = 8 with room for boards of pairwise distinct hits (the 4096
# entries per tuple of the 8x3 set do not hold the solved rows)
T8M4 = tuple((t, (t + 5) % 16, (t + 11) % 16, (t + 14) % 16) for t in range(8))
SPECS = {"1x1": ((0,),), "2x4": NR.TUPLES_2x4, "8x3": T8M3, "4x6": NR.TUPLES_4x6, "8x4": T8M4}
SMALL = ("1x1", "2x4", "8x3")       # 4x6 (256 MiB) never has an ea or an acc beside it
STAGE_BOUNDS = ((16, 25), (27,))    # above the index clamp: stage and index disagree on a 17
CAP_LEARN = 27                      # values, act and learning steps: boards and prev
SEARCH_CAP = {1: 24, 2: 24, 3: 24, 4: 23, 5: 22}  # depth -> root exponents, so the tree stays <= 27
DEEP_CAP = 22                       # G2048_DEEPSEARCH_MAX_EXPONENT, declared for every depth
HEADROOM = 1 << 27                  # what the wide tables leave free at both ends of int32
ROW_24 = (24, 24, 23, 23, 22, 22, 0, 0, 1, 2, 1, 2, 0, 0, 1, 1)
COLOUR = (np.arange(16) // 4 + np.arange(16) % 4) % 2
DELTAS = (INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX)
FLAT_LIBS = ("td", "tc", "lam", "mean", "meantc")
STAGED_LIBS = ("stage", "stagemean", "stagemeantc")
LIBS = FLAT_LIBS + STAGED_LIBS
TC_LIBS = ("tc", "meantc", "stagemeantc")
SUM_LIBS = ("td", "tc", "lam", "stage")  # every hit adds its own delta: collisions pile up
LRS = ((1, 31), (1 << 16, 31), (1, 0), (1 << 16, 16), (0, 0))


# ------------------------------------------------------------------ tables
def table(name, shape, device="cpu", seed=0):
    """A torch int32 table [T, E] or, staged, [S, T, E].  "full": uniform over [INT32_MIN + 1,
    INT32_MAX] from a generator of `device`; "max": INT32_MAX; "min": INT32_MIN, staged
    INT32_MIN + 1 (INT32_MIN is UNSET there); "edge_unset" (staged): stage 0 full, the stages
    above half UNSET and half INT32_MIN + 1."""
    import torch

    staged = len(shape) == 3
    if name == "max":
        return torch.full(shape, INT32_MAX, dtype=torch.int32, device=device)
    if name == "min":
        return torch.full(shape, INT32_MIN + (1 if staged else 0), dtype=torch.int32, device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(shape, dtype=torch.int32, device=device)

    def fill(rows):  # one [E] row at a time: the int64 draw of a 4x6 row is 128 MiB
        for row in rows.view(-1, shape[-1]):
            row.copy_(torch.randint(INT32_MIN + 1, INT32_MAX + 1, row.shape, generator=g,
                                    device=device, dtype=torch.int64))

    if name == "full":
        fill(out)
    elif name == "edge_unset":
        assert staged and shape[0] > 1
        fill(out[0])
        unset = torch.rand(out[1:].shape, generator=g, device=device) < 0.5
        out[1:] = torch.where(unset, UNSET, INT32_MIN + 1).to(torch.int32)
    else:
        raise ValueError(name)
    return out


def wide_table(shape, seed):
    """numpy int32, uniform within +-(2^31 - 2^27): a value of 8 T entries needs up to 38 bits and
    an entry may still receive 2^27 in either direction."""
    rng = np.random.default_rng(seed)
    return rng.integers(INT32_MIN + HEADROOM, INT32_MAX - HEADROOM, shape, endpoint=True,
                        dtype=np.int64).astype(np.int32)


def wide_staged(shape, seed, edge=False):
    """Stage 0 wide, the stages above half UNSET; the other half wide or, with `edge`,
    INT32_MIN + 1 (the smallest value an entry may hold, next to UNSETs in the same burst)."""
    rng = np.random.default_rng(seed + 1)
    out = wide_table(shape, seed)
    if edge:
        out[1:] = INT32_MIN + 1
    out[1:][rng.random(out[1:].shape) < 0.5] = UNSET
    return out


def flat_table(shape, seed, level=1 << 30, noise=1 << 10):
    """Every entry within `noise` of `level`: V is about 8 T * level (2^36 at T = 8) on every
    board, so the error of a non-terminal low board is small although no value fits 32 bits."""
    rng = np.random.default_rng(seed)
    return (level + rng.integers(-noise, noise, shape, endpoint=True)).astype(np.int32)


def lut_shape(tuples, bounds=None):
    flat = (len(tuples), 16 ** len(tuples[0]))
    return flat if bounds is None else (len(bounds) + 1, *flat)


# ------------------------------------------------------------------ boards
def checker(a, b):
    """A terminal board: no two neighbours are equal (a != b, both > 0)."""
    assert a != b and a > 0 and b > 0
    return np.where(COLOUR == 0, a, b).astype(np.uint8)


def dense_board(rng, cap, empties):
    b = rng.integers(max(1, cap - 3), cap + 1, 16)
    b[rng.choice(16, empties, replace=False)] = 0
    return b.astype(np.uint8)


def high_boards(rng, n, cap, fills=(0.3, 0.6, 0.9, 1.0)):
    """n boards u8 [n, 16] of exponents up to `cap`, the crafted ones first: all `cap` (at 27 every
    move merges sixteen 27s into eight 28s, a gain of exactly 2^31), cap / cap - 1 stripes, a
    terminal checkerboard, the 24s row where it fits, dense boards with 0..3 empty cells; then
    mixed fills with exponents drawn from 1..cap."""
    out = [np.full(16, cap), np.repeat([cap, cap - 1, cap, cap - 1], 4), checker(cap, cap - 1)]
    if cap >= 24:
        out.append(np.array(ROW_24))
    out += [dense_board(rng, cap, e) for e in range(4)]
    out = [np.asarray(b, np.uint8) for b in out][:n]
    if len(out) < n:
        m = n - len(out)
        fill = rng.choice(fills, size=(m, 1))
        mixed = rng.integers(1, cap + 1, (m, 16)) * (rng.random((m, 16)) < fill)
        out += list(mixed.astype(np.uint8))
    return np.stack(out)


def low_boards(rng, n, hi=4):
    """Boards of exponents up to `hi` with a tile and an empty cell, so each has a legal move (no
    target of 0) and its gain stays below 2^(hi + 4)."""
    b = rng.integers(1, hi + 1, (n, 16)) * (rng.random((n, 16)) < rng.choice((0.4, 0.7, 0.95),
                                                                              size=(n, 1)))
    for row in b:
        i, j = rng.choice(16, 2, replace=False)
        row[i], row[j] = 0, rng.integers(1, hi + 1)
    return b.astype(np.uint8)


def distinct_prev(tuples, n, seed, seen=None, highs=(0, 16, 17, 25, 26, 27)):
    """n afterstates whose 8 T n hits are pairwise distinct, and distinct from `seen` (a set of
    (t, idx) that is extended): exponents 1..14 and, in turn, one cell raised to one of `highs`
    (it reads as 15 in the index and decides the stage)."""
    rng = np.random.default_rng(seed)
    ref, keep = NR.Net(tuples), []
    seen = set() if seen is None else seen
    for _try in range(2000 * n):
        if len(keep) == n:
            break
        p = rng.integers(1, 15, 16)
        h = highs[len(keep) % len(highs)]
        if h:
            p[rng.integers(16)] = h
        keys = ref.indices(p)
        if len(set(keys)) == len(keys) and seen.isdisjoint(keys):
            seen.update(keys)
            keep.append(p.astype(np.uint8))
    assert len(keep) == n, f"{n} boards of distinct hits do not fit this spec"
    return np.stack(keep)


# ------------------------------------------------------------------ solved rows
@dataclass
class Row:
    prev: np.ndarray          # its 8 T hits are pairwise distinct and nobody else's
    board: np.ndarray         # terminal: target 0, err = -V(prev)
    entries: dict             # {(t, idx): value} under prev, summing to -err
    lr_num: int
    lr_shift: int
    err: int
    delta: int
    older: list = field(default_factory=list)  # further afterstates of distinct hits (the ring)


def err_for(delta, lr_num, lr_shift):
    """An err with (err * lr_num) >> lr_shift == delta; for delta == 0 the largest one."""
    if delta == 0:
        err = ((1 << lr_shift) - 1) // lr_num
        assert err > 0, "a zero delta from a non-zero err needs lr_num < 2^lr_shift"
    else:
        err = -((-delta << lr_shift) // lr_num)  # the ceiling of delta * 2^lr_shift / lr_num
    assert (err * lr_num) >> lr_shift == delta
    return err


def solved_rows(tuples, lr=(1, 2), seed=0, seen=None, deltas=DELTAS, older=0):
    """One Row per wanted delta.  The entries under prev share -err evenly; all have the sign
    opposite to delta's (or are 0), so entry + delta stays inside int32 and off INT32_MIN."""
    ref = NR.Net(tuples)
    seen = set() if seen is None else seen
    prevs = distinct_prev(tuples, len(deltas) * (1 + older), seed, seen)
    rows = []
    for k, delta in enumerate(deltas):
        prev = prevs[k * (1 + older)]
        err = err_for(delta, *lr)
        keys = ref.indices(prev)
        base, rem = divmod(-err, len(keys))
        entries = {key: base + (j < rem) for j, key in enumerate(keys)}
        assert sum(entries.values()) == -err
        assert all(INT32_MIN < v + delta <= INT32_MAX and INT32_MIN < v <= INT32_MAX
                   for v in entries.values())
        board = checker(27 - k % 3, 26 - 2 * (k % 2) - k % 3)
        rows.append(Row(prev, board, entries, *lr, err, delta,
                        list(prevs[k * (1 + older) + 1:(k + 1) * (1 + older)])))
    return rows


# ------------------------------------------------------------------ the guard
class OutOfDomain(AssertionError):
    pass


class InDomain:
    """with InDomain(net, tc): <one reference step>.  `net` is the ntuple_ref.Net or
    ntstage_ref.StagedNet the step writes, `tc` the object holding the E and A dicts (or None).
    While it is open every ntuple_ref.wrap32 of the references is watched: one that changes its
    argument is a delta or a table entry that left int32.  On leaving, a staged entry equal to
    UNSET, |E| > A and A >= 2^62 are looked for.  Any of them raises OutOfDomain."""

    def __init__(self, net=None, tc=None):
        self.net, self.tc, self.bad = net, tc, []

    def _wrap32(self, x):
        w = self._orig(x)
        if w != x:
            who = sys._getframe(1).f_code.co_name
            self.bad.append(f"{'delta' if who == 'delta_of' else 'entry'} {x} wrapped to {w}")
        return w

    def __enter__(self):
        self._orig = NR.wrap32
        NR.wrap32 = self._wrap32
        return self

    def __exit__(self, exc_type, exc, tb):
        NR.wrap32 = self._orig
        if exc_type is not None:
            return False
        if isinstance(self.net, SR.StagedNet):
            self.bad += [f"staged entry {(s, *k)} landed on UNSET"
                         for s, st in enumerate(self.net.stages) for k, v in st.items()
                         if v == UNSET]
        if self.tc is not None:
            for k, a in self.tc.A.items():
                if abs(self.tc.E[k]) > a or a > TR.MAX_A:
                    self.bad.append(f"(E, A) = ({self.tc.E[k]}, {a}) at {k}")
        if self.bad:
            raise OutOfDomain("; ".join(self.bad[:4]) + f" ({len(self.bad)} in all)")
        return False


# ------------------------------------------------------------------ learning cases
@dataclass
class Call:
    boards: np.ndarray        # u8 [n, 16]
    history: list             # per board its afterstates, latest first ([] = no prev)
    lr: tuple


@dataclass
class Case:
    tuples: tuple
    bounds: tuple | None      # None: one table
    lut: np.ndarray           # int32 [T, E] or [S, T, E]
    calls: list
    ea: np.ndarray | None = None   # int64 [..., 2] for the TC libraries (None: zeros)
    lam: tuple = (3, 1)            # (H, lam_shift) of the lambda library
    rows: list = field(default_factory=list)  # the solved rows of each call


class RefSide:
    """The reference of one library over a Case's dense tables, every step inside InDomain.
    Each call sets the per-board state from the call's history, as the GPU side does; the table
    and the accumulators carry over."""

    def __init__(self, case: Case, lib: str):
        assert (case.bounds is not None) == (lib in STAGED_LIBS)
        self.case, self.lib = case, lib
        if case.bounds is None:
            self.net = NR.Net(case.tuples, base=case.lut)
        else:
            self.net = SR.StagedNet(case.tuples, case.bounds, base=case.lut)
        self.tc = None
        if lib in TC_LIBS:
            ea0 = case.ea
            base_ea = None if ea0 is None else (lambda *k: (int(ea0[k][0]), int(ea0[k][1])))
            kind = {"tc": TR.TC, "meantc": MTR.MeanTC, "stagemeantc": SMTR.StagedMeanTC}[lib]
            self.tc = kind(self.net, base_ea)

    @staticmethod
    def state(call: Call):
        prev = [[int(x) for x in h[0]] if len(h) else [0] * 16 for h in call.history]
        return prev, [int(len(h) > 0) for h in call.history]

    @staticmethod
    def ring(call: Call, H):
        """The lambda ring of a call's history: head[i] = i mod H, the k-th latest afterstate in
        plane (head - k) mod H, depth = the number of afterstates."""
        n = len(call.boards)
        hist = [[[0] * 16 for _ in range(n)] for _ in range(H)]
        head, depth = [i % H for i in range(n)], [min(len(h), H) for h in call.history]
        for i, h in enumerate(call.history):
            for k in range(depth[i]):
                hist[(head[i] - k) % H][i] = [int(x) for x in h[k]]
        return hist, head, depth

    def step(self, call: Call):
        """(actions, errs, deltas, state): state = (prev, has_prev), for lambda (hist, head,
        depth), after the step."""
        lib, net = self.lib, self.net
        prev, has = self.state(call)
        with InDomain(net, self.tc):
            if lib in ("td", "stage"):
                out = net.td_step(call.boards, prev, has, *call.lr)
            elif lib in TC_LIBS:
                out = self.tc.step(call.boards, prev, has, *call.lr)
            elif lib == "mean":
                out = MR.step(net, call.boards, prev, has, *call.lr)
            elif lib == "stagemean":
                out = SMR.step(net, call.boards, prev, has, *call.lr)
            else:
                lam = LR.Lam(net, len(call.boards), *self.case.lam)
                lam.hist, lam.head, lam.depth = self.ring(call, lam.H)
                out = lam.step(call.boards, *call.lr)
                return (*out, (lam.hist, lam.head, lam.depth))
        return (*out, (prev, has))

    def want_lut(self):
        want = self.case.lut.copy()
        if self.case.bounds is None:
            for k, v in self.net.touched.items():
                want[k] = v
        else:
            for s, st in enumerate(self.net.stages):
                for k, v in st.items():
                    want[(s, *k)] = v
        return want

    def want_ea(self):
        want = (np.zeros((*self.case.lut.shape, 2), np.int64) if self.case.ea is None
                else self.case.ea.copy())
        for k, a in self.tc.A.items():
            want[k] = (self.tc.E[k], a)
        return want


def seeded_ea(rng, shape, top=False):
    """In-domain accumulators int64 [*shape, 2].  The classes of test_nttc_gpu.py's random_ea (A =
    0, A around 2^16, E = +-A, E = 0, A of 1..46 bits) and, with `top`, on half of the entries A in
    [2^61, 2^62 - 2^40) with E in {0, A, -A, uniform}: the 2^40 is room for what two calls add."""
    kind = rng.integers(0, 8, shape)
    a = rng.integers(0, 1 << 45, shape, endpoint=True) >> rng.integers(0, 45, shape)
    a = np.where(kind == 0, 0, np.where(kind == 1, (1 << 16) + rng.integers(-2, 3, shape), a))
    if top:
        big = rng.integers(1 << 61, (1 << 62) - (1 << 40), shape)
        a = np.where(rng.random(shape) < 0.5, big, a)
    e = rng.integers(-a, a, endpoint=True)
    e = np.where(kind == 2, a, np.where(kind == 3, -a, np.where(kind == 4, 0, e)))
    return np.stack([e, a], axis=-1).astype(np.int64)


def _stage_of(bounds, board):
    return sum(1 for b in bounds if int(max(board)) >= b)


def exact_case(lib, spec="2x4", bounds=None, seed=0, lam=(3, 1), ea=None):
    """The solved rows in one batch with two boards without a previous afterstate among them, two
    calls: lr = 1 / 4 and then 2^16 / 2^18 (the same rate through a 48-bit product) on fresh rows
    over other entries.  Staged: the rows' entries sit at prev's own stage or, every other row, at
    stage 0 under an UNSET, so the step promotes them first.  `ea`: None (fresh), or "seeded":
    the rows' entries get rates of 1/3, 0, 1 and an A in [2^61, 2^62)."""
    tuples = SPECS[spec]
    rng = np.random.default_rng(1000 + seed)
    lut = np.zeros(lut_shape(tuples, bounds), np.int32)
    if bounds is not None:
        lut[1:] = UNSET
    seeds = ((1, 3), (0, 7), (5, 5), (-(1 << 61), 1 << 61), (0, 3 << 60), ((1 << 61) + 12345,
                                                                         (1 << 62) - (1 << 34)))
    ea0 = np.zeros((*lut.shape, 2), np.int64) if ea == "seeded" else None
    seen, calls, all_rows = set(), [], []
    for c, lr in enumerate(((1, 2), (1 << 16, 18))):
        rows = solved_rows(tuples, lr, 2000 + 10 * seed + c, seen, older=lam[0] - 1)
        for k, row in enumerate(rows):
            s = _stage_of(bounds, row.prev) if bounds is not None else None
            for j, (key, v) in enumerate(row.entries.items()):
                at = key if s is None else ((s if k % 2 == 0 else 0), *key)
                lut[at] = v
                if ea0 is not None:
                    ea0[key if s is None else (s, *key)] = seeds[(j + k) % len(seeds)]
            if s is not None:  # the older afterstates' entries are 0 at stage 0: nothing to set
                pass
        free = high_boards(rng, 2, CAP_LEARN)
        boards = np.stack([free[0]] + [r.board for r in rows[:3]] + [free[1]]
                          + [r.board for r in rows[3:]])
        history = ([[]] + [[r.prev, *r.older] for r in rows[:3]] + [[]]
                   + [[r.prev, *r.older][:1 + k % lam[0]] for k, r in enumerate(rows[3:])])
        calls.append(Call(boards, history, lr))
        all_rows.append(rows)
    return Case(tuples, bounds, lut, calls, ea0, lam, all_rows)


def wide_case(lib, spec, bounds, n, lr, seed):
    """Wide values at an extreme rate, one call.  (1, 31), (0, 0): a wide table, boards and prev
    from high_boards(27).  (2^16, 31): the same, but under a sum rule prev has pairwise distinct
    hits, so that an entry receives one delta (< 2^27) and not 8 n of them.  (1, 0), (2^16, 16):
    delta = err, so a flat table of 2^30s and low boards with a legal move; |err| < 2^19 there
    and 8 n hits of it stay below 2^30."""
    tuples = SPECS[spec]
    rng = np.random.default_rng(3000 + seed)
    shape = lut_shape(tuples, bounds)
    H = 3
    if lr in ((1, 0), (1 << 16, 16)):
        lut = flat_table(shape, seed)
        boards = low_boards(rng, n)
        history = [[low_boards(rng, 1)[0] for _ in range(H)] for _ in range(n)]
    else:
        lut = wide_table(shape, seed) if bounds is None else wide_staged(shape, seed)
        boards = high_boards(rng, n, CAP_LEARN)
        if lr == (1 << 16, 31) and lib in SUM_LIBS:
            older = H if lib == "lam" else 1
            prevs = distinct_prev(tuples, n * older, 4000 + seed)
            history = [list(prevs[i * older:(i + 1) * older]) for i in range(n)]
        else:
            prevs = high_boards(rng, n * H, CAP_LEARN)[rng.permutation(n * H)]
            history = [list(prevs[i * H:(i + 1) * H]) for i in range(n)]
    for i in range(0, n, 7):  # some boards without a previous afterstate
        history[i] = []
    for i in range(1, n, 5):  # and some shallower rings
        history[i] = history[i][:1 + i % H]
    return Case(tuples, bounds, lut, [Call(boards, history, lr)], None, (H, 1))


def tc_seed_case(lib, spec, bounds, seed, n=65):
    """The TC libraries on seeded accumulators whose A reaches [2^61, 2^62): a wide table, high
    boards, lr = (1, 31), and the same call twice, so every such entry is hit twice."""
    tuples = SPECS[spec]
    rng = np.random.default_rng(5000 + seed)
    shape = lut_shape(tuples, bounds)
    lut = wide_table(shape, seed) if bounds is None else wide_staged(shape, seed)
    ea = seeded_ea(rng, shape, top=True)
    boards = high_boards(rng, n, CAP_LEARN)
    prevs = high_boards(rng, n, CAP_LEARN)[rng.permutation(n)]
    call = Call(boards, [[p] for p in prevs], (1, 31))
    return Case(tuples, bounds, lut, [call, call], ea)


def edge_unset_case(lib, spec, bounds, lr, seed, n=65):
    """A staged learning step over upper stages of UNSET / INT32_MIN + 1: the policy launch must
    read INT32_MIN + 1 as a value and fall through an UNSET beside it.  At lr = (0, 0) prev is high
    too (its UNSET entries are promoted, nothing is added); at (1, 31) prev is a low board of stage
    0, whose wide entries have room for the deltas."""
    tuples = SPECS[spec]
    rng = np.random.default_rng(6000 + seed)
    lut = wide_staged(lut_shape(tuples, bounds), seed, edge=True)
    boards = high_boards(rng, n, CAP_LEARN)
    prevs = high_boards(rng, n, CAP_LEARN) if lr == (0, 0) else low_boards(rng, n, hi=14)
    ea = seeded_ea(rng, lut.shape) if lib in TC_LIBS else None
    return Case(tuples, bounds, lut, [Call(boards, [[p] for p in prevs], lr)], ea)


def learning_cases():
    """[(id, lib, build)]: every learning case of tests/test_domain_edge_gpu.py; build() -> Case.
    tests/test_domain_edge.py runs each of them through the reference inside InDomain."""
    out = []

    def add(name, lib, fn, *args, **kw):
        out.append((f"{lib}-{name}", lib, lambda: fn(lib, *args, **kw)))

    for li, lib in enumerate(LIBS):
        bounds = STAGE_BOUNDS[li % 2] if lib in STAGED_LIBS else None
        for si, spec in enumerate(("2x4", "8x4")):
            add(f"exact-{spec}", lib, exact_case, spec, bounds, 10 * li + si)
        if lib in TC_LIBS:
            add("exact-seeded", lib, exact_case, "2x4", bounds, 10 * li + 5, ea="seeded")
            for si, spec in enumerate(SMALL):
                add(f"seeds-{spec}", lib, tc_seed_case, spec, bounds, 10 * li + si)
        if lib == "lam":
            add("exact-H2-s31", lib, exact_case, "2x4", None, 10 * li + 6, lam=(2, 31))
        for ni, n in enumerate((2, 65, 129)):
            for ri, lr in enumerate(LRS):
                spec = SMALL[(ni + ri + li) % 3]
                if lr == (1 << 16, 31) and lib in SUM_LIBS:
                    spec = "2x4"  # the only small spec that holds 8 n (H n) distinct hits
                add(f"wide-n{n}-lr{lr[0]}_{lr[1]}-{spec}", lib, wide_case, spec, bounds, n, lr,
                    100 * li + 10 * ni + ri)
        if lib in STAGED_LIBS:
            for ri, lr in enumerate(((0, 0), (1, 31))):
                for bi, b in enumerate(STAGE_BOUNDS):
                    add(f"edge_unset-lr{lr[0]}_{lr[1]}-b{bi}", lib, edge_unset_case,
                        SMALL[1 + (ri + bi) % 2], b, lr, 10 * li + 2 * ri + bi)
    return out
