"""Truncated TD(lambda) learning (g2048.ntlambda) next to TD(0) (g2048.ntuple): launch times by
HIP events and playing strength.

--mode time.  For each named tuple set and each row a fresh trainer is made on a copy of the same
random int32 table and the same seed: `--boards` fresh boards are played forward `--play` random
steps (auto-reset on), then the trainer steps H + 2 times so that every ring is as full as its
episode allows.  Then the learning call alone is timed `--reps` times with an event pair, with the
trainer's own env.step between the timed calls (untimed), so every call meets the afterstates the
board really went through:

    td_step          the yardstick: g2048_ntuple_td_step from libg2048_ntuple.so, in this process
    lambda H=h       g2048_ntlambda_step at horizon h (H = 1 is the same rule as td_step and, from
                     the same table and seed, meets the same boards)
    ... lr=0         the same call with every delta 0: both launches, no adds

adds = over the timed calls, the (board, k) pairs with delta_k != 0, times 8 T; adds per second =
adds / (the call - its lr=0 run), counted before merging.  At the default rate of 65 536 boards
(2^-18) the deltas on the random table are around 2^4, so afterstates more than 4 steps back get
delta_k = 0 and add nothing; `--lr-shift 12` makes every afterstate of the ring add.  us per extra
afterstate = (lambda H=h - lambda H=1) / (h - 1).  With a `--lib` built with
-DG2048_NTLAMBDA_COUNT_BYPASS the rows also print the share of adds that found no slot in the
block's merge table and went straight to memory (the times of such a build are not the
library's).  `--lib` also times other builds, such as one with -DG2048_NTLAMBDA_SLOT_BITS=14.

--mode strength2x4.  TD(0) (horizon 1) and TD(lambda) at each of `--horizons` on TUPLES_2x4,
`--boards` boards, the default rate, the same seeds: the mean merge score of the last 200 finished
episodes and the largest |entry| after every `--chunk` steps up to `--steps`.

--mode strength4x6.  The same rules on TUPLES_4x6 for `--seconds` of wall time per rule, then
`--games` games of play("ntuple") and of play("ntuple_search") at depth 2 on each table.

    python tools/ntlambda_bench.py [--mode time] [--boards 65536] [--sets 2x4 4x6]
                                   [--horizons 1 2 3 5] [--lam-shift 1] [--lib PATH] [--out FILE]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning-2048_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def debug_counts(ntlambda, reset=True):
    """(adds, adds straight to memory) of a counting build since the last reset, else None."""
    lib = ntlambda.load()
    try:
        fn = lib.g2048_ntlambda_debug_counts
    except AttributeError:
        return None
    fn.restype, fn.argtypes = C.c_int, [C.POINTER(C.c_uint64 * 2), C.c_int]
    out = (C.c_uint64 * 2)()
    ntlambda.check(fn(C.byref(out), int(reset)), "g2048_ntlambda_debug_counts")
    return int(out[0]), int(out[1])


def time_mode(args, torch, ntuple, ntlambda):
    dev = torch.device("cuda:0")
    n = args.boards
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        T = len(tuples)
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        table = torch.randint(-(1 << 20), 1 << 20, (T, 16 ** len(tuples[0])), generator=gen,
                              device=dev, dtype=torch.int32)
        med = {}
        specs = [("td_step", 0)] + [(f"lambda H={h}", h) for h in args.horizons]
        for what, h in specs:
            for lr_num in (0, 1):
                label = what + ("" if lr_num else " lr=0")
                net = ntuple.NTupleNetwork(tuples, device=dev)
                net.lut.copy_(table)
                if h == 0:
                    tr = ntuple.NTupleTrainer(net, n, seed=args.seed, lr_shift=args.lr_shift)
                else:
                    tr = ntlambda.TDLambdaTrainer(net, n, horizon=h, lam_shift=args.lam_shift,
                                                  seed=args.seed, lr_shift=args.lr_shift)
                for _ in range(args.play):
                    tr.env.step(None)
                tr.step(max(h, 1) + 2 + args.warmup)
                torch.cuda.synchronize()
                debug_counts(ntlambda)

                def call():
                    if h == 0:
                        net.td_step(tr.env.board, tr.prev, tr.has_prev, lr_num, tr.lr_shift,
                                    tr.actions, tr.delta, tr.err)
                    else:
                        tr.lam.step(tr.env.board, lr_num, tr.lr_shift, tr.actions, tr.delta,
                                    tr.err)

                ms, adds, adding = [], 0, 0
                for _ in range(args.reps):
                    depth = (tr.has_prev if h == 0 else tr.lam.depth).to(torch.int64)
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call()
                    e1.record()
                    e1.synchronize()
                    ms.append(e0.elapsed_time(e1))
                    mag = tr.delta.to(torch.int64).abs()
                    for k in range(max(h, 1)):
                        live = (depth > k) & ((mag >> (k * args.lam_shift)) != 0)
                        adds += int(live.sum()) * 8 * T
                    adding += int(((depth > 0) & (mag != 0)).sum())
                    tr.env.step(tr.actions, reward=tr.reward, done=tr.done, legal=tr.legal)
                torch.cuda.synchronize()
                counts = debug_counts(ntlambda) if h else None
                med[label] = statistics.median(ms)
                row = {"set": name, "table_bytes": table.numel() * 4, "boards": n, "call": label,
                       "horizon": h, "lam_shift": args.lam_shift if h else None,
                       "lr_shift": tr.lr_shift,
                       "us_median": med[label] * 1e3, "us_min": min(ms) * 1e3,
                       "us_max": max(ms) * 1e3, "reps": len(ms),
                       "boards_per_s": n / (med[label] * 1e-3)}
                extra = ""
                if lr_num:
                    gap = (med[label] - med[label + " lr=0"]) * 1e-3
                    row["adds_per_call"] = adds / len(ms)
                    row["adding_boards_per_call"] = adding / len(ms)
                    row["adds_per_s"] = adds / len(ms) / gap if gap > 0 else None
                    if row["adds_per_s"]:
                        extra += (f"  {row['adds_per_s']:.3e} adds/s over the lr=0 run "
                                  f"({row['adds_per_call']:.0f} adds per call)")
                    if h > 1 and "lambda H=1" in med:
                        row["us_per_extra_afterstate"] = ((med[label] - med["lambda H=1"]) * 1e3
                                                          / (h - 1))
                        extra += f"  {row['us_per_extra_afterstate']:.1f} us per extra afterstate"
                    if h and "td_step" in med:
                        row["ratio_to_td"] = med[label] / med["td_step"]
                        extra += f"  {row['ratio_to_td']:.2f}x td"
                    if counts is not None and counts[0]:
                        row["counted_adds"], row["direct_adds"] = counts
                        row["bypass_share"] = counts[1] / counts[0]
                        extra += (f"  {100 * row['bypass_share']:.2f} % of {counts[0]} adds "
                                  f"bypassed the merge table")
                rows.append(row)
                print(f"{name} (lut {row['table_bytes'] >> 10} KiB) n={n} {label:17s} "
                      f"{row['us_median']:9.1f} us (min {row['us_min']:.1f}, max "
                      f"{row['us_max']:.1f})  {row['boards_per_s']:.3e} boards/s{extra}",
                      flush=True)
                tr.env.check_errors()
                del tr, net
                torch.cuda.empty_cache()
        if debug_counts(ntlambda, reset=False) is None:
            print(f"{name}: the share of adds that bypass the merge table needs a --lib built with "
                  f"-DG2048_NTLAMBDA_COUNT_BYPASS", flush=True)
    return {"play": args.play, "lib": ntlambda.LIB_PATH, "rows": rows}


def largest(net, torch):
    return int(net.lut.to(torch.int64).abs().max())


def make_trainer(ntuple, ntlambda, net, args, h, seed):
    kw = dict(seed=seed, p4=0.5, lr_shift=args.lr_shift, log_slots=64)
    if h == 1 and not args.lambda_at_h1:  # TD(0) through libg2048_ntuple.so, the rule to beat
        return ntuple.NTupleTrainer(net, args.boards, **kw)
    return ntlambda.TDLambdaTrainer(net, args.boards, horizon=h, lam_shift=args.lam_shift, **kw)


def strength2x4(args, torch, ntuple, ntlambda):
    import numpy as np

    rows = []
    for seed in args.seeds:
        for h in args.horizons:
            net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cuda:0")
            tr = make_trainer(ntuple, ntlambda, net, args, h, seed)
            scores, done = [], 0
            while done < args.steps:
                tr.step(args.chunk)
                done += args.chunk
                scores += tr.episodes()["score"].tolist()
                row = {"horizon": h, "lam_shift": args.lam_shift, "seed": seed,
                       "boards": args.boards, "lr_shift": tr.lr_shift, "steps": done,
                       "episodes": len(scores), "mean_last_200": float(np.mean(scores[-200:])),
                       "largest_entry": largest(net, torch)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            tr.env.check_errors()
    return {"rows": rows}


def strength4x6(args, torch, ntuple, ntlambda):
    import numpy as np

    from g2048.player import BatchedPlayer

    rows = []
    for h in args.horizons:
        net = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device="cuda:0")
        tr = make_trainer(ntuple, ntlambda, net, args, h, args.seeds[0])
        torch.cuda.synchronize()
        scores, done, t0, mark = [], 0, time.time(), args.seconds / 4
        while time.time() - t0 < args.seconds:
            tr.step(args.chunk)
            done += args.chunk
            scores = (scores + tr.episodes(strict=False)["score"].tolist())[-2000:]
            if time.time() - t0 >= mark:
                mark += args.seconds / 4
                print(json.dumps({"horizon": h, "steps": done, "seconds": time.time() - t0,
                                  "mean_last_200": float(np.mean(scores[-200:])),
                                  "largest_entry": largest(net, torch)}), flush=True)
        torch.cuda.synchronize()
        row = {"horizon": h, "lam_shift": args.lam_shift, "boards": args.boards,
               "lr_shift": tr.lr_shift, "steps": done, "board_steps": done * args.boards,
               "train_seconds": time.time() - t0,
               "train_mean_last_200": float(np.mean(scores[-200:])),
               "largest_entry": largest(net, torch)}
        tr.env.check_errors()
        del tr
        torch.cuda.empty_cache()
        for policy, kw in (("ntuple", {}), ("ntuple_search", {"search_depth": 2})):
            res = BatchedPlayer(args.games, device="cuda:0", seed=args.seeds[0] + 1000, ntuple=net,
                                p4=0.5, **kw).play(policy)
            row[policy] = {"mean_score": float(res.merge_score.mean()),
                           "max_tile_hist": {int(k): int(v)
                                             for k, v in zip(*res.max_tile_frequency())}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del net
        torch.cuda.empty_cache()
    return {"rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=["time", "strength2x4", "strength4x6"])
    ap.add_argument("--boards", type=int, default=None,
                    help="default: 65536 (time), 256 (strength2x4), 4096 (strength4x6)")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--horizons", type=int, nargs="+", default=None,
                    help="default: 1 2 3 5 (time), 1 3 5 (strength; 1 is TD(0))")
    ap.add_argument("--lam-shift", type=int, default=1)
    ap.add_argument("--lambda-at-h1", action="store_true",
                    help="strength modes: horizon 1 through libg2048_ntlambda.so instead of "
                         "NTupleTrainer (the same rule)")
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--lib", default=None, help="another build of libg2048_ntlambda.so to load")
    ap.add_argument("--seeds", type=int, nargs="+", default=[61])
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--lr-shift", type=int, default=None, help="default: default_lr_shift(boards)")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = {"time": 65536, "strength2x4": 256, "strength4x6": 4096}[args.mode]
    if args.horizons is None:
        args.horizons = [1, 2, 3, 5] if args.mode == "time" else [1, 3, 5]

    import torch

    import g2048  # noqa: F401
    from g2048 import ntlambda, ntuple

    if not torch.cuda.is_available():
        raise SystemExit("ntlambda_bench needs a GPU")
    if args.lib:
        ntlambda.LIB_PATH = os.path.abspath(args.lib)
        ntlambda._lib = None
    ntlambda.load()
    out = {"time": time_mode, "strength2x4": strength2x4,
           "strength4x6": strength4x6}[args.mode](args, torch, ntuple, ntlambda)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
