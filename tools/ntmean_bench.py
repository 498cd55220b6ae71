"""Batch-mean TD learning (g2048.ntmean) next to TD(0) (g2048.ntuple): launch times by HIP events
and playing strength.

--mode cost (tools/nttc_bench.py's method).  For each named tuple set the table is filled with
random int32, `--boards` fresh boards are played forward `--play` random steps (auto-reset on),
then a TD(0) trainer and a batch-mean trainer on copies of the same table meet the same boards and
the same previous afterstates, and each call is warmed up and then timed `--reps` times with an
event pair:

    td_step           the yardstick: g2048_ntuple_td_step on these boards, in this process
    mean_step lr=0    the three launches, every delta 0: nothing is gathered or applied
    mean_step         the three launches: two 64-bit atomic adds per distinct entry of a block,
                      then one or two returning exchanges, a division and a 32-bit add per entry
    mean_step+step    mean_step followed by env.step (the training loop's body)

With --uniform the boards and the previous afterstates are uniformly random exponents 0..11: no
entry is hot.  `--lib` times another build of the library, such as one compiled with another
-DG2048_NTMEAN_SLOT_BITS.  After the sets, the per-step time of both trainers' `step(k)` at
`--trainer-boards` boards (wall time over `--trainer-steps` steps, host enqueue included), where
the extra launch shows.

--mode strength2x4.  TD(0) and batch-mean self-play on TUPLES_2x4, `--boards` boards, each rule at
its default rate (or --lr-shift / --mean-lr-shifts), the same seeds: the mean merge score of the
last 200 finished episodes and the largest |entry| after every `--chunk` steps up to `--steps`.

--mode strength4x6.  TD(0) at its default and batch-mean at each of --mean-lr-shifts on TUPLES_4x6
for `--seconds` of wall time per rule, then `--games` games of play("ntuple") and of
play("ntuple_search") at depth 2 on each table: training means at the quarter marks, mean score,
max-tile counts, largest |entry|.

    python tools/ntmean_bench.py [--mode cost] [--boards 65536] [--sets 2x4 4x6] [--uniform]
                                 [--lib PATH] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning-2048_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def cost_mode(args, torch, ntuple, ntmean):
    dev = torch.device("cuda:0")
    n = args.boards
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        net = ntuple.NTupleNetwork(tuples, device=dev)
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=gen, device=dev,
                                    dtype=torch.int32))
        tr = ntuple.NTupleTrainer(net, n, seed=args.seed)
        for _ in range(args.play):
            tr.env.step(None)
        tr.step(2)  # every board gets a previous afterstate
        torch.cuda.synchronize()
        boards = tr.env.board.clone()
        tr.step(1)
        torch.cuda.synchronize()
        # both rules alternate between two consecutive states of the batch, so every call meets
        # afterstates of other boards than its own and errors that do not vanish
        pair = (boards, tr.env.board.clone())
        if args.uniform:
            def fresh():
                return torch.randint(0, 12, (n, 16), generator=gen, device=dev, dtype=torch.uint8)
            pair, prev0 = (fresh(), fresh()), fresh()
            tr.prev.copy_(prev0)
            tr.has_prev.fill_(1)
        # the batch-mean trainer: a copy of the table, the same per-board state and the TD(0)
        # trainer's rate (the cost does not depend on it), and an env of its own played forward
        # the same way for the mean_step+step row
        mn_net = ntuple.NTupleNetwork(tuples, device=dev)
        mn_net.lut.copy_(net.lut)
        mn_tr = ntmean.MeanTrainer(mn_net, n, seed=args.seed, lr_shift=tr.lr_shift)
        for _ in range(args.play):
            mn_tr.env.step(None)
        mn_tr.step(3)
        mn_tr.prev.copy_(tr.prev)
        mn_tr.has_prev.copy_(tr.has_prev)
        torch.cuda.synchronize()
        with_prev = int(tr.has_prev.sum())
        flip = {"td": 0, "mean": 0}

        def td(lr_num):
            flip["td"] ^= 1
            net.td_step(pair[flip["td"]], tr.prev, tr.has_prev, lr_num, tr.lr_shift, tr.actions,
                        tr.delta, tr.err)

        def mean(lr_num):
            flip["mean"] ^= 1
            mn_tr.mean.mean_step(pair[flip["mean"]], mn_tr.prev, mn_tr.has_prev, lr_num,
                                 mn_tr.lr_shift, mn_tr.actions, mn_tr.delta, mn_tr.err)

        calls = [("td_step lr=0", lambda: td(0), tr), ("td_step", lambda: td(1), tr),
                 ("mean_step lr=0", lambda: mean(0), mn_tr), ("mean_step", lambda: mean(1), mn_tr),
                 ("mean_step+step", lambda: mn_tr.step(1), mn_tr)]
        if args.uniform:  # the env's boards are played ones
            calls.pop()
        med = {}
        for what, fn, owner in calls:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if args.uniform:
                    owner.prev.copy_(prev0)
                    owner.has_prev.fill_(1)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med[what] = statistics.median(ms)
            row = {"set": name, "table_bytes": net.lut.numel() * 4,
                   "acc_bytes": mn_tr.mean.acc.numel() * 8, "boards": n, "call": what,
                   "us_median": med[what] * 1e3, "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3,
                   "reps": len(ms), "boards_per_s": n / (med[what] * 1e-3)}
            extra = ""
            if what in ("td_step", "mean_step"):
                row["boards_with_prev"] = with_prev
                row["nonzero_deltas"] = int((owner.delta != 0).sum())
            if what.startswith("mean_step") and what.replace("mean_", "td_") in med:
                row["ratio_to_td"] = med[what] / med[what.replace("mean_", "td_")]
                extra += f"  {row['ratio_to_td']:.2f}x td"
            rows.append(row)
            print(f"{name} (lut {row['table_bytes'] >> 10} KiB, acc {row['acc_bytes'] >> 10} KiB) "
                  f"n={n} {what:15s} {row['us_median']:9.1f} us (min {row['us_min']:.1f}, max "
                  f"{row['us_max']:.1f})  {row['boards_per_s']:.3e} boards/s{extra}", flush=True)
        assert not bool(mn_tr.mean.acc.any()), "acc is not all zero after the timed calls"
        tr.env.check_errors()
        mn_tr.env.check_errors()
        del tr, mn_tr, net, mn_net
        torch.cuda.empty_cache()
    # the trainers' loop at a narrow batch: wall time per step(k) iteration, enqueue included
    if not args.uniform and args.trainer_steps > 0:
        for name in args.sets:
            tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
            for rule, cls in (("td", ntuple.NTupleTrainer), ("mean", ntmean.MeanTrainer)):
                tr = cls(ntuple.NTupleNetwork(tuples, device=dev), args.trainer_boards,
                         seed=args.seed)
                tr.step(200)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(args.trainer_steps)
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / args.trainer_steps * 1e6
                rows.append({"set": name, "boards": args.trainer_boards,
                             "call": f"{rule} trainer step", "us_per_step": us,
                             "steps": args.trainer_steps})
                print(f"{name} n={args.trainer_boards} {rule:4s} trainer.step: {us:.1f} us per "
                      f"step over {args.trainer_steps} steps (wall)", flush=True)
                del tr
                torch.cuda.empty_cache()
    return {"play": args.play, "uniform": args.uniform,
            "lib": os.path.relpath(ntmean.LIB_PATH, ROOT), "rows": rows}


def largest(net, torch):
    return int(net.lut.to(torch.int64).abs().max())


def rules_of(args):
    """[(rule, lr_shift)]: TD(0) at --lr-shift (None = its default), batch-mean at each of
    --mean-lr-shifts (None = its default)."""
    out = [("td", args.lr_shift)] if "td" in args.rules else []
    if "mean" in args.rules:
        out += [("mean", s) for s in (args.mean_lr_shifts or [None])]
    return out


def make(rule, shift, net, boards, seed, ntuple, ntmean):
    cls = ntuple.NTupleTrainer if rule == "td" else ntmean.MeanTrainer
    return cls(net, boards, seed=seed, p4=0.5, lr_shift=shift, log_slots=64)


def strength2x4(args, torch, ntuple, ntmean):
    import numpy as np

    rows = []
    for seed in args.seeds:
        for rule, shift in rules_of(args):
            net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cuda:0")
            tr = make(rule, shift, net, args.boards, seed, ntuple, ntmean)
            scores, done = [], 0
            while done < args.steps:
                tr.step(args.chunk)
                done += args.chunk
                scores += tr.episodes()["score"].tolist()
                row = {"rule": rule, "seed": seed, "boards": args.boards, "lr_shift": tr.lr_shift,
                       "steps": done, "episodes": len(scores),
                       "mean_last_200": float(np.mean(scores[-200:])),
                       "largest_entry": largest(net, torch)}
                rows.append(row)
                print(json.dumps(row), flush=True)
            tr.env.check_errors()
    return {"rows": rows}


def strength4x6(args, torch, ntuple, ntmean):
    import numpy as np

    from g2048.player import BatchedPlayer

    rows = []
    for rule, shift in rules_of(args):
        net = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device="cuda:0")
        tr = make(rule, shift, net, args.boards, args.seeds[0], ntuple, ntmean)
        torch.cuda.synchronize()
        scores, done, t0, mark, marks = [], 0, time.time(), args.seconds / 4, []
        while time.time() - t0 < args.seconds:
            tr.step(args.chunk)
            done += args.chunk
            scores = (scores + tr.episodes(strict=False)["score"].tolist())[-2000:]
            if time.time() - t0 >= mark:
                mark += args.seconds / 4
                marks.append({"rule": rule, "lr_shift": tr.lr_shift, "steps": done,
                              "seconds": time.time() - t0,
                              "mean_last_200": float(np.mean(scores[-200:])),
                              "largest_entry": largest(net, torch)})
                print(json.dumps(marks[-1]), flush=True)
        torch.cuda.synchronize()
        row = {"rule": rule, "boards": args.boards, "lr_shift": tr.lr_shift, "steps": done,
               "board_steps": done * args.boards, "train_seconds": time.time() - t0,
               "train_mean_last_200": float(np.mean(scores[-200:])), "marks": marks,
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
    ap.add_argument("--mode", default="cost", choices=["cost", "strength2x4", "strength4x6"])
    ap.add_argument("--boards", type=int, default=None,
                    help="default: 65536 (cost), 256 (strength2x4), 4096 (strength4x6)")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--uniform", action="store_true",
                    help="boards and previous afterstates of uniformly random exponents 0..11 "
                         "instead of played ones: no entry is hot")
    ap.add_argument("--trainer-boards", type=int, default=4096)
    ap.add_argument("--trainer-steps", type=int, default=2000,
                    help="steps of the cost mode's trainer-loop rows (0 = skip them)")
    ap.add_argument("--lib", default=None, help="another build of libg2048_ntmean.so to load")
    ap.add_argument("--seeds", type=int, nargs="+", default=[61])
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--lr-shift", type=int, default=None,
                    help="TD(0)'s rate; default: default_lr_shift(boards)")
    ap.add_argument("--mean-lr-shifts", type=int, nargs="+", default=None,
                    help="batch-mean's rates, one run each; default: default_mean_lr_shift(spec)")
    ap.add_argument("--rules", nargs="+", default=["td", "mean"], choices=["td", "mean"],
                    help="the strength modes' learning rules")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = {"cost": 65536, "strength2x4": 256, "strength4x6": 4096}[args.mode]

    import torch

    import g2048  # noqa: F401
    from g2048 import ntmean, ntuple

    if not torch.cuda.is_available():
        raise SystemExit("ntmean_bench needs a GPU")
    if args.lib:
        ntmean.LIB_PATH = os.path.abspath(args.lib)
        ntmean._lib = None
    ntmean.load()
    out = {"cost": cost_mode, "strength2x4": strength2x4,
           "strength4x6": strength4x6}[args.mode](args, torch, ntuple, ntmean)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
