"""Temporal-coherence learning (g2048.nttc) next to TD(0) (g2048.ntuple): launch times by HIP
events and playing strength.

--mode time (tools/ntuple_bench.py's method).  For each named tuple set the table is filled with
random int32, `--boards` fresh boards are played forward `--play` random steps (auto-reset on),
then a TD(0) trainer and a TC trainer on copies of the same table meet the same boards and the
same previous afterstates, and each call is warmed up and then timed `--reps` times with an event
pair:

    td_step          the yardstick: g2048_ntuple_td_step on these boards, in this process
    tc_step lr=0     both launches, every delta 0: no hand-over, no adds
    tc_step          both launches: + a 16-byte gather, the rate, the hand-over and three atomic
                     adds (one 32-bit, two 64-bit) per entry
    tc_step+step     tc_step followed by env.step (the training loop's body)

entry updates per second = boards with a non-zero delta * 8 T / (tc_step - its lr=0 run); each
entry update is one 32-bit and two 64-bit atomic adds before merging.  With --uniform the boards
and the previous afterstates are uniformly random exponents 0..11: no entry is hot, so that figure
is the scatter rate without contention.  `--lib` times another build of the library, such as one
compiled with -DG2048_NTTC_MERGE=0 (one atomic per add) or another -DG2048_NTTC_SLOT_BITS.

--mode strength2x4.  TD(0) and TC self-play on TUPLES_2x4, `--boards` boards, the default rate,
the same seeds: the mean merge score of the last 200 finished episodes and the largest |entry|
after every `--chunk` steps up to `--steps`.

--mode strength4x6.  TD(0) and TC self-play on TUPLES_4x6 for `--seconds` of wall time per rule,
then `--games` games of play("ntuple") and of play("ntuple_search") at depth 2 on each table:
mean score, max-tile counts, largest |entry|.

    python tools/nttc_bench.py [--mode time] [--boards 65536] [--sets 2x4 4x6] [--uniform]
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


def time_mode(args, torch, ntuple, nttc):
    dev = torch.device("cuda:0")
    n = args.boards
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        T = len(tuples)
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
        # the TC trainer: a copy of the table, the same per-board state, and an env of its own
        # played forward the same way for the tc_step+step row
        tc_net = ntuple.NTupleNetwork(tuples, device=dev)
        tc_net.lut.copy_(net.lut)
        tc_tr = nttc.TCTrainer(tc_net, n, seed=args.seed)
        for _ in range(args.play):
            tc_tr.env.step(None)
        tc_tr.step(3)
        tc_tr.prev.copy_(tr.prev)
        tc_tr.has_prev.copy_(tr.has_prev)
        torch.cuda.synchronize()
        with_prev = int(tr.has_prev.sum())
        flip = {"td": 0, "tc": 0}

        def td(lr_num):
            flip["td"] ^= 1
            net.td_step(pair[flip["td"]], tr.prev, tr.has_prev, lr_num, tr.lr_shift, tr.actions,
                        tr.delta, tr.err)

        def tc(lr_num):
            flip["tc"] ^= 1
            tc_tr.tc.tc_step(pair[flip["tc"]], tc_tr.prev, tc_tr.has_prev, lr_num, tc_tr.lr_shift,
                             tc_tr.actions, tc_tr.delta, tc_tr.err, tc_tr.work)

        calls = [("td_step lr=0", lambda: td(0), tr), ("td_step", lambda: td(1), tr),
                 ("tc_step lr=0", lambda: tc(0), tc_tr), ("tc_step", lambda: tc(1), tc_tr),
                 ("tc_step+step", lambda: tc_tr.step(1), tc_tr)]
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
                   "ea_bytes": tc_tr.tc.ea.numel() * 8, "boards": n, "call": what,
                   "us_median": med[what] * 1e3, "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3,
                   "reps": len(ms), "boards_per_s": n / (med[what] * 1e-3)}
            extra = ""
            if what in ("td_step", "tc_step"):
                row["boards_with_prev"] = with_prev
                row["nonzero_deltas"] = int((owner.delta != 0).sum())
                gap = (med[what] - med[what + " lr=0"]) * 1e-3
                row["entry_updates_per_s"] = (row["nonzero_deltas"] * 8 * T / gap
                                              if gap > 0 else None)
                if row["entry_updates_per_s"]:
                    extra = (f"  {row['entry_updates_per_s']:.3e} entry updates/s over the lr=0 "
                             f"run ({row['nonzero_deltas']} boards add)")
            if what.startswith("tc_step") and what.replace("tc_", "td_") in med:
                row["ratio_to_td"] = med[what] / med[what.replace("tc_", "td_")]
                extra += f"  {row['ratio_to_td']:.2f}x td"
            rows.append(row)
            print(f"{name} (lut {row['table_bytes'] >> 10} KiB, ea {row['ea_bytes'] >> 10} KiB) "
                  f"n={n} {what:13s} {row['us_median']:9.1f} us (min {row['us_min']:.1f}, max "
                  f"{row['us_max']:.1f})  {row['boards_per_s']:.3e} boards/s{extra}", flush=True)
        tr.env.check_errors()
        tc_tr.env.check_errors()
        del tr, tc_tr, net, tc_net
        torch.cuda.empty_cache()
    return {"play": args.play, "uniform": args.uniform, "lib": nttc.LIB_PATH, "rows": rows}


def largest(net, torch):
    return int(net.lut.to(torch.int64).abs().max())


def strength2x4(args, torch, ntuple, nttc):
    import numpy as np

    rows = []
    for seed in args.seeds:
        for rule in args.rules:
            net = ntuple.NTupleNetwork(ntuple.TUPLES_2x4, device="cuda:0")
            cls = ntuple.NTupleTrainer if rule == "td" else nttc.TCTrainer
            tr = cls(net, args.boards, seed=seed, p4=0.5, lr_shift=args.lr_shift, log_slots=64)
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


def strength4x6(args, torch, ntuple, nttc):
    import numpy as np

    from g2048.player import BatchedPlayer

    rows = []
    for rule in args.rules:
        net = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device="cuda:0")
        cls = ntuple.NTupleTrainer if rule == "td" else nttc.TCTrainer
        tr = cls(net, args.boards, seed=args.seeds[0], p4=0.5, lr_shift=args.lr_shift,
                 log_slots=64)
        torch.cuda.synchronize()
        scores, done, t0, mark = [], 0, time.time(), args.seconds / 4
        while time.time() - t0 < args.seconds:
            tr.step(args.chunk)
            done += args.chunk
            scores = (scores + tr.episodes(strict=False)["score"].tolist())[-2000:]
            if time.time() - t0 >= mark:
                mark += args.seconds / 4
                print(json.dumps({"rule": rule, "steps": done, "seconds": time.time() - t0,
                                  "mean_last_200": float(np.mean(scores[-200:])),
                                  "largest_entry": largest(net, torch)}), flush=True)
        torch.cuda.synchronize()
        row = {"rule": rule, "boards": args.boards, "lr_shift": tr.lr_shift, "steps": done,
               "board_steps": done * args.boards, "train_seconds": time.time() - t0,
               "train_mean_last_200": float(np.mean(scores[-200:])),
               "largest_entry": largest(net, torch)}
        if rule == "tc":
            row["largest_A"] = int(tr.tc.ea[..., 1].max())
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
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--uniform", action="store_true",
                    help="boards and previous afterstates of uniformly random exponents 0..11 "
                         "instead of played ones: no entry is hot")
    ap.add_argument("--lib", default=None, help="another build of libg2048_nttc.so to load")
    ap.add_argument("--seeds", type=int, nargs="+", default=[61])
    ap.add_argument("--steps", type=int, default=4000)
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--lr-shift", type=int, default=None, help="default: default_lr_shift(boards)")
    ap.add_argument("--rules", nargs="+", default=["td", "tc"], choices=["td", "tc"],
                    help="the strength modes' learning rules")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = {"time": 65536, "strength2x4": 256, "strength4x6": 4096}[args.mode]

    import torch

    import g2048  # noqa: F401
    from g2048 import nttc, ntuple

    if not torch.cuda.is_available():
        raise SystemExit("nttc_bench needs a GPU")
    if args.lib:
        nttc.LIB_PATH = os.path.abspath(args.lib)
        nttc._lib = None
    nttc.load()
    out = {"time": time_mode, "strength2x4": strength2x4,
           "strength4x6": strength4x6}[args.mode](args, torch, ntuple, nttc)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
