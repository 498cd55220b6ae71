"""The per-board restart pool (g2048.ntrestart) in the self-play loop: what it costs per step and
what it does to playing strength.

--mode cost.  For each `--boards` count three NTupleTrainers on TUPLES_4x6 tables of their own,
equal seeds: `pool` (a RestartPool with `--levels`), `none` (restart=None) and `bare` (no
trainer loop at all: the tool enqueues (td_step, env.step) itself, the loop as it was before the
keyword existed).  After `--warmup` chunks of each, `--reps` chunks of step(`--chunk`) are timed
with an event pair, alternating rep by rep between the three in one process; reported per step:
median, min and max.

--mode strength (tools/nttc_bench.py's protocol).  Self-play on TUPLES_4x6 with 4 096 boards,
p(4) = 0.5, seed 61 and the default rate for `--seconds` of wall time per row in step(`--chunk`)
chunks, then `--games` games of play("ntuple") and of the depth-2 search on one seed.  A row is
`bounds/levels[/stagger]`: bounds `single` or a comma list, levels `none` or a comma list.  Per
row: steps, set entries per stage, the share of boards at or above each bound (the boards as they
stand at the end of every chunk) and of finished episodes whose largest tile reached it (the
episode log), slots set per level, training and play scores, max-tile counts.

    python tools/ntrestart_bench.py --mode cost [--boards 4096 65536] [--out FILE]
    python tools/ntrestart_bench.py --mode strength [--rows single/none single/0,11 ...]
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

ROWS = ["single/none", "single/0,11", "11/none", "11/0,11", "11,12/0,11,12", "11/0,11/stagger"]


def cost(args, torch, g2048):
    rows = []
    for n in args.boards:
        levels = tuple(int(e) for e in args.levels.split(","))

        def trainer(pool):
            net = g2048.NTupleNetwork(g2048.TUPLES_4x6, device="cuda:0")
            kw = {"restart": g2048.RestartPool(n, levels, device="cuda:0")} if pool else {}
            return g2048.NTupleTrainer(net, n, seed=args.seed, **kw)

        trs = {"pool": trainer(True), "none": trainer(False), "bare": trainer(False)}

        def bare(k, tr=trs["bare"]):
            for _ in range(k):
                tr.net.td_step(tr.env.board, tr.prev, tr.has_prev, tr.lr_num, tr.lr_shift,
                               tr.actions, tr.delta, tr.err)
                tr.env.step(tr.actions, reward=tr.reward, done=tr.done, legal=tr.legal)

        run = {"pool": trs["pool"].step, "none": trs["none"].step, "bare": bare}
        for _ in range(args.warmup):
            for f in run.values():
                f(args.chunk)
        torch.cuda.synchronize()
        ms = {k: [] for k in run}
        for _ in range(args.reps):
            for key, f in run.items():
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                e0.record()
                f(args.chunk)
                e1.record()
                e1.synchronize()
                ms[key].append(e0.elapsed_time(e1))
        for tr in trs.values():
            tr.env.check_errors()
        row = {"boards": n, "chunk": args.chunk, "reps": args.reps, "levels": levels,
               "slots_set": trs["pool"].restart.counts()}
        for key, v in ms.items():
            per = [x * 1e3 / args.chunk for x in v]
            row[key] = {"us_median": statistics.median(per), "us_min": min(per),
                        "us_max": max(per)}
        rows.append(row)
        print(f"n={n}: us per step, median (min - max) of {args.reps} chunks of {args.chunk}: "
              + "; ".join(f"{k} {row[k]['us_median']:.2f} ({row[k]['us_min']:.2f} - "
                          f"{row[k]['us_max']:.2f})" for k in ms)
              + f"; slots set per level {row['slots_set']}", flush=True)
        del trs, run, bare
        torch.cuda.empty_cache()
    return {"rows": rows}


def strength(args, torch, g2048):
    import numpy as np

    from g2048.ntstage import UNSET
    from g2048.player import BatchedPlayer

    rows = []
    for spec in args.rows:
        parts = spec.split("/")
        bounds = () if parts[0] == "single" else tuple(int(b) for b in parts[0].split(","))
        levels = None if parts[1] == "none" else tuple(int(e) for e in parts[1].split(","))
        stagger = len(parts) > 2 and parts[2] == "stagger"
        staged = parts[0] != "single"
        if staged:
            net = g2048.StagedNTupleNetwork(g2048.TUPLES_4x6, bounds, device="cuda:0")
        else:
            net = g2048.NTupleNetwork(g2048.TUPLES_4x6, device="cuda:0")
        pool = (None if levels is None
                else g2048.RestartPool(args.boards, levels, device="cuda:0", stagger=stagger))
        tr = g2048.NTupleTrainer(net, args.boards, seed=args.seed, p4=0.5, log_slots=64,
                                 restart=pool)
        marks = bounds if bounds else (11, 12)  # the single table: the same tiles, for comparison
        torch.cuda.synchronize()
        scores, tops, done, t0, quarter, quarters = [], [], 0, time.time(), args.seconds / 4, []
        share = np.zeros(len(marks))
        while time.time() - t0 < args.seconds:
            tr.step(args.chunk)
            done += args.chunk
            ep = tr.episodes(strict=False)
            scores = (scores + ep["score"].tolist())[-2000:]
            tops += ep["max_exp"].tolist()
            top = tr.env.board.amax(dim=1)
            share += np.array([float((top >= b).float().mean()) for b in marks])
            if time.time() - t0 >= quarter:
                quarter += args.seconds / 4
                quarters.append(float(np.mean(scores[-200:])))
        torch.cuda.synchronize()
        lut = net.lut if not staged else torch.where(net.lut != UNSET, net.lut,
                                                     torch.zeros_like(net.lut))
        tops = np.array(tops)
        row = {"row": spec, "boards": args.boards, "lr_shift": tr.lr_shift, "steps": done,
               "train_seconds": time.time() - t0, "train_mean_quarters": quarters,
               "train_mean_last_200": float(np.mean(scores[-200:])), "episodes": len(tops),
               "marks": marks,
               "board_share_at_or_above": (share / (done / args.chunk)).tolist(),
               "episode_share_at_or_above": [float((tops >= b).mean()) for b in marks],
               "largest_entry": int(lut.to(torch.int64).abs().max())}
        if staged:
            row["set_counts"] = net.set_counts()
        else:
            row["set_counts"] = [int((net.lut != 0).sum())]
        if pool is not None:
            row["slots_set"] = pool.counts()
        tr.env.check_errors()
        del tr, lut
        torch.cuda.empty_cache()
        for policy in ("ntuple", "ntstage_search" if staged else "ntuple_search"):
            res = BatchedPlayer(args.games, device="cuda:0", seed=args.seed + 1000, ntuple=net,
                                p4=0.5, search_depth=2).play(policy)
            row["ntuple" if policy == "ntuple" else "search2"] = {
                "mean_score": float(res.merge_score.mean()),
                "max_tile_hist": {int(k): int(v) for k, v in zip(*res.max_tile_frequency())}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del net, pool
        torch.cuda.empty_cache()
    return {"rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="cost", choices=["cost", "strength"])
    ap.add_argument("--boards", type=int, nargs="+", default=None,
                    help="default: 4096 65536 (cost), 4096 (strength)")
    ap.add_argument("--levels", default="0,11", help="cost mode: the pool's rotation")
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=61)
    ap.add_argument("--rows", nargs="+", default=ROWS)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = [4096, 65536] if args.mode == "cost" else [4096]
    if args.mode == "strength":
        args.boards = args.boards[0]

    import torch

    import g2048

    if not torch.cuda.is_available():
        raise SystemExit("ntrestart_bench needs a GPU")
    g2048.ntrestart.load()
    out = {"cost": cost, "strength": strength}[args.mode](args, torch, g2048)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
