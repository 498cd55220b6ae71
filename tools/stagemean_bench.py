"""Batch-mean TD learning on the multi-stage network (g2048.stagemean) next to the single-table
batch-mean step (g2048.ntmean) and the staged TD(0) step (g2048.ntstage): launch times by HIP
events and playing strength.  Modelled on tools/ntmean_bench.py.

--mode cost (DESIGN 4.17's method).  For each named tuple set a single table is filled with random
int32, `--boards` fresh boards are played forward `--play` random steps (auto-reset on) and two
consecutive states of the batch are kept; every rule below then alternates between them from the
same previous afterstates, is warmed up and is timed `--reps` times with an event pair, each at
lr = 0 (nothing gathered or applied; the staged policy launch still promotes) and at lr = 1:

    mean_step          the yardstick: g2048_ntmean_step on the single table
    stagemean S=1      g2048_stagemean_step with no bounds on a copy of that table (fully set)
    stage td_step      g2048_ntstage_td_step, bounds --bounds, stage 0 = the table, the rest UNSET
                       before the warm-up
    stagemean          g2048_stagemean_step on the same staged table

Random play reaches no late stage, so the two staged rows of this mode see stage-0 boards only;
--mode cost-trained is the measurement with boards in every stage.  Then the wall time per step
of StagedMeanTrainer.step(k) at `--trainer-boards` boards next to MeanTrainer and
NTupleTrainer(staged).

--mode cost-trained.  For each named set a staged network (4x6: --bounds, 2x4: --bounds-2x4, whose
games end long before a 2048 tile) is trained by StagedMeanTrainer at `--trainer-boards` boards for
`--train-seconds`; a second StagedMeanTrainer of `--boards` boards then plays `--spread-steps`
steps on that table, so that its boards spread over the phases of a game, and one more step gives
a board state and the previous afterstates that belong to it.  The table, prev and has_prev are
kept; every timed call starts from copies of them (restored outside the event pair, so the table
is cold in the caches for every rule alike), which makes each repetition the same work,
promotions included:

    mean_step          g2048_ntmean_step on the single table net.resolved(0)
    stage td_step      g2048_ntstage_td_step on the trained staged table
    stagemean          g2048_stagemean_step on the trained staged table

each at lr = 0 and lr = 1.  Recorded besides: the boards per stage of prev, and from one
stagemean call at lr = 1 per stage the entries it promoted and the entries it changed (promoted or
moved); promoted / changed is the share of the distinct entries written that the call found UNSET,
that is, that fell through.

--mode strength.  One row of DESIGN 4.12's 60-second 4 x 6 protocol per process: `--row` is one of
single (MeanTrainer on one table), staged (StagedMeanTrainer, bounds --bounds), staged_pool (the
same with RestartPool levels 0 and the first bound); --boards boards, p(4) = 0.5, --seed, for
--seconds of wall time; then --games games of the greedy player and of the depth-2 search
(play("ntuple_search") for the single table, play("ntstage_search") for a staged one).  Reports the
training means, the per-stage set counts and the largest |entry| at the quarter marks, and the
steps achieved.

    python tools/stagemean_bench.py [--mode cost] [--boards 65536] [--sets 2x4 4x6] [--out F.json]
    python tools/stagemean_bench.py --mode cost-trained [--train-seconds 20] [--spread-steps 4000]
    python tools/stagemean_bench.py --mode strength --row staged_pool --bounds 11 12
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


def timed(torch, fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms) * 1e3, min(ms) * 1e3, max(ms) * 1e3


def cost_mode(args, torch, g2048):
    from g2048 import ntmean, ntstage, ntuple, stagemean

    dev = torch.device("cuda:0")
    n, bounds = args.boards, tuple(args.bounds)
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
        first = tr.env.board.clone()
        tr.step(1)
        torch.cuda.synchronize()
        pair = (first, tr.env.board.clone())
        prev0, has0, shift = tr.prev.clone(), tr.has_prev.clone(), tr.lr_shift
        table = net.lut.clone()
        del tr
        stages = sorted(set(ntstage.StagedNTupleNetwork(tuples, bounds, device="cpu")
                            .stage_of(prev0.cpu()).tolist()))

        def rule(kind):
            """(step(lr_num), acc or None) of one rule on its own copy of the table and state."""
            prev, has = prev0.clone(), has0.clone()
            out = (torch.zeros(n, dtype=torch.uint8, device=dev),
                   torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.zeros(n, dtype=torch.int64, device=dev))
            flip = [0]
            if kind == "mean_step":
                own = ntuple.NTupleNetwork(tuples, device=dev)
                own.lut.copy_(table)
                state = ntmean.MeanState(own)
                call = state.mean_step
            else:
                own = ntstage.StagedNTupleNetwork(tuples, () if kind == "stagemean S=1" else bounds,
                                                  device=dev)
                own.lut[0].copy_(table)
                state = None if kind == "stage td_step" else stagemean.StagedMeanState(own)
                call = own.td_step if state is None else state.mean_step

            def step(lr_num):
                flip[0] ^= 1
                call(pair[flip[0]], prev, has, lr_num, shift, *out)

            return step, state, out

        for kind in ("mean_step", "stagemean S=1", "stage td_step", "stagemean"):
            step, state, out = rule(kind)
            for lr_num in (0, 1):
                med, lo, hi = timed(torch, lambda: step(lr_num), args.warmup, args.reps)
                row = {"set": name, "boards": n, "call": kind, "lr_num": lr_num, "us_median": med,
                       "us_min": lo, "us_max": hi, "reps": args.reps,
                       "bounds": list(bounds) if kind in ("stage td_step", "stagemean") else [],
                       "stages_of_prev": stages, "nonzero_deltas": int((out[1] != 0).sum())}
                rows.append(row)
                print(f"{name} n={n} {kind:14s} lr={lr_num} {med:9.1f} us (min {lo:.1f}, max "
                      f"{hi:.1f})  {n / (med * 1e-6):.3e} boards/s", flush=True)
            if state is not None:
                assert not bool(state.acc.any()), "acc is not all zero after the timed calls"
            del step, state, out
            torch.cuda.empty_cache()
        del net, table
        torch.cuda.empty_cache()
    if args.trainer_steps > 0:
        for name in args.sets:
            tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
            makers = (("mean", lambda: ntmean.MeanTrainer(
                          ntuple.NTupleNetwork(tuples, device=dev), args.trainer_boards,
                          seed=args.seed)),
                      ("staged td", lambda: ntuple.NTupleTrainer(
                          ntstage.StagedNTupleNetwork(tuples, bounds, device=dev),
                          args.trainer_boards, seed=args.seed)),
                      ("staged mean", lambda: stagemean.StagedMeanTrainer(
                          ntstage.StagedNTupleNetwork(tuples, bounds, device=dev),
                          args.trainer_boards, seed=args.seed)))
            for what, make in makers:
                tr = make()
                tr.step(200)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.step(args.trainer_steps)
                torch.cuda.synchronize()
                us = (time.perf_counter() - t0) / args.trainer_steps * 1e6
                rows.append({"set": name, "boards": args.trainer_boards,
                             "call": f"{what} trainer step", "us_per_step": us,
                             "steps": args.trainer_steps})
                print(f"{name} n={args.trainer_boards} {what:11s} trainer.step: {us:.1f} us per "
                      f"step over {args.trainer_steps} steps (wall)", flush=True)
                del tr
                torch.cuda.empty_cache()
    return {"play": args.play, "rows": rows}


def cost_trained_mode(args, torch, g2048):
    from g2048 import ntmean, ntstage, ntuple, stagemean

    dev = torch.device("cuda:0")
    n = args.boards
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        bounds = tuple(args.bounds_2x4 if name == "2x4" else args.bounds)
        net = ntstage.StagedNTupleNetwork(tuples, bounds, device=dev)
        tr = stagemean.StagedMeanTrainer(net, args.trainer_boards, seed=args.seed, p4=0.5)
        torch.cuda.synchronize()
        t0, trained = time.time(), 0
        while time.time() - t0 < args.train_seconds:
            tr.step(args.chunk)
            trained += args.chunk
            torch.cuda.synchronize()
        shift = tr.lr_shift
        acc = tr.mean  # one workspace per network: the wide trainer and the timed calls share it
        del tr
        wide = stagemean.StagedMeanTrainer(net, n, mean=acc, seed=args.seed + 1, p4=0.5)
        wide.step(args.spread_steps + 1)
        torch.cuda.synchronize()
        wide.env.check_errors()
        boards, prev0, has0 = wide.env.board.clone(), wide.prev.clone(), wide.has_prev.clone()
        del wide
        table = net.lut.clone()
        stage = net.stage_of(prev0)[has0 != 0]
        per_stage = [int((stage == s).sum()) for s in range(net.n_stages)]
        plain = net.resolved(0)
        plain_table, plain_acc = plain.lut.clone(), ntmean.MeanState(plain)
        prev, has = prev0.clone(), has0.clone()
        out = (torch.zeros(n, dtype=torch.uint8, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.int64, device=dev))

        def restore():
            net.lut.copy_(table)
            plain.lut.copy_(plain_table)
            prev.copy_(prev0)
            has.copy_(has0)

        # one call's writes, per stage: promoted = newly set, changed = promoted or moved
        restore()
        acc.mean_step(boards, prev, has, 1, shift, *out)
        promoted = [a - b for a, b in zip(net.set_counts(),
                                          [int(x) for x in (table != ntstage.UNSET)
                                           .sum(dim=(1, 2)).tolist()])]
        changed = [int(x) for x in (net.lut != table).sum(dim=(1, 2)).tolist()]
        info = {"set": name, "bounds": list(bounds), "boards": n, "train_seconds": args.train_seconds,
                "train_steps": trained, "train_boards": args.trainer_boards,
                "spread_steps": args.spread_steps, "boards_with_prev": int(has0.sum()),
                "prev_per_stage": per_stage, "nonzero_deltas": int((out[1] != 0).sum()),
                "set_counts": [int(x) for x in (table != ntstage.UNSET).sum(dim=(1, 2)).tolist()],
                "promoted_per_stage": promoted, "changed_per_stage": changed}
        rows.append(info)
        print(json.dumps(info), flush=True)
        calls = (("mean_step", plain_acc.mean_step), ("stage td_step", net.td_step),
                 ("stagemean", acc.mean_step))
        for kind, call in calls:
            for lr_num in (0, 1):
                ms = []
                for rep in range(args.warmup + args.reps):
                    restore()
                    e0 = torch.cuda.Event(enable_timing=True)
                    e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    call(boards, prev, has, lr_num, shift, *out)
                    e1.record()
                    e1.synchronize()
                    if rep >= args.warmup:
                        ms.append(e0.elapsed_time(e1) * 1e3)
                med = statistics.median(ms)
                rows.append({"set": name, "boards": n, "call": kind, "lr_num": lr_num,
                             "us_median": med, "us_min": min(ms), "us_max": max(ms),
                             "reps": len(ms), "bounds": list(bounds)})
                print(f"{name} trained n={n} {kind:14s} lr={lr_num} {med:9.1f} us (min "
                      f"{min(ms):.1f}, max {max(ms):.1f})", flush=True)
        assert not bool(acc.acc.any()) and not bool(plain_acc.acc.any())
        del net, table, plain, plain_table, plain_acc, acc
        torch.cuda.empty_cache()
    return {"rows": rows}


def strength_mode(args, torch, g2048):
    import numpy as np

    from g2048 import ntmean, ntstage, ntuple, stagemean
    from g2048.player import BatchedPlayer

    dev, bounds = "cuda:0", tuple(args.bounds)
    kw = dict(seed=args.seed, p4=0.5, log_slots=64)
    if args.row == "single":
        net = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device=dev)
        tr = ntmean.MeanTrainer(net, args.boards, **kw)
    else:
        net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_4x6, bounds, device=dev)
        if args.row == "staged_pool":
            kw["restart"] = g2048.RestartPool(args.boards, (0, bounds[0]), device=dev)
        tr = stagemean.StagedMeanTrainer(net, args.boards, **kw)

    def table_state():
        if args.row == "single":
            return {"largest_entry": int(net.lut.to(torch.int64).abs().max())}
        lut = torch.where(net.lut != ntstage.UNSET, net.lut, torch.zeros_like(net.lut))
        return {"largest_entry": int(lut.to(torch.int64).abs().max()),
                "set_counts": net.set_counts()}

    torch.cuda.synchronize()
    scores, done, t0, mark, marks = [], 0, time.time(), args.seconds / 4, []
    while time.time() - t0 < args.seconds:
        tr.step(args.chunk)
        done += args.chunk
        scores = (scores + tr.episodes(strict=False)["score"].tolist())[-2000:]
        if time.time() - t0 >= mark:
            mark += args.seconds / 4
            marks.append({"steps": done, "seconds": time.time() - t0,
                          "mean_last_200": float(np.mean(scores[-200:])), **table_state()})
            print(json.dumps(marks[-1]), flush=True)
    torch.cuda.synchronize()
    row = {"row": args.row, "bounds": list(bounds) if args.row != "single" else [],
           "boards": args.boards, "seed": args.seed, "lr_shift": tr.lr_shift, "steps": done,
           "train_seconds": time.time() - t0,
           "train_mean_last_200": float(np.mean(scores[-200:])), "marks": marks, **table_state()}
    tr.env.check_errors()
    del tr
    torch.cuda.empty_cache()
    search = "ntuple_search" if args.row == "single" else "ntstage_search"
    for policy, pkw in (("ntuple", {}), (search, {"search_depth": 2})):
        res = BatchedPlayer(args.games, device=dev, seed=args.seed + 1000, ntuple=net, p4=0.5,
                            **pkw).play(policy)
        row[policy] = {"mean_score": float(res.merge_score.mean()),
                       "max_tile_hist": {int(k): int(v)
                                         for k, v in zip(*res.max_tile_frequency())}}
    print(json.dumps(row), flush=True)
    return {"rows": [row]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="cost", choices=["cost", "cost-trained", "strength"])
    ap.add_argument("--boards", type=int, default=None,
                    help="cost: 65536; strength: 4096")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--bounds", type=int, nargs="*", default=[11])
    ap.add_argument("--bounds-2x4", type=int, nargs="*", default=[7],
                    help="cost-trained: the 2x4 set's bounds")
    ap.add_argument("--train-seconds", type=float, default=20.0)
    ap.add_argument("--spread-steps", type=int, default=4000)
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=None, help="cost: 0x2048; strength: 61")
    ap.add_argument("--trainer-boards", type=int, default=4096)
    ap.add_argument("--trainer-steps", type=int, default=2000, help="0 skips the trainer rows")
    ap.add_argument("--row", default="staged", choices=["single", "staged", "staged_pool"])
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = 4096 if args.mode == "strength" else 65536
    if args.seed is None:
        args.seed = 61 if args.mode == "strength" else 0x2048

    import torch

    import g2048

    g2048.load_native()
    for mod in (g2048.ntuple, g2048.ntstage, g2048.ntmean, g2048.stagemean):
        mod.load()
    mode = {"cost": cost_mode, "cost-trained": cost_trained_mode, "strength": strength_mode}
    result = mode[args.mode](args, torch, g2048)
    result.update(mode=args.mode, device=torch.cuda.get_device_name(0))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
