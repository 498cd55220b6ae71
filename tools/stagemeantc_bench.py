"""Temporal-coherence learning on the batch-mean rule for the multi-stage network
(g2048.stagemeantc) next to the staged TD(0) step, the staged batch-mean step and the single-table
batch-mean TC step: launch times by HIP events and playing strength.  Modelled on
tools/stagemean_bench.py and tools/ntmeantc_bench.py.  One process per row of a table, each under
its own time limit.

--mode cost (DESIGN 4.17's method).  For each named tuple set a single table is filled with random
int32, `--boards` fresh boards are played forward `--play` random steps (auto-reset on) and two
consecutive states of the batch are kept; every rule below then alternates between them from the
same previous afterstates, in this process, is warmed up `--warmup` times and is timed `--reps`
times with an event pair (median, min - max), each at lr = 0 (nothing gathered or applied; the
staged policy launch still promotes) and at lr = 1:

    meantc_step           g2048_ntmeantc_step on the single table, zero ea
    stage td_step         g2048_ntstage_td_step, bounds --bounds, stage 0 = the table, rest UNSET
    stagemean             g2048_stagemean_step on the same staged table
    stagemeantc           g2048_stagemeantc_step on the same staged table, zero ea
    stagemeantc trained   the same from the ea that `--trained-steps` steps of
                          StagedMeanTCTrainer at `--trainer-boards` boards left

Random play reaches no late stage, so the staged rows see stage-0 boards only: what they measure
is the cost of the staged index, of the promotion and of the (E, A) traffic.  Then the wall time
per step of the trainers' step(k) at `--trainer-boards` boards.

--mode strength.  One row of DESIGN 4.12's 60-second 4 x 6 protocol per process: `--row` is one of
single_meantc (MeanTCTrainer on one table), staged_mean (StagedMeanTrainer), staged_meantc
(StagedMeanTCTrainer), staged_meantc_pool (the same with RestartPool levels 0 and the first
bound); staged rows with bounds --bounds; --boards boards, p(4) = 0.5, --seed, each rule at its
default rate (or --lr-shift), for --seconds of wall time; then --games games of the greedy player
and of the depth-2 search (play("ntuple_search") for the single table, play("ntstage_search") for
a staged one).  Reports the training means, the per-stage set counts, the largest |entry| and,
for the TC rows, the per-stage histogram of rate(E, A) at the quarter marks.

    python tools/stagemeantc_bench.py [--mode cost] [--boards 65536] [--sets 2x4 4x6] [--out F]
    python tools/stagemeantc_bench.py --mode strength --row staged_meantc_pool --bounds 11 12
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

BINS = ((0, 1 << 12), (1 << 12, 1 << 14), (1 << 14, 1 << 15), (1 << 15, (1 << 16) + 1))


def rate_histogram(ea, torch):
    """Over the entries with A > 0: the share of rate(E, A) in [0, 2^12), [2^12, 2^14),
    [2^14, 2^15), [2^15, 2^16], the median rate and the count.  The header's integer rate."""
    A = ea[..., 1].reshape(-1)
    keep = A > 0
    a, e = A[keep], ea[..., 0].reshape(-1)[keep].abs()
    if a.numel() == 0:
        return {"entries": 0}
    s = torch.zeros_like(a)
    for k in range(16, 62):
        s += (a >> k) > 0
    rate = ((e >> s) << 16) // (a >> s)
    return {"entries": int(a.numel()),
            "share": [float(((rate >= lo) & (rate < hi)).sum()) / a.numel() for lo, hi in BINS],
            "median_rate": int(rate.median()),
            "at_full_rate": float((rate == 1 << 16).sum()) / a.numel()}


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


KINDS = ("meantc_step", "stage td_step", "stagemean", "stagemeantc", "stagemeantc trained")


def cost_mode(args, torch, g2048):
    from g2048 import ntmeantc, ntstage, ntuple, stagemean, stagemeantc

    dev = torch.device("cuda:0")
    n, bounds = args.boards, tuple(args.bounds)
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        # the ea of a trained run, at the trainer-loop width
        tnet = ntstage.StagedNTupleNetwork(tuples, bounds, device=dev)
        ttr = stagemeantc.StagedMeanTCTrainer(tnet, args.trainer_boards, seed=args.seed, p4=0.5)
        ttr.step(args.trained_steps)
        torch.cuda.synchronize()
        trained_ea = ttr.state.ea.clone()
        hist = [rate_histogram(trained_ea[s], torch) for s in range(tnet.n_stages)]
        del ttr, tnet
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
        del tr, net

        def rule(kind):
            """(step(lr_num), state or None, outputs) of one rule on its own copy of the table."""
            prev, has = prev0.clone(), has0.clone()
            out = (torch.zeros(n, dtype=torch.uint8, device=dev),
                   torch.zeros(n, dtype=torch.int32, device=dev),
                   torch.zeros(n, dtype=torch.int64, device=dev))
            flip = [0]
            if kind == "meantc_step":
                own = ntuple.NTupleNetwork(tuples, device=dev)
                own.lut.copy_(table)
                state = ntmeantc.MeanTCState(own)
                call = state.meantc_step
            else:
                own = ntstage.StagedNTupleNetwork(tuples, bounds, device=dev)
                own.lut[0].copy_(table)
                if kind == "stage td_step":
                    state, call = None, own.td_step
                elif kind == "stagemean":
                    state = stagemean.StagedMeanState(own)
                    call = state.mean_step
                else:
                    state = stagemeantc.StagedMeanTCState(own)
                    if kind.endswith("trained"):
                        state.ea.copy_(trained_ea)
                    call = state.meantc_step

            def step(lr_num):
                flip[0] ^= 1
                call(pair[flip[0]], prev, has, lr_num, shift, *out)

            return step, state, out

        med = {}
        for kind in KINDS:
            step, state, out = rule(kind)
            for lr_num in (0, 1):
                us, lo, hi = timed(torch, lambda: step(lr_num), args.warmup, args.reps)
                med[(kind, lr_num)] = us
                row = {"set": name, "boards": n, "call": kind, "lr_num": lr_num, "us_median": us,
                       "us_min": lo, "us_max": hi, "reps": args.reps,
                       "bounds": [] if kind == "meantc_step" else list(bounds),
                       "nonzero_deltas": int((out[1] != 0).sum())}
                extra = ""
                if kind.startswith("stagemeantc"):
                    for yard in KINDS[:3]:
                        row["ratio_to_" + yard] = us / med[(yard, lr_num)]
                        extra += f"  {us / med[(yard, lr_num)]:.2f}x {yard}"
                rows.append(row)
                print(f"{name} n={n} {kind:20s} lr={lr_num} {us:9.1f} us (min {lo:.1f}, max "
                      f"{hi:.1f}){extra}", flush=True)
            if state is not None:
                assert not bool(state.acc.any()), "acc is not all zero after the timed calls"
            if hasattr(state, "ea"):
                assert bool((state.ea[..., 0].abs() <= state.ea[..., 1]).all())
            del step, state, out
            torch.cuda.empty_cache()
        rows.append({"set": name, "call": "trained ea", "steps": args.trained_steps,
                     "boards": args.trainer_boards, "bounds": list(bounds),
                     "rates_per_stage": hist})
        print(f"{name} trained ea after {args.trained_steps} steps: {json.dumps(hist)}",
              flush=True)
        del table, trained_ea
        torch.cuda.empty_cache()
    if args.trainer_steps > 0:
        for name in args.sets:
            tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6

            def staged():
                return ntstage.StagedNTupleNetwork(tuples, bounds, device=dev)

            makers = (("meantc", lambda: ntmeantc.MeanTCTrainer(
                          ntuple.NTupleNetwork(tuples, device=dev), args.trainer_boards,
                          seed=args.seed)),
                      ("staged td", lambda: ntuple.NTupleTrainer(staged(), args.trainer_boards,
                                                                 seed=args.seed)),
                      ("staged mean", lambda: stagemean.StagedMeanTrainer(
                          staged(), args.trainer_boards, seed=args.seed)),
                      ("staged meantc", lambda: stagemeantc.StagedMeanTCTrainer(
                          staged(), args.trainer_boards, seed=args.seed)))
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
                print(f"{name} n={args.trainer_boards} {what:13s} trainer.step: {us:.1f} us per "
                      f"step over {args.trainer_steps} steps (wall)", flush=True)
                del tr
                torch.cuda.empty_cache()
    return {"play": args.play, "rows": rows}


def strength_mode(args, torch, g2048):
    import numpy as np

    from g2048 import ntmeantc, ntstage, ntuple, stagemean, stagemeantc
    from g2048.player import BatchedPlayer

    dev, bounds = "cuda:0", tuple(args.bounds)
    kw = dict(seed=args.seed, p4=0.5, log_slots=64, lr_shift=args.lr_shift)
    single = args.row == "single_meantc"
    if single:
        net = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device=dev)
        tr = ntmeantc.MeanTCTrainer(net, args.boards, **kw)
    else:
        net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_4x6, bounds, device=dev)
        if args.row == "staged_meantc_pool":
            kw["restart"] = g2048.RestartPool(args.boards, (0, bounds[0]), device=dev)
        cls = stagemean.StagedMeanTrainer if args.row == "staged_mean" \
            else stagemeantc.StagedMeanTCTrainer
        tr = cls(net, args.boards, **kw)

    def table_state():
        if single:
            out = {"largest_entry": int(net.lut.to(torch.int64).abs().max())}
        else:
            lut = torch.where(net.lut != ntstage.UNSET, net.lut, torch.zeros_like(net.lut))
            out = {"largest_entry": int(lut.to(torch.int64).abs().max()),
                   "set_counts": net.set_counts()}
        if hasattr(tr, "state"):
            ea = tr.state.ea
            out["rates_per_stage"] = ([rate_histogram(ea, torch)] if single else
                                      [rate_histogram(ea[s], torch) for s in range(ea.shape[0])])
        return out

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
    row = {"row": args.row, "bounds": [] if single else list(bounds), "boards": args.boards,
           "seed": args.seed, "lr_shift": tr.lr_shift, "steps": done,
           "train_seconds": time.time() - t0,
           "train_mean_last_200": float(np.mean(scores[-200:])), "marks": marks, **table_state()}
    tr.env.check_errors()
    del tr
    torch.cuda.empty_cache()
    search = "ntuple_search" if single else "ntstage_search"
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
    ap.add_argument("--mode", default="cost", choices=["cost", "strength"])
    ap.add_argument("--boards", type=int, default=None, help="cost: 65536; strength: 4096")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--bounds", type=int, nargs="*", default=[11])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=None, help="cost: 0x2048; strength: 61")
    ap.add_argument("--trainer-boards", type=int, default=4096)
    ap.add_argument("--trainer-steps", type=int, default=2000, help="0 skips the trainer rows")
    ap.add_argument("--trained-steps", type=int, default=2000,
                    help="StagedMeanTCTrainer steps behind the cost mode's trained ea")
    ap.add_argument("--row", default="staged_meantc",
                    choices=["single_meantc", "staged_mean", "staged_meantc",
                             "staged_meantc_pool"])
    ap.add_argument("--lr-shift", type=int, default=None, help="default: the rule's own default")
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

    if not torch.cuda.is_available():
        raise SystemExit("stagemeantc_bench needs a GPU")
    g2048.load_native()
    for mod in (g2048.ntuple, g2048.ntstage, g2048.stagemean, g2048.ntmeantc, g2048.stagemeantc):
        mod.load()
    mode = {"cost": cost_mode, "strength": strength_mode}
    result = mode[args.mode](args, torch, g2048)
    result.update(mode=args.mode, device=torch.cuda.get_device_name(0))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
