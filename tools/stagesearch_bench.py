"""The expectimax over the multi-stage n-tuple network (g2048.stagesearch) next to the search over
the single table (g2048.ntsearch): launch times by HIP events and playing strength.

--mode time (tools/ntstage_bench.py's method).  For each named tuple set a single table is filled
with random int32 and, for each batch size, fresh boards are played forward `--play` random steps
(auto-reset on).  On those boards each staged search is timed `--reps` times with an event pair,
alternating rep by rep with `g2048_ntsearch_expectimax` on the single table at the same depth (the
yardstick: the existing library, not the code under test), after `--warmup` calls of each, for
three staged tables built from the same single table:

    S=1          one stage, no UNSET: the stage computation and the UNSET tests alone
    S=2 unset    bound 1, so every board and every leaf is of stage 1, whose entries are all
                 UNSET: every gather falls through and is read a second time
    S=2 trained  bound `--bound`, after `--train-steps` steps of self-play on it: the mix of set
                 and UNSET entries a training run meets, roots and leaves in both stages

--mode strength.  What valuing every leaf at its own stage buys over one frozen stage.  `2x4`:
StagedNTupleNetwork(TUPLES_2x4, bounds (7,)) trained as
tests/test_ntstage_gpu.py::test_staged_self_play_learns trains it (256 boards, `--steps` steps,
seed 61).  `4x6:BOUNDS`: tools/ntstage_bench.py's strength4x6 protocol (4 096 boards, `--seconds`
of wall time).  Then `--games` games on one seed for each of: play("ntuple"), ntstage_search at
depths 1, 2 and 3 (depth 3 on the 2x4 table only), and the single-table search at depth 2 over
resolved(0) and over resolved(S - 1): mean score, mean moves, max-tile counts, wall time.

    python tools/stagesearch_bench.py [--mode time] [--sets 2x4 4x6] [--sizes 1024 65536]
                                      [--depths 1 2 3] [--bound 6] [--out FILE]
                                      [--lib OTHER_BUILD.so] [--ntsearch-lib OTHER_BUILD.so]
    python tools/stagesearch_bench.py --mode strength [--nets 2x4 4x6:11] [--seconds 60]
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


def time_mode(args, torch, g2048):
    from g2048 import ntsearch, ntstage, ntuple, stagesearch

    dev = torch.device("cuda:0")
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        net = ntuple.NTupleNetwork(tuples, device=dev)
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=gen, device=dev,
                                    dtype=torch.int32))
        trained = ntstage.StagedNTupleNetwork.from_network(net, (args.bound,))
        ttr = ntuple.NTupleTrainer(trained, args.train_boards, seed=args.seed)
        for _ in range(args.play):
            ttr.env.step(None)
        ttr.step(args.train_steps)
        ttr.env.check_errors()
        del ttr
        configs = [("S=1", ntstage.StagedNTupleNetwork.from_network(net, ())),
                   ("S=2 unset", ntstage.StagedNTupleNetwork.from_network(net, (1,))),
                   ("S=2 trained", trained)]
        for n in args.sizes:
            env = g2048.VecEnv2048(n, seed=args.seed, device=dev, p4=args.p4)
            for _ in range(args.play):
                env.step(None)
            torch.cuda.synchronize()
            env.check_errors()
            boards = env.board.clone()
            share = [float((trained.stage_of(boards) == s).float().mean()) for s in (0, 1)]
            print(f"{name} n={n}: share of the timed boards in stage 0 / 1 at bound "
                  f"{args.bound}: {share[0]:.3f} / {share[1]:.3f}", flush=True)
            out = [(torch.empty(n, dtype=torch.uint8, device=dev),
                    torch.empty((n, 4), dtype=torch.int64, device=dev)) for _ in range(2)]
            for config, staged in configs:
                for depth in args.depths:
                    calls = {"single": lambda: ntsearch.expectimax(
                                 net, boards, depth, args.p4, values_out=out[0][1],
                                 actions_out=out[0][0]),
                             "staged": lambda: stagesearch.expectimax(
                                 staged, boards, depth, args.p4, values_out=out[1][1],
                                 actions_out=out[1][0])}
                    for _ in range(args.warmup):
                        for fn in calls.values():
                            fn()
                    torch.cuda.synchronize()
                    ms = {"single": [], "staged": []}
                    for _ in range(args.reps):
                        for key, fn in calls.items():
                            e0 = torch.cuda.Event(enable_timing=True)
                            e1 = torch.cuda.Event(enable_timing=True)
                            e0.record()
                            fn()
                            e1.record()
                            e1.synchronize()
                            ms[key].append(e0.elapsed_time(e1))
                    med = {k: statistics.median(v) for k, v in ms.items()}
                    row = {"set": name, "config": config, "boards": n, "depth": depth,
                           "table_bytes": staged.lut.numel() * 4,
                           "set_counts": staged.set_counts(),
                           "us_median": med["staged"] * 1e3, "us_min": min(ms["staged"]) * 1e3,
                           "us_max": max(ms["staged"]) * 1e3,
                           "single_us_median": med["single"] * 1e3,
                           "single_us_min": min(ms["single"]) * 1e3,
                           "single_us_max": max(ms["single"]) * 1e3, "reps": args.reps,
                           "us": [m * 1e3 for m in ms["staged"]],
                           "single_us": [m * 1e3 for m in ms["single"]],
                           "ratio": med["staged"] / med["single"],
                           # the identities: S = 1 and the lifted table search as the single one
                           "equal_to_single": bool(torch.equal(out[0][1], out[1][1]))}
                    if config == "S=2 trained":
                        row["bound"], row["stage_share"] = args.bound, share
                    rows.append(row)
                    print(f"{name} {config:11s} n={n:6d} depth={depth} {row['us_median']:11.1f} us "
                          f"(min {row['us_min']:.1f}, max {row['us_max']:.1f})  single table "
                          f"{row['single_us_median']:11.1f} us (min {row['single_us_min']:.1f}, "
                          f"max {row['single_us_max']:.1f})  {row['ratio']:.2f}x  values equal: "
                          f"{row['equal_to_single']}", flush=True)
        del net, configs, trained
        torch.cuda.empty_cache()
    return {"play": args.play, "p4": args.p4, "bound": args.bound, "lib": args.lib,
            "ntsearch_lib": args.ntsearch_lib,
            "train_steps": args.train_steps, "train_boards": args.train_boards, "rows": rows}


def strength_mode(args, torch, g2048):
    import numpy as np

    from g2048 import ntstage, ntuple
    from g2048.player import BatchedPlayer

    out = []
    for spec in args.nets:
        name, _, bounds = spec.partition(":")
        if name == "2x4":
            bounds = tuple(int(b) for b in bounds.split(",")) if bounds else (7,)
            net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_2x4, bounds, device="cuda:0")
            tr = ntuple.NTupleTrainer(net, 256, seed=args.seed, p4=0.5, lr_num=1, lr_shift=10,
                                      log_slots=64)
            t0, done = time.time(), 0
            while done < args.steps:
                tr.step(1000)
                tr.episodes()
                done += 1000
        else:
            bounds = tuple(int(b) for b in bounds.split(",")) if bounds else (11,)
            net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_4x6, bounds, device="cuda:0")
            tr = ntuple.NTupleTrainer(net, 4096, seed=args.seed, p4=0.5, log_slots=64)
            torch.cuda.synchronize()
            t0, done = time.time(), 0
            while time.time() - t0 < args.seconds:
                tr.step(1000)
                tr.episodes(strict=False)
                done += 1000
        torch.cuda.synchronize()
        tr.env.check_errors()
        head = {"net": name, "bounds": list(bounds), "train_steps": done, "boards": tr.n,
                "train_seconds": time.time() - t0, "set_counts": net.set_counts()}
        print(json.dumps(head), flush=True)
        del tr
        torch.cuda.empty_cache()
        top = net.n_stages - 1
        policies = [("ntuple", net, "ntuple", 2), ("ntstage_search d1", net, "ntstage_search", 1),
                    ("ntstage_search d2", net, "ntstage_search", 2)]
        if name == "2x4":
            policies.append(("ntstage_search d3", net, "ntstage_search", 3))
        policies += [("resolved(0).search d2", net.resolved(0), "ntuple_search", 2),
                     (f"resolved({top}).search d2", net.resolved(top), "ntuple_search", 2)]
        rows = []
        for label, player_net, policy, depth in policies:
            t0 = time.time()
            res = BatchedPlayer(args.games, device="cuda:0", seed=args.seed + 1000,
                                ntuple=player_net, p4=0.5, search_depth=depth).play(policy)
            row = {"policy": label, "games": args.games,
                   "mean_score": float(res.merge_score.mean()),
                   "median_score": float(np.median(res.merge_score)),
                   "mean_moves": float(res.moves.mean()),
                   "max_tile_hist": {int(k): int(v) for k, v in zip(*res.max_tile_frequency())},
                   "stuck": int(res.stuck.sum()), "seconds": time.time() - t0}
            rows.append(row)
            print(json.dumps(row), flush=True)
        out.append({**head, "rows": rows})
        del net, policies
        torch.cuda.empty_cache()
    return {"nets": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=["time", "strength"])
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--p4", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=None, help="default: 0x2048 (time), 61 (strength)")
    ap.add_argument("--bound", type=int, default=6,
                    help="time mode: the bound of the trained two-stage table")
    ap.add_argument("--train-steps", type=int, default=300,
                    help="time mode: self-play steps on the trained two-stage table")
    ap.add_argument("--train-boards", type=int, default=65536,
                    help="time mode: boards of that self-play")
    ap.add_argument("--nets", nargs="+", default=["2x4"],
                    help="strength: `2x4` or `4x6`, with `:b0,b1,...` for other bounds than (7,) "
                         "and (11,)")
    ap.add_argument("--steps", type=int, default=4000, help="strength, 2x4: training steps")
    ap.add_argument("--seconds", type=float, default=60.0, help="strength, 4x6: training time")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--lib", default=None,
                    help="time another build of libg2048_stagesearch.so (such as the parent "
                         "commit's, or one with -DG2048_STAGESEARCH_LEAF_TUPLES=3)")
    ap.add_argument("--ntsearch-lib", default=None,
                    help="another build of libg2048_ntsearch.so, the library it alternates with")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.seed is None:
        args.seed = {"time": 0x2048, "strength": 61}[args.mode]

    import torch

    import g2048

    if not torch.cuda.is_available():
        raise SystemExit("stagesearch_bench needs a GPU")
    if args.lib:
        g2048.stagesearch.LIB_PATH = os.path.abspath(args.lib)
    if args.ntsearch_lib:
        g2048.ntsearch.LIB_PATH = os.path.abspath(args.ntsearch_lib)
    g2048.stagesearch.load()
    out = {"time": time_mode, "strength": strength_mode}[args.mode](args, torch, g2048)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
