"""The multi-stage n-tuple network (g2048.ntstage) next to the single table (g2048.ntuple): launch
times by HIP events and playing strength.

--mode time (tools/ntuple_bench.py's method).  For each named tuple set a single table is filled
with random int32, `--boards` fresh boards are played forward `--play` random steps (auto-reset
on) and given previous afterstates by two TD steps.  Then, on those boards, each call of the
staged library is timed `--reps` times with an event pair, alternating rep by rep with the same
call of libg2048_ntuple.so on the single table (the yardstick), after `--warmup` calls of each:

    values, act, td_step lr=0 (both launches, every delta 0: promotion but no adds), td_step

for three staged tables built from the same single table:

    S=1          one stage, no UNSET: the stage computation and the UNSET test alone
    S=2 unset    bound 1, so every board is of stage 1, whose entries are all UNSET: every lookup
                 falls through and takes the second gather round.  The td rows promote what they
                 touch, so stage 1 is refilled with UNSET before every timed call (outside the
                 event pair).
    S=2 fresh    bound `--bound`, stage 1 all UNSET when the timing starts (not refilled): the
                 same stages as the next row before any training
    S=2 trained  bound `--bound`, after `--train-steps` steps of self-play on it: the mix of set
                 and UNSET entries a training run meets

With --uniform the timed boards and the previous afterstates are uniformly random exponents
0..11 (no entry is hot: the early-game entries a played batch shares do not occur); their largest
tile is 11 on three boards in four, so `--bound 11` splits them.

--mode strength4x6 (tools/nttc_bench.py's protocol).  Self-play on TUPLES_4x6 for `--seconds` of
wall time per rule in step(`--chunk`) chunks, the training mean at every quarter, then `--games`
games of play("ntuple"): mean score, max-tile counts, set entries per stage, largest |entry|.
The rules: `single` (one table, TD(0)), and one staged network per `--bounds` list.

    python tools/ntstage_bench.py [--mode time] [--boards 65536] [--sets 2x4 4x6] [--uniform]
                                  [--bound 6] [--out FILE]
    python tools/ntstage_bench.py --mode strength4x6 [--rules single 11 11,12] [--seconds 60]
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


class State:
    """The per-board state and outputs of one network's td_step."""

    def __init__(self, torch, net, tr):
        self.net = net
        self.prev, self.has_prev = tr.prev.clone(), tr.has_prev.clone()
        self.actions, self.delta = torch.zeros_like(tr.actions), torch.zeros_like(tr.delta)
        self.err = torch.zeros_like(tr.err)
        self.values = torch.zeros(tr.n, dtype=torch.int64, device=tr.prev.device)
        self.q = torch.zeros((tr.n, 4), dtype=torch.int64, device=tr.prev.device)
        self.lr_shift = tr.lr_shift
        self.flip = 0

    def call(self, what, pair):
        self.flip ^= 1
        boards = pair[self.flip]
        if what == "values":
            self.net.values(boards, out=self.values)
        elif what == "act":
            self.net.act(boards, q_out=self.q, actions_out=self.actions)
        else:
            self.net.td_step(boards, self.prev, self.has_prev, 0 if what == "td_step lr=0" else 1,
                             self.lr_shift, self.actions, self.delta, self.err)


def time_mode(args, torch, ntuple, ntstage):
    dev = torch.device("cuda:0")
    n = args.boards
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        net = ntuple.NTupleNetwork(tuples, device=dev)
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=gen, device=dev,
                                    dtype=torch.int32))
        lut0 = net.lut.clone()
        tr = ntuple.NTupleTrainer(net, n, seed=args.seed)
        for _ in range(args.play):
            tr.env.step(None)
        tr.step(2)  # every board gets a previous afterstate
        torch.cuda.synchronize()
        boards = tr.env.board.clone()
        tr.step(1)
        torch.cuda.synchronize()
        # every call alternates between two consecutive states of the batch, so it meets
        # afterstates of other boards than its own and errors that do not vanish
        pair = (boards, tr.env.board.clone())
        if args.uniform:
            def fresh():
                return torch.randint(0, 12, (n, 16), generator=gen, device=dev, dtype=torch.uint8)
            pair = (fresh(), fresh())
            tr.prev.copy_(fresh())
            tr.has_prev.fill_(1)
        net.lut.copy_(lut0)
        trained = ntstage.StagedNTupleNetwork.from_network(net, (args.bound,))
        ttr = ntuple.NTupleTrainer(trained, n, seed=args.seed)
        for _ in range(args.play):
            ttr.env.step(None)
        ttr.step(args.train_steps)
        ttr.env.check_errors()
        configs = [("S=1", ntstage.StagedNTupleNetwork.from_network(net, ())),
                   ("S=2 unset", ntstage.StagedNTupleNetwork.from_network(net, (1,))),
                   ("S=2 fresh", ntstage.StagedNTupleNetwork.from_network(net, (args.bound,))),
                   ("S=2 trained", trained)]
        del ttr
        stage_share = [float((trained.stage_of(pair[0]) == s).float().mean()) for s in (0, 1)]
        print(f"{name}: share of the timed boards in stage 0 / 1 at bound {args.bound}: "
              f"{stage_share[0]:.3f} / {stage_share[1]:.3f}", flush=True)
        torch.cuda.synchronize()
        for config, staged in configs:
            for what in ("values", "act", "td_step lr=0", "td_step"):
                a, b = State(torch, net, tr), State(torch, staged, tr)
                unset = config == "S=2 unset" and what.startswith("td_step")
                for _ in range(args.warmup):
                    a.call(what, pair)
                    b.call(what, pair)
                torch.cuda.synchronize()
                ms = {"single": [], "staged": []}
                for _ in range(args.reps):
                    for key, st in (("single", a), ("staged", b)):
                        if unset and key == "staged":
                            staged.lut[1].fill_(ntstage.UNSET)
                        e0 = torch.cuda.Event(enable_timing=True)
                        e1 = torch.cuda.Event(enable_timing=True)
                        e0.record()
                        st.call(what, pair)
                        e1.record()
                        e1.synchronize()
                        ms[key].append(e0.elapsed_time(e1))
                med = {k: statistics.median(v) for k, v in ms.items()}
                row = {"set": name, "config": config, "call": what, "boards": n,
                       "table_bytes": staged.lut.numel() * 4, "set_counts": staged.set_counts(),
                       "us_median": med["staged"] * 1e3, "us_min": min(ms["staged"]) * 1e3,
                       "us_max": max(ms["staged"]) * 1e3,
                       "single_us_median": med["single"] * 1e3,
                       "single_us_min": min(ms["single"]) * 1e3,
                       "single_us_max": max(ms["single"]) * 1e3, "reps": args.reps,
                       "ratio": med["staged"] / med["single"]}
                if what == "td_step":
                    row["nonzero_deltas"] = int((b.delta != 0).sum())
                    row["single_nonzero_deltas"] = int((a.delta != 0).sum())
                if config in ("S=2 fresh", "S=2 trained"):
                    row["bound"], row["stage_share"] = args.bound, stage_share
                rows.append(row)
                print(f"{name} {config:11s} n={n} {what:12s} {row['us_median']:8.1f} us (min "
                      f"{row['us_min']:.1f}, max {row['us_max']:.1f})  single table "
                      f"{row['single_us_median']:8.1f} us (min {row['single_us_min']:.1f}, max "
                      f"{row['single_us_max']:.1f})  {row['ratio']:.2f}x  set entries "
                      f"{row['set_counts']}"
                      + (f"  boards that add {row['nonzero_deltas']} (single "
                         f"{row['single_nonzero_deltas']})" if what == "td_step" else ""),
                      flush=True)
                net.lut.copy_(lut0)  # the yardstick's table does not drift from config to config
        tr.env.check_errors()
        del tr, net, configs, trained
        torch.cuda.empty_cache()
    return {"play": args.play, "uniform": args.uniform, "bound": args.bound, "train_steps": args.train_steps, "rows": rows}


def largest(net, torch, unset=None):
    lut = net.lut if unset is None else torch.where(net.lut != unset, net.lut,
                                                    torch.zeros_like(net.lut))
    return int(lut.to(torch.int64).abs().max())


def strength4x6(args, torch, ntuple, ntstage):
    import numpy as np

    from g2048.player import BatchedPlayer

    rows = []
    for rule in args.rules:
        if rule == "single":
            net, unset = ntuple.NTupleNetwork(ntuple.TUPLES_4x6, device="cuda:0"), None
        else:
            bounds = tuple(int(b) for b in rule.split(","))
            net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_4x6, bounds, device="cuda:0")
            unset = ntstage.UNSET
        tr = ntuple.NTupleTrainer(net, args.boards, seed=args.seed, p4=0.5,
                                  lr_shift=args.lr_shift, log_slots=64)
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
                                  "largest_entry": largest(net, torch, unset)}), flush=True)
        torch.cuda.synchronize()
        row = {"rule": rule, "boards": args.boards, "lr_shift": tr.lr_shift, "steps": done,
               "board_steps": done * args.boards, "train_seconds": time.time() - t0,
               "train_mean_last_200": float(np.mean(scores[-200:])),
               "largest_entry": largest(net, torch, unset)}
        if unset is not None:
            row["set_counts"] = net.set_counts()
        tr.env.check_errors()
        del tr
        torch.cuda.empty_cache()
        res = BatchedPlayer(args.games, device="cuda:0", seed=args.seed + 1000, ntuple=net,
                            p4=0.5).play("ntuple")
        row["ntuple"] = {"mean_score": float(res.merge_score.mean()),
                         "max_tile_hist": {int(k): int(v)
                                           for k, v in zip(*res.max_tile_frequency())}}
        rows.append(row)
        print(json.dumps(row), flush=True)
        del net
        torch.cuda.empty_cache()
    return {"rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="time", choices=["time", "strength4x6"])
    ap.add_argument("--boards", type=int, default=None,
                    help="default: 65536 (time), 4096 (strength4x6)")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=None, help="default: 0x2048 (time), 61 (strength)")
    ap.add_argument("--uniform", action="store_true",
                    help="time mode: boards and previous afterstates of uniformly random "
                         "exponents 0..11 instead of played ones: no entry is hot")
    ap.add_argument("--bound", type=int, default=6,
                    help="time mode: the bound of the trained two-stage table")
    ap.add_argument("--train-steps", type=int, default=300,
                    help="time mode: self-play steps on the trained two-stage table")
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--lr-shift", type=int, default=None, help="default: default_lr_shift(boards)")
    ap.add_argument("--rules", nargs="+", default=["single", "11", "11,12"],
                    help="strength4x6: `single` or a comma-separated list of bounds")
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.boards is None:
        args.boards = {"time": 65536, "strength4x6": 4096}[args.mode]
    if args.seed is None:
        args.seed = {"time": 0x2048, "strength4x6": 61}[args.mode]

    import torch

    import g2048  # noqa: F401
    from g2048 import ntstage, ntuple

    if not torch.cuda.is_available():
        raise SystemExit("ntstage_bench needs a GPU")
    ntstage.load()
    out = {"time": time_mode, "strength4x6": strength4x6}[args.mode](args, torch, ntuple, ntstage)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"mode": args.mode, **out}, f, indent=1)


if __name__ == "__main__":
    main()
