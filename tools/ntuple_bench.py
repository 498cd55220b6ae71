"""Launch times of the n-tuple network kernels (g2048.ntuple) by HIP events.

For each named tuple set (TUPLES_2x4 in a 512 KiB table, TUPLES_4x6 in a 256 MiB table) the table
is filled with random int32, `--boards` fresh boards are played forward `--play` random steps
(auto-reset on), and four calls are warmed up and then timed `--reps` times with an event pair
each:

    values           V(board)                                   8 T gathers per board
    act              q, action and afterstate                   up to 32 T gathers per board
    td_step lr=0     both launches, every delta 0               up to 40 T gathers, no atomics
    td_step          both launches                              ... + 8 T atomic adds per board
    td_step+step     td_step followed by env.step (the training loop's body)

The difference between the two td_step rows prices the scatter: atomic adds per second =
boards with a non-zero delta * 8 T / that difference.

With --uniform the boards and the previous afterstates are uniformly random exponents 0..11
(no entry is hot), which separates the scatter rate from the contention on the early-game
entries that played boards share.

    python tools/ntuple_bench.py [--boards 65536] [--sets 2x4 4x6] [--uniform] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning-2048_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--boards", type=int, default=65536)
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--uniform", action="store_true",
                    help="boards and previous afterstates of uniformly random exponents 0..11 "
                         "instead of played ones: no entry is hot, so the td_step rows price "
                         "the scatter without contention")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import g2048
    from g2048 import ntuple

    if not torch.cuda.is_available():
        raise SystemExit("ntuple_bench needs a GPU: timings come from HIP events")
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
        # td_step alternates between two consecutive states of the batch, so every call meets
        # afterstates of other boards than its own and errors that do not vanish
        pair, flip = (boards, tr.env.board.clone()), [0]
        if args.uniform:
            def fresh():
                return torch.randint(0, 12, (n, 16), generator=gen, device=dev, dtype=torch.uint8)
            boards, pair, prev0 = fresh(), (fresh(), fresh()), fresh()
            tr.has_prev.fill_(1)
        with_prev = int(tr.has_prev.sum())
        vals = torch.empty(n, dtype=torch.int64, device=dev)
        q = torch.empty((n, 4), dtype=torch.int64, device=dev)
        after = torch.empty((n, 16), dtype=torch.uint8, device=dev)
        T = len(tuples)

        def td(lr_num):
            flip[0] ^= 1
            net.td_step(pair[flip[0]], tr.prev, tr.has_prev, lr_num, tr.lr_shift, tr.actions,
                        tr.delta, tr.err)

        calls = [("values", lambda: net.values(boards, out=vals)),
                 ("act", lambda: net.act(boards, q_out=q, actions_out=tr.actions,
                                         after_out=after)),
                 ("td_step lr=0", lambda: td(0)),
                 ("td_step", lambda: td(1)),
                 ("td_step+step", lambda: tr.step(1))]
        if args.uniform:  # the env's boards are played ones
            calls.pop()
        med = {}
        for what, fn in calls:
            for _ in range(args.warmup):
                fn()
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if args.uniform and what.startswith("td_step"):
                    tr.prev.copy_(prev0)
                    tr.has_prev.fill_(1)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med[what] = statistics.median(ms)
            row = {"set": name, "table_bytes": net.lut.numel() * 4, "boards": n, "call": what,
                   "us_median": med[what] * 1e3, "us_min": min(ms) * 1e3, "us_max": max(ms) * 1e3,
                   "reps": len(ms), "boards_per_s": n / (med[what] * 1e-3)}
            if what == "td_step":
                row["boards_with_prev"] = with_prev
                row["nonzero_deltas"] = int((tr.delta != 0).sum())
                gap = (med["td_step"] - med["td_step lr=0"]) * 1e-3
                row["atomic_adds_per_s"] = row["nonzero_deltas"] * 8 * T / gap if gap > 0 else None
            rows.append(row)
            extra = (f"  {row['atomic_adds_per_s']:.3e} atomic adds/s over the lr=0 run "
                     f"({row['nonzero_deltas']} boards add)"
                     if row.get("atomic_adds_per_s") else "")
            print(f"{name} ({row['table_bytes'] >> 10} KiB) n={n} {what:13s} "
                  f"{row['us_median']:9.1f} us (min {row['us_min']:.1f}, max {row['us_max']:.1f})"
                  f"  {row['boards_per_s']:.3e} boards/s{extra}", flush=True)
        tr.env.check_errors()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"play": args.play, "uniform": args.uniform, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
