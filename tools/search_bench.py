"""Launch time of the expectimax search kernel (g2048.search.expectimax) by HIP events.

Boards are mid-game states: fresh boards played forward `--play` steps by the depth-1 search
policy (auto-reset on, so a few are early-game again).  For each depth and batch size the launch
is warmed up, then timed `--reps` times with an event pair each; the table gives the median and
the spread, boards/s, and leaf evaluations/s.  The leaves per board are counted on the CPU over
a sample of the boards by walking the same tree (tests/expectimax_ref.py's slide), not measured.

    python tools/search_bench.py [--depths 1 2 3] [--sizes 1024 65536] [--out FILE.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning-2048_amd"), os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def leaf_counter():
    """leaves(board bytes, d): heuristic-or-terminal evaluations under a max node searched d
    more player moves deep (a pure function of the node, so it is memoised)."""
    import expectimax_ref as R

    memo = {}

    def under_move(after, d):
        return sum(leaves(after[:c] + bytes([e]) + after[c + 1:], d)
                   for c in range(16) if after[c] == 0 for e in (1, 2))

    def leaves(key, d):
        got = memo.get((key, d))
        if got is None:
            if d == 0 or not R.has_move(key):
                got = 1
            else:
                got = 0
                for a in range(4):
                    after = bytes(R.move(key, a)[0])
                    if after != key:
                        got += under_move(after, d - 1)
            memo[(key, d)] = got
        return got

    def root(board, depth):
        key = bytes(int(x) for x in board)
        total = 0
        for a in range(4):
            after = bytes(R.move(key, a)[0])
            if after != key:
                total += under_move(after, depth - 1)
        return total

    return root


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--depths", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--sizes", type=int, nargs="+", default=[1024, 65536])
    ap.add_argument("--play", type=int, default=150, help="depth-1 policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=48, help="boards walked for the leaf count")
    ap.add_argument("--p4", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import g2048
    from g2048 import search

    if not torch.cuda.is_available():
        raise SystemExit("search_bench needs a GPU: timings come from HIP events")
    dev = torch.device("cuda:0")
    count_leaves = leaf_counter()
    rows = []
    for n in args.sizes:
        env = g2048.VecEnv2048(n, seed=args.seed, device=dev, p4=args.p4)
        acts = torch.empty(n, dtype=torch.uint8, device=dev)
        vals = torch.empty((n, 4), dtype=torch.int64, device=dev)
        for _ in range(args.play):
            search.expectimax(env.board, 1, p4=args.p4, values=False, actions_out=acts)
            env.step(acts)
        torch.cuda.synchronize()
        boards = env.board.clone()
        host = boards.cpu().numpy()
        pick = np.random.default_rng(args.seed).choice(n, min(args.sample, n), replace=False)
        empties = float((host == 0).sum(axis=1).mean())
        for depth in args.depths:
            leaves = statistics.fmean(count_leaves(host[i], depth) for i in pick)
            for _ in range(args.warmup):
                search.expectimax(boards, depth, p4=args.p4, actions_out=acts, values_out=vals)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                search.expectimax(boards, depth, p4=args.p4, actions_out=acts, values_out=vals)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            row = {"boards": n, "depth": depth, "ms_median": med, "ms_min": min(ms),
                   "ms_max": max(ms), "reps": len(ms), "mean_empty_cells": empties,
                   "leaves_per_board": leaves, "boards_per_s": n / (med * 1e-3),
                   "leaves_per_s": n * leaves / (med * 1e-3)}
            rows.append(row)
            print(f"n={n:6d} depth={depth}  {med:10.4f} ms (min {min(ms):.4f}, max {max(ms):.4f})"
                  f"  {row['boards_per_s']:.3e} boards/s  {leaves:10.0f} leaves/board"
                  f"  {row['leaves_per_s']:.3e} leaves/s", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"p4": args.p4, "play": args.play, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
