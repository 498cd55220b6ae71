"""Cost of the greedy afterstate policy alone: NTupleNetwork.act (k_policy<T, false>) and
StagedNTupleNetwork.act (k_stage_policy<T, false>) on played boards, all three outputs asked for,
into tensors allocated once.  Median, min and max of `--reps` event-timed calls after `--warmup`.

    python tools/ntact_bench.py [--boards 65536] [--sets 2x4 4x6] [--bounds 11] [--out FILE.json]
"""
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
    ap.add_argument("--bounds", type=int, nargs="*", default=[11])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0x2048)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import g2048
    from g2048 import ntstage, ntuple

    dev, n = torch.device("cuda:0"), args.boards
    env = g2048.VecEnv2048(n, seed=args.seed, device=dev)
    for _ in range(args.play):
        env.step(None)
    boards = env.board.clone()
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        gen = torch.Generator(device=dev).manual_seed(args.seed)
        flat = ntuple.NTupleNetwork(tuples, device=dev)
        flat.lut.copy_(torch.randint(-(1 << 20), 1 << 20, flat.lut.shape, generator=gen,
                                     device=dev, dtype=torch.int32))
        staged = ntstage.StagedNTupleNetwork(tuples, tuple(args.bounds), device=dev)
        staged.lut[0].copy_(flat.lut)  # the stages above stay UNSET and fall through
        out = dict(q_out=torch.zeros(n, 4, dtype=torch.int64, device=dev),
                   actions_out=torch.zeros(n, dtype=torch.uint8, device=dev),
                   after_out=torch.zeros(n, 16, dtype=torch.uint8, device=dev))
        for call, net in (("ntuple act", flat), ("ntstage act", staged)):
            for _ in range(args.warmup):
                net.act(boards, **out)
            torch.cuda.synchronize()
            ms = []
            for _ in range(args.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                net.act(boards, **out)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            row = {"set": name, "boards": n, "call": call,
                   "us_median": statistics.median(ms) * 1e3, "us_min": min(ms) * 1e3,
                   "us_max": max(ms) * 1e3, "reps": args.reps}
            rows.append(row)
            print(f"{name} n={n} {call:12s} {row['us_median']:9.1f} us (min {row['us_min']:.1f}, "
                  f"max {row['us_max']:.1f})", flush=True)
        del flat, staged, out
        torch.cuda.empty_cache()
    env.check_errors()
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
