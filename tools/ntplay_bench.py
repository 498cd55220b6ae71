"""The on-device n-tuple player (g2048.ntplay): what a whole play() costs next to the
move-by-move policy of the same depth, and what one move costs inside a steps() call.

--mode cost.  For each named tuple set a table is trained for `--train-steps` TD(0) steps on
`--train-boards` boards (its quality only sets how long the games are; the mean number of moves is
reported).  For each number of games and each depth, play("ntuple_fused") and its yardstick --
play("ntuple") at depth 1, play("ntuple_search") at depth 2, whose code this library does not
touch -- run in the same process on the same seed, so both play the same games (checked: every
row says whether max_tile, merge_score and moves were equal).  `--reps` repetitions alternate
between the two after one untimed call of each; a repetition is timed by an event pair on the
current stream around the whole play() and by the host clock around play() and a synchronize;
the minimum and the maximum are reported.  Then one steps(`--k`) call on a fresh env of that
many boards is timed by an event pair, `--reps` times after one warm-up call, each on an env
re-dealt from the same seed: time / k is the cost of a move inside the launch.

--mode resources.  No GPU: compiles the library's source to assembly with the library's flags and
writes the kernels' register, scratch and LDS figures from the code-object metadata.

    python tools/ntplay_bench.py --mode cost [--sets 2x4 4x6] [--games 256 4096] [--depths 1 2]
                                 [--out profiles/ntplay/cost]
    python tools/ntplay_bench.py --mode resources [--out profiles/ntplay/resource_usage.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "reinforcement-learning-2048_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def resources_mode(args):
    import __graft_entry__ as G

    src = os.path.join(G.CSRC, G.NTPLAY_SRCS[0])
    flags = [x for x in G.src_flags(src) if x not in ("-shared", "-fPIC")]
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "ntplay.s")
        subprocess.run([G.HIPCC, *flags, "--cuda-device-only", "-S", src, "-o", out], check=True,
                       capture_output=True)
        text = open(out).read()
    lines = ["k_play / k_tick of libg2048_ntplay.so (gfx950, the library's flags): the code-object",
             "metadata, one row per kernel in the order of the metadata (tools/ntplay_bench.py --mode",
             "resources).  No kernel uses scratch or LDS and no VGPR is spilled.  The move loop keeps",
             "more loop-invariant scalars than there are SGPRs (the nibble shifts of the tuples, the",
             "20 key words of the Philox rounds, the kernel arguments): the compiler parks the excess",
             "in lanes of one or two VGPRs (sgpr_spill; a v_readlane reads one back), not in memory.",
             "k_search<d> of the search libraries holds 48 / 136 / 168 VGPRs (DESIGN 4.21).", ""]
    for k in re.split(r"\n  - ", text.split("amdhsa.kernels:")[1])[1:]:
        if ".vgpr_count" not in k:
            continue

        def g(key):
            return re.search(r"\." + key + r":\s*(\S+)", k).group(1)

        name = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout
        name = name.strip().replace("(anonymous namespace)::", "").replace("void ", "")
        name = name.split("(")[0].replace("g2048::nt::", "")
        lines.append(f"{name:26s} vgpr {g('vgpr_count'):>3s}  sgpr {g('sgpr_count'):>3s}  scratch "
                     f"{g('private_segment_fixed_size')}  lds {g('group_segment_fixed_size')}  "
                     f"vgpr_spill {g('vgpr_spill_count')}  sgpr_spill {g('sgpr_spill_count')}")
    with open(args.out or os.path.join(ROOT, "profiles", "ntplay", "resource_usage.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def cost_mode(args):
    import numpy as np
    import torch

    import g2048
    from g2048 import ntplay, ntuple
    from g2048.player import BatchedPlayer

    dev = torch.device("cuda:0")
    rows, moves_rows, text = [], [], []

    def say(line):
        print(line, flush=True)
        text.append(line)

    say(f"method: tools/ntplay_bench.py --mode cost; tables after {args.train_steps} TD(0) steps "
        f"on {args.train_boards} boards, seed {args.seed}; {args.reps} repetitions alternating "
        f"fused / yardstick after one untimed call of each; event pair and host clock around a "
        f"whole play(); check_every = {args.check_every}")
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        net = ntuple.NTupleNetwork(tuples, device=dev)
        tr = ntuple.NTupleTrainer(net, args.train_boards, seed=args.seed, p4=0.5, lr_num=1,
                                  lr_shift=10, log_slots=64)
        for _ in range(args.train_steps // 500):
            tr.step(500)
            tr.episodes(strict=False)
        del tr
        torch.cuda.synchronize()
        for games in args.games:
            for depth in args.depths:
                yard = "ntuple" if depth == 1 else "ntuple_search"
                kw = dict(device=dev, seed=args.seed, ntuple=net, search_depth=depth,
                          check_every=args.check_every)
                res, ev, host = {}, {"ntuple_fused": [], yard: []}, {"ntuple_fused": [], yard: []}
                for rep in range(args.reps + 1):
                    for policy in ("ntuple_fused", yard):
                        player = BatchedPlayer(games, **kw)
                        torch.cuda.synchronize()
                        e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                        t0 = time.perf_counter()
                        e0.record()
                        res[policy] = player.play(policy)
                        e1.record()
                        torch.cuda.synchronize()
                        t1 = time.perf_counter()
                        if rep:
                            ev[policy].append(e0.elapsed_time(e1))
                            host[policy].append((t1 - t0) * 1e3)
                a, b = res["ntuple_fused"], res[yard]
                equal = all(np.array_equal(getattr(a, k), getattr(b, k))
                            for k in ("max_tile", "merge_score", "moves", "stuck"))
                row = {"set": name, "games": games, "depth": depth, "yardstick": yard,
                       "same_games": bool(equal), "moves_mean": float(a.moves.mean()),
                       "moves_max": int(a.moves.max()),
                       "fused_event_ms": [min(ev["ntuple_fused"]), max(ev["ntuple_fused"])],
                       "fused_host_ms": [min(host["ntuple_fused"]), max(host["ntuple_fused"])],
                       "yard_event_ms": [min(ev[yard]), max(ev[yard])],
                       "yard_host_ms": [min(host[yard]), max(host[yard])]}
                row["ratio_min_over_min"] = row["yard_host_ms"][0] / row["fused_host_ms"][0]
                rows.append(row)
                say(f"{name} games={games} depth={depth}: fused {row['fused_host_ms'][0]:.1f}-"
                    f"{row['fused_host_ms'][1]:.1f} ms host ({row['fused_event_ms'][0]:.1f}-"
                    f"{row['fused_event_ms'][1]:.1f} ms events), {yard} "
                    f"{row['yard_host_ms'][0]:.1f}-{row['yard_host_ms'][1]:.1f} ms host "
                    f"({row['yard_event_ms'][0]:.1f}-{row['yard_event_ms'][1]:.1f} ms events); "
                    f"x{row['ratio_min_over_min']:.1f} (min over min); mean moves "
                    f"{row['moves_mean']:.0f}, longest game {row['moves_max']}; same games: "
                    f"{equal}")
                # one steps(k) call on fresh boards
                us = []
                for rep in range(args.reps + 1):
                    env = g2048.VecEnv2048(games, seed=args.seed, device=dev, autoreset=False)
                    torch.cuda.synchronize()
                    e0, e1 = (torch.cuda.Event(enable_timing=True) for _ in range(2))
                    e0.record()
                    ntplay.steps(net, env, args.k, depth)
                    e1.record()
                    e1.synchronize()
                    if rep:
                        us.append(e0.elapsed_time(e1) * 1e3 / args.k)
                    env.check_errors()
                mrow = {"set": name, "boards": games, "depth": depth, "k": args.k,
                        "us_per_move": [min(us), max(us)]}
                moves_rows.append(mrow)
                say(f"{name} boards={games} depth={depth}: one steps({args.k}) call, "
                    f"{min(us):.2f}-{max(us):.2f} us per move")
        del net
    slower = [r for r in rows if r["games"] == 256 and r["ratio_min_over_min"] < 1.0]
    say("condition (at 256 games the fused policy is not slower than its yardstick at either "
        "depth): " + ("holds" if not slower else "FAILS at " + ", ".join(
            f"{r['set']} depth {r['depth']}" for r in slower)))
    out = args.out or os.path.join(ROOT, "profiles", "ntplay", "cost")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out + ".txt", "w") as f:
        f.write("\n".join(text) + "\n")
    with open(out + ".json", "w") as f:
        json.dump({"args": vars(args), "play": rows, "steps": moves_rows}, f, indent=1)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=("cost", "resources"), default="cost")
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=("2x4", "4x6"))
    ap.add_argument("--games", nargs="+", type=int, default=[256, 4096])
    ap.add_argument("--depths", nargs="+", type=int, default=[1, 2])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--k", type=int, default=64)
    ap.add_argument("--check-every", type=int, default=32)
    ap.add_argument("--train-boards", type=int, default=256)
    ap.add_argument("--train-steps", type=int, default=4000)
    ap.add_argument("--seed", type=int, default=61)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    (resources_mode if args.mode == "resources" else cost_mode)(args)


if __name__ == "__main__":
    main()
