"""Backward episode learning on the staged batch-mean TC rule (g2048.stageback) next to the staged
batch-mean TC step it is built from: launch times by HIP events and playing strength.  Modelled on
tools/stagedelay_bench.py.

--mode cost (DESIGN 4.22's method).  For each named tuple set a table is filled with random int32
and, for each batch size, fresh boards are played forward `--play` random steps (auto-reset on)
and two consecutive states of the batch are kept, with the afterstates the forward rule saw.  Every
rule below alternates between the two states on its own copy of the table, in this process; it is
warmed up `--warmup` times and timed `--reps` times with an event pair (median, min - max), at
lr = 1 / 2^shift of the TC default:

    stagemeantc          StagedMeanTCState.meantc_step, bounds --bounds, stage 0 = the table
    stageback L=l        BackwardState.step on the same staged table, for each l of --horizons

The backward step is timed in its steady state, every board replaying: each board's replay buffer
holds an episode of l afterstates drawn from the played ones (each board its own sequence) with
rep_k = 0, and warm-up plus timed calls are fewer than the smallest l, so no replay runs out.
Every call also records, as in training.

--mode strength (DESIGN 4.20's one-minute protocol).  `--row` staged_meantc or stageback on the
4 x 6 set with bounds --bounds, --boards boards, p(4) = 0.5, --seed, the default rate, for
--seconds of wall time; then --games games of the greedy player and of the depth-2
play("ntstage_search").

    python tools/stageback_bench.py [--mode cost] [--sizes 4096 65536] [--sets 2x4 4x6] [--out F]
    python tools/stageback_bench.py --mode strength --row stageback --horizon 8192 --seed 61
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


def fill_replay(torch, state, pool, seed, chunk=64):
    """Every board's replay buffer (buffer 1 while cur = 0) holds an episode of L afterstates of
    `pool`, each board its own sequence, with gains that are multiples of 4; rep_n = L."""
    n, L = state.n, state.horizon
    gen = torch.Generator(device=pool.device).manual_seed(seed)
    start = torch.randint(0, len(pool), (n, 1), generator=gen, device=pool.device)
    for s0 in range(0, L, chunk):
        slots = torch.arange(s0, min(s0 + chunk, L), device=pool.device)
        state.traj[:, 1, s0:s0 + len(slots)] = pool[(start + 7919 * slots[None, :]) % len(pool)]
    state.gain[:, 1] = 4 * torch.randint(0, 128, (n, L), generator=gen, device=pool.device,
                                         dtype=torch.int32)
    state.rep_n.fill_(L)


def cost_mode(args, torch, g2048):
    from g2048 import ntmeantc, ntstage, ntuple, stageback, stagemeantc

    dev = torch.device("cuda:0")
    bounds = tuple(args.bounds)
    if args.warmup + args.reps >= min(args.horizons):
        raise SystemExit("warmup + reps must stay below the smallest horizon: every timed call "
                         "is to replay on every board")
    rows = []
    for name in args.sets:
        tuples = ntuple.TUPLES_2x4 if name == "2x4" else ntuple.TUPLES_4x6
        shift = ntmeantc.default_meantc_lr_shift(tuples)
        for n in args.sizes:
            net = ntuple.NTupleNetwork(tuples, device=dev)
            gen = torch.Generator(device=dev).manual_seed(args.seed)
            net.lut.copy_(torch.randint(-(1 << 20), 1 << 20, net.lut.shape, generator=gen,
                                        device=dev, dtype=torch.int32))
            tr = ntuple.NTupleTrainer(net, n, seed=args.seed)
            for _ in range(args.play):
                tr.env.step(None)
            tr.step(2)  # every board gets a previous afterstate
            torch.cuda.synchronize()
            first, pool = tr.env.board.clone(), [tr.prev[tr.has_prev != 0].clone()]
            tr.step(1)
            torch.cuda.synchronize()
            pair = (first, tr.env.board.clone())
            prev0, has0 = tr.prev.clone(), tr.has_prev.clone()
            pool = torch.cat(pool + [prev0[has0 != 0]])
            table = net.lut.clone()
            del tr, net

            def rule(kind, L):
                flip = [0]
                act = torch.zeros(n, dtype=torch.uint8, device=dev)
                err = torch.zeros(n, dtype=torch.int64, device=dev)
                delta = torch.zeros(n, dtype=torch.int32, device=dev)
                own = ntstage.StagedNTupleNetwork(tuples, bounds, device=dev)
                own.lut[0].copy_(table)
                if kind == "stagemeantc":
                    state = stagemeantc.StagedMeanTCState(own)
                    prev, has = prev0.clone(), has0.clone()
                    call = lambda b: state.meantc_step(b, prev, has, 1, shift, act, delta,  # noqa: E731
                                                       err)
                else:
                    state = stageback.BackwardState(own, n, L)
                    fill_replay(torch, state, pool, args.seed + L)
                    x = torch.zeros((n, 16), dtype=torch.uint8, device=dev)
                    rep = torch.zeros(n, dtype=torch.uint8, device=dev)
                    call = lambda b: state.step(b, 1, shift, act, delta, x, rep, err)  # noqa: E731

                def step():
                    flip[0] ^= 1
                    call(pair[flip[0]])

                return step, state, delta

            base = None
            for kind, L in [("stagemeantc", 0)] + [("stageback", h) for h in args.horizons]:
                step, state, delta = rule(kind, L)
                us, lo, hi = timed(torch, step, args.warmup, args.reps)
                if kind == "stagemeantc":
                    base = us
                row = {"set": name, "boards": n, "call": kind, "horizon": L, "us_median": us,
                       "us_min": lo, "us_max": hi, "reps": args.reps,
                       "ratio_to_stagemeantc": us / base,
                       "nonzero_deltas": int((delta != 0).sum())}
                if kind == "stageback":
                    kept = torch.minimum(state.rep_n, torch.full_like(state.rep_n, L))
                    row["replaying"] = int((state.rep_k < kept).sum())
                    row["state_bytes"] = state.traj.numel() + 4 * state.gain.numel()
                rows.append(row)
                print(f"{name} n={n} {kind:12s} L={L:5d} {us:9.1f} us (min {lo:.1f}, max {hi:.1f})  "
                      f"{us / base:.3f}x stagemeantc  nonzero deltas {row['nonzero_deltas']}"
                      + (f"  replaying {row['replaying']}" if kind == "stageback" else ""),
                      flush=True)
                assert not bool(state.acc.any()), "acc is not all zero after the timed calls"
                del step, state, delta
                torch.cuda.empty_cache()
            del table, pair, pool
            torch.cuda.empty_cache()
    return {"play": args.play, "bounds": list(bounds), "rows": rows}


def strength_mode(args, torch, g2048):
    import numpy as np

    from g2048 import ntstage, ntuple, stageback, stagemeantc
    from g2048.player import BatchedPlayer

    dev, bounds = "cuda:0", tuple(args.bounds)
    kw = dict(seed=args.seed, p4=0.5, log_slots=64)
    net = ntstage.StagedNTupleNetwork(ntuple.TUPLES_4x6, bounds, device=dev)
    if args.row == "stageback":
        tr = stageback.BackwardTrainer(net, args.boards, horizon=args.horizon, **kw)
    else:
        tr = stagemeantc.StagedMeanTCTrainer(net, args.boards, **kw)
    torch.cuda.synchronize()
    scores, done, t0 = [], 0, time.time()
    while time.time() - t0 < args.seconds:
        tr.step(args.chunk)
        done += args.chunk
        scores = (scores + tr.episodes(strict=False)["score"].tolist())[-2000:]
    torch.cuda.synchronize()
    lut = torch.where(net.lut != ntstage.UNSET, net.lut, torch.zeros_like(net.lut))
    row = {"row": args.row, "bounds": list(bounds), "boards": args.boards, "seed": args.seed,
           "lr_shift": tr.lr_shift, "steps": done, "train_seconds": time.time() - t0,
           "train_mean_last_200": float(np.mean(scores[-200:])),
           "largest_entry": int(lut.to(torch.int64).abs().max()), "set_counts": net.set_counts()}
    if args.row == "stageback":
        st = tr.state
        kept = torch.minimum(st.rep_n, torch.full_like(st.rep_n, st.horizon))
        row.update(horizon=args.horizon, replaying_at_the_end=int((st.rep_k < kept).sum()),
                   longest_episode_replayed=int(st.rep_n.max()))
    tr.env.check_errors()
    del tr, lut
    torch.cuda.empty_cache()
    for policy, pkw in (("ntuple", {}), ("ntstage_search", {"search_depth": 2})):
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
    ap.add_argument("--sizes", type=int, nargs="+", default=[4096, 65536])
    ap.add_argument("--sets", nargs="+", default=["2x4", "4x6"], choices=["2x4", "4x6"])
    ap.add_argument("--bounds", type=int, nargs="*", default=[11])
    ap.add_argument("--horizons", type=int, nargs="+", default=[64, 8192])
    ap.add_argument("--play", type=int, default=150, help="random-policy steps before timing")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=None, help="cost: 0x2048; strength: 61")
    ap.add_argument("--row", default="stageback", choices=["staged_meantc", "stageback"])
    ap.add_argument("--horizon", type=int, default=8192)
    ap.add_argument("--boards", type=int, default=4096, help="strength: boards of the trainer")
    ap.add_argument("--chunk", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.seed is None:
        args.seed = 61 if args.mode == "strength" else 0x2048

    import torch

    import g2048

    if not torch.cuda.is_available():
        raise SystemExit("stageback_bench needs a GPU")
    g2048.load_native()
    for mod in (g2048.ntuple, g2048.ntstage, g2048.ntmeantc, g2048.stagemeantc, g2048.stageback):
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
