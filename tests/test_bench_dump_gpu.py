"""bench.py --dump-outputs: the arrays the last timed launch left, against the CPU oracle.  The
headline leg runs in this process at a small size (1000 boards, K = 5, 3 timed launches); the
clock settle replays the timed graph for a TIME, so the dump is reproducible only because the env
state is put back after it -- the oracle, stepped once per launch that counts, must agree bit for
bit, and the dumped clock shows that --steps set the number of timed launches."""
import os
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from oracle import oracle as O  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_dump_outputs_equal_oracle(tmp_path):
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need an MI355X (torch.cuda.is_available() is False)")
    n, k, steps, warm, seed = 1000, 5, 3, 2, 0x2048
    out = str(tmp_path / "dump")
    args = bench.parse(["--gpus", "1", "--steps", str(steps), "--warmup", str(warm), "--boards",
                        str(n), "--rollout-k", str(k), "--settle-ms", "5", "--dump-outputs", out])
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    ro = bench.bench_rollout(args, 1, 0, dev, dump_dir=args.dump_outputs)
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in sorted(os.listdir(out))}
    assert set(got) == set(ro["dumped"]) == {
        "board", "score_start", "episodes", "clock", "replay_s", "replay_s2", "replay_a",
        "replay_r", "replay_d", "replay_count"}
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert sum(a.nbytes for a in got.values()) < 64e6
    # launches before the dump: one eager call ahead of the capture, one replay of the graph of
    # `steps` launches, the warm-up, (the settle, undone), the timed launches
    launches = 1 + steps + warm + steps
    ref, ref_rb = O.OracleEnv(n, seed=seed), O.OracleReplay(n * k)
    for _ in range(launches * k):
        ref.step(O.MODE_RANDOM, replay=ref_rb)
    assert np.array_equal(got["clock"], ref.clock.astype(np.float64))
    assert np.array_equal(got["board"], ref.board.astype(np.float32))
    assert np.array_equal(got["episodes"], ref.ep.astype(np.float64))
    assert np.array_equal(got["score_start"][:, 0], ref.meta[:, 0].astype(np.float64))
    for name in ("s", "s2", "a", "r", "d"):
        want = getattr(ref_rb, name)
        assert np.array_equal(got["replay_" + name], want.astype(got["replay_" + name].dtype)), name
    assert got["replay_count"].tolist() == [n * k]
