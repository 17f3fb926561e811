"""The driver's bench.py contract, exercised on CPU: one JSON line on
stdout with the required schema, sane values, and the documented defaults.
(The driver runs `python bench.py --gpus N --steps K --warmup W` verbatim —
BENCH_rNN.json / SCALE_rNN.json depend on this shape.)"""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.timeout(600)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run_bench(args):
    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), *args],
        capture_output=True, text=True, timeout=540, cwd=REPO)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly ONE JSON line expected: {out.stdout}"
    return json.loads(lines[0])


def test_bench_json_contract_cpu():
    r = _run_bench(["--model", "tiny", "--batch-size", "4", "--seq-len",
                    "16", "--steps", "3", "--warmup", "1",
                    "--dtype", "fp32"])
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in r, key
    assert r["metric"] == "samples_per_sec"
    assert r["n_gpus"] == 1 and r["steps"] == 3 and r["warmup"] == 1
    assert r["value"] > 0 and r["ms_per_step"] > 0
    assert r["higher_is_better"] is True
    assert r["scaling"] == "weak"
    assert r["data"] == "synthetic"
    cfg = r["config"]
    assert cfg["global_batch"] == 4 and cfg["seq_len"] == 16
    assert cfg["parallelism"] == "dp1"
    # value is the whole-job aggregate: samples/s consistent with ms/step
    expect = 4 * 1000.0 / r["ms_per_step"]
    assert abs(r["value"] - expect) / expect < 0.05


def test_bench_dump_outputs_reproducible_cpu(tmp_path):
    """--dump-outputs writes the last timed step's arrays as float32 .npy;
    equal arguments give equal inputs, so two runs agree; --full is accepted
    and leaves the result line's meaning alone."""
    import numpy as np
    common = ["--model", "tiny", "--batch-size", "4", "--seq-len", "16",
              "--steps", "3", "--warmup", "1", "--dtype", "fp32"]
    a, b = tmp_path / "a", tmp_path / "b"
    ra = _run_bench([*common, "--dump-outputs", str(a)])
    rb = _run_bench([*common, "--full", "--dump-outputs", str(b)])
    for r in (ra, rb):
        assert r["metric"] == "samples_per_sec" and r["steps"] == 3
        assert r["ms_per_step"] > 0 and r["dtype"] == "fp32"
    names = sorted(p.name for p in a.iterdir())
    assert names == ["logits.npy", "loss.npy", "params_sample.npy"]
    assert names == sorted(p.name for p in b.iterdir())
    total = 0
    for n in names:
        xa, xb = np.load(a / n), np.load(b / n)
        assert xa.dtype == np.float32 and np.isfinite(xa).all(), n
        np.testing.assert_array_equal(xa, xb, err_msg=n)
        total += xa.nbytes
    assert total <= 64 * 2**20
    assert np.load(a / "logits.npy").shape == (4, 6)
    assert np.load(a / "loss.npy").shape == (1,)

    # a different --steps is a different last step: the dump follows it
    c = tmp_path / "c"
    _run_bench([*common[:-6], "--steps", "2", "--warmup", "1",
                "--dtype", "fp32", "--dump-outputs", str(c)])
    assert not np.array_equal(np.load(a / "params_sample.npy"),
                              np.load(c / "params_sample.npy"))


def test_bench_multirank_contract_cpu():
    """The driver's SCALE launch shape (torchrun, N ranks) on CPU/gloo:
    rendezvous, DDP wrap, max-over-ranks timing, ONE JSON line from rank 0
    with the aggregate value."""
    env = dict(os.environ)
    env.pop("RANK", None); env.pop("WORLD_SIZE", None)
    env.pop("LOCAL_RANK", None); env.pop("MASTER_PORT", None)
    out = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29599", os.path.join(REPO, "bench.py"),
         "--gpus", "2", "--model", "tiny", "--batch-size", "4",
         "--seq-len", "16", "--steps", "2", "--warmup", "1",
         "--dtype", "fp32"],
        capture_output=True, text=True, timeout=540, cwd=REPO, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, f"exactly ONE JSON line: {out.stdout[-500:]}"
    r = json.loads(lines[0])
    assert r["n_gpus"] == 2
    assert r["config"]["global_batch"] == 8
    assert r["config"]["parallelism"] == "dp2"
    assert r["config"]["backend"] == "gloo"
    assert r["value"] > 0
