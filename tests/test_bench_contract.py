"""The driver's bench contract, end-to-end on CPU/gloo: the EXACT launch
shape the round-end SCALE run uses (`python -m torch.distributed.run
--nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W`)
must produce one JSON line from rank 0 with the required fields — so an
8-GPU node holds no surprises (VERDICT round-1 item 1)."""

import json
import os
import socket
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_bench_contract_two_ranks_gloo():
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    env["MASTER_ADDR"] = "127.0.0.1"
    # CPU/gloo by design: two ranks cannot share one GPU over RCCL
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
         "--steps", "2", "--warmup", "1", "--clients", "24",
         "--samples-per-client", "24"],
        cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    line = next(l for l in r.stdout.splitlines() if l.startswith("{"))
    rec = json.loads(line)
    assert rec["metric"] == "fl_rounds_per_sec"
    assert rec["n_gpus"] == 2 and rec["steps"] == 2 and rec["warmup"] == 1
    assert rec["value"] > 0 and rec["higher_is_better"] is True
    for key in ["ms_per_step", "vs_baseline", "dtype", "data", "config",
                "scaling", "unit"]:
        assert key in rec
    # exactly one JSON line (rank 1 must not print)
    assert sum(1 for l in r.stdout.splitlines()
               if l.startswith('{"metric"')) == 1


def _run_bench(extra):
    env = dict(os.environ)
    env.pop("RANK", None), env.pop("WORLD_SIZE", None)
    # the option plumbing is under test, not the kernels: run on the CPU
    # everywhere, where a round is bit-reproducible
    env["HIP_VISIBLE_DEVICES"] = env["CUDA_VISIBLE_DEVICES"] = ""
    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "2",
         "--warmup", "1", "--clients", "24", "--samples-per-client", "24"]
        + extra, cwd=REPO, env=env, capture_output=True, text=True,
        timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith('{"metric"')]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed round's results as float
    .npy files, identical from run to run with the same arguments; --full
    is accepted and keeps the result line's meaning."""
    import numpy as np
    recs = [_run_bench(["--dump-outputs", str(tmp_path / "a")]),
            _run_bench(["--dump-outputs", str(tmp_path / "b"), "--full"])]
    for rec in recs:
        assert rec["metric"] == "fl_rounds_per_sec" and rec["steps"] == 2
        assert rec["unit"] == "rounds/s" and rec["higher_is_better"] is True
        assert rec["dtype"] == "fp32" and rec["ms_per_step"] > 0
        assert abs(rec["value"] * rec["ms_per_step"] - 1000.0) < 1e-6 * 1000
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["client_train_losses.npy", "global_params.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64)
        assert a.size > 0 and np.isfinite(a).all()
        assert a.shape == b.shape and np.array_equal(a, b)
        total += a.nbytes
    assert total <= 64 * 10 ** 6
    # 10 clients per round -> one training loss per sampled client
    assert np.load(tmp_path / "a" / "client_train_losses.npy").shape == (10,)
