"""One DGA server round on the CNN mega round against the same round on
the stream pool (``use_mega_round: false``, the path DGA took before):
softmax on train_loss, local DP in clip-only mode, 6 clients of the
cv_cnn_femnist model with ragged shards (45 rows, bs 20).

* per-client aggregation weights ``wt``: 1e-6 relative (the two paths'
  fp32 losses differ at ~1e-7 and exp preserves that);
* the server's weight update after the round: 1e-5 relative, the bound
  tests/test_mega_round_gpu.py holds these two drivers to.
One round only: multi-round comparisons under clipping are chaotic.  The
worker asserts through the driver's call counter that the mega round ran
in one run and not in the other, so a silent fallback cannot pass.
"""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))

WORKER = r"""
import os, sys, torch
sys.path.insert(0, os.environ["REPO"])
from msrflute_amd.comm import runtime as rt_mod
from msrflute_amd.config import FLUTEConfig
from msrflute_amd.core import client as client_mod
from msrflute_amd.core.client import ClientPool, fused_round_dga
from msrflute_amd.core.server import OptimizationServer
from msrflute_amd.models import make_model
from msrflute_amd.ops.arena import ParameterArena
from msrflute_amd.ops.fused_optim import make_arena_optimizer
from tools.create_data import make_femnist_blob
from msrflute_amd.models.generic_data import ArrayDataset

MAX_GRAD = 0.05

def run(mega):
    rt_mod.set_runtime(None)
    rt = rt_mod.init_runtime(backend="nccl", seed=99)
    cfg = {
        "model_config": {"model_type": "CNN",
                         "model_folder": "experiments/cv_cnn_femnist/model.py",
                         "num_classes": 62},
        "dp_config": {"enable_local_dp": True, "eps": -1.0,
                      "max_grad": MAX_GRAD, "max_weight": 1.0},
        "privacy_metrics_config": {"apply_metrics": False},
        "strategy": "DGA",
        "server_config": {
            "wantRL": False, "resume_from_checkpoint": False,
            "do_profiling": False,
            "optimizer_config": {"type": "sgd", "lr": 1.0},
            "annealing_config": {"type": "step_lr", "step_interval": "epoch",
                                 "gamma": 1.0, "step_size": 100},
            "val_freq": 10**9, "rec_freq": 10**9,
            "initial_val": False, "initial_rec": False,
            "max_iteration": 1, "num_clients_per_iteration": 6,
            "data_config": {"val": {"batch_size": 64, "val_data": None},
                            "test": {"batch_size": 64, "test_data": None}},
            "type": "model_optimization", "aggregate_median": "softmax",
            "weight_train_loss": "train_loss", "softmax_beta": 1.0,
            "initial_lr_client": 0.1, "lr_decay_factor": 1.0,
            "best_model_criterion": "loss", "fall_back_to_best_model": False,
            "seed": 99},
        "client_config": {
            "use_mega_round": mega,
            "parallel_clients": 4,
            "do_profiling": False, "ignore_subtask": False,
            "data_config": {"train": {"batch_size": 20,
                                      "list_of_train_data": None,
                                      "desired_max_samples": 10000,
                                      "max_grad_norm": 10.0}},
            "type": "optimization",
            "optimizer_config": {"type": "sgd", "lr": 0.1}},
    }
    config = FLUTEConfig.from_dict(cfg)
    assert fused_round_dga(config) is not None
    config["model_path"] = os.environ["OUT"] + f"/m_{int(mega)}"
    os.makedirs(config["model_path"], exist_ok=True)
    blob = make_femnist_blob(n_users=12, samples_per_user=45, seed=3)
    ds = ArrayDataset(blob, test_only=False, user_idx=-1, args={},
                      x_shape=(28, 28))
    ds.user_data = blob["user_data"]
    ds.user_data_label = blob["user_data_label"]
    client_mod.train_dataset = ds
    torch.manual_seed(5)
    model = make_model(cfg["model_config"])
    arena = ParameterArena(model, bind_grads=True)
    w0 = arena.data.clone()
    opt = make_arena_optimizer(dict(cfg["server_config"]["optimizer_config"]),
                               arena)
    server = OptimizationServer(
        num_clients=12, model=model, optimizer=opt, ss_scheduler=None,
        data_path=None, model_path=config["model_path"],
        server_train_dataloader=None, config=config, idx_val_clients=[],
        idx_test_clients=[], runtime=rt, arena=arena,
        task="cv_cnn_femnist")
    server.run_stats = {k: [] for k in [
        "secsPerClientRound", "secsPerClient", "secsPerClientTraining",
        "secsPerClientSetup", "secsPerClientFull",
        "secsPerRoundHousekeeping", "secsPerRoundTotal",
        "communicationCosts"]}
    assert isinstance(server.executor, ClientPool)
    wts = {}
    real = server.strategy.process_individual_payload
    def spy(worker_trainer, payload, client_id=None):
        wts[client_id] = payload["weight"]
        return real(worker_trainer, payload, client_id=client_id)
    server.strategy.process_individual_payload = spy
    server.run_one_round(0, housekeeping=False)
    torch.cuda.synchronize()
    driver = server.executor._mega
    norms = None
    if mega:
        # the mega driver ran this round, once, for all 6 clients
        assert driver is not None and driver.calls == 1, driver
        assert driver.dga is not None
        assert server.executor.perf_acc["clients"] == 6
        norms = driver.dga_out[6:12].cpu().tolist()
    else:
        assert driver is None, "the pool run must not build the mega driver"
    return arena.data.clone() - w0, wts, norms

u_pool, wt_pool, _ = run(mega=False)
u_mega, wt_mega, norms = run(mega=True)
print("wt pool:", wt_pool)
print("wt mega:", wt_mega)
print("pseudo-gradient norms:", norms, "max_grad:", MAX_GRAD)
assert sorted(wt_pool) == sorted(wt_mega) and len(wt_pool) == 6
for cid, w in wt_pool.items():
    assert 0 < w < 1 and 0 < wt_mega[cid] < 1
    assert abs(wt_mega[cid] - w) <= 1e-6 * w, (cid, w, wt_mega[cid])
assert len(set(wt_pool.values())) == 6
assert any(n > MAX_GRAD for n in norms), "the clip did not engage"
rel = float((u_mega - u_pool).norm() / u_pool.norm())
print("rel update diff:", rel, "update norm:", float(u_pool.norm()))
assert float(u_pool.norm()) > 0
assert rel <= 1e-5, rel
print("DGA_MEGA_OK")
"""


def test_dga_mega_round_matches_pool_round(tmp_path):
    env = dict(os.environ)
    env.update(REPO=REPO, PYTHONPATH=REPO, OUT=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", WORKER], env=env,
                       capture_output=True, text=True, timeout=600,
                       cwd=REPO)
    print(r.stdout[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "DGA_MEGA_OK" in r.stdout
