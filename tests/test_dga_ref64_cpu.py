"""Ties tests/dga_ref64.py (the float64 model the GPU tests hold the DGA
tail to) to production: ``DGA("client").generate_client_payload`` plus
``accumulate_flat_grad`` run in torch float64 on a toy ParameterArena
trainer with a set loss and stats must give the model's weight and
accumulate.

Bound 1e-12 relative: both sides are float64 chains of at most ten
operations on the same inputs (1e-16 each); no sort or reduction tree is
involved except the norm's sum, whose order changes it by ~1e-16 * sqrt(P)
at P = 37.
"""

import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import dga_ref64 as ref
from msrflute_amd.ops.arena import ParameterArena
from msrflute_amd.strategies.dga import DGA
from msrflute_amd.strategies.utils import accumulate_flat_grad

RTOL = 1e-12
BS = 4
COUNTS = [9, 4, 1]


def _config(median, wtl, beta, clip, max_grad):
    cfg = {
        "strategy": "DGA",
        "model_config": {},
        "client_config": {},
        "server_config": {"aggregate_median": median,
                          "weight_train_loss": wtl, "softmax_beta": beta},
    }
    if clip:
        cfg["dp_config"] = {"enable_local_dp": True, "eps": -1.0,
                            "max_grad": max_grad, "max_weight": 1.0}
    return cfg


def _toy(seed=0):
    """server [P], params [K, P] float32 and {sum, sumsq} stats of a toy
    model with P = 37."""
    torch.manual_seed(seed)
    model = torch.nn.Sequential(torch.nn.Linear(5, 5), torch.nn.Linear(6, 1))
    P = sum(p.numel() for p in model.parameters())
    gen = np.random.default_rng(seed)
    server = gen.standard_normal(P).astype(np.float32)
    params = (server[None, :] + np.array([[0.3], [0.02], [1.5]])
              * gen.standard_normal((3, P))).astype(np.float32)
    stats = np.abs(gen.standard_normal(6)).astype(np.float32)
    stats[1::2] += 3.0   # sumsq large enough that the variance is positive
    return model, server, params, stats


def _production(model, server, params, loss, stats, cfg):
    """What the eager DGA round does with these clients, in float64."""
    K, P = params.shape
    strategy = DGA("client", cfg)
    worker = SimpleNamespace(arena=ParameterArena(model, bind_grads=False,
                                                  dtype=torch.float64))
    worker.arena.grad = torch.zeros(P, dtype=torch.float64)
    weights = []
    for k in range(K):
        arena = ParameterArena(model, bind_grads=False, dtype=torch.float64)
        # the pseudo-gradient as the round forms it: one float32 subtract
        arena.grad = torch.from_numpy(
            (server - params[k]).astype(np.float64))
        n = max(-(-COUNTS[k] // BS) * P, 1)
        s, q = float(stats[2 * k]), float(stats[2 * k + 1])
        mean = s / n
        trainer = SimpleNamespace(
            arena=arena, train_loss=float(loss[k]), num_samples=COUNTS[k],
            sufficient_stats={"mean": mean,
                              "mag": math.sqrt(max(q / n, 0.0)),
                              "var": max(q / n - mean ** 2, 0.0),
                              "norm": math.sqrt(max(q, 0.0))})
        payload = strategy.generate_client_payload(trainer)
        weights.append(payload["weight"])
        if payload["weight"] != 0.0:   # FedAvg.process_individual_payload
            accumulate_flat_grad(worker, payload["grad"])
    return np.array(weights), worker.arena.grad.numpy()


def _check(median, wtl, beta, loss, clip, max_grad_of=None):
    model, server, params, stats = _toy()
    loss = np.asarray(loss, dtype=np.float32)
    source = "mean" if median == "mean" else (
        wtl if wtl in ref.SOURCES else "mag")
    max_grad = 0.0
    if clip:
        norms = ref.dga_tail(server, params, loss, stats, COUNTS, BS,
                             source, beta, True, 1.0)["norm"]
        max_grad = max_grad_of(norms)
    want = ref.dga_tail(server, params, loss, stats, COUNTS, BS, source,
                        beta, clip, max_grad, f32_coef=False)
    got_w, got_acc = _production(
        model, server, params, loss, stats,
        _config(median, wtl, beta, clip, max_grad))
    np.testing.assert_allclose(got_w, want["weight"], rtol=RTOL, atol=0)
    scale = np.abs(want["accum"]).max()
    assert np.abs(got_acc - want["accum"]).max() <= RTOL * max(scale, 1e-300)
    return want


LOSS = [4.5, 2.4, 0.3]


@pytest.mark.parametrize("wtl", ["train_loss", "mag_var_loss",
                                 "mag_mean_loss", "mag_loss"])
@pytest.mark.parametrize("clip", [False, True])
def test_softmax_sources(wtl, clip):
    # max_grad between the norms: clients on both sides of the clip
    want = _check("softmax", wtl, 1.5, LOSS, clip,
                  lambda n: float(np.sqrt(n.min() * n.max())))
    assert (want["weight"] > 0).all() and (want["weight"] < 1).all()
    assert len(set(want["weight"])) == 3
    if clip:
        assert (want["c"] < want["weight"]).any()
        assert (want["c"] == want["weight"]).any()


@pytest.mark.parametrize("clip", [False, True])
def test_mean_aggregation_is_weight_one(clip):
    want = _check("mean", "train_loss", 1.0, LOSS, clip,
                  lambda n: float(n.min() * 0.5))
    assert (want["weight"] == 1.0).all()
    if clip:
        assert (want["c"] < 1.0).all()


def test_overflow_nan_and_above_100_branches():
    # tw = loss / count: -2000 overflows exp (MIN_WEIGHT), NaN is dropped,
    # -5 gives e^5 = 148 -> 100
    want = _check("softmax", "train_loss", 1.0,
                  [-2000.0 * COUNTS[0], float("nan"), -5.0], False)
    assert want["weight"].tolist() == [ref.MIN_WEIGHT, 0.0, 100.0]


def test_all_weights_zero_accumulates_nothing():
    want = _check("softmax", "train_loss", 1.0, [float("nan")] * 3, True,
                  lambda n: float(n.min() * 0.5))
    assert (want["weight"] == 0).all() and (want["accum"] == 0).all()


def test_model_branches_directly():
    assert ref.softmax_weight(1.0, -1e6) == ref.MIN_WEIGHT
    assert ref.softmax_weight(1.0, float("inf")) == 0.0     # exp(-inf)
    assert ref.softmax_weight(1.0, float("-inf")) == 0.0    # exp(+inf): inf
    assert ref.softmax_weight(1.0, float("nan")) == 0.0
    assert ref.softmax_weight(2.0, -3.0) == 100.0
    assert ref.softmax_weight(2.0, 0.5) == math.exp(-1.0)
    # a negative variance estimate clamps to 0, the empty count to 1
    assert ref.training_weight("mag_var_loss", 0, 8.0, 1.0, 4, 4, 2) == 0.0
    assert ref.training_weight("train_loss", 3.0, 0, 0, 0, 4, 2) == 3.0
