"""The DGA gate of the mega rounds (``core.client.fused_round_dga``): which
DGA configs end the round in the device tail, with which spec, and that
every option the tail does not implement sends the round to the pool."""

import copy

import pytest

from msrflute_amd.core.client import fused_round_dga, fused_round_mu
from msrflute_amd.ops.mega_round import DGA_MODES, DGASpec


def _cfg():
    return {
        "strategy": "DGA",
        "model_config": {"model_type": "CNN"},
        "server_config": {"aggregate_median": "softmax",
                          "weight_train_loss": "train_loss",
                          "softmax_beta": 2.5},
        "client_config": {"optimizer_config": {"type": "sgd"}},
        "dp_config": {"enable_local_dp": True, "eps": -1.0,
                      "max_grad": 0.5, "max_weight": 1.0},
        "privacy_metrics_config": {"apply_metrics": False},
    }


def _with(path, value):
    cfg = copy.deepcopy(_cfg())
    node = cfg
    for key in path[:-1]:
        node = node.setdefault(key, {})
    node[path[-1]] = value
    return cfg


def test_base_config_gets_its_spec():
    assert fused_round_dga(_cfg()) == DGASpec("train_loss", 2.5, True, 0.5)


def test_spec_binding_arguments():
    kw = DGASpec("mag_var_loss", 1.5, True, 0.25).kwargs()
    assert kw == {"dga_mode": DGA_MODES["mag_var_loss"], "dga_beta": 1.5,
                  "dga_clip": True, "dga_max_grad": 0.25}


@pytest.mark.parametrize("wtl,source", [
    ("train_loss", "train_loss"), ("mag_var_loss", "mag_var_loss"),
    ("mag_mean_loss", "mag_mean_loss"), ("mag_loss", "mag"),
    ("anything_else", "mag")])
def test_weight_sources(wtl, source):
    spec = fused_round_dga(_with(("server_config", "weight_train_loss"), wtl))
    assert spec.source == source and spec.beta == 2.5


def test_default_source_is_train_loss():
    cfg = _cfg()
    del cfg["server_config"]["weight_train_loss"]
    assert fused_round_dga(cfg).source == "train_loss"


def test_mean_aggregation_has_weight_one_and_keeps_the_clip():
    spec = fused_round_dga(_with(("server_config", "aggregate_median"),
                                 "mean"))
    assert spec == DGASpec("mean", 0.0, True, 0.5)


def test_local_dp_off_or_absent_means_no_clip():
    off = fused_round_dga(_with(("dp_config", "enable_local_dp"), False))
    assert off == DGASpec("train_loss", 2.5, False, 0.0)
    cfg = _cfg()
    del cfg["dp_config"]
    assert fused_round_dga(cfg) == off
    assert fused_round_dga(_with(("dp_config",), None)) == off


# every condition of the gate, flipped one at a time
REJECTED = [
    (("strategy",), "FedAvg"),
    (("strategy",), "FedProx"),
    (("strategy",), "FedLabels"),
    (("server_config", "fast_aggregation"), False),
    (("server_config", "wantRL"), True),
    (("server_config", "stale_prob"), 0.1),
    (("server_config", "type"), "personalization"),
    (("server_config", "aggregate_median"), "median"),
    (("dump_norm_stats",), True),
    (("privacy_metrics_config", "apply_metrics"), True),
    (("model_config", "freeze_layer"), "fc1"),
    (("client_config", "num_skips_threshold"), 0),
    (("client_config", "num_skips_threshold"), 3),
    (("client_config", "stats_on_smooth_grad"), True),
    (("client_config", "quant_thresh"), 1e-6),
    (("dp_config", "eps"), 0.0),      # noised local DP
    (("dp_config", "eps"), 10.0),
    (("dp_config", "max_grad"), 0.0),
]


@pytest.mark.parametrize("path,value", REJECTED)
def test_each_condition_alone_sends_the_round_to_the_pool(path, value):
    assert fused_round_dga(_cfg()) is not None
    assert fused_round_dga(_with(path, value)) is None


# the same switches in their off position stay eligible
ACCEPTED = [
    (("server_config", "fast_aggregation"), True),
    (("server_config", "wantRL"), False),
    (("server_config", "stale_prob"), 0.0),
    (("server_config", "stale_prob"), None),
    (("server_config", "type"), "model_optimization"),
    (("dump_norm_stats",), False),
    (("privacy_metrics_config",), None),
    (("model_config", "freeze_layer"), None),
    (("client_config", "num_skips_threshold"), -1),
    (("client_config", "stats_on_smooth_grad"), False),
    (("client_config", "quant_thresh"), None),
]


@pytest.mark.parametrize("path,value", ACCEPTED)
def test_switches_in_their_off_position_stay_eligible(path, value):
    assert fused_round_dga(_with(path, value)) == fused_round_dga(_cfg())


def test_fedavg_and_fedprox_keep_their_own_gate():
    for strategy, mu in (("FedAvg", 0.0), ("FedProx", 0.25)):
        cfg = _with(("strategy",), strategy)
        cfg["client_config"]["mu"] = 0.25
        assert fused_round_dga(cfg) is None
        assert fused_round_mu(strategy, cfg["client_config"],
                              cfg["model_config"], False) == mu
    # and DGA stays out of fused_round_mu
    assert fused_round_mu("DGA", _cfg()["client_config"], {}, False) is None
