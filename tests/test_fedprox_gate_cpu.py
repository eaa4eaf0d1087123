"""The gate of the whole-round drivers (``core.client.fused_round_mu``):
which strategy / config runs them, and with which proximal coefficient."""

import pytest

from msrflute_amd.core.client import fused_round_mu


def test_fedavg_runs_with_mu_zero():
    mu = fused_round_mu("FedAvg", {"mu": 0.5}, {})
    assert mu == 0.0 and mu is not None


def test_fedprox_runs_with_its_mu():
    assert fused_round_mu("FedProx", {"mu": 0.25}, {}) == 0.25
    assert fused_round_mu("FedProx", {"mu": 1}, None) == 1.0


def test_fedprox_default_mu_is_process_rounds():
    assert fused_round_mu("FedProx", {}, {}) == 0.001


@pytest.mark.parametrize("strategy", ["DGA", "FedLabels"])
def test_other_strategies_stay_out(strategy):
    assert fused_round_mu(strategy, {"mu": 0.25}, {}) is None


@pytest.mark.parametrize("strategy", ["FedAvg", "FedProx"])
def test_frozen_layer_skips_threshold_and_privacy_stay_out(strategy):
    cc = {"mu": 0.25}
    assert fused_round_mu(strategy, cc, {"freeze_layer": "fc1"}) is None
    assert fused_round_mu(strategy, dict(cc, num_skips_threshold=0),
                          {}) is None
    assert fused_round_mu(strategy, dict(cc, num_skips_threshold=3),
                          {}) is None
    assert fused_round_mu(strategy, cc, {}, True) is None
    # the same configs with the feature off are eligible
    assert fused_round_mu(strategy, dict(cc, num_skips_threshold=-1),
                          {"freeze_layer": None}, False) is not None
