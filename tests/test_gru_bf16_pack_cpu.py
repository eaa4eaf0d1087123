"""bf16 weight layouts of the fused GRU recurrence (ops/lstm.py): shape,
element map, round to nearest even and half-word order."""

import os

import pytest
import torch
import yaml

H = 512
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mp", [None, "bf16"])
def test_client_sets_bf16_recurrent_on_gru(mp):
    """mixed_precision: bf16 reaches the dynamically loaded GRUCellSeq of
    the client's model replica; without it the attribute stays off."""
    from msrflute_amd.config import FLUTEConfig
    from msrflute_amd.core.client import ClientExecutor
    from msrflute_amd.models import make_model
    from msrflute_amd.ops.arena import ParameterArena

    with open(os.path.join(REPO, "configs", "nlg_gru.yaml")) as f:
        cfg = yaml.safe_load(f)
    if mp:
        cfg["client_config"]["mixed_precision"] = mp
    config = FLUTEConfig.from_dict(cfg)
    arena = ParameterArena(make_model(config["model_config"]))
    ex = ClientExecutor(config, "nlg_gru", None, arena)
    assert ex.model.rnn.bf16_recurrent is (mp == "bf16")
    assert type(ex.model.rnn).bf16_recurrent is False


def test_gru_bf16_packs_layout_and_rounding():
    from msrflute_amd.ops.lstm import _gru_pack_bwd_bf16, _gru_pack_fwd_bf16

    torch.manual_seed(3)
    w = torch.randn(3 * H, H) / 16
    # bf16 keeps 8 significant bits: 1 + 2^-8 and 1 + 3 * 2^-8 are exact
    # ties (to even: down to 1, up to 1 + 2^-6), 1 + 2^-8 -+ 2^-12 sit on
    # either side of the boundary
    planted = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,
                            1 + 2.0 ** -8 - 2.0 ** -12,
                            1 + 2.0 ** -8 + 2.0 ** -12])
    w[5, 8:12] = planted
    w[1000, 500:504] = -planted
    ref = w.bfloat16()
    assert ref[5, 8:12].float().tolist() == [1.0, 1 + 2.0 ** -6, 1.0,
                                             1 + 2.0 ** -7]

    fwd, bwd = _gru_pack_fwd_bf16(w), _gru_pack_bwd_bf16(w)
    for p, shape in ((fwd, (H // 8, 3 * H, 8)), (bwd, (3 * H // 8, H, 8))):
        assert p.dtype == torch.bfloat16 and p.is_contiguous()
        assert p.shape == shape
    # (kk, j, d) = bf16(W[j, 8kk+d]);  (jg, h, d) = bf16(W[8jg+d, h])
    assert torch.equal(fwd, ref.t().reshape(H // 8, 8, 3 * H).permute(0, 2, 1))
    assert torch.equal(bwd, ref.reshape(3 * H // 8, 8, H).permute(0, 2, 1))
    kk, j, d = 1, 5, 1                      # the second planted tie
    assert fwd[kk, j, d] == ref[j, 8 * kk + d] == 1 + 2.0 ** -6
    jg, h, d = 125, 502, 0                  # W[1000, 502]
    assert bwd[jg, h, d] == ref[8 * jg + d, h] == -1.0
    # element d even is the low half of its 32-bit word
    for p in (fwd, bwd):
        words = p.view(torch.int32)
        bits = p.view(torch.int16).to(torch.int32) & 0xffff
        assert torch.equal(words & 0xffff, bits[..., 0::2])
        assert torch.equal((words >> 16) & 0xffff, bits[..., 1::2])
