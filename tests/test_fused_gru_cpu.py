"""``FusedGRU`` is ``nn.GRU`` on the CPU: same state dict, same init draws,
same results; the fednewsrec net holds it under the parent's keys."""

import importlib.util
import os

import torch
from torch import nn

from msrflute_amd.ops.lstm import FusedGRU

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fused_gru_is_nn_gru_on_cpu():
    torch.manual_seed(3)
    fused = FusedGRU(5, 12, num_layers=2)
    torch.manual_seed(3)
    ref = nn.GRU(5, 12, num_layers=2, batch_first=True)
    assert [(k, v.shape) for k, v in fused.state_dict().items()] == \
        [(k, v.shape) for k, v in ref.state_dict().items()]
    x = torch.randn(3, 7, 5)
    for a, e in zip(fused(x), ref(x)):
        assert torch.equal(a, e)
    hx = torch.randn(2, 3, 12)
    assert torch.equal(fused(x, hx)[0], ref(x, hx)[0])


def test_fednewsrec_has_no_rnnbase_and_keeps_its_keys():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_keys",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    model = mod.FEDNEWS({"vocab_size": 50, "embed_dim": 8})
    assert not any(isinstance(m, nn.RNNBase) for m in model.modules())
    sd = model.state_dict()
    gru = {k: tuple(v.shape) for k, v in sd.items() if ".gru." in k}
    assert gru == {
        "net.user_encoder.gru.weight_ih_l0": (1200, 400),
        "net.user_encoder.gru.weight_hh_l0": (1200, 400),
        "net.user_encoder.gru.bias_ih_l0": (1200,),
        "net.user_encoder.gru.bias_hh_l0": (1200,),
    }
    # the keys around the GRU are the parent's too: nothing of the
    # unregistered fallback leaks into the state dict
    assert not any("_fallback" in k for k in sd)
    assert [k.split(".")[2] for k in sd if k.startswith("net.user_encoder.")
            ] == ["attn"] * 3 + ["pool_attn"] * 4 + ["gru"] * 4 + \
        ["pool_fuse"] * 4
