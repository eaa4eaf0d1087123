"""On the CPU the fused attentive pooling is never chosen: fednewsrec's
``AttentivePooling`` gives what it gave with the flag off, under the same
keys.  (The kernels read ``dense.weight`` as it is; there is no packed
layout to check.)"""

import copy
import importlib.util
import os

import torch

from msrflute_amd.ops.attention import fused_attentive_pool_available

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model_module():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_pool_cpu",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fused_attentive_pool_unavailable_on_cpu():
    assert not fused_attentive_pool_available(28, 400, 200, torch.zeros(1))


def test_attentive_pooling_flag_is_inert_on_cpu():
    torch.manual_seed(6)
    off = _model_module().AttentivePooling(24, hidden=12).eval()
    on = copy.deepcopy(off)
    on.fused = True
    x = torch.randn(2, 7, 24)
    assert not off.fused and torch.equal(on(x), off(x))


def test_fednewsrec_pooling_keys_unchanged():
    sd = _model_module().FEDNEWS({"vocab_size": 50, "embed_dim": 8}) \
        .state_dict()
    assert len(sd) == 25
    want = {"dense.weight": (200, 400), "dense.bias": (200,),
            "dense2.weight": (1, 200), "dense2.bias": (1,)}
    assert {k: tuple(v.shape) for k, v in sd.items() if ".pool" in k} == {
        f"net.{pool}.{k}": shape for k, shape in want.items()
        for pool in ("doc_encoder.pool", "user_encoder.pool_attn",
                     "user_encoder.pool_fuse")}
