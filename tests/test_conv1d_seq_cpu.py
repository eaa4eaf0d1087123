"""The fused title convolution off the GPU: the packed weight's layout,
what ``fused_conv1d_relu_available`` turns down, and fednewsrec's
``fused_conv`` flag falling back to ``nn.Conv1d`` bit for bit."""

import importlib.util
import os
from types import SimpleNamespace

import pytest
import torch
from torch.nn import functional as F

from msrflute_amd.ops.conv1d import (_conv1d_pack,
                                     fused_conv1d_relu_available)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_conv1d_pack_layout():
    w = torch.randn(12, 8, 3)
    wp = _conv1d_pack(w)
    assert wp.shape == (3, 12, 8) and wp.is_contiguous()
    for k in range(3):
        assert torch.equal(wp[k], w[:, :, k])


@pytest.mark.parametrize("T,Cin,Cout,KW,is_cuda", [
    (30, 300, 400, 3, False), (2, 300, 400, 3, True),
    (65, 300, 400, 3, True), (30, 6, 400, 3, True), (30, 300, 400, 6, True)])
def test_fused_conv1d_relu_unavailable(T, Cin, Cout, KW, is_cuda):
    """A CPU tensor, T < KW, T = 65, Cin = 6, KW = 6.  Only ``is_cuda`` and
    ``dtype`` of the tensor are looked at, so a stand-in serves where there
    is no GPU; the task's own shape is served wherever the extension is."""
    from msrflute_amd.ops import HAS_EXT
    x = SimpleNamespace(is_cuda=is_cuda, dtype=torch.float32)
    assert not fused_conv1d_relu_available(T, Cin, Cout, KW, x)
    x.is_cuda = True
    assert fused_conv1d_relu_available(30, 300, 400, 3, x) == HAS_EXT


def test_fednewsrec_conv_flag_is_inert_on_cpu():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_conv_cpu",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    click, sample = (torch.randint(0, 50, (2, 5, 7)) for _ in range(2))
    losses = []     # through net, not loss(): loss() moves its batch to a GPU
    for flag in (False, True):
        torch.manual_seed(9)
        model = mod.FEDNEWS({"vocab_size": 50, "embed_dim": 8,
                             "fused_conv": flag})
        model.set_train()
        assert model.net.doc_encoder.fused_conv is flag
        torch.manual_seed(10)
        scores, _ = model.net(click, sample)
        losses.append(F.cross_entropy(scores, torch.tensor([0, 3])))
    assert torch.equal(*losses)
