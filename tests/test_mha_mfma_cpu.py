"""``fused_mha``'s ``impl`` argument, and fednewsrec with
``fused_attention: mfma`` on the CPU: the same keys, and SDPA on head
views, since no fused attention is ever chosen there."""

import pytest
import torch
from torch.nn import functional as F

from msrflute_amd.ops.attention import fused_mha
from test_mha_small_cpu import _model_module


def test_fused_mha_unknown_impl():
    q = torch.zeros(1, 2, 8)
    with pytest.raises(ValueError):
        fused_mha(q, q, q, 2, impl="nope")


def test_fednewsrec_mfma_flag_on_cpu():
    mod = _model_module()
    model = mod.FEDNEWS({"fused_attention": "mfma", "vocab_size": 50,
                         "embed_dim": 8})
    assert len(model.state_dict()) == 25
    attn = model.net.user_encoder.attn
    assert attn.fused == "mfma" and model.net.doc_encoder.attn.fused == "mfma"
    torch.manual_seed(5)
    x = torch.randn(2, 7, 400)
    q, k, v = (w(x).view(2, 7, 20, 20).transpose(1, 2)
               for w in (attn.wq, attn.wk, attn.wv))
    want = F.scaled_dot_product_attention(q, k, v).transpose(1, 2) \
        .reshape(2, 7, 400)
    assert torch.equal(attn(x), want)
