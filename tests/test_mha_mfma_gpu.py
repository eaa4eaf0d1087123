"""Short-sequence attention on the fp32 MFMA (csrc/mha_mfma.hip) through
``fused_mha(..., impl="mfma")`` and fednewsrec's ``SelfAttention``.

The noise-floor rule of tests/test_mha_small_gpu.py, with its helpers:
relative L2 against float64, floor = the same computation in torch float32
on the CPU, kernel error <= 4 x floor; where the float64 tensor is exactly
zero the kernel's must be too."""

import copy
import importlib.util
import os

import pytest
import torch

from msrflute_amd.ops.attention import fused_mha
from test_mha_small_gpu import NAMES, _attention, _check, _inputs, _rel_l2

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fused(q, k, v, heads, do):
    q, k, v = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = fused_mha(q, k, v, heads, impl="mfma")
    return dict(zip(NAMES, (o,) + torch.autograd.grad(o, [q, k, v],
                                                      do.cuda())))


def _against_float64(tag, q, k, v, do, heads):
    ref32 = _attention(q, k, v, heads, do)
    ref64 = _attention(*(t.double() for t in (q, k, v)), heads, do.double())
    _check(tag, _fused(q, k, v, heads, do), ref32, ref64)
    return ref32, ref64


@pytest.mark.parametrize("N,L,heads,d", [
    (1, 1, 1, 4), (2, 5, 3, 20), (1, 17, 5, 8), (1, 33, 3, 12),
    (3, 28, 20, 20), (1, 50, 20, 20), (2, 64, 2, 32)])
def test_mha_mfma_against_float64(N, L, heads, d):
    _, ref64 = _against_float64(f"mfma N={N} L={L} heads={heads} d={d}",
                                *_inputs(N, L, heads, d), heads)
    if L == 1:
        assert not ref64["dq"].any() and not ref64["dk"].any()


def test_mha_mfma_large_scores():
    """Scores of a few hundred: exp overflows float32 above 88 without the
    max subtraction.  No saved lse is rounded on the way to the backward."""
    q, k, v, do = _inputs(2, 28, 3, 20)
    q = q * 60.0
    scores = torch.einsum("nihd,njhd->nhij", q.view(2, 28, 3, 20),
                          k.view(2, 28, 3, 20)) / 20 ** 0.5
    assert scores.max() > 200.0
    ref32, ref64 = _against_float64("mfma large scores", q, k, v, do, 3)
    for name in NAMES:
        assert torch.isfinite(ref32[name]).all()
        assert _rel_l2(ref32[name], ref64[name]) > 0.0


def test_mha_mfma_strided_inputs_bit_equal():
    from msrflute_amd.ops import _C
    torch.manual_seed(7)
    N, L, heads, d = 2, 28, 5, 20
    E = heads * d
    qkv = torch.randn(N, L, 3 * E, device="cuda")
    do = torch.randn(N, L, E, device="cuda")
    outs = []
    for q, k, v in (qkv.split(E, dim=2),
                    [t.contiguous() for t in qkv.split(E, dim=2)]):
        outs.append((_C.mha_mfma_fwd(q, k, v, heads),)
                    + tuple(_C.mha_mfma_bwd(q, k, v, do, heads)))
    assert not qkv.split(E, dim=2)[1].is_contiguous()
    for a, e in zip(*outs):
        assert torch.equal(a, e)


@pytest.mark.parametrize("L", [28, 50])
def test_mha_mfma_head_independence(L):
    """Problem (n, hd) alone (N = 1, heads = 1) is bit-equal to the same
    problem inside a larger call; hd = 4 is a last block's only head."""
    torch.manual_seed(L)
    N, heads, d, n, hd = 2, 5, 20, 1, 4
    q, k, v, do = torch.randn(4, N, L, heads * d).unbind(0)
    big = _fused(q, k, v, heads, do)
    cut = (slice(n, n + 1), slice(None), slice(hd * d, (hd + 1) * d))
    one = _fused(*(t[cut].contiguous() for t in (q, k, v)), 1,
                 do[cut].contiguous())
    for name in NAMES:
        assert torch.equal(big[name][cut], one[name]), name


def test_self_attention_module_mfma():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_mha_mfma",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(400)
    attn = mod.SelfAttention(400, 20, 20, fused="mfma")
    x, dy = torch.randn(3, 28, 400), torch.randn(3, 28, 400)
    sides = []
    for dev, dt in (("cuda", torch.float32), ("cpu", torch.float32),
                    ("cpu", torch.float64)):
        m = copy.deepcopy(attn).to(dev, dt)
        xi = x.detach().to(dev, dt).requires_grad_(True)
        y = m(xi)
        y.backward(dy.to(dev, dt))
        side = {"y": y, "dx": xi.grad}
        side.update((f"d{n}", p.grad) for n, p in m.named_parameters())
        sides.append(side)
    assert len(sides[2]) == 5 and m.fused == "mfma"
    _check("SelfAttention(400, 20, 20, mfma)", *sides)
