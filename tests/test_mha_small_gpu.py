"""Fused short-sequence attention (csrc/mha_small.hip) through
``msrflute_amd.ops.attention.fused_mha`` and fednewsrec's ``SelfAttention``.

Numerics follow the noise-floor rule of docs/kernels.md: relative L2
against float64, floor = the same computation in torch float32 on the CPU,
kernel error <= 4 x floor; where the float64 tensor is exactly zero the
kernel's must be too."""

import copy
import importlib.util
import os

import pytest
import torch

from msrflute_amd.ops.attention import fused_mha, fused_mha_available

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("o", "dq", "dk", "dv")


def _attention(q, k, v, heads, do):
    """Plain softmax(q k^T / sqrt(d)) v on [N, L, heads*d]: o, dq, dk, dv."""
    q, k, v = (t.clone().requires_grad_(True) for t in (q, k, v))
    N, L, E = q.shape
    qh, kh, vh = (t.view(N, L, heads, E // heads).transpose(1, 2)
                  for t in (q, k, v))
    p = torch.softmax(qh @ kh.transpose(-1, -2) / (E // heads) ** 0.5, dim=-1)
    o = (p @ vh).transpose(1, 2).reshape(N, L, E)
    return dict(zip(NAMES, (o,) + torch.autograd.grad(o, [q, k, v], do)))


def _fused(q, k, v, heads, do):
    q, k, v = (t.cuda().requires_grad_(True) for t in (q, k, v))
    o = fused_mha(q, k, v, heads)
    return dict(zip(NAMES, (o,) + torch.autograd.grad(o, [q, k, v],
                                                      do.cuda())))


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).norm() / ref.norm()).item()


def _check(tag, got, ref32, ref64):
    for name, r64 in ref64.items():
        assert torch.isfinite(got[name]).all(), (tag, name)
        if not r64.any():
            assert not got[name].any(), (tag, name)
            continue
        err, floor = _rel_l2(got[name], r64), _rel_l2(ref32[name], r64)
        print(f"{tag} {name}: kernel {err:.3e} floor {floor:.3e}")
        assert err <= 4 * floor, (tag, name, err, floor)


def _inputs(N, L, heads, d):
    torch.manual_seed(1000 * L + 10 * heads + d)
    return torch.randn(4, N, L, heads * d).unbind(0)


def _against_float64(tag, q, k, v, do, heads):
    ref32 = _attention(q, k, v, heads, do)
    ref64 = _attention(*(t.double() for t in (q, k, v)), heads, do.double())
    _check(tag, _fused(q, k, v, heads, do), ref32, ref64)
    return ref32, ref64


@pytest.mark.parametrize("N,L,heads,d", [
    (1, 1, 1, 4), (2, 5, 3, 20), (1, 33, 3, 8), (3, 28, 20, 20),
    (1, 50, 20, 20), (2, 64, 2, 32)])
def test_mha_small_against_float64(N, L, heads, d):
    assert fused_mha_available(L, d, torch.empty(1, device="cuda"))
    _, ref64 = _against_float64(f"N={N} L={L} heads={heads} d={d}",
                                *_inputs(N, L, heads, d), heads)
    if L == 1:
        assert not ref64["dq"].any() and not ref64["dk"].any()


def test_mha_small_large_scores():
    """Scores of a few hundred: exp overflows float32 above 88 without the
    max subtraction."""
    q, k, v, do = _inputs(2, 28, 3, 20)
    q = q * 60.0
    scores = torch.einsum("nihd,njhd->nhij", q.view(2, 28, 3, 20),
                          k.view(2, 28, 3, 20)) / 20 ** 0.5
    assert scores.max() > 200.0
    ref32, ref64 = _against_float64("large scores", q, k, v, do, 3)
    for name in NAMES:
        assert torch.isfinite(ref32[name]).all()
        assert _rel_l2(ref32[name], ref64[name]) > 0.0


def test_mha_small_strided_inputs_bit_equal():
    from msrflute_amd.ops import _C
    torch.manual_seed(7)
    N, L, heads, d = 2, 28, 5, 20
    E = heads * d
    qkv = torch.randn(N, L, 3 * E, device="cuda")
    do = torch.randn(N, L, E, device="cuda")
    outs = []
    for q, k, v in (qkv.split(E, dim=2),
                    [t.contiguous() for t in qkv.split(E, dim=2)]):
        o, lse = _C.mha_small_fwd(q, k, v, heads)
        outs.append((o, lse) + tuple(_C.mha_small_bwd(q, k, v, o, lse, do)))
    assert not qkv.split(E, dim=2)[1].is_contiguous()
    for a, e in zip(*outs):
        assert torch.equal(a, e)


@pytest.mark.parametrize("L", [28, 50])
def test_mha_small_head_independence(L):
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


def test_self_attention_module():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_mha",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(400)
    attn = mod.SelfAttention(400, 20, 20, fused=True)
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
    assert len(sides[2]) == 5
    _check("SelfAttention(400, 20, 20)", *sides)
