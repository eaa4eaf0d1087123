"""Fused attentive pooling (csrc/attn_pool.hip) through
``msrflute_amd.ops.attention.fused_attentive_pool`` and fednewsrec's
``AttentivePooling``.

Numerics follow the noise-floor rule of docs/kernels.md: relative L2
against float64, floor = the same formula in torch float32 on the CPU,
kernel error <= 4 x floor; where the float64 tensor is exactly zero the
kernel's must be too.  The gradient of b2 is exact zeros by contract and
stays out of the ratio."""

import copy
import importlib.util
import os

import pytest
import torch

from msrflute_amd.ops.attention import (fused_attentive_pool,
                                        fused_attentive_pool_available)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("y", "dx", "dW1", "db1", "dw2", "db2")


def _pool(x, w1, b1, w2, b2, dy, op=None):
    """The plain formula (or ``op``) and its gradients, on the inputs' own
    device and dtype."""
    ins = [t.clone().requires_grad_(True) for t in (x, w1, b1, w2, b2)]
    if op is None:
        xr, w1r, b1r, w2r, b2r = ins
        a = torch.tanh(xr @ w1r.t() + b1r) @ w2r + b2r
        y = (torch.softmax(a, dim=1).unsqueeze(-1) * xr).sum(1)
    else:
        y = op(*ins)
    return dict(zip(NAMES, (y,) + torch.autograd.grad(y, ins, dy)))


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


def _inputs(N, L, D, Hd):
    torch.manual_seed(1000 * L + D + Hd)
    return (torch.randn(N, L, D), torch.randn(Hd, D) / D ** 0.5,
            0.1 * torch.randn(Hd), torch.randn(Hd) / Hd ** 0.5,
            torch.randn(1), torch.randn(N, D))


def _against_float64(tag, ins):
    ref32 = _pool(*ins)
    ref64 = _pool(*(t.double() for t in ins))
    got = _pool(*(t.cuda() for t in ins), op=fused_attentive_pool)
    assert not got.pop("db2").any()
    ref32.pop("db2"), ref64.pop("db2")
    _check(tag, got, ref32, ref64)
    return got, ref32, ref64


@pytest.mark.parametrize("N,L,D,Hd", [
    (1, 1, 4, 4), (3, 2, 400, 200), (2, 17, 20, 12), (3, 28, 400, 200),
    (1, 50, 400, 200), (2, 64, 512, 256)])
def test_attn_pool_against_float64(N, L, D, Hd):
    assert fused_attentive_pool_available(L, D, Hd,
                                          torch.empty(1, device="cuda"))
    ins = _inputs(N, L, D, Hd)
    got, _, ref64 = _against_float64(f"N={N} L={L} D={D} Hd={Hd}", ins)
    if L == 1:
        assert not any(ref64[n].any() for n in ("dW1", "db1", "dw2"))
        assert torch.equal(got["y"].cpu(), ins[0][:, 0])
        assert torch.equal(got["dx"].cpu()[:, 0], ins[5])


def test_attn_pool_large_scores():
    """Scores beyond 88: exp overflows float32 without the max
    subtraction."""
    x, w1, b1, w2, b2, dy = _inputs(3, 28, 400, 200)
    w2 = w2 * 40.0
    a = torch.tanh(x @ w1.t() + b1) @ w2 + b2
    assert a.abs().max() > 88.0
    _, ref32, _ = _against_float64("large scores", (x, w1, b1, w2, b2, dy))
    assert all(torch.isfinite(t).all() for t in ref32.values())


@pytest.mark.parametrize("L", [28, 2])
def test_attn_pool_sequence_independence(L):
    """Sequence n = 1 of an N = 3 call is bit-equal to the same sequence run
    alone, whatever rows of the block's tile it lands in."""
    from msrflute_amd.ops import _C
    x, w1, b1, w2, b2, dy = (t.cuda() for t in _inputs(3, L, 400, 200))

    def run(x, dy):
        y, p, e = _C.attn_pool_fwd(x, w1, b1, w2, b2, True)
        return (y, p, e) + tuple(_C.attn_pool_bwd(x, e, p, w1, w2, dy))

    for big, one in zip(run(x, dy), run(x[1:2].clone(), dy[1:2].clone())):
        assert torch.equal(big[1:2], one)


def test_attentive_pooling_module():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_pool",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(400)
    pool = mod.AttentivePooling(400).eval()
    pool.fused = True
    x, dy = torch.randn(3, 28, 400), torch.randn(3, 400)
    sides = []
    for dev, dt in (("cuda", torch.float32), ("cpu", torch.float32),
                    ("cpu", torch.float64)):
        m = copy.deepcopy(pool).to(dev, dt)
        xi = x.detach().to(dev, dt).requires_grad_(True)
        y = m(xi)
        y.backward(dy.to(dev, dt))
        sides.append({"y": y, "dx": xi.grad, "dW1": m.dense.weight.grad,
                      "db1": m.dense.bias.grad, "dw2": m.dense2.weight.grad})
        if dev == "cuda":
            assert not m.dense2.bias.grad.any()
    _check("AttentivePooling(400)", *sides)
