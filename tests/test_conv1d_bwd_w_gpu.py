"""Conv1d + ReLU backward-weights (csrc/conv1d_bwd_w.hip) through
``_C.conv1d_relu_bwd_w`` and ``fused_conv1d_relu``.

Noise-floor rule of docs/kernels.md: relative L2 against ``F.conv1d`` +
``relu`` autograd in float64 on the CPU, floor = the same in float32 on the
CPU, kernel error <= 4 x floor; where the float64 tensor is exactly zero the
kernel's must be too."""

import pytest
import torch
from torch.nn import functional as F

from msrflute_amd.ops.conv1d import _conv1d_pack, fused_conv1d_relu

pytestmark = pytest.mark.gpu

SLABS = (70, 30, 20, 12, 3)


def _inputs(N, T, Cin, Cout, KW):
    torch.manual_seed(1000 * T + Cin + Cout + KW)
    return (torch.randn(N, T, Cin),
            torch.randn(Cout, Cin, KW) / (Cin * KW) ** 0.5,
            0.1 * torch.randn(Cout), torch.randn(N, T - KW + 1, Cout))


def _ref(x, w, b, dy):
    """y, dW, db of ``F.conv1d`` + ``relu`` in the inputs' dtype."""
    w, b = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.relu(F.conv1d(x.transpose(1, 2), w, b)).transpose(1, 2)
    return (y.detach(),) + torch.autograd.grad(y, (w, b), dy)


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("N,T,Cin,Cout,KW", [
    (1, 1, 4, 4, 1), (5, 3, 8, 8, 3), (3, 7, 20, 12, 2), (2, 9, 36, 68, 4),
    (3, 30, 300, 400, 3), (2, 64, 512, 512, 5), SLABS])
def test_conv1d_bwd_w_against_float64(N, T, Cin, Cout, KW):
    from msrflute_amd.ops import _C
    if (N, T, Cin, Cout, KW) == SLABS:
        # ragged last slab, a slab boundary inside a sequence
        S, slab = _C.conv1d_bwd_w_slabs(N, T), _C.CONV1D_BWD_W_SLAB
        assert S >= 2 and S == -(-N * T // slab) and N * T % slab != 0
        assert slab % T != 0
    ins = _inputs(N, T, Cin, Cout, KW)
    ref32, ref64 = _ref(*ins), _ref(*(t.double() for t in ins))
    x, w, b, dy = (t.cuda() for t in ins)
    y = _C.conv1d_relu_fwd(x, _conv1d_pack(w), b)
    # the gradients are compared at one mask, not across a flipped entry
    assert torch.equal(y.cpu() > 0, ref64[0] > 0)
    got = _C.conv1d_relu_bwd_w(x, y, dy, KW)
    for name, g, r32, r64 in zip(("dW", "db"), got, ref32[1:], ref64[1:]):
        assert g.shape == r64.shape and torch.isfinite(g).all(), name
        if not r64.any():
            assert not g.any(), name
            continue
        err, floor = _rel_l2(g, r64), _rel_l2(r32, r64)
        print(f"{(N, T, Cin, Cout, KW)} {name}: kernel {err:.3e} "
              f"floor {floor:.3e}")
        assert err <= 4 * floor, (name, err, floor)


def test_conv1d_bwd_w_bit_equal_and_wired():
    """Two calls are bit-equal, and ``fused_conv1d_relu``'s dW and db, with
    and without a gradient for x, are the direct call's."""
    from msrflute_amd.ops import _C
    x, w, b, dy = (t.cuda() for t in _inputs(*SLABS))
    y = _C.conv1d_relu_fwd(x, _conv1d_pack(w), b)
    dW, db = _C.conv1d_relu_bwd_w(x, y, dy, SLABS[4])
    again = _C.conv1d_relu_bwd_w(x, y, dy, SLABS[4])
    assert torch.equal(dW, again[0]) and torch.equal(db, again[1])
    for need_dx in (False, True):
        xi = x.clone().requires_grad_(need_dx)
        wi, bi = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        fused_conv1d_relu(xi, wi, bi).backward(dy)
        assert (xi.grad is not None) == need_dx
        assert torch.equal(wi.grad, dW) and torch.equal(bi.grad, db)
