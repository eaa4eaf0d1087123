"""Fused Conv1d + bias + ReLU on ``[N, T, C]`` rows (csrc/conv1d_seq.hip).

``fused_conv1d_relu(x, weight, bias)`` is
``relu(conv1d(x.transpose(1, 2), weight, bias)).transpose(1, 2)`` for a
stride-1, unpadded ``nn.Conv1d``, computed in the layout the rest of a
sequence model uses: ``x [N, T, Cin]`` in, ``y [N, T - KW + 1, Cout]`` out,
both contiguous, no transposed view on either side.  One launch forward on
the fp32 MFMA with bias and ReLU in its epilogue.  Backward, the weight and
bias gradients are a split-K MFMA kernel over the flat rows and its fold
(csrc/conv1d_bwd_w.hip), which read ``x``, ``y`` and ``dy`` as they are and
write ``dW`` in ``nn.Conv1d``'s layout; ``dx`` is one more launch, made only
when ``x`` needs a gradient.
"""

import torch

from . import HAS_EXT, _C
from .attention import _aligned

MAX_T, MAX_C, MAX_KW = 64, 512, 5


def fused_conv1d_relu_available(T, Cin, Cout, KW, x):
    """True when ``fused_conv1d_relu`` serves sequence length ``T``,
    ``Cin`` -> ``Cout`` channels, kernel width ``KW`` and tensor ``x``:
    1 <= KW <= 5, KW <= T <= 64, Cin and Cout multiples of 4 in 4..512,
    float32 on the GPU, extension built."""
    return HAS_EXT and x.is_cuda and x.dtype == torch.float32 \
        and 1 <= KW <= MAX_KW and KW <= T <= MAX_T \
        and Cin % 4 == 0 and 4 <= Cin <= MAX_C \
        and Cout % 4 == 0 and 4 <= Cout <= MAX_C


def _conv1d_pack(weight):
    """``nn.Conv1d``'s ``[Cout, Cin, KW]`` weight as the kernels read it:
    ``Wp[k, c, e] = weight[c, e, k]``, ``[KW, Cout, Cin]`` contiguous.  The
    forward reads ``Wp[k]`` as B^T and the backward as B; one pack serves
    both."""
    return weight.detach().permute(2, 0, 1).contiguous()


class _Conv1dReLU(torch.autograd.Function):
    """Saves x, y and the packed weight.  With ``dz = dy (y > 0)`` on T rows
    per sequence, the rows t > T - KW exactly zero, and the flat rows
    r = n T + t, ``dW[:, :, k] = dz[0 : R - k]^T x[k : R]`` is free of
    cross-sequence terms and ``db = sum_r dz``: ``_C.conv1d_relu_bwd_w``
    computes both from x, y and dy, masking while it stages.  Without ``dx``
    that is the whole backward."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, wp = _aligned(x), _conv1d_pack(weight)
        y = _C.conv1d_relu_fwd(x, wp, _aligned(bias.detach()))
        ctx.save_for_backward(x, y, wp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, wp = ctx.saved_tensors
        dy = _aligned(dy)
        dw, db = _C.conv1d_relu_bwd_w(x, y, dy, wp.shape[0])
        dx = _C.conv1d_relu_bwd(y, wp, dy, True)[0] \
            if ctx.needs_input_grad[0] else None
        return dx, dw, db


def fused_conv1d_relu(x, weight, bias):
    """x [N, T, Cin], weight [Cout, Cin, KW] (``nn.Conv1d``'s own), bias
    [Cout] -> relu(conv) [N, T - KW + 1, Cout].  Raises when the shape,
    dtype or device is not one ``fused_conv1d_relu_available`` accepts."""
    if not HAS_EXT:
        raise RuntimeError(
            "fused_conv1d_relu needs the msrflute_amd._C extension")
    return _Conv1dReLU.apply(x, weight, bias)
