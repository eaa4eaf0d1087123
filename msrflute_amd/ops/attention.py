"""Fused multi-head attention for short sequences (csrc/mha_small.hip).

``fused_mha(q, k, v, heads)`` is ``softmax(q k^T / sqrt(d)) v`` per head on
``[N, L, heads*d]`` tensors in the layout the projection GEMMs produce: no
``[N, heads, L, d]`` view or copy on the way in or out, no mask, no dropout,
not causal.  One launch forward, one backward.  q, k and v may be
contiguous or three slices of one ``[N, L, 3*heads*d]`` buffer.
"""

import torch

from . import HAS_EXT, _C

MAX_L, MAX_D = 64, 32


def fused_mha_available(L, d, x):
    """True when ``fused_mha`` serves sequence length ``L``, head dimension
    ``d`` and tensor ``x``: 1 <= L <= 64, d % 4 == 0, 4 <= d <= 32, float32
    on the GPU, extension built."""
    return HAS_EXT and x.is_cuda and x.dtype == torch.float32 \
        and 1 <= L <= MAX_L and d % 4 == 0 and 4 <= d <= MAX_D


def _rows(t):
    """``t`` as the kernel reads it: unit element stride, rows a constant
    multiple of 4 floats apart, 16-byte aligned base (the bindings check);
    anything else is copied."""
    N, L, _ = t.shape
    S = t.stride(1) if L > 1 else t.stride(0)
    ok = t.stride(2) == 1 and S % 4 == 0 and t.data_ptr() % 16 == 0 \
        and (N == 1 or t.stride(0) == L * S)
    return t if ok else t.contiguous()


class _MHASmall(torch.autograd.Function):
    """Saves q, k, v, o and lse [N, heads, L]; the backward recomputes the
    probabilities from them."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        q, k, v = _rows(q), _rows(k), _rows(v)
        if not (q.stride() == k.stride() == v.stride()):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        o, lse = _C.mha_small_fwd(q, k, v, heads)
        ctx.save_for_backward(q, k, v, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        dq, dk, dv = _C.mha_small_bwd(q, k, v, o, lse, do.contiguous())
        return dq, dk, dv, None


def fused_mha(q, k, v, heads):
    """[N, L, heads*d] x 3 -> [N, L, heads*d], scale 1/sqrt(d).  Raises when
    the shape, dtype or device is not one ``fused_mha_available`` accepts."""
    if not HAS_EXT:
        raise RuntimeError("fused_mha needs the msrflute_amd._C extension")
    return _MHASmall.apply(q, k, v, int(heads))
