"""Fused multi-head attention for short sequences (csrc/mha_small.hip,
csrc/mha_mfma.hip).

``fused_mha(q, k, v, heads)`` is ``softmax(q k^T / sqrt(d)) v`` per head on
``[N, L, heads*d]`` tensors in the layout the projection GEMMs produce: no
``[N, heads, L, d]`` view or copy on the way in or out, no mask, no dropout,
not causal.  One launch forward, one backward.  q, k and v may be
contiguous or three slices of one ``[N, L, 3*heads*d]`` buffer.
``impl="lanes"`` (the default) gives a lane one query row (mha_small.hip);
``impl="mfma"`` gives a wave one (sequence, head) problem on the fp32 MFMA
(mha_mfma.hip) and saves nothing but q, k and v.

``fused_attentive_pool(x, w1, b1, w2, b2)`` is additive attention pooling
(csrc/attn_pool.hip): ``softmax_L(tanh(x w1^T + b1) . w2 + b2)``-weighted
sum of the rows of ``x``, one launch forward and one backward on the fp32
MFMA, with the three weight gradients left to library GEMMs.
"""

import torch

from . import HAS_EXT, _C

MAX_L, MAX_D = 64, 32
POOL_MAX_D, POOL_MAX_HD = 512, 256


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


class _MHAMfma(torch.autograd.Function):
    """Saves q, k, v only: the backward recomputes the scores, the row
    maxima and sums with the forward's instructions, and takes
    D = sum_j P dP from its registers, so neither o nor an lse is read."""

    @staticmethod
    def forward(ctx, q, k, v, heads):
        q, k, v = _rows(q), _rows(k), _rows(v)
        if not (q.stride() == k.stride() == v.stride()):
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        ctx.save_for_backward(q, k, v)
        ctx.heads = heads
        return _C.mha_mfma_fwd(q, k, v, heads)

    @staticmethod
    def backward(ctx, do):
        q, k, v = ctx.saved_tensors
        dq, dk, dv = _C.mha_mfma_bwd(q, k, v, _aligned(do), ctx.heads)
        return dq, dk, dv, None


_IMPLS = {"lanes": _MHASmall, "mfma": _MHAMfma}


def fused_mha(q, k, v, heads, impl="lanes"):
    """[N, L, heads*d] x 3 -> [N, L, heads*d], scale 1/sqrt(d), by
    mha_small.hip (``impl="lanes"``) or mha_mfma.hip (``impl="mfma"``).
    Raises when the shape, dtype or device is not one
    ``fused_mha_available`` accepts, and ``ValueError`` for any other
    ``impl``."""
    if impl not in _IMPLS:
        raise ValueError(f"fused_mha: impl must be one of {sorted(_IMPLS)}, "
                         f"got {impl!r}")
    if not HAS_EXT:
        raise RuntimeError("fused_mha needs the msrflute_amd._C extension")
    return _IMPLS[impl].apply(q, k, v, int(heads))


def fused_attentive_pool_available(L, D, Hd, x):
    """True when ``fused_attentive_pool`` serves sequence length ``L``, width
    ``D``, hidden width ``Hd`` and tensor ``x``: 1 <= L <= 64, D % 4 == 0,
    4 <= D <= 512, Hd % 4 == 0, 4 <= Hd <= 256, float32 on the GPU,
    extension built."""
    return HAS_EXT and x.is_cuda and x.dtype == torch.float32 \
        and 1 <= L <= MAX_L and D % 4 == 0 and 4 <= D <= POOL_MAX_D \
        and Hd % 4 == 0 and 4 <= Hd <= POOL_MAX_HD


def _aligned(t):
    """``t`` as the pooling kernels read it: contiguous on a 16-byte aligned
    base (the bindings check).  A parameter that is a view into a flat
    arena need not be; it is copied."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class _AttnPool(torch.autograd.Function):
    """Saves x, e = tanh(x w1^T + b1) [N, L, Hd] and p [N, L].  The backward
    kernel gives dx, dz (the gradient at the pre-activation) and da (at the
    scores); the weight gradients are library GEMMs on them, as in the
    recurrences.  The gradient of b2 is returned as exact zeros: softmax is
    shift-invariant, so it is mathematically 0, and what autograd returns
    for the unfused chain there is rounding noise."""

    @staticmethod
    def forward(ctx, x, w1, b1, w2, b2):
        x, w1, b1, w2, b2 = (_aligned(t) for t in (x, w1, b1, w2, b2))
        save = any(ctx.needs_input_grad)
        y, p, e = _C.attn_pool_fwd(x, w1, b1, w2, b2, save)
        if save:
            ctx.save_for_backward(x, e, p, w1, w2)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, e, p, w1, w2 = ctx.saved_tensors
        dx, dz, da = _C.attn_pool_bwd(x, e, p, w1, w2, _aligned(dy))
        dz, e = dz.flatten(0, 1), e.flatten(0, 1)
        return (dx, dz.t() @ x.flatten(0, 1), dz.sum(0), da.flatten() @ e,
                dy.new_zeros(1))


def fused_attentive_pool(x, w1, b1, w2, b2):
    """x [N, L, D], w1 [Hd, D], b1 [Hd], w2 [Hd] (or [1, Hd]), b2 [1] ->
    [N, D].  Raises when the shape, dtype or device is not one
    ``fused_attentive_pool_available`` accepts."""
    if not HAS_EXT:
        raise RuntimeError(
            "fused_attentive_pool needs the msrflute_amd._C extension")
    return _AttnPool.apply(x, w1, b1, w2.reshape(-1), b2)
