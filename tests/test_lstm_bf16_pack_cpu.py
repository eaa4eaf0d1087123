"""bf16 weight layouts of the fused LSTM recurrence
(ops/lstm._pack_fwd_bf16 / _pack_bwd_bf16): the element mapping the
kernels of csrc/lstm_seq.hip index by, stack pass-through, and
round-to-nearest-even values.  Pure tensor code — runs without a GPU."""

import torch

from msrflute_amd.ops.lstm import _pack_bwd_bf16, _pack_fwd_bf16

H = 8


def _distinct(offset=0):
    """[4H, H] of distinct small integers (exact in bf16: |v| <= 256)."""
    return (torch.arange(4 * H * H, dtype=torch.float32) - 128 + offset) \
        .reshape(4 * H, H)


def test_pack_fwd_bf16_layout():
    w = _distinct()
    assert w.unique().numel() == w.numel()
    p = _pack_fwd_bf16(w)
    assert p.dtype == torch.bfloat16 and p.is_contiguous()
    assert tuple(p.shape) == (H // 8, 4 * H, 8)
    for kk in range(H // 8):
        for j in range(4 * H):
            for d in range(8):
                assert p[kk, j, d].item() == w[j, 8 * kk + d].item(), \
                    (kk, j, d)


def test_pack_bwd_bf16_layout():
    w = _distinct()
    p = _pack_bwd_bf16(w)
    assert p.dtype == torch.bfloat16 and p.is_contiguous()
    assert tuple(p.shape) == (4 * H // 8, H, 8)
    for jg in range(4 * H // 8):
        for h in range(H):
            for d in range(8):
                assert p[jg, h, d].item() == w[8 * jg + d, h].item(), \
                    (jg, h, d)


def test_pack_bf16_even_element_is_low_half_of_its_word():
    """The kernels widen a 32-bit word with u << 16 (element d even) and
    u & 0xffff0000 (d odd)."""
    w = _distinct()
    for p in (_pack_fwd_bf16(w), _pack_bwd_bf16(w)):
        words = p.view(torch.int32)              # [..., 4] per 8 elements
        lo = (words << 16).view(torch.float32)
        hi = (words & -65536).view(torch.float32)
        assert torch.equal(lo, p[..., 0::2].float())
        assert torch.equal(hi, p[..., 1::2].float())


def test_pack_bf16_stack_passes_through():
    w = torch.stack([_distinct(), -_distinct(1)])      # [K = 2, 4H, H]
    pf, pb = _pack_fwd_bf16(w), _pack_bwd_bf16(w)
    assert tuple(pf.shape) == (2, H // 8, 4 * H, 8)
    assert tuple(pb.shape) == (2, 4 * H // 8, H, 8)
    assert pf.is_contiguous() and pb.is_contiguous()
    for k in range(2):
        assert torch.equal(pf[k], _pack_fwd_bf16(w[k]))
        assert torch.equal(pb[k], _pack_bwd_bf16(w[k]))
    assert not torch.equal(pf[0], pf[1])


def test_pack_bf16_rounds_to_nearest_even():
    torch.manual_seed(0)
    w = torch.randn(4 * H, H) / 16               # not bf16-representable
    # truncation would give 1 + 2^-8 -> 1; nearest gives 1 + 2^-7
    w[5, 3] = 1 + 2.0 ** -8 + 2.0 ** -9
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3*2^-8 -> 1 + 2^-6
    w[6, 3] = 1 + 2.0 ** -8
    w[7, 3] = 1 + 3 * 2.0 ** -8
    wb = w.to(torch.bfloat16)
    assert not torch.equal(wb.float(), w)
    pf, pb = _pack_fwd_bf16(w), _pack_bwd_bf16(w)
    assert torch.equal(
        pf, wb.t().reshape(H // 8, 8, 4 * H).transpose(1, 2))
    assert torch.equal(pb, wb.reshape(4 * H // 8, 8, H).transpose(1, 2))
    assert pf[0, 5, 3].item() == 1 + 2.0 ** -7
    assert pb[0, 3, 5].item() == 1 + 2.0 ** -7
    assert pf[0, 6, 3].item() == 1.0
    assert pf[0, 7, 3].item() == 1 + 2.0 ** -6
