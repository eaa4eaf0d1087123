"""Fused LSTM sequence kernels vs torch nn.LSTM (GPU only): forward
outputs and ALL gradients (weights, biases, input) must match."""

import pytest
import torch

@pytest.mark.gpu
def test_fused_lstm_matches_nn_lstm():
    from msrflute_amd.ops.lstm import FusedLSTM

    torch.manual_seed(3)
    B, T, E, H, L = 4, 80, 8, 256, 2
    fused = FusedLSTM(E, H, num_layers=L).cuda()
    ref = torch.nn.LSTM(E, H, num_layers=L, batch_first=True).cuda()
    ref.load_state_dict(fused.state_dict())

    x1 = torch.randn(B, T, E, device="cuda", requires_grad=True)
    x2 = x1.detach().clone().requires_grad_(True)

    out1, _ = fused(x1)
    out2, _ = ref(x2)
    assert torch.allclose(out1, out2, rtol=1e-4, atol=1e-5), \
        (out1 - out2).abs().max().item()

    g = torch.randn_like(out1)
    out1.backward(g)
    out2.backward(g)
    assert torch.allclose(x1.grad, x2.grad, rtol=1e-3, atol=1e-5), \
        (x1.grad - x2.grad).abs().max().item()
    for (n1, p1), (n2, p2) in zip(fused.named_parameters(),
                                  ref.named_parameters()):
        assert n1 == n2
        assert torch.allclose(p1.grad, p2.grad, rtol=1e-3, atol=1e-4), \
            (n1, (p1.grad - p2.grad).abs().max().item())


@pytest.mark.gpu
def test_lstm_seq_stacked_matches_single_client():
    """The recurrence over K = 2 stacked clients (3 rows each, DIFFERENT
    W_hh) against a K = 1 call on each client alone.  The kernels are
    deterministic and a row's arithmetic does not depend on K, so h_seq
    and the gate gradients must be bit-equal — anything else is a row ->
    client indexing bug.  dW_hh goes through a differently batched GEMM."""
    from msrflute_amd.ops.lstm import _LSTMSeq

    torch.manual_seed(17)
    K, rpc, T, H = 2, 3, 5, 256
    # both clients see the SAME inputs, so only W_hh tells them apart
    xp = torch.randn(rpc, T, 4 * H, device="cuda").repeat(K, 1, 1) \
        .requires_grad_(True)
    w = (torch.randn(K, 4 * H, H, device="cuda") / 16).requires_grad_(True)
    dh = torch.randn(K * rpc, T, H, device="cuda")

    h = _LSTMSeq.apply(xp, w, rpc)
    dxp, dw = torch.autograd.grad(h, [xp, w], dh)
    for k in range(K):
        rows = slice(k * rpc, (k + 1) * rpc)
        xp_k = xp[rows].detach().clone().requires_grad_(True)
        w_k = w[k:k + 1].detach().clone().requires_grad_(True)
        h_k = _LSTMSeq.apply(xp_k, w_k, rpc)
        dxp_k, dw_k = torch.autograd.grad(h_k, [xp_k, w_k], dh[rows])
        assert torch.equal(h[rows], h_k), k
        assert torch.equal(dxp[rows], dxp_k), k
        assert torch.allclose(dw[k], dw_k[0], rtol=1e-3, atol=1e-4), \
            (k, (dw[k] - dw_k[0]).abs().max().item())
    # each client's rows really ran that client's weights
    assert not torch.equal(h[:rpc], h[rpc:])


def test_fused_lstm_cpu_fallback_is_exact():
    from msrflute_amd.ops.lstm import FusedLSTM
    torch.manual_seed(5)
    fused = FusedLSTM(8, 256, num_layers=2)
    ref = torch.nn.LSTM(8, 256, num_layers=2, batch_first=True)
    ref.load_state_dict(fused.state_dict())
    x = torch.randn(3, 12, 8)
    o1, _ = fused(x)
    o2, _ = ref(x)
    assert torch.allclose(o1, o2)


@pytest.mark.gpu
def test_fused_gru_matches_composite():
    """Fused GRU sequence vs the composite torch loop: forward + all
    gradients (w_ih via gi, w_hh, b_hh, input)."""
    import os
    from importlib.machinery import SourceFileLoader
    from msrflute_amd.ops.lstm import fused_gru_seq
    from msrflute_amd.ops import reference as ref_ops

    torch.manual_seed(11)
    B, T, H = 6, 25, 512
    w_hh = torch.nn.Linear(H, 3 * H).cuda()
    gi1 = torch.randn(B, T, 3 * H, device="cuda", requires_grad=True)
    gi2 = gi1.detach().clone().requires_grad_(True)

    # composite reference (reference GRU2 cell semantics)
    h = gi2.new_zeros(B, H)
    hs = []
    for t in range(T):
        g_h = w_hh(h)
        h = ref_ops.gru_gates(gi2[:, t], g_h, h)
        hs.append(h)
    out2 = torch.stack(hs, dim=1)

    out1 = fused_gru_seq(gi1, w_hh.weight, w_hh.bias)
    assert torch.allclose(out1, out2, rtol=1e-4, atol=1e-5), \
        (out1 - out2).abs().max().item()

    g = torch.randn_like(out1)
    w1g = torch.autograd.grad(out1, [gi1, w_hh.weight, w_hh.bias], g,
                              retain_graph=True)
    w2g = torch.autograd.grad(out2, [gi2, w_hh.weight, w_hh.bias], g)
    for a, b, name in zip(w1g, w2g, ["gi", "w_hh", "b_hh"]):
        assert torch.allclose(a, b, rtol=1e-3, atol=1e-4), \
            (name, (a - b).abs().max().item())
