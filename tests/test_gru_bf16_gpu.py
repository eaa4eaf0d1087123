"""bf16 weight streaming of the fused GRU recurrence (csrc/gru_seq.hip).

Contract: the bf16 kernel pair computes the fp32 pair at
``W_hh.bfloat16().float()`` bit for bit (bf16 is a storage format; every
product lands in the same accumulator chain in the same order), and
matches a float64 GRU2 loop at the rounded weights under the noise-floor
rule of docs/kernels.md: relative L2, floor = the same loop in torch
float32 on the CPU, kernel error <= 4 x floor."""

import importlib.util
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
H = 512
NAMES = ("h_seq", "dgi", "dW_hh", "db_hh")


def _gru_loop(gi, w, b, dh):
    """Plain GRU2 cell loop (gates r, z, n; zero state): h_seq and
    d<h_seq, dh> / d(gi, w, b)."""
    gi, w, b = (t.clone().requires_grad_(True) for t in (gi, w, b))
    h = gi.new_zeros(gi.shape[0], H)
    hs = []
    for t in range(gi.shape[1]):
        i_r, i_z, i_n = gi[:, t].chunk(3, dim=1)
        h_r, h_z, h_n = (h @ w.t() + b).chunk(3, dim=1)
        r, z = torch.sigmoid(i_r + h_r), torch.sigmoid(i_z + h_z)
        n = torch.tanh(i_n + r * h_n)
        h = n + z * (h - n)
        hs.append(h)
    h_seq = torch.stack(hs, dim=1)
    return (h_seq,) + torch.autograd.grad(h_seq, [gi, w, b], dh)


def _fused(gi, w, b, dh, **kw):
    from msrflute_amd.ops.lstm import fused_gru_seq
    gi, w, b = (t.cuda().requires_grad_(True) for t in (gi, w, b))
    h = fused_gru_seq(gi, w, b, **kw)
    return (h.detach(),) + torch.autograd.grad(h, [gi, w, b], dh.cuda())


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).norm() / ref.norm()).item()


@pytest.mark.parametrize("B,T", [(1, 1), (1, 2), (3, 7)])
def test_gru_seq_bf16(B, T):
    torch.manual_seed(10 * B + T)
    gi = torch.randn(B, T, 3 * H)
    w = torch.randn(3 * H, H) / H ** 0.5    # not bf16-representable
    b = torch.randn(3 * H) / 8
    dh = torch.randn(B, T, H)
    wr = w.bfloat16().float()
    got = _fused(gi, w, b, dh, bf16_weights=True)
    assert got[2].dtype == torch.float32 and got[2].shape == w.shape

    # bit-equal to the existing fp32 call on the rounded weights
    for name, a, e in zip(NAMES, got, _fused(gi, wr, b, dh)):
        assert torch.equal(a, e), (name, (a - e).abs().max().item())
    if T > 1:   # the path really rounds
        assert not torch.equal(got[0], _fused(gi, w, b, dh)[0])

    ref64 = _gru_loop(gi.double(), wr.double(), b.double(), dh.double())
    ref32 = _gru_loop(gi, wr, b, dh)
    for name, a, r32, r64 in zip(NAMES, got, ref32, ref64):
        if not r64.any():                   # dW_hh at T = 1: h_{t-1} = 0
            assert T == 1 and name == "dW_hh"
            assert not r32.any() and not a.any()
            continue
        err, floor = _rel_l2(a, r64), _rel_l2(r32, r64)
        print(f"B={B} T={T} {name}: kernel {err:.3e} floor {floor:.3e}")
        assert err <= 4 * floor, (name, err, floor)


def test_gru_cell_seq_bf16_recurrent():
    spec = importlib.util.spec_from_file_location(
        "nlg_gru_model_bf16",
        os.path.join(REPO, "experiments", "nlg_gru", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(41)
    assert mod.GRUCellSeq.bf16_recurrent is False
    cell = mod.GRUCellSeq(160, H).cuda()
    twin = mod.GRUCellSeq(160, H).cuda()
    twin.load_state_dict(cell.state_dict())
    cell.bf16_recurrent = True
    emb = torch.randn(3, 5, 160, device="cuda")
    with torch.no_grad():
        cell.eval(), twin.eval()            # fp32 on the unrounded masters
        assert torch.equal(cell(emb)[0], twin(emb)[0])
        eval_out = cell(emb)[0]
        twin.w_hh.weight.copy_(twin.w_hh.weight.bfloat16().float())
        cell.train(), twin.train()
        assert torch.equal(cell(emb)[0], twin(emb)[0])
        assert not torch.equal(cell(emb)[0], eval_out)
