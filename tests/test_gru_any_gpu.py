"""Any-H fused GRU recurrence (csrc/gru_seq_any.hip), its K-stacked
contract, ``FusedGRU`` and ``GRUCellSeq`` at a hidden size other than 512.

Numerics follow the noise-floor rule of docs/kernels.md: relative L2
against float64, floor = the same computation in torch float32 on the CPU,
kernel error <= 4 x floor."""

import copy
import importlib.util
import os

import pytest
import torch
from torch import nn

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _gru_loop(gi, w, b, dh):
    """Plain GRU2 cell loop (gates r, z, n; zero state): h_seq and
    d<h_seq, dh> / d(gi, w, b)."""
    gi, w, b = (t.clone().requires_grad_(True) for t in (gi, w, b))
    h = gi.new_zeros(gi.shape[0], w.shape[1])
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


def _rel_l2(a, ref):
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    return ((a - ref).norm() / ref.norm()).item()


def _check(tag, got, ref32, ref64):
    """got / ref32 / ref64: dicts name -> tensor; 4 x floor on each."""
    for name, r64 in ref64.items():
        err, floor = _rel_l2(got[name], r64), _rel_l2(ref32[name], r64)
        print(f"{tag} {name}: kernel {err:.3e} floor {floor:.3e}")
        assert err <= 4 * floor, (tag, name, err, floor)


def _inputs(K, rows, T, H, seed):
    torch.manual_seed(seed)
    return (torch.randn(K * rows, T, 3 * H),
            torch.randn(K, 3 * H, H) / H ** 0.5,
            torch.randn(K, 3 * H) / 8, torch.randn(K * rows, T, H))


def _any_pair(gi, w, b, dh, rows_per_client):
    """The new entries on a [K, 3H, H] stack: all five outputs."""
    from msrflute_amd.ops import _C
    from msrflute_amd.ops.lstm import _gru_pack_bwd, _gru_pack_fwd
    gi, w, b, dh = (t.cuda() for t in (gi, w, b, dh))
    h_seq, gates, ghn = _C.gru_seq_any_fwd(gi, _gru_pack_fwd(w), b,
                                           rows_per_client)
    dgi, dgh = _C.gru_seq_any_bwd(gates, ghn, h_seq, _gru_pack_bwd(w), dh,
                                  rows_per_client)
    return h_seq, gates, ghn, dgi, dgh


# Shipped counts: forward 16 resident groups per gate column, streamed
# unroll 2 (NG = H/4); backward 8 resident groups, streamed unroll 5
# (NG = 3H/4).
#   H = 4:   NG 1 / 3, everything resident, 4 live lanes of one wave, T = 1
#            (dW_hh exactly zero)
#   H = 12:  backward NG = 9 = REG + 1, a single streamed group (the forward,
#            NG = 3, is resident)
#   H = 68:  forward NG = 17 = REG + 1, a single streamed group; 2 waves, 4
#            live lanes in the second; backward streams 43 = 8 x 5 + 3
#   H = 400: 448 threads (48 idle lanes in the last wave); forward streams
#            84 = 42 x 2, backward 292 = 58 x 5 + 2
@pytest.mark.parametrize("H,rows,T", [(4, 1, 1), (12, 3, 2), (68, 1, 7),
                                      (400, 3, 7)])
def test_gru_any_against_float64(H, rows, T):
    from msrflute_amd.ops.lstm import fused_gru_seq
    gi, w, b, dh = _inputs(1, rows, T, H, 100 * H + 10 * rows + T)
    w, b = w[0], b[0]
    names = ("h_seq", "dgi", "dW_hh", "db_hh")
    g, wc, bc = (t.cuda().requires_grad_(True) for t in (gi, w, b))
    h = fused_gru_seq(g, wc, bc)
    got = dict(zip(names, (h.detach(),) + torch.autograd.grad(
        h, [g, wc, bc], dh.cuda())))
    ref32 = dict(zip(names, _gru_loop(gi, w, b, dh)))
    ref64 = dict(zip(names, _gru_loop(*(t.double() for t in (gi, w, b, dh)))))
    if T == 1:      # h_{t-1} = 0: dW_hh is exactly zero on all three sides
        for side in (got, ref32, ref64):
            assert not side.pop("dW_hh").any()
    _check(f"H={H} rows={rows} T={T}", got, ref32, ref64)


@pytest.mark.parametrize("B,T", [(1, 2), (3, 7)])
def test_gru_any_bit_equal_to_h512_pair(B, T):
    from msrflute_amd.ops import _C
    from msrflute_amd.ops.lstm import _gru_pack_bwd, _gru_pack_fwd
    gi, w, b, dh = _inputs(1, B, T, 512, 10 * B + T)
    new = _any_pair(gi, w, b, dh, B)
    gi, w, b, dh = gi.cuda(), w[0].cuda(), b[0].cuda(), dh.cuda()
    h_seq, gates, ghn = _C.gru_seq_fwd(gi, _gru_pack_fwd(w), b)
    old = (h_seq, gates, ghn) + tuple(
        _C.gru_seq_bwd(gates, ghn, h_seq, _gru_pack_bwd(w), dh))
    for name, a, e in zip(("h_seq", "gates", "ghn", "dgi", "dgh"), new, old):
        assert torch.equal(a, e), (name, (a - e).abs().max().item())


@pytest.mark.parametrize("H", [68, 400])
def test_gru_any_stacked_equals_single(H):
    gi, w, b, dh = _inputs(2, 3, 5, H, H)
    assert not torch.equal(w[0], w[1])
    stacked = _any_pair(gi, w, b, dh, 3)
    for k in range(2):
        rows = slice(3 * k, 3 * k + 3)
        single = _any_pair(gi[rows], w[k:k + 1], b[k:k + 1], dh[rows], 3)
        for a, e in zip(stacked, single):
            assert torch.equal(a[rows], e)


def _module_sides(fused, ref, x, dys):
    """(``fused`` on the GPU, ``ref`` in float32 and in float64 on the CPU):
    outputs, input gradient and parameter gradients, each as a dict."""
    sides = []
    for m, dev, dt in ((fused, "cuda", torch.float32),
                       (ref, "cpu", torch.float32),
                       (ref, "cpu", torch.float64)):
        m = copy.deepcopy(m).to(dev, dt)
        xi = x.detach().to(dev, dt).requires_grad_(True)
        outs = m(xi)
        sum((o * d.to(dev, dt)).sum() for o, d in zip(outs, dys)).backward()
        side = {f"out{i}": o for i, o in enumerate(outs)}
        side["dx"] = xi.grad
        side.update((f"d{n}", p.grad) for n, p in m.named_parameters())
        sides.append(side)
    return sides


@pytest.mark.parametrize("H", [36, 400])
def test_fused_gru_module(H):
    from msrflute_amd.ops.lstm import FusedGRU
    torch.manual_seed(H)
    fused = FusedGRU(5, H, num_layers=2)
    ref = nn.GRU(5, H, num_layers=2, batch_first=True)
    ref.load_state_dict(fused.state_dict())
    x = torch.randn(3, 7, 5)
    dys = (torch.randn(3, 7, H), torch.randn(2, 3, H))
    got, ref32, ref64 = _module_sides(fused, ref, x, dys)
    assert got["out1"].shape == (2, 3, H) and len(ref64) == 11
    _check(f"FusedGRU H={H}", got, ref32, ref64)


@pytest.mark.parametrize("train", [True, False])
def test_gru_cell_seq_h32(train):
    spec = importlib.util.spec_from_file_location(
        "nlg_gru_model_any",
        os.path.join(REPO, "experiments", "nlg_gru", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    from msrflute_amd.ops.lstm import fused_gru_available
    torch.manual_seed(32)
    cell = mod.GRUCellSeq(16, 32).train(train)
    x = torch.randn(3, 7, 16)
    assert fused_gru_available(32, x.cuda())
    dys = (torch.randn(3, 8, 32), torch.randn(3, 32))
    got, ref32, ref64 = _module_sides(cell, cell, x, dys)
    _check(f"GRUCellSeq train={train}", got, ref32, ref64)
