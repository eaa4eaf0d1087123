"""Fused LSTM recurrence at hidden sizes 64 and 128 (k_lstm_seq_small_*)
against float64 under the noise-floor rule of docs/kernels.md: floor = the
same computation in torch float32 on the CPU; error <= 4 x floor <= 1e-3."""

import importlib.util
import os

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [64, 128]


def _rel_l2(a, ref):
    """Relative L2; absolute against a zero reference (dW_hh at T = 1)."""
    a, ref = a.detach().cpu().double(), ref.detach().cpu().double()
    n = ref.norm().item()
    return (a - ref).norm().item() / (n if n > 0 else 1.0)


def _check(name, got, ref32, ref64):
    err, floor = _rel_l2(got, ref64), _rel_l2(ref32, ref64)
    print(f"{name}: kernel {err:.3e} floor {floor:.3e}")
    assert 4 * floor <= 1e-3, (name, floor)
    assert err <= 4 * floor, (name, err, floor)


def _lstm_loop(xp, w, rpc, dh):
    """Plain LSTM (gates i, f, g, o; zero state) on xp [R, T, 4H] with client
    r // rpc's w [K, 4H, H]: h_seq and d<h_seq, dh> / d(xp, w)."""
    xp, w = xp.clone().requires_grad_(True), w.clone().requires_grad_(True)
    R, T, H4 = xp.shape
    wr = w.repeat_interleave(rpc, 0)
    h = c = xp.new_zeros(R, H4 // 4)
    hs = []
    for t in range(T):
        z = xp[:, t] + torch.bmm(wr, h.unsqueeze(2)).squeeze(2)
        i, f, g, o = z.chunk(4, dim=1)
        c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
        h = torch.sigmoid(o) * torch.tanh(c)
        hs.append(h)
    h_seq = torch.stack(hs, dim=1)
    return (h_seq,) + torch.autograd.grad(h_seq, [xp, w], dh)


@pytest.mark.gpu
@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("K,rpc,T", [(1, 1, 1), (1, 3, 7), (2, 3, 5)])
def test_lstm_seq_small_matches_float64(H, K, rpc, T):
    from msrflute_amd.ops.lstm import _LSTMSeq
    torch.manual_seed(100 * H + 10 * K + T)
    xp = torch.randn(K * rpc, T, 4 * H)
    w = torch.randn(K, 4 * H, H) / H ** 0.5
    dh = torch.randn(K * rpc, T, H)
    ref64 = _lstm_loop(xp.double(), w.double(), rpc, dh.double())
    ref32 = _lstm_loop(xp, w, rpc, dh)
    xg, wg = (t.cuda().requires_grad_(True) for t in (xp, w))
    h = _LSTMSeq.apply(xg, wg, rpc)
    got = (h,) + torch.autograd.grad(h, [xg, wg], dh.cuda())
    names = ("h_seq", "dxp", "dW_hh")
    for name, a, r32, r64 in zip(names, got, ref32, ref64):
        _check(f"H={H} K={K} rpc={rpc} T={T} {name}", a, r32, r64)


@pytest.mark.gpu
@pytest.mark.parametrize("H", SIZES)
def test_lstm_seq_small_activations_elementwise(H):
    """The kernels' own sigmoid / tanh element by element: at T = 1 the
    pre-activations are xp itself (h_0 = 0).  The g inputs walk across the
    tanh branch point 0.625; the others are 50 x randn with +-88, +-100 and
    +-1000 planted (saturation, the +-87 clamp of the exponential).
    Bound, in u = 2^-24 on values <= 1: e^x is v_exp_f32 (2 u) + correction
    and fma ~ 3.5 u, then 1 + e and the division: 5.5 u.  Asserted: 8 u."""
    from msrflute_amd.ops import _C
    torch.manual_seed(H)
    R, u = 4, 2.0 ** -24
    xp = 50 * torch.randn(R, 1, 4 * H)
    xp[:, 0, 2 * H:3 * H] = torch.linspace(-1.5, 1.5, R * H).view(R, H)
    xp[0, 0, [0, H, 3 * H, 1, H + 1, 3 * H + 1]] = torch.tensor(
        [100., -100., 1000., -1000., 88., -88.])
    i, f, g, o = xp.double()[:, 0].chunk(4, dim=1)
    ref = torch.cat([i.sigmoid(), f.sigmoid(), g.tanh(), o.sigmoid()], 1)
    w = torch.randn(1, 4 * H, H, device="cuda") / H ** 0.5
    gates = _C.lstm_seq_fwd(xp.cuda(), w, R)[1]
    err = (gates[:, 0].cpu().double() - ref).abs().max().item()
    print(f"H={H} gates {err / u:.2f} u")
    assert err <= 8 * u, err / u


@pytest.mark.gpu
@pytest.mark.parametrize("H", SIZES)
@pytest.mark.parametrize("gate", range(4))
def test_lstm_seq_small_propagates_nan(H, gate):
    """A NaN pre-activation stays visible: NaN exactly where the float64
    loop has it, every other row and every earlier step bit-unchanged."""
    from msrflute_amd.ops.lstm import _LSTMSeq
    torch.manual_seed(31 * H + gate)
    R, T = 3, 4
    xp = torch.randn(R, T, 4 * H)
    w = torch.randn(1, 4 * H, H) / H ** 0.5
    clean = _LSTMSeq.apply(xp.cuda(), w.cuda(), R).cpu()
    xp[1, 2, gate * H + 5] = float("nan")
    nan = _lstm_loop(xp.double(), w.double(), R,
                     torch.zeros(R, T, H).double())[0].isnan()
    got = _LSTMSeq.apply(xp.cuda(), w.cuda(), R).cpu()
    assert nan[1, 2, 5] and nan[1, 3].all() and nan.sum() == H + 1
    assert torch.equal(got.isnan(), nan)
    assert torch.equal(got[~nan], clean[~nan])


@pytest.mark.gpu
@pytest.mark.parametrize("H", SIZES)
def test_lstm_seq_small_stacked_matches_single_client(H):
    """K = 2 clients, different W_hh, same inputs, against two K = 1 calls:
    anything but bit equality is a row -> client indexing bug."""
    from msrflute_amd.ops.lstm import _LSTMSeq
    torch.manual_seed(17 + H)
    K, rpc, T = 2, 3, 5
    xp = torch.randn(rpc, T, 4 * H, device="cuda").repeat(K, 1, 1) \
        .requires_grad_(True)
    w = (torch.randn(K, 4 * H, H, device="cuda") / H ** 0.5) \
        .requires_grad_(True)
    dh = torch.randn(K * rpc, T, H, device="cuda")
    h = _LSTMSeq.apply(xp, w, rpc)
    dxp, = torch.autograd.grad(h, [xp], dh)
    for k in range(K):
        rows = slice(k * rpc, (k + 1) * rpc)
        xp_k = xp[rows].detach().clone().requires_grad_(True)
        h_k = _LSTMSeq.apply(xp_k, w[k:k + 1].detach(), rpc)
        dxp_k, = torch.autograd.grad(h_k, [xp_k], dh[rows])
        assert torch.equal(h[rows], h_k), k
        assert torch.equal(dxp[rows], dxp_k), k
    assert not torch.equal(h[:rpc], h[rpc:])


@pytest.mark.gpu
@pytest.mark.parametrize("H", SIZES)
def test_fused_lstm_small_module_matches_float64(H):
    from msrflute_amd.ops.lstm import FusedLSTM
    torch.manual_seed(7 + H)
    fused = FusedLSTM(5, H, num_layers=2)
    x = torch.randn(3, 7, 5)
    g = torch.randn(3, 7, H)

    def run(mod, x, g):
        x = x.clone().requires_grad_(True)
        out, _ = mod(x)
        out.backward(g)
        return [out, x.grad] + [p.grad for _, p in mod.named_parameters()]

    def twin(dtype):
        ref = torch.nn.LSTM(5, H, num_layers=2, batch_first=True)
        ref.load_state_dict(fused.state_dict())
        return run(ref.to(dtype), x.to(dtype), g.to(dtype))

    ref64, ref32 = twin(torch.float64), twin(torch.float32)
    fused.cuda()
    assert fused._use_fused(x.cuda())
    got = run(fused, x.cuda(), g.cuda())
    names = ["out", "dx"] + [n for n, _ in fused.named_parameters()]
    assert len(got) == len(ref64) == len(names)
    for name, a, r32, r64 in zip(names, got, ref32, ref64):
        _check(f"H={H} {name}", a, r32, r64)


def test_ecg_model_uses_fused_lstm_with_nn_lstm_names():
    from msrflute_amd.ops.lstm import FusedLSTM
    spec = importlib.util.spec_from_file_location(
        "ecg_cnn_model_small_lstm",
        os.path.join(REPO, "experiments", "ecg_cnn", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(5)
    net = mod.SuperNet({"hid_size": 16})
    assert isinstance(net.net.lstm, FusedLSTM)
    assert [k for k in net.state_dict() if ".lstm." in k] == [
        "net.lstm.weight_ih_l0", "net.lstm.weight_hh_l0",
        "net.lstm.bias_ih_l0", "net.lstm.bias_hh_l0"]
    ref = torch.nn.LSTM(8, 64, batch_first=True)
    ref.load_state_dict(net.net.lstm.state_dict())
    x = torch.randn(3, 12, 8)
    assert torch.allclose(net.net.lstm(x)[0], ref(x)[0])
