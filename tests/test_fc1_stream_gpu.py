"""The fc1 kernels of the flagship CNN (csrc/fused_cnn.hip) after the
streaming rewrite: sub-chunked forward GEMM, batched fold, column-remapped
backward kernels with the bias sums folded into backward-weights.

Every output element is checked against a float64 reference taken client
by client on the float32 inputs.  The bound is derived, not tuned: a
float32 chain of n additions/fmas has error at most n * 2^-24 * sum(|x| *
|y|) over the reduction (first order, any summation order), with n the
chain length plus fold terms: 9216 + 65 forward (144-k MFMA chains, 64
partials and the bias), 128 backward-data, bs backward-weight and bias.

Shapes (K clients, rows per client): one row, 17 rows (crosses the 16-row
MFMA tile), the full 32-row tile, two clients of 3 rows, and three clients
of 5 rows — an odd K, so a client base that is only 8-byte aligned in a
stacked operand is exercised.  Every client has its own weights.

Two input kinds.  ``random``: no structure a column permutation could hide
behind.  ``index``: a2 / w3 hold (column index + 9216 * row) * 2^-18, exact
in float32, and the backward kernels get a one-hot dz3 row per sample, so
every term but one is exactly zero and the outputs must equal the selected
index values bit for bit: a swapped column lands on a different exact
value.
"""

import numpy as np
import pytest
import torch

import philox_oracle as po

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C

EPS = 2.0 ** -24
SHAPES = [(1, 1), (1, 17), (1, 32), (2, 3), (3, 5)]
IDS = ["1x1", "1x17", "1x32", "2x3", "3x5"]


def _gen(seed):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    return g


def _rand(g, *shape):
    return torch.randn(*shape, device="cuda", dtype=torch.float32,
                       generator=g)


def _index(rows):
    """[rows, 9216] of (column + 9216 * row) * 2^-18: integers below 2^24
    times a power of two, so exact in float32 and all distinct"""
    assert rows * 9216 < 2 ** 24
    v = torch.arange(rows * 9216, device="cuda", dtype=torch.float64)
    return (v * 2.0 ** -18).to(torch.float32).view(rows, 9216)


def _one_hot_dz(K, bs):
    """row b of client k is 1.0 at unit (37 * b + 11 * k) % 128 (distinct
    units within a client: 37 is odd and bs <= 32 < 128)"""
    dz = torch.zeros(K, bs, 128, device="cuda", dtype=torch.float32)
    for k in range(K):
        for b in range(bs):
            dz[k, b, (37 * b + 11 * k) % 128] = 1.0
    return dz


def _check(name, out, ref, tol):
    """every element finite and within its own bound"""
    out = out.double()
    assert torch.isfinite(out).all(), name
    excess = (out - ref).abs() - tol
    worst = excess.max().item()
    print(f"{name}: max |err| {(out - ref).abs().max().item():.3e}, "
          f"min slack {-worst:.3e}")
    assert worst <= 0.0, (name, worst)


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def shape(request):
    return request.param


@pytest.mark.parametrize("kind", ["random", "index"])
def test_fc1_fwd(shape, kind):
    K, bs = shape
    B = K * bs
    g = _gen(100 + B)
    if kind == "random":
        a2 = _rand(g, K, bs, 9216)
        w3 = _rand(g, K, 128, 9216) * 0.02
    else:
        a2 = _index(B).view(K, bs, 9216)
        w3 = _index(K * 128).view(K, 128, 9216) * 2.0 ** -10
    b3 = _rand(g, K, 128)
    a64, w64, b64 = a2.double(), w3.double(), b3.double()
    ref = torch.einsum("kbn,kjn->kbj", a64, w64) + b64[:, None, :]
    mag = torch.einsum("kbn,kjn->kbj", a64.abs(), w64.abs()) \
        + b64.abs()[:, None, :]
    z3, a3, m3 = _C.dbg_fc1_fwd_mfma(a2.reshape(-1).contiguous(),
                                     w3.reshape(-1).contiguous(),
                                     b3.reshape(-1).contiguous(),
                                     B, 0.0, 123, 0)
    _check("z3", z3.view(K, bs, 128), ref, (9216 + 65) * EPS * mag)
    assert torch.equal(a3, z3.clamp(min=0))
    assert int(m3.min()) == 1


@pytest.mark.parametrize("kind", ["random", "index"])
def test_fc1_bwd_x(shape, kind):
    K, bs = shape
    B = K * bs
    g = _gen(200 + B)
    if kind == "random":
        dz3 = _rand(g, K, bs, 128)
        w3 = _rand(g, K, 128, 9216)
    else:
        dz3 = _one_hot_dz(K, bs)
        w3 = _index(K * 128).view(K, 128, 9216)
    d64, w64 = dz3.double(), w3.double()
    ref = torch.einsum("kbj,kjn->kbn", d64, w64)
    mag = torch.einsum("kbj,kjn->kbn", d64.abs(), w64.abs())
    da2 = _C.dbg_fc1_bwd_x_mfma(dz3.reshape(-1).contiguous(),
                                w3.reshape(-1).contiguous(), B)
    da2 = da2.view(K, bs, 9216)
    _check("da2", da2, ref, 128 * EPS * mag)
    if kind == "index":
        assert torch.equal(da2.double(), ref)


@pytest.mark.parametrize("kind", ["random", "index"])
def test_fc1_bwd_w_and_bias(shape, kind):
    K, bs = shape
    B = K * bs
    g = _gen(300 + B)
    if kind == "random":
        dz3 = _rand(g, K, bs, 128)
        a2 = _rand(g, K, bs, 9216)
    else:
        dz3 = _one_hot_dz(K, bs)
        a2 = _index(B).view(K, bs, 9216)
    d64, a64 = dz3.double(), a2.double()
    ref_w = torch.einsum("kbj,kbn->kjn", d64, a64)
    mag_w = torch.einsum("kbj,kbn->kjn", d64.abs(), a64.abs())
    ref_b, mag_b = d64.sum(1), d64.abs().sum(1)
    dw3, db3 = _C.dbg_fc1_bwd_w_mfma(dz3.reshape(-1).contiguous(),
                                     a2.reshape(-1).contiguous(), B, K)
    dw3, db3 = dw3.view(K, 128, 9216), db3.view(K, 128)
    _check("dw3", dw3, ref_w, bs * EPS * mag_w)
    _check("db3", db3, ref_b, bs * EPS * mag_b)
    if kind == "index":
        assert torch.equal(dw3.double(), ref_w)
        assert torch.equal(db3.double(), ref_b)


def _shifted(t, shift):
    """flat copy of t whose first element sits `shift` floats past a
    512-byte-aligned allocation: 2 -> an 8-byte-aligned base (what odd
    clients of a parameter stack with P % 4 == 2 have), 1 -> 4-byte"""
    buf = torch.empty(t.numel() + shift, device="cuda", dtype=torch.float32)
    view = buf[shift:]
    view.copy_(t.reshape(-1))
    assert view.data_ptr() % 16 == (4 * shift) % 16
    return view


@pytest.mark.parametrize("shift", [2, 1], ids=["8B", "4B"])
def test_fc1_bases_not_16_byte_aligned(shift):
    """the kernels pick their global access width from the addresses; the
    stacked debug operands are 16-byte aligned, so the narrower paths are
    driven with shifted views (K = 3 clients of 5 rows)"""
    K, bs = 3, 5
    B = K * bs
    g = _gen(500 + shift)
    a2 = _rand(g, K, bs, 9216)
    w3 = _rand(g, K, 128, 9216) * 0.02
    b3 = _rand(g, K, 128)
    dz3 = _rand(g, K, bs, 128)
    a64, w64, b64, d64 = a2.double(), w3.double(), b3.double(), dz3.double()
    a2s, w3s = _shifted(a2, shift), _shifted(w3, shift)

    z3, _, _ = _C.dbg_fc1_fwd_mfma(a2.reshape(-1), w3s, b3.reshape(-1),
                                   B, 0.0, 123, 0)
    ref = torch.einsum("kbn,kjn->kbj", a64, w64) + b64[:, None, :]
    mag = torch.einsum("kbn,kjn->kbj", a64.abs(), w64.abs()) \
        + b64.abs()[:, None, :]
    _check("z3", z3.view(K, bs, 128), ref, (9216 + 65) * EPS * mag)
    # same chains whatever the access width
    z3a, _, _ = _C.dbg_fc1_fwd_mfma(a2.reshape(-1), w3.reshape(-1),
                                    b3.reshape(-1), B, 0.0, 123, 0)
    assert torch.equal(z3, z3a)

    da2 = _C.dbg_fc1_bwd_x_mfma(dz3.reshape(-1), w3s, B)
    _check("da2", da2.view(K, bs, 9216),
           torch.einsum("kbj,kjn->kbn", d64, w64),
           128 * EPS * torch.einsum("kbj,kjn->kbn", d64.abs(), w64.abs()))
    assert torch.equal(da2, _C.dbg_fc1_bwd_x_mfma(dz3.reshape(-1),
                                                  w3.reshape(-1), B))

    dw3, db3 = _C.dbg_fc1_bwd_w_mfma(dz3.reshape(-1), a2s, B, K)
    _check("dw3", dw3.view(K, 128, 9216),
           torch.einsum("kbj,kbn->kjn", d64, a64),
           bs * EPS * torch.einsum("kbj,kbn->kjn", d64.abs(), a64.abs()))
    _check("db3", db3.view(K, 128), d64.sum(1), bs * EPS * d64.abs().sum(1))
    dw3a, _ = _C.dbg_fc1_bwd_w_mfma(dz3.reshape(-1), a2.reshape(-1), B, K)
    assert torch.equal(dw3, dw3a)


@pytest.mark.parametrize("seed,offset", [(99, 1), (2 ** 40 + 12345, 7)])
def test_fc1_fwd_dropout_mask_matches_oracle(seed, offset):
    K, bs = 2, 5
    B = K * bs
    g = _gen(400)
    a2 = _rand(g, B, 9216)
    w3, b3 = _rand(g, K, 128, 9216) * 0.02, _rand(g, K, 128)
    z3, a3, m3 = _C.dbg_fc1_fwd_mfma(a2.reshape(-1).contiguous(),
                                     w3.reshape(-1).contiguous(),
                                     b3.reshape(-1).contiguous(),
                                     B, 0.5, seed, offset)
    # the debug entry gives every client the same seed; the Philox index
    # is client-local, so each client's mask is the oracle's for bs rows
    want = torch.from_numpy(
        np.ascontiguousarray(po.fc1_mask(seed, offset, bs, 0.5))).cuda()
    m3 = m3.view(K, bs, 128)
    for k in range(K):
        assert torch.equal(m3[k], want), k
    keep = m3.bool().view(B, 128)
    z3, a3 = z3.view(B, 128), a3.view(B, 128)
    assert torch.equal(a3[keep], z3.clamp(min=0)[keep] / 0.5)
    assert (a3[~keep] == 0).all()
