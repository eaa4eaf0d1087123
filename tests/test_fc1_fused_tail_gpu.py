"""The fused fc1 tail of the FedAvg mega round (csrc/fused_cnn.hip,
k_fc1_tail_sumsq_mb + k_fc1_tail_clip_sgd_mb): the gradient norm and the
clip + SGD update with dW3 re-formed in registers from dz3 and a2 instead of
stored and read back.

Oracle: the stored path, not the code under test.  ``dbg_fc1_bwd_w_mfma``
gives dW3 and db3, they are placed in a [K, P] gradient stack whose other
segments are seeded random, and ``mega_clip_sgd`` runs on a copy of the
parameters.  The new path (``dbg_fc1_fused_tail``) runs on another copy with
the W3 segment of its gradient stack filled with NaN, so any read of that
segment shows in the norm and in the weights.

Asserted: parameters bit-equal; the clipped stats within 2^-22 relative (two
float ulps: f64 sums of another grouping, cast to float); the f64 sums
within 1e-12 relative; the W3 rows of a client whose dz3 is all zero
bit-unchanged; and the parameters against a float64 closed form, client by
client, within a derived bound (below).

Shapes (K clients, rows per client) at C = 62: one row, 17 rows (crosses
the 16-row MFMA tile), the workload's 20, two clients of 3 and three of 5
rows (odd clients of the stack sit at 8-byte-aligned bases: P % 4 == 2).
(2, 3) at C = 61: P is odd, client 1's base is 4-byte aligned, the dword
path.  ``max_norm``: a power of two below the norm (clips), 2^40 (scale 1)
and 0 (clipping off).  Input kinds: ``random``, and ``index`` of
test_fc1_stream_gpu.py (one-hot dz3 rows, exact index values in a2, zero
weights): with lr a power of two and scale 1 every W3 weight is an exact,
distinct multiple of its column's index value, so a swapped column lands on
another weight.  The random kind runs at lr = 0.1: lr * g is inexact there,
so bit-equality also pins the update to the stored path's one fma.

The float64 bound, first order.  A dW3 element is a float chain of bs fmas:
|g - g64| <= tg = bs * 2^-24 * sum_b |dz3| |a2|; every other gradient
element is an input (tg = 0).  The norm moves by at most ||tg||_2 plus its
cast to float, so the scale max_norm / (norm + eps) has relative error at
most rs = ||tg||_2 / norm + 4 * 2^-24 (cast, add, divide, and the eps that
the closed form also adds).  The update rounds g * scale once and the fma
once: |w - w64| <= lr * scale * tg + lr * scale * |g64| * (rs + 2^-24)
+ 2^-24 * |w64|.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C

EPS = 2.0 ** -24
# random: a learning rate whose products are inexact, so that an update
# compiled as multiply + subtract instead of one fma shows; index: a power
# of two, exact weights.  Both as the float the kernels read.
LRS = {"random": float(torch.tensor(0.1, dtype=torch.float32)),
       "index": 2.0 ** -6}
OW3 = 18816            # conv1 + conv2 parameters come first
W3N = 128 * 9216
SHAPES = [(1, 1, 62), (1, 17, 62), (1, 20, 62), (2, 3, 62), (3, 5, 62),
          (2, 3, 61)]
IDS = ["1x1", "1x17", "1x20", "2x3", "3x5", "2x3-C61"]
MODES = ["clip", "above", "off"]


def _P(C):
    return OW3 + W3N + 128 + 129 * C


def _index(rows):
    assert rows * 9216 < 2 ** 24
    v = torch.arange(rows * 9216, device="cuda", dtype=torch.float64)
    return (v * 2.0 ** -18).to(torch.float32).view(rows, 9216)


def _one_hot_dz(K, bs):
    dz = torch.zeros(K, bs, 128, device="cuda", dtype=torch.float32)
    for k in range(K):
        for b in range(bs):
            dz[k, b, (37 * b + 11 * k) % 128] = 1.0
    return dz


_BASE = {}


def _base(K, bs, C, kind, idle=None):
    """inputs and the stored gradient stack of one case, built once"""
    key = (K, bs, C, kind, idle)
    if key in _BASE:
        return _BASE[key]
    P = _P(C)
    g = torch.Generator(device="cuda")
    g.manual_seed(900 + 31 * K + bs + C)

    def rand(*shape):
        return torch.randn(*shape, device="cuda", dtype=torch.float32,
                           generator=g)

    if kind == "random":
        dz3, a2 = rand(K, bs, 128), rand(K, bs, 9216)
        params = rand(K, P) * 0.05
    else:
        dz3, a2 = _one_hot_dz(K, bs), _index(K * bs).view(K, bs, 9216)
        params = torch.zeros(K, P, device="cuda", dtype=torch.float32)
    if idle is not None:
        dz3[idle] = 0.0
    grads = rand(K, P)
    dw3, db3 = _C.dbg_fc1_bwd_w_mfma(dz3.reshape(-1), a2.reshape(-1), K * bs,
                                     K)
    grads[:, OW3:OW3 + W3N] = dw3.view(K, W3N)
    grads[:, OW3 + W3N:OW3 + W3N + 128] = db3.view(K, 128)
    norm = grads.double().pow(2).sum(1).sqrt()          # [K]
    _BASE[key] = (dz3, a2, params, grads, norm)
    return _BASE[key]


def _max_norm(mode, norm):
    if mode == "off":
        return 0.0
    if mode == "above":
        return 2.0 ** 40
    # the power of two at least a factor 2 below every client's norm
    return 2.0 ** (math.floor(math.log2(norm.min().item())) - 1)


def _run_pair(K, bs, C, kind, mode, idle=None):
    dz3, a2, params, grads, norm = _base(K, bs, C, kind, idle)
    max_norm = _max_norm(mode, norm)
    lr_t = torch.full((1,), LRS[kind], device="cuda", dtype=torch.float32)
    out = {}
    for path in ("stored", "fused"):
        p = params.clone().view(-1)
        gr = grads.clone()
        acc = torch.full((2 * K,), 7.0, device="cuda", dtype=torch.float64)
        stats = torch.zeros(2 * K, device="cuda", dtype=torch.float32)
        if path == "stored":
            _C.mega_clip_sgd(p, gr.view(-1), K, acc, max_norm, lr_t, stats)
        else:
            gr[:, OW3:OW3 + W3N] = float("nan")
            _C.dbg_fc1_fused_tail(p, gr.view(-1), dz3.reshape(-1),
                                  a2.reshape(-1), K * bs, K, C, acc,
                                  max_norm, lr_t, stats)
        out[path] = (p.view(K, -1), acc, stats)
    return out, max_norm


def _rel(a, b):
    return ((a - b).abs() / b.abs()).max().item()


@pytest.mark.parametrize("kind", ["random", "index"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_tail_matches_stored_path(shape, mode, kind):
    K, bs, C = shape
    out, max_norm = _run_pair(K, bs, C, kind, mode)
    (p_s, acc_s, st_s), (p_f, acc_f, st_f) = out["stored"], out["fused"]
    assert torch.isfinite(acc_f).all() and torch.isfinite(p_f).all()
    r_acc, r_st = _rel(acc_f, acc_s), _rel(st_f.double(), st_s.double())
    print(f"max_norm {max_norm:g}: acc rel {r_acc:.3e}, stats rel "
          f"{r_st:.3e}, params differing "
          f"{(p_f != p_s).sum().item()}")
    assert r_acc <= 1e-12
    assert r_st <= 2.0 ** -22
    assert torch.equal(p_f, p_s)
    if mode == "clip":
        # it did clip: the weights are not those of scale = 1
        _, _, _, grads, norm = _base(K, bs, C, kind)
        assert (norm > max_norm).all()


def test_idle_client_w3_unchanged():
    """client 1 of 3 has an all-zero dz3 (its epoch is over): its W3 rows
    keep their bits, the others move as on the stored path"""
    K, bs, C = 3, 5, 62
    out, _ = _run_pair(K, bs, C, "random", "clip", idle=1)
    params = _base(K, bs, C, "random", 1)[2]
    p_s, p_f = out["stored"][0], out["fused"][0]
    assert torch.equal(p_f, p_s)
    assert torch.equal(p_f[1, OW3:OW3 + W3N], params[1, OW3:OW3 + W3N])
    assert not torch.equal(p_f[0, OW3:OW3 + W3N], params[0, OW3:OW3 + W3N])


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_fused_tail_against_float64(shape, mode):
    K, bs, C = shape
    dz3, a2, params, grads, _ = _base(K, bs, C, "random")
    out, max_norm = _run_pair(K, bs, C, "random", mode)
    p_f = out["fused"][0]
    worst = -float("inf")
    for k in range(K):
        d64, a64 = dz3[k].double(), a2[k].double()
        g64 = grads[k].double()
        g64[OW3:OW3 + W3N] = (d64.t() @ a64).view(-1)
        tg = torch.zeros_like(g64)
        tg[OW3:OW3 + W3N] = bs * EPS * (d64.abs().t() @ a64.abs()).view(-1)
        norm = g64.pow(2).sum().sqrt().item()
        clips = max_norm > 0.0 and norm > max_norm
        scale = max_norm / (norm + 1e-6) if clips else 1.0
        rs = (tg.norm().item() / norm + 4 * EPS) if clips else 0.0
        lr = LRS["random"]
        w64 = params[k].double() - lr * scale * g64
        tol = (lr * scale * tg + lr * scale * g64.abs() * (rs + EPS)
               + EPS * w64.abs())
        excess = ((p_f[k].double() - w64).abs() - tol).max().item()
        worst = max(worst, excess)
    print(f"min slack {-worst:.3e}")
    assert worst <= 0.0
