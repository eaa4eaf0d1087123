"""Tile edges of the register-blocked f32 conv2 MFMA kernels
(csrc/fused_cnn.hip: k_conv2_fwd_mfma_mb, k_conv2_bwd_x_mfma_mb,
k_conv2_bwd_w_mfma_mb) through their dbg_* entries.

The kernels stage raw a1 / dz2 rows (a slab of output rows for the
forward, a zero-padded band for backward-data, row chunks for
backward-weight) and form the im2col address in the k-loop, so what can
go wrong sits at the seams: the halo, the first and last channel chunk,
the last partial position tile, the n-column -> ci plane map and the
row -> client map of the stack.  Tolerances against torch are the ones
tests/test_mfma_gpu.py uses; the stack and determinism checks are
bitwise.  Every case is at most 15 images.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C

FWD_X_TOL = dict(rtol=1e-4, atol=5e-4)
DW_TOL = dict(rtol=1e-3, atol=1e-3)


def _rand(gen, *shape):
    return torch.randn(*shape, device="cuda", dtype=torch.float32,
                       generator=gen)


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _flat(t):
    return t.reshape(-1).contiguous()


def _fwd(a1, w2, b2):
    B = a1.shape[0]
    return _C.dbg_conv2_fwd_mfma(_flat(a1), _flat(w2), _flat(b2),
                                 B).view(B, 64, 24, 24)


def _bwd_x(dz2, w2, a1):
    B = a1.shape[0]
    return _C.dbg_conv2_bwd_x_mfma(_flat(dz2), _flat(w2), _flat(a1),
                                   B).view(B, 32, 26, 26)


def _bwd_w(dz2, a1, K):
    dw2, db2 = _C.dbg_conv2_bwd_w_mfma(_flat(dz2), _flat(a1), a1.shape[0], K)
    return dw2.view(K, 64, 288), db2.view(K, 64)


def _ref_bwd_x(a1, w2, dz2):
    x = a1.clamp(min=0).detach().requires_grad_(True)
    F.conv2d(x, w2).backward(dz2)
    return x.grad * (a1 > 0)


def _ref_bwd_w(a1, dz2):
    w = torch.zeros(64, 32, 3, 3, device="cuda", requires_grad=True)
    F.conv2d(a1, w).backward(dz2)
    return w.grad.view(64, 288)


@pytest.fixture(scope="module")
def stack():
    """K = 3 clients x 5 rows: 15 images, odd, no multiple of any tile"""
    g = _gen(10)
    K, bs = 3, 5
    return dict(K=K, bs=bs,
                a1=_rand(g, K * bs, 32, 26, 26),
                w2=_rand(g, K, 64, 32, 3, 3), b2=_rand(g, K, 64),
                dz2=_rand(g, K * bs, 64, 24, 24))


def _rows(t, k, bs):
    return t[k * bs:(k + 1) * bs]


def test_stack_invariance_fwd(stack):
    K, bs = stack["K"], stack["bs"]
    a1 = stack["a1"].abs()
    out = _fwd(a1, stack["w2"], stack["b2"])
    for k in range(K):
        one = _fwd(_rows(a1, k, bs), stack["w2"][k:k + 1],
                   stack["b2"][k:k + 1])
        assert torch.equal(_rows(out, k, bs), one), k


def test_stack_invariance_bwd_x(stack):
    K, bs = stack["K"], stack["bs"]
    out = _bwd_x(stack["dz2"], stack["w2"], stack["a1"])
    for k in range(K):
        one = _bwd_x(_rows(stack["dz2"], k, bs), stack["w2"][k:k + 1],
                     _rows(stack["a1"], k, bs))
        assert torch.equal(_rows(out, k, bs), one), k


def test_stack_invariance_bwd_w(stack):
    K, bs = stack["K"], stack["bs"]
    a1 = stack["a1"].abs()
    dw2, db2 = _bwd_w(stack["dz2"], a1, K)
    for k in range(K):
        dw1, db1 = _bwd_w(_rows(stack["dz2"], k, bs), _rows(a1, k, bs), 1)
        assert torch.equal(dw2[k], dw1[0]), k
        assert torch.equal(db2[k], db1[0]), k


def test_run_to_run_determinism(stack):
    K = stack["K"]
    a1 = stack["a1"]
    assert torch.equal(_fwd(a1.abs(), stack["w2"], stack["b2"]),
                       _fwd(a1.abs(), stack["w2"], stack["b2"]))
    assert torch.equal(_bwd_x(stack["dz2"], stack["w2"], a1),
                       _bwd_x(stack["dz2"], stack["w2"], a1))
    first, second = _bwd_w(stack["dz2"], a1, K), _bwd_w(stack["dz2"], a1, K)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])


def test_bwd_x_borders():
    """single ones at the corners and one mid-edge position of dz2, in
    the first and last co: the halo, the zero rows above and below the
    image, both ends of the co range and output positions 672..675 (the
    last, partial tile of 676)"""
    g = _gen(11)
    a1 = _rand(g, 1, 32, 26, 26).abs() + 0.1  # mask passes everything
    w2 = _rand(g, 1, 64, 32, 3, 3)
    dz2 = torch.zeros(1, 64, 24, 24, device="cuda")
    for co in (0, 63):
        for y, x in ((0, 0), (0, 23), (23, 0), (23, 23), (12, 23)):
            dz2[0, co, y, x] = 1.0
    ref = _ref_bwd_x(a1, w2[0], dz2)
    out = _bwd_x(dz2, w2, a1)
    assert torch.allclose(out, ref, **FWD_X_TOL), \
        (out - ref).abs().max().item()
    last = out.reshape(1, 32, 676)[:, :, 672:]
    assert torch.allclose(last, ref.reshape(1, 32, 676)[:, :, 672:],
                          **FWD_X_TOL)
    assert last.abs().max().item() > 0  # the (23,23) one reaches them


@pytest.fixture(scope="module")
def corner_a1():
    """a1 zero except the last input element of the last channel and the
    first of the first"""
    a1 = torch.zeros(1, 32, 26, 26, device="cuda")
    a1[0, 31, 25, 25] = 1.5
    a1[0, 0, 0, 0] = -2.0
    return a1


def test_fwd_edges(corner_a1):
    g = _gen(12)
    w2, b2 = _rand(g, 1, 64, 32, 3, 3), _rand(g, 1, 64)
    ref = F.relu(F.conv2d(corner_a1, w2[0], b2[0]))
    out = _fwd(corner_a1, w2, b2)
    assert torch.allclose(out, ref, **FWD_X_TOL), \
        (out - ref).abs().max().item()
    # the two outputs the two non-zero inputs reach, before the bias
    for co in (0, 63):
        for (y, x), v in (((23, 23), 1.5 * w2[0, co, 31, 2, 2]),
                          ((0, 0), -2.0 * w2[0, co, 0, 0, 0])):
            want = torch.relu(v + b2[0, co])
            assert torch.allclose(out[0, co, y, x], want, **FWD_X_TOL)


def test_bwd_w_edges(corner_a1):
    g = _gen(13)
    dz2 = _rand(g, 1, 64, 24, 24)
    ref = _ref_bwd_w(corner_a1, dz2)
    dw2, db2 = _bwd_w(dz2, corner_a1, 1)
    assert torch.allclose(dw2[0], ref, **DW_TOL), \
        (dw2[0] - ref).abs().max().item()
    assert torch.allclose(db2[0], dz2.sum(dim=(0, 2, 3)), **DW_TOL)
    # n = 0 is (ci 0, kh 0, kw 0), n = 287 is (ci 31, kh 2, kw 2): each
    # sees exactly one non-zero input
    for co in (0, 63):
        assert torch.allclose(dw2[0, co, 0], -2.0 * dz2[0, co, 0, 0],
                              **DW_TOL)
        assert torch.allclose(dw2[0, co, 287], 1.5 * dz2[0, co, 23, 23],
                              **DW_TOL)
        assert torch.allclose(dw2[0, co, [0, 287]], ref[co, [0, 287]],
                              **DW_TOL)


def test_fwd_slab_seams():
    g = _gen(14)
    a1 = _rand(g, 2, 32, 26, 26).abs()
    w2, b2 = _rand(g, 1, 64, 32, 3, 3), _rand(g, 1, 64)
    ref = F.relu(F.conv2d(a1, w2[0], b2[0]))
    out = _fwd(a1, w2, b2)  # K = 1, bs = 2
    assert torch.allclose(out, ref, **FWD_X_TOL), \
        (out - ref).abs().max().item()
    rows = int(_C.CONV2_FWD_SLAB_ROWS)
    seams = list(range(rows, 24, rows))
    assert seams, "the forward tiling has no slab boundary to check"
    for r in seams:
        for y in (r - 1, r):  # last row of one slab, first of the next
            assert torch.allclose(out[:, :, y], ref[:, :, y], **FWD_X_TOL), \
                (y, (out[:, :, y] - ref[:, :, y]).abs().max().item())
