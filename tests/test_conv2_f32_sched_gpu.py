"""Tile loop of the f32 conv2 backward-weights MFMA kernel
(csrc/fused_cnn.hip: k_conv2_bwd_w_mfma_mb) through its dbg_* entry.

The kernel walks its tiles with blocks blockIdx.x, blockIdx.x + gridDim.x,
.., the next tile's first chunk fetched during the current tile's last
MFMAs, and the launcher sizes the grid from the device's occupancy.
`max_blocks` caps that grid, so the same input can be run by one block
that walks every tile, by two that hand over between tiles, and by a grid
whose last stride is ragged: the result may not depend on it, bit for bit.
Against torch the tolerance is that of test_conv2_f32_tiles_gpu.py.
Every case is at most 15 images.
"""

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C

DW_TOL = dict(rtol=1e-3, atol=1e-3)
W_TILES = 9   # backward-weight tiles per image: 288 columns / 32


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _rand(gen, *shape):
    return torch.randn(*shape, device="cuda", dtype=torch.float32,
                       generator=gen)


def _flat(t):
    return t.reshape(-1).contiguous()


def _bwd_w(dz2, a1, K, max_blocks=0):
    dw2, db2 = _C.dbg_conv2_bwd_w_mfma(_flat(dz2), _flat(a1), a1.shape[0], K,
                                       max_blocks)
    return dw2.view(K, 64, 288), db2.view(K, 64)


def _ref_bwd_w(a1, dz2):
    w = torch.zeros(64, 32, 3, 3, device="cuda", requires_grad=True)
    F.conv2d(a1, w).backward(dz2)
    return w.grad.view(64, 288)


@pytest.fixture(scope="module")
def stack():
    """K = 3 clients x 5 rows: 15 images, 135 tiles: more than 8, so the
    XCD deal permutes them, and a multiple of no capped grid used below"""
    g = _gen(20)
    K, bs = 3, 5
    return dict(K=K, bs=bs,
                a1=_rand(g, K * bs, 32, 26, 26),
                dz2=_rand(g, K * bs, 64, 24, 24))


@pytest.fixture(scope="module")
def stack_default(stack):
    """the result at the default grid, computed once"""
    return dict(dw=_bwd_w(stack["dz2"], stack["a1"], stack["K"]))


@pytest.mark.parametrize("max_blocks", [1, 2, 7])
def test_grid_independence_bwd_w(stack, stack_default, max_blocks):
    dw2, db2 = _bwd_w(stack["dz2"], stack["a1"], stack["K"], max_blocks)
    assert torch.equal(dw2, stack_default["dw"][0])
    assert torch.equal(db2, stack_default["dw"][1])


@pytest.fixture(scope="module")
def one_image():
    g = _gen(21)
    a1 = _rand(g, 1, 32, 26, 26)
    dz2 = _rand(g, 1, 64, 24, 24)
    return dict(a1=a1, dz2=dz2, ref_w=_ref_bwd_w(a1, dz2))


@pytest.mark.parametrize("max_blocks", [0, W_TILES - 1])
def test_one_image_bwd_w(one_image, max_blocks):
    """B = 1: the default grid is one block per tile; one block fewer makes
    exactly one block take a second tile"""
    dw2, db2 = _bwd_w(one_image["dz2"], one_image["a1"], 1, max_blocks)
    ref = one_image["ref_w"]
    assert torch.allclose(dw2[0], ref, **DW_TOL), \
        (dw2[0] - ref).abs().max().item()
    assert torch.allclose(db2[0], one_image["dz2"].sum(dim=(0, 2, 3)),
                          **DW_TOL)


# ci planes that straddle an edge between two 32-column tiles of dW2
# (column n = 9 ci + 3 kh + kw): 32 nb / 9 for the nb with 32 nb % 9 != 0
STRADDLING = sorted({32 * nb // 9 for nb in range(1, 9) if 32 * nb % 9})


@pytest.mark.parametrize("ci", STRADDLING)
def test_bwd_w_column_seams(one_image, ci):
    a1 = torch.zeros(1, 32, 26, 26, device="cuda")
    a1[0, ci] = one_image["a1"][0, ci]
    ref = _ref_bwd_w(a1, one_image["dz2"])
    dw2, _ = _bwd_w(one_image["dz2"], a1, 1, 4)
    assert torch.allclose(dw2[0], ref, **DW_TOL), \
        (dw2[0] - ref).abs().max().item()
    cols = slice(9 * ci, 9 * ci + 9)
    assert ref[:, cols].abs().max().item() > 0
    other = torch.ones(288, dtype=torch.bool, device="cuda")
    other[cols] = False
    assert (dw2[0][:, other] == 0).all()


def test_stack_invariance_capped(stack):
    K, bs = stack["K"], stack["bs"]
    dz2, a1 = stack["dz2"], stack["a1"]
    dw2, db2 = _bwd_w(dz2, a1, K, 4)
    for k in range(K):
        rows = slice(k * bs, (k + 1) * bs)
        dw1, db1 = _bwd_w(dz2[rows], a1[rows], 1, 4)
        assert torch.equal(dw2[k], dw1[0]), k
        assert torch.equal(db2[k], db1[0]), k


def test_run_to_run_determinism_capped(stack):
    dz2, a1, K = stack["dz2"], stack["a1"], stack["K"]
    first, second = _bwd_w(dz2, a1, K, 11), _bwd_w(dz2, a1, K, 11)
    assert torch.equal(first[0], second[0])
    assert torch.equal(first[1], second[1])
