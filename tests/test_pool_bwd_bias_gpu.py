"""The pool / dropout backward that also sums the conv2 bias gradient
(csrc/fused_cnn.hip: k_pool_drop_bwd_bias_mb through
dbg_pool_drop_bwd_bias).

* dz2 must equal a numpy scatter exactly: element d of a cell's 2x2
  window is the cell's gradient gg iff pidx == d | 4 (argmax d with the
  ReLU gate bit set), else 0; gg = m2 ? da2 * float32(1 / (1 - p1)) : 0
  under dropout and da2 at p1 = 0.
* db2 must equal, bit for bit, a float32 emulation of the kernel's
  summation chain per (client, channel): thread t of 256 adds elements
  t, t + 256, .. of the client's bs * 576 in that order, every wave runs
  the 32, 16, .., 1 shuffle-down tree, and the four wave sums are added
  in wave order.  (Padding the ragged last stride with +0 changes no
  partial: a partial starts at +0 and is never -0.)

Shapes: (K, bs) = (2, 3) (1728 elements per channel, a ragged last
stride), (1, 1) and (1, 20) (the benchmark's 45 full strides).  pidx is
random over 0..7, so cells with gate 0 occur, and m2 is random 0 / 1.
"""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C


def _scatter(da2, pidx, m2, p1):
    if p1 > 0:
        inv_keep = np.float32(1.0 / (1.0 - p1))
        gg = np.where(m2 == 1, da2 * inv_keep, np.float32(0))
    else:
        gg = da2
    gg = gg.astype(np.float32)
    B = da2.shape[0]
    dz2 = np.zeros((B, 64, 24, 24), dtype=np.float32)
    for d in range(4):
        dz2[:, :, (d >> 1)::2, (d & 1)::2] = np.where(
            pidx == (d | 4), gg, np.float32(0))
    return dz2


def _bias_chain(dz2, K, bs):
    """float32 emulation of the block sum, all K * 64 blocks at once"""
    n = bs * 576
    v = dz2.reshape(K, bs, 64, 576).transpose(0, 2, 1, 3).reshape(K * 64, n)
    strides = (n + 255) // 256
    pad = np.zeros((K * 64, strides * 256), dtype=np.float32)
    pad[:, :n] = v
    pad = pad.reshape(K * 64, strides, 256)
    s = np.zeros((K * 64, 256), dtype=np.float32)
    for j in range(strides):
        s = s + pad[:, j]
    s = s.reshape(K * 64, 4, 64)
    d = 32
    while d > 0:
        s[:, :, :d] = s[:, :, :d] + s[:, :, d:2 * d]
        d >>= 1
    tt = np.zeros(K * 64, dtype=np.float32)
    for w in range(4):
        tt = tt + s[:, w, 0]
    assert tt.dtype == np.float32
    return tt


@pytest.mark.parametrize("p1", [0.25, 0.0])
@pytest.mark.parametrize("K,bs", [(2, 3), (1, 1), (1, 20)])
def test_dz2_and_bias_chain_exact(K, bs, p1):
    B = K * bs
    g = torch.Generator().manual_seed(100 * K + bs)
    da2 = torch.randn(B, 64, 12, 12, generator=g)
    pidx = torch.randint(0, 8, (B, 64, 12, 12), generator=g,
                         dtype=torch.uint8)
    m2 = torch.randint(0, 2, (B, 64, 12, 12), generator=g, dtype=torch.uint8)
    dz2, db2 = _C.dbg_pool_drop_bwd_bias(
        da2.reshape(-1).cuda(), pidx.reshape(-1).cuda(),
        m2.reshape(-1).cuda(), bs, K, p1)
    torch.cuda.synchronize()
    dz2 = dz2.cpu().numpy().reshape(B, 64, 24, 24)
    db2 = db2.cpu().numpy()
    want = _scatter(da2.numpy(), pidx.numpy(), m2.numpy(), p1)
    # the cases hold what they are meant to: dropped cells, closed gates
    assert (m2 == 0).any() and (pidx < 4).any() and (pidx >= 4).any()
    assert np.array_equal(dz2, want), int((dz2 != want).sum())
    want_b = _bias_chain(want, K, bs)
    print("db2 max |kernel - chain|", np.abs(db2 - want_b).max(),
          "max |chain - fp64 sum|",
          np.abs(want_b - want.reshape(K, bs, 64, 576).astype(np.float64)
                 .sum(axis=(1, 3)).reshape(-1)).max())
    assert np.array_equal(db2, want_b), np.abs(db2 - want_b).max()
