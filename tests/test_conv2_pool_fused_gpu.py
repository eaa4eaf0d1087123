"""The f32 conv2 forward with the maxpool + dropout epilogue
(csrc/fused_cnn.hip: k_conv2_fwd_pool_mfma_mb through
dbg_conv2_fwd_pool_mfma) against the unfused pair it replaces.

The reference is built from the r2 that dbg_conv2_fwd_mfma returns for
the same inputs: 2x2 maximum, np.argmax (first maximum = the kernel's
strict >), gate = max > 0, the keep mask of tests/philox_oracle.py under
the key (seed_k, client-local cell >> 2, offset) and
a2 = keep ? max * float32(1 / (1 - p1)) : 0.  The epilogue changes no
output's k-chain and no tie-break, so every comparison is bitwise.

Cases: K = 2 clients x 3 rows with different W2 / b2 / seed per client
(one seed with a non-zero high word) and K = 1 x 1 row, offset 3,
p1 in {0, 0.25}.  One image is all zero, so every window of it ties and
must give index 0; its client has negative biases on half the channels,
so ties occur with gate 0 and with gate 1.
"""

import functools

import numpy as np
import pytest
import torch

import philox_oracle as po

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from msrflute_amd import _C

OFFSET = 3
SEEDS = (5, (1 << 32) * 77 + 3)
ZERO_ROW = 4        # row 1 of client 1 in the K = 2 x 3 case


@functools.lru_cache(maxsize=None)
def _inputs(K, bs):
    """a1 / W2 / b2 of the case and the unfused kernel's r2, computed once"""
    g = torch.Generator(device="cuda").manual_seed(20 + K * 7 + bs)
    B = K * bs
    a1 = torch.randn(B, 32, 26, 26, device="cuda", generator=g).clamp(min=0)
    w2 = torch.randn(K, 64, 32, 3, 3, device="cuda", generator=g) * 0.1
    b2 = torch.randn(K, 64, device="cuda", generator=g) * 0.1
    if K > 1:
        a1[ZERO_ROW] = 0.0
        b2[1, :32] = -b2[1, :32].abs() - 0.01
        b2[1, 32:] = b2[1, 32:].abs() + 0.01
    flat = [t.reshape(-1).contiguous() for t in (a1, w2, b2)]
    r2 = _C.dbg_conv2_fwd_mfma(*flat, B).view(B, 64, 24, 24).cpu().numpy()
    return flat, r2


def _reference(r2, K, bs, p1):
    B = K * bs
    # [B, 64, 12, 12, 4] windows in the order (0,0), (0,1), (1,0), (1,1)
    win = r2.reshape(B, 64, 12, 2, 12, 2).transpose(0, 1, 2, 4, 3, 5)
    win = win.reshape(B, 64, 12, 12, 4)
    idx = np.argmax(win, axis=-1)
    mx = win.max(axis=-1)
    gate = mx > 0
    pidx = (idx | (gate.astype(np.int64) << 2)).astype(np.uint8)
    keep = np.concatenate([po.pool_mask(SEEDS[k], OFFSET, bs, p1)
                           for k in range(K)])
    inv_keep = np.float32(1.0 / (1.0 - p1))
    a2 = np.where(keep == 1, mx * inv_keep, np.float32(0)).astype(np.float32)
    return a2, pidx, keep, idx, gate


@pytest.mark.parametrize("p1", [0.0, 0.25])
@pytest.mark.parametrize("K,bs", [(2, 3), (1, 1)])
def test_fused_epilogue_equals_unfused_pair(K, bs, p1):
    flat, r2 = _inputs(K, bs)
    seeds = torch.tensor(SEEDS[:K], dtype=torch.int64)
    a2, pidx, m2 = _C.dbg_conv2_fwd_pool_mfma(*flat, bs, K, p1, seeds,
                                              OFFSET)
    torch.cuda.synchronize()
    shape = (K * bs, 64, 12, 12)
    a2 = a2.cpu().numpy().reshape(shape)
    pidx = pidx.cpu().numpy().reshape(shape)
    m2 = m2.cpu().numpy().reshape(shape)
    want_a2, want_pidx, want_m2, idx, gate = _reference(r2, K, bs, p1)
    assert np.array_equal(pidx, want_pidx), int((pidx != want_pidx).sum())
    assert np.array_equal(m2, want_m2), int((m2 != want_m2).sum())
    assert np.array_equal(a2, want_a2), int((a2 != want_a2).sum())
    if p1 == 0.0:
        assert m2.min() == 1
    else:
        assert 0.70 < m2.mean() < 0.80, m2.mean()
    if K > 1:
        # the all-zero image: every window ties -> index 0, gate by bias
        assert (idx[ZERO_ROW] == 0).all()
        assert not gate[ZERO_ROW, :32].any() and gate[ZERO_ROW, 32:].all()
        assert (pidx[ZERO_ROW, :32] == 0).all()
        assert (pidx[ZERO_ROW, 32:] == 4).all()
        # and the random images use every argmax value
        assert set(np.unique(pidx & 3)) == {0, 1, 2, 3}
