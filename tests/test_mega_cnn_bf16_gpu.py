"""The two CNN drivers on the bf16 path against each other at K > 1:
``MegaRound(use_bf16=True)`` trains the three clients of
tests/test_mega_cnn_reference_gpu.py (bs = 4, counts (9, 4, 1): steps
3 / 1 / 1, ragged last batches, two clients idle from step 1) in one round,
and ``FusedCNNEpoch(use_bf16=True)`` trains each of them alone on its shard
rows with the same order and seed.  Both run the same ``_mb`` / ``_mb_bf16``
kernels on the same inputs, so slot k of ``params_stack`` is held to the
epoch's arena at the bound the two fp32 drivers are held to
(tests/test_mega_round_gpu.py, tests/test_cnn_epoch_prox_gpu.py): relative
1e-5 in the 2-norm; loss and the two clip stats at relative 1e-4, the loss
tolerance of tests/test_fused_cnn_gpu.py.

The max_norms are those of ``_case`` (fp64 norms x 0.25 / x 4), which leaves
room for bf16's few-percent change of the norms; that the regime held under
bf16 is confirmed from each client's reported sum of squares.  The masks the
round leaves in ``work_b`` are keyed like the fp32 driver's and are compared
with the same oracle calls as in tests/test_mega_cnn_reference_gpu.py.
"""

import functools

import numpy as np
import pytest
import torch

import cnn_ref64 as ref
import philox_oracle as po
from test_mega_cnn_reference_gpu import (ACCUM_SCALE, BS, CLIENT_IDS, COUNTS,
                                         P1, P2, SEED_MASK, SEEDS, _arena,
                                         _case, _mega, _orders, _store)

pytestmark = pytest.mark.gpu

STEPS = (3, 1, 1)
W_BOUND = {"clip": 1e-5, "free": 1e-5}
SCALAR_RTOL = 1e-4
# A clipped step's sum of squares is max_norm^2 in exact arithmetic; the
# reported one is a float32 sum over float32-rounded elements (2^-23
# relative on each square, plus the rounding of the chunked adds), so it may
# land a few ulps above.  1e-5 covers that and is five orders below the 16x
# by which an unclipped step (norm >= 4 max_norm) would overshoot.
SSQ_SLACK = 1e-5


def _epoch_bf16(C, k, max_norm, lr):
    """Client k alone on the per-client driver; (weights, loss, stats)."""
    from msrflute_amd.ops.fused_cnn import FusedCNNEpoch
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    _, _, x, y, row_bases = _store(C)
    lo = row_bases[k]
    fc = FusedCNNEpoch(arena, C, BS, P1, P2, max_norm, use_bf16=True)
    n, nb = fc.run_epoch(x[lo:lo + COUNTS[k]].cuda(),
                         y[lo:lo + COUNTS[k]].cuda(),
                         _orders(COUNTS, SEEDS)[k], lr, SEEDS[k] & SEED_MASK)
    torch.cuda.synchronize()
    assert (n, nb) == (COUNTS[k], STEPS[k])
    w = arena.data.cpu().clone()
    arena.data.copy_(w0)
    return w, fc.loss_acc.cpu()[0], fc.stats_acc.cpu()


def _mega_bf16(C, max_norm, lr):
    from msrflute_amd.ops.fused_cnn import MegaRound
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    store, ds, _, _, _ = _store(C)
    mr = MegaRound(arena, C, BS, P1, P2, max_norm, use_bf16=True)
    g = torch.Generator().manual_seed(9)
    accum = (ACCUM_SCALE * torch.randn(arena.total, generator=g)).cuda()
    outs = mr.run(store, ds, CLIENT_IDS, list(SEEDS), lr, arena, accum)
    torch.cuda.synchronize()
    assert outs is not None and len(outs) == 3
    assert torch.equal(arena.data.cpu(), w0)
    return mr


@functools.lru_cache(maxsize=None)
def _fp32_ssq(C, regime):
    """Per-client sum of squares the fp32 mega driver reports."""
    c = _case(C, regime)
    mr, _, _ = _mega(C, c["max_norm"], c["lr"])
    return [float(v) for v in mr.stats_out.cpu()[1:6:2]]


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_mega_bf16_matches_epoch_bf16(C, regime):
    c = _case(C, regime)
    _, w0 = _arena(C)
    P = w0.numel()
    mr = _mega_bf16(C, c["max_norm"], c["lr"])
    stack = mr.params_stack[:3 * P].cpu().view(3, P)
    loss, stats = mr.loss_out.cpu(), mr.stats_out.cpu()
    ssq32 = _fp32_ssq(C, regime) if regime == "free" else None
    fails = []
    for k in range(3):
        w, e_loss, e_stats = _epoch_bf16(C, k, c["max_norm"], c["lr"])
        assert not torch.equal(w, w0)
        rel = float((stack[k] - w).norm() / w.norm())
        scal = {"loss": ref.rel_err(loss[k], e_loss),
                "sum": ref.rel_err(stats[2 * k], e_stats[0]),
                "ssq": ref.rel_err(stats[2 * k + 1], e_stats[1])}
        print(f"client {k}: weights rel {rel:.3e}  "
              + "  ".join(f"{n} rel {float(v):.3e}" for n, v in scal.items()))
        if rel > W_BOUND[regime]:
            fails.append((k, "weights", rel))
        fails += [(k, n, float(v)) for n, v in scal.items()
                  if v > SCALAR_RTOL]
        # the regime held under bf16, on both drivers
        for ssq in (float(stats[2 * k + 1]), float(e_stats[1])):
            if regime == "clip":
                assert ssq <= STEPS[k] * c["max_norm"] ** 2 * (1 + SSQ_SLACK), \
                    (k, ssq)
            else:
                assert ssq >= 0.8 * ssq32[k], (k, ssq, ssq32[k])
    assert not fails, fails

    # masks left by the last step (t = 2): only client 0's row 0 is active
    G = 3 * BS
    wb = mr.work_b.cpu().numpy()
    seed0 = SEEDS[0] & SEED_MASK
    assert np.array_equal(wb[G * 9216:G * 9216 + 9216],
                          po.pool_mask(seed0, 2, 1, P1).reshape(-1))
    assert np.array_equal(wb[2 * G * 9216:2 * G * 9216 + 128],
                          po.fc1_mask(seed0, 2, 1, P2).reshape(-1))
