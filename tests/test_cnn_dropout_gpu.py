"""The per-client fused CNN epoch with dropout ON (p1 = 0.25, p2 = 0.5,
the production setting) against an independent float64 reference.

* The masks the kernels leave in ``FusedCNNEpoch.work_b`` must equal the
  numpy Philox oracle (tests/philox_oracle.py) bit for bit: this pins the
  key ``(seed, li >> 2, batch index)``, the lane pick ``li & 3`` of the
  4-cell draw and the fc1 stream.
* A 3-batch epoch (4 + 4 + 1 rows) must match tests/cnn_ref64.py replayed
  under those masks, per parameter segment, with clipping engaged at
  every batch and with clipping never engaged: this pins the 1/(1-p)
  scaling and the mask gating of forward and backward.

Bound.  For each case the same replay also runs in torch float32 on the
CPU; ``floor`` is the largest per-segment relative L2 error of that fp32
replay against float64, and every kernel figure must be within
``FACTOR * floor`` (the factor covers the kernels' fmaf chains, split-K
order and fast exp/log against torch's own fp32 reductions).  The case is
rejected as misconfigured unless ``FACTOR * floor <= 1e-3``.  Updates
``w_after - w_before`` are compared, not weights: a weight's rounding
hides a wrong small step.  Measured figures: docs/kernels.md.
"""

import functools

import numpy as np
import pytest
import torch

import cnn_ref64 as ref
import philox_oracle as po

pytestmark = pytest.mark.gpu

BS, P1, P2, LR = 4, 0.25, 0.5, 0.1
SEEDS = (5, (1 << 32) * 77 + 3)   # the second one has a non-zero high word
# headroom over the fp32 replay's own error; the worst measured kernel
# figure is 1.1 x floor (docs/kernels.md), a wrong scale or mask is > 1e4 x
FACTOR = 4.0
N_ROWS = 9                        # batches of 4 + 4 + 1 rows


@functools.lru_cache(maxsize=None)
def _arena(C):
    from msrflute_amd.models import make_model
    from msrflute_amd.ops.arena import ParameterArena
    torch.manual_seed(3)
    model = make_model({"model_type": "CNN",
                        "model_folder": "experiments/cv_cnn_femnist/model.py",
                        "num_classes": C})
    arena = ParameterArena(model, bind_grads=True)
    return arena, arena.data.cpu().clone()


def _run(C, xs, ys, order, lr, seed, max_norm, bs=BS):
    """One fused epoch from the initial weights; returns the driver."""
    from msrflute_amd.ops.fused_cnn import FusedCNNEpoch
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    arena.grad.zero_()
    fc = FusedCNNEpoch(arena, C, bs=bs, p1=P1, p2=P2, max_grad_norm=max_norm)
    fc.run_epoch(xs.cuda(), ys.cuda(), order, lr, seed)
    torch.cuda.synchronize()
    return fc


@functools.lru_cache(maxsize=None)
def _kernel_masks(seed, n_rows, bs=BS):
    """(m2, m3) bytes that an epoch of n_rows rows leaves behind: the
    masks of its LAST batch in the leading rows of each buffer."""
    g = torch.Generator().manual_seed(1)
    xs = torch.randn(n_rows, 28, 28, generator=g)
    ys = torch.randint(0, 5, (n_rows,), generator=g)
    fc = _run(5, xs, ys, torch.arange(n_rows), LR, seed, 10.0, bs=bs)
    wb = fc.work_b.cpu().numpy()
    return (wb[bs * 9216:2 * bs * 9216].copy(),
            wb[2 * bs * 9216:2 * bs * 9216 + bs * 128].copy())


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_rows,t,rows", [(4, 0, 4), (8, 1, 4), (12, 2, 4),
                                           (5, 1, 1)])
def test_masks_equal_oracle(seed, n_rows, t, rows):
    m2, m3 = _kernel_masks(seed, n_rows)
    want2 = po.pool_mask(seed, t, rows, P1).reshape(-1)
    want3 = po.fc1_mask(seed, t, rows, P2).reshape(-1)
    assert set(np.unique(m2[:rows * 9216])) <= {0, 1}
    bad2 = int((m2[:rows * 9216] != want2).sum())
    bad3 = int((m3[:rows * 128] != want3).sum())
    assert bad2 == 0 and bad3 == 0, (bad2, bad3)


def test_masks_depend_on_batch_and_seed():
    a2, a3 = _kernel_masks(SEEDS[0], 4)
    b2, b3 = _kernel_masks(SEEDS[0], 8)
    c2, c3 = _kernel_masks(SEEDS[1], 4)
    assert not np.array_equal(a2, b2) and not np.array_equal(a3, b3)
    assert not np.array_equal(a2, c2) and not np.array_equal(a3, c3)


@pytest.mark.parametrize("seed", SEEDS)
def test_pool_mask_lane_statistics(seed):
    # bs = 8, one batch: 73728 cells, 18432 per li & 3 lane
    m2, _ = _kernel_masks(seed, 8, bs=8)
    lanes = m2.reshape(-1, 4).astype(np.float64)
    n = lanes.shape[0]
    assert n == 18432
    sigma = np.sqrt(0.75 * 0.25 / n)
    rates = lanes.mean(0)
    print("lane keep rates", rates, "sigma", sigma)
    assert (np.abs(rates - 0.75) < 5 * sigma).all(), rates
    r = np.corrcoef(lanes.T)
    off = r[~np.eye(4, dtype=bool)]
    print("lane correlations", off)
    assert (np.abs(off) < 5 / np.sqrt(n)).all(), r


@functools.lru_cache(maxsize=None)
def _case(C, regime):
    """Data, the float64 and float32 replays and the bound of one case."""
    _, w0 = _arena(C)
    g = torch.Generator().manual_seed(40 + C)
    xs = torch.randn(N_ROWS, 28, 28, generator=g)
    ys = torch.randint(0, C, (N_ROWS,), generator=g)
    order = torch.randperm(N_ROWS, generator=g)
    masks = po.epoch_masks(SEEDS[1], P1, P2)
    xs64 = xs.double()

    def replay(rows, max_norm, lr, dtype=torch.float64):
        return ref.epoch(w0, C, xs64, ys, rows, BS, masks, P1, P2, max_norm,
                         lr, dtype=dtype)

    # the two max_norm values come from the reference's own norms
    free = replay(order, -1.0, LR)
    if regime == "clip":
        max_norm, lr = 0.25 * min(free["norms"]), 4 * LR
    else:
        max_norm, lr = 4.0 * max(free["norms"]), LR
    out = {"xs": xs, "ys": ys, "order": order, "max_norm": max_norm,
           "lr": lr}
    for tag, rows in (("epoch", order), ("batch", order[:BS])):
        r64 = replay(rows, max_norm, lr)
        r32 = replay(rows, max_norm, lr, dtype=torch.float32)
        engaged = [n > max_norm for n in r64["norms"]]
        assert all(engaged) if regime == "clip" else not any(engaged), \
            (r64["norms"], max_norm)
        upd64 = r64["w"] - w0.double()
        errs = ref.seg_rel_err(r32["w"] - w0, upd64, C)
        if tag == "batch":
            errs = ref.seg_rel_err(r32["grad"], r64["grad"], C)
        floor = max(errs.values())
        assert FACTOR * floor <= 1e-3, ("misconfigured case", errs)
        out[tag] = {"r64": r64, "upd64": upd64, "floor": floor,
                    "floors": errs}
    return out


def _check(what, errs, floor):
    bound = FACTOR * floor
    for name, e in errs.items():
        print(f"{what:>14} {name:>6}: err {e:.3e}  floor {floor:.3e}  "
              f"ratio {e / floor:.2f}")
    worst = max(errs, key=errs.get)
    assert errs[worst] <= bound, (what, worst, errs[worst], bound)


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_epoch_matches_fp64_under_kernel_masks(C, regime):
    c = _case(C, regime)
    _, w0 = _arena(C)
    e = c["epoch"]
    print("floors", {k: f"{v:.2e}" for k, v in e["floors"].items()})
    fc = _run(C, c["xs"], c["ys"], c["order"], c["lr"], SEEDS[1],
              c["max_norm"])
    upd = fc.arena.data.cpu() - w0
    _check("update", ref.seg_rel_err(upd, e["upd64"], C), e["floor"])
    r64 = e["r64"]
    _check("loss/stats", {
        "loss": ref.rel_err(fc.loss_acc, r64["loss"]),
        "sum_g": ref.rel_err(fc.stats_acc[0], r64["stats"][0]),
        "sum_g2": ref.rel_err(fc.stats_acc[1], r64["stats"][1]),
    }, e["floor"])


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_one_batch_gradient_matches_fp64(C, regime):
    c = _case(C, regime)
    b = c["batch"]
    rows = c["order"][:BS]
    fc = _run(C, c["xs"][rows], c["ys"][rows], torch.arange(BS), c["lr"],
              SEEDS[1], c["max_norm"])
    _check("arena.grad", ref.seg_rel_err(fc.arena.grad, b["r64"]["grad"], C),
           b["floor"])
