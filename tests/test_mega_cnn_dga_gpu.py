"""The cross-client CNN mega round under DGA (``MegaRound(dga=spec)`` ->
``launch_cnn_round_mega`` ending in k_dga_normsq_mb / k_dga_accum_mb) with
dropout ON.

Shape: that of tests/test_mega_cnn_reference_gpu.py (K = 3, counts 9 / 4 /
1, bs = 4, C in {5, 62}, its arena, store, seeds and ``round_accum``
start).  The per-batch chain is FedAvg's, so the trained stack must be the
FedAvg round's bit for bit; the tail is held to the float64 model of
tests/dga_ref64.py applied to the driver's OWN ``params_stack``,
``loss_out`` and ``stats_out``: weights and norms to 1e-12, the
``round_accum`` delta to FACTOR x floor (floor = the same tail in float32
on the CPU; the case is rejected unless FACTOR x floor <= 1e-3).
"""

import numpy as np
import pytest
import torch

import dga_ref64 as ref
from msrflute_amd.ops.mega_round import DGASpec
from test_mega_cnn_reference_gpu import (ACCUM_SCALE, BS, CLIENT_IDS, COUNTS,
                                         FACTOR, LR, P1, P2, SEEDS, _arena,
                                         _store)

pytestmark = pytest.mark.gpu

MAX_NORM = 10.0
BETA = 1.0


def _mega(C, dga=None):
    """One mega round; returns (driver, outputs, start, round_accum)."""
    from msrflute_amd.ops.fused_cnn import MegaRound
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    store, ds, _, _, _ = _store(C)
    mr = MegaRound(arena, C, BS, P1, P2, MAX_NORM, dga=dga)
    g = torch.Generator().manual_seed(9)
    start = ACCUM_SCALE * torch.randn(arena.total, generator=g)
    accum = start.cuda()
    outs = mr.run(store, ds, list(CLIENT_IDS), list(SEEDS), LR, arena, accum)
    torch.cuda.synchronize()
    assert outs is not None and [cid for cid, _ in outs] == list(CLIENT_IDS)
    assert mr.calls == 1
    assert torch.equal(arena.data.cpu(), w0)   # the server arena is read only
    return mr, outs, start, accum.cpu()


def _driver_state(mr, P):
    K = len(COUNTS)
    return (mr.params_stack[:K * P].cpu().view(K, P).numpy(),
            mr.loss_out[:K].cpu().numpy(), mr.stats_out[:2 * K].cpu().numpy())


@pytest.mark.parametrize("source,clip", [
    ("train_loss", True), ("train_loss", False), ("mag_var_loss", False),
    ("mag_mean_loss", True), ("mag", False), ("mean", True)])
@pytest.mark.parametrize("C", [5, 62])
def test_mega_dga_round_matches_fp64_tail(C, source, clip):
    _, w0 = _arena(C)
    P = w0.numel()
    fed, fed_outs, _, _ = _mega(C)
    stack_fed, loss_fed, stats_fed = _driver_state(fed, P)
    # max_grad between the clients' norms: both sides of the clip run
    norms = ref.dga_tail(w0.numpy(), stack_fed, loss_fed, stats_fed, COUNTS,
                         BS, "mean", BETA, True, 1.0)["norm"]
    max_grad = float(np.sqrt(norms.min() * norms.max())) if clip else 0.0
    # beta scaled so that the weights are neither all ~1 nor all ~0
    tw = [abs(ref.training_weight(source, loss_fed[k], stats_fed[2 * k],
                                  stats_fed[2 * k + 1], COUNTS[k], BS, P))
          for k in range(3)] if source != "mean" else [1.0]
    beta = BETA / max(tw)
    spec = DGASpec(source, beta, clip, max_grad)

    mr, outs, start, accum = _mega(C, dga=spec)
    stack, loss, stats = _driver_state(mr, P)
    # the per-batch chain is untouched: FedAvg's stack, loss and stats
    assert np.array_equal(stack, stack_fed)
    np.testing.assert_allclose(loss, loss_fed, rtol=1e-6, atol=0)
    np.testing.assert_allclose(stats, stats_fed, rtol=1e-6, atol=0)

    args = (w0.numpy(), stack, loss, stats, COUNTS, BS, source, beta, clip,
            max_grad)
    start64 = start.numpy().astype(np.float64)
    want = ref.dga_tail(*args, accum=start.numpy())
    delta64 = want["accum"] - start64
    floor = ref.rel_l2(ref.dga_tail_f32(*args, accum=start.numpy())
                       .astype(np.float64) - start64, delta64)
    assert FACTOR * floor <= 1e-3, ("misconfigured case", floor)
    err = ref.rel_l2(accum.numpy().astype(np.float64) - start64, delta64)
    print(f"C={C} {source} clip={clip}: weights {want['weight']} norms "
          f"{want['norm']} err {err:.3e} floor {floor:.3e}")
    K = 3
    out = mr.dga_out[:3 * K].cpu().numpy().reshape(3, K)
    np.testing.assert_allclose(out[0], want["weight"], rtol=1e-12, atol=0)
    np.testing.assert_allclose(out[1], want["norm"], rtol=1e-12, atol=0)
    assert err <= FACTOR * floor, (err, floor)
    if clip:
        assert (want["norm"] > max_grad).any()
        assert (want["norm"] < max_grad).any()
    if source != "mean":
        # (a negative mean gives a weight above 1)
        assert (want["weight"] > 0).all() and (want["weight"] < 100).all()
        assert len(set(want["weight"])) == 3
    # the driver reports the device's weights; the lazy triple is FedAvg's
    for k, (_, meta) in enumerate(outs):
        assert meta["pl"]["weight"] == out[0][k]
        assert meta["pl"]["pooled"] and meta["pl"]["grad"] is None
        assert meta["ns"] == COUNTS[k]
        assert meta["_lazy"][2] == fed_outs[k][1]["_lazy"][2]
    for k, (_, meta) in enumerate(fed_outs):
        assert meta["pl"]["weight"] == float(COUNTS[k])


@pytest.mark.parametrize("C", [5, 62])
def test_zero_weight_client_contributes_nothing(C):
    """beta so large that exp underflows for every client: all weights are
    0 and ``round_accum`` keeps its bits."""
    mr, outs, start, accum = _mega(C, dga=DGASpec("train_loss", 1e6, True,
                                                  1e-3))
    assert all(meta["pl"]["weight"] == 0.0 for _, meta in outs)
    assert torch.equal(accum, start)


@pytest.mark.parametrize("C", [5, 62])
def test_fedavg_round_is_untouched_by_a_dga_round(C):
    """A FedAvg MegaRound before and after a DGA one in the same process:
    bit-equal ``round_accum`` and stack."""
    _, w0 = _arena(C)
    P = w0.numel()
    before, _, _, accum_before = _mega(C)
    stack_before = before.params_stack[:3 * P].cpu()
    _mega(C, dga=DGASpec("train_loss", 0.5, True, 1e-3))
    after, _, _, accum_after = _mega(C)
    assert torch.equal(accum_after, accum_before)
    assert torch.equal(after.params_stack[:3 * P].cpu(), stack_before)
    assert not torch.equal(accum_before, ACCUM_SCALE * torch.randn(
        P, generator=torch.Generator().manual_seed(9)))
