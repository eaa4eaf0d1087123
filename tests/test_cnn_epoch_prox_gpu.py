"""The per-client fused CNN epoch under FedProx
(``FusedCNNEpoch.run_epoch(prox=(1.0, server))`` -> ``launch_cnn_epoch``,
whose clip / stats / SGD tail then runs the ProxArgs kernel pair at K = 1)
over client 0's 4 + 4 + 1-row epoch of tests/cnn_prox_case.py, against
float64 with that file's bound, in both clip regimes — and against the
mega driver training the same client alone (relative 1e-5 on the trained
arena, the tolerance tests/test_mega_round_gpu.py holds the two drivers
to).
"""

import pytest
import torch

import cnn_prox_case as pc
import cnn_ref64 as ref
from test_mega_cnn_reference_gpu import (BS, CLIENT_IDS, P1, P2, SEED_MASK,
                                         SEEDS, _arena, _check)

pytestmark = pytest.mark.gpu


def _epoch(C, max_norm, lr, prox=True):
    """Client 0's epoch on the arena; returns (trained weights, loss,
    stats) on the CPU."""
    from msrflute_amd.ops.fused_cnn import FusedCNNEpoch
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    x, y, _, _, row_bases = pc.data(C)
    lo = row_bases[0]
    shard_x = x[lo:lo + pc.COUNTS[0]].cuda()
    shard_y = y[lo:lo + pc.COUNTS[0]].cuda()
    server = w0.cuda()
    fc = FusedCNNEpoch(arena, C, BS, P1, P2, max_norm)
    order = pc.case(C, "free")["orders"][0]
    n, nb = fc.run_epoch(shard_x, shard_y, order, lr, SEEDS[0] & SEED_MASK,
                         prox=(pc.MU, server) if prox else None)
    torch.cuda.synchronize()
    assert (n, nb) == (9, 3)
    assert torch.equal(server.cpu(), w0)       # the server copy is read only
    w = arena.data.cpu().clone()
    arena.data.copy_(w0)
    return w, fc.loss_acc.cpu()[0], fc.stats_acc.cpu()


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_epoch_prox_matches_fp64_and_mega(C, regime):
    c = pc.case(C, regime)
    _, w0 = _arena(C)
    r = c["r64"][0]
    w, loss, stats = _epoch(C, c["max_norm"], c["lr"])
    _check("epoch upd", ref.seg_rel_err(w - w0, c["upd64"][0], C),
           c["floor"])
    _check("loss/stats", {"loss": ref.rel_err(loss, r["loss"]),
                          "sum": ref.rel_err(stats[0], r["stats"][0]),
                          "ssq": ref.rel_err(stats[1], r["stats"][1])},
           c["floor"])

    # the mega driver on the same client alone
    from msrflute_amd.ops.fused_cnn import MegaRound
    arena, _ = _arena(C)
    store, ds = pc.store(C)
    mr = MegaRound(arena, C, BS, P1, P2, c["max_norm"], mu=pc.MU)
    accum = torch.zeros(arena.total, device="cuda")
    outs = mr.run(store, ds, [CLIENT_IDS[0]], [SEEDS[0]], c["lr"], arena,
                  accum)
    torch.cuda.synchronize()
    assert outs is not None
    w_mega = mr.params_stack[:w0.numel()].cpu()
    rel = float((w - w_mega).norm() / w_mega.norm())
    print(f"epoch vs mega: rel {rel:.3e}")
    assert rel <= 1e-5, rel


@pytest.mark.parametrize("C", [5])
def test_epoch_without_prox_is_unchanged_by_the_argument(C):
    """``prox=None`` and ``prox=(0.0, server)`` both run today's FedAvg
    tail: the same bits."""
    from msrflute_amd.ops.fused_cnn import FusedCNNEpoch
    c = pc.case(C, "free")
    arena, w0 = _arena(C)
    x, y, _, _, row_bases = pc.data(C)
    lo = row_bases[0]
    shard_x, shard_y = x[lo:lo + 9].cuda(), y[lo:lo + 9].cuda()
    out = []
    for prox in (None, (0.0, w0.cuda())):
        arena.data.copy_(w0)
        fc = FusedCNNEpoch(arena, C, BS, P1, P2, c["max_norm"])
        fc.run_epoch(shard_x, shard_y, c["orders"][0], c["lr"],
                     SEEDS[0] & SEED_MASK, prox=prox)
        torch.cuda.synchronize()
        out.append(arena.data.cpu().clone())
    arena.data.copy_(w0)
    w_avg, _, _ = _epoch(C, c["max_norm"], c["lr"], prox=False)
    assert torch.equal(out[0], out[1]) and torch.equal(out[0], w_avg)
    w_prox, _, _ = _epoch(C, c["max_norm"], c["lr"])
    assert not torch.equal(w_prox, w_avg)
