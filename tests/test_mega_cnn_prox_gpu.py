"""The cross-client CNN mega round under FedProx (``MegaRound(mu=1)`` ->
``launch_cnn_round_mega`` -> the ProxArgs instantiations of ``k_sumsq_mb``
/ ``k_clip_sgd_mb``) with dropout ON against float64.

Case, bound and the conditions the case itself must meet:
tests/cnn_prox_case.py.  Checked per client and per parameter segment: the
update ``w - w0``, the ``round_accum`` delta, and loss / sum g / sum g^2.

The idle rule: a client that has finished its epoch has ``w != w_g`` but
gets no proximal term and no regulariser, so it stays bit-unchanged while
the others go on (an ungated term would keep pulling it back).
"""

import pytest
import torch

import cnn_prox_case as pc
import cnn_ref64 as ref
from test_mega_cnn_reference_gpu import (ACCUM_SCALE, BS, CLIENT_IDS, P1, P2,
                                         SEEDS, _arena, _check)

pytestmark = pytest.mark.gpu

COUNTS = pc.COUNTS


def _mega(C, max_norm, lr, client_sel=(0, 1, 2), mu=pc.MU):
    """Run the mega round for the selected clients; returns (driver,
    round_accum start, round_accum)."""
    from msrflute_amd.ops.fused_cnn import MegaRound
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    store, ds = pc.store(C)
    mr = MegaRound(arena, C, BS, P1, P2, max_norm, mu=mu)
    g = torch.Generator().manual_seed(9)
    start = (ACCUM_SCALE * torch.randn(arena.total, generator=g))
    accum = start.cuda()
    outs = mr.run(store, ds, [CLIENT_IDS[k] for k in client_sel],
                  [SEEDS[k] for k in client_sel], lr, arena, accum)
    torch.cuda.synchronize()
    assert outs is not None and len(outs) == len(client_sel)
    for k, (cid, meta) in zip(client_sel, outs):
        assert cid == CLIENT_IDS[k] and meta["ns"] == COUNTS[k]
    assert torch.equal(arena.data.cpu(), w0)   # the server arena is read only
    return mr, start, accum.cpu()


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_mega_prox_round_matches_fp64(C, regime):
    c = pc.case(C, regime)
    _, w0 = _arena(C)
    P = w0.numel()
    print("floors", [{k: f"{v:.2e}" for k, v in f.items()}
                     for f in c["floors"]])
    print(f"separation from mu = 0: update {c['sep']:.2e}, "
          f"loss {c['loss_sep']:.2e}")
    mr, start, accum = _mega(C, c["max_norm"], c["lr"])
    stack = mr.params_stack[:3 * P].cpu().view(3, P)
    for k in range(3):
        _check(f"client {k} upd", ref.seg_rel_err(stack[k] - w0,
                                                  c["upd64"][k], C),
               c["floor"])
    want = sum(-float(COUNTS[k]) * c["upd64"][k] for k in range(3))
    _check("round_accum", ref.seg_rel_err(accum - start, want, C),
           c["floor"])
    loss, stats = mr.loss_out.cpu(), mr.stats_out.cpu()
    scal = {}
    for k in range(3):
        r = c["r64"][k]
        scal[f"loss{k}"] = ref.rel_err(loss[k], r["loss"])
        scal[f"sum{k}"] = ref.rel_err(stats[2 * k], r["stats"][0])
        scal[f"ssq{k}"] = ref.rel_err(stats[2 * k + 1], r["stats"][1])
    _check("loss/stats", scal, c["floor"])


@pytest.mark.parametrize("C", [5, 62])
def test_finished_prox_clients_stay_bit_unchanged(C):
    """Clients 1 and 2 alone run TWO steps; in the three-step round client
    1 idles through step 2 and client 2 through steps 1 and 2, both away
    from the server weights, and must end exactly where they ended
    alone."""
    c = pc.case(C, "free")
    _, w0 = _arena(C)
    P = w0.numel()
    mr3, _, _ = _mega(C, c["max_norm"], c["lr"])
    stack3 = mr3.params_stack[:3 * P].cpu().view(3, P)
    loss3, stats3 = mr3.loss_out.cpu(), mr3.stats_out.cpu()
    mr2, _, _ = _mega(C, c["max_norm"], c["lr"], client_sel=(1, 2))
    stack2 = mr2.params_stack[:2 * P].cpu().view(2, P)
    loss2, stats2 = mr2.loss_out.cpu(), mr2.stats_out.cpu()
    assert not torch.equal(stack2[0], w0) and not torch.equal(stack2[1], w0)
    assert torch.equal(stack3[1], stack2[0])
    assert torch.equal(stack3[2], stack2[1])
    # the single-row client's loss is one add plus a zero regulariser
    # (w == w_g at its only step) and is exact; the rest is folded with
    # atomics whose order is free and repeats to rounding
    assert torch.equal(loss3[2], loss2[1])
    assert torch.allclose(loss3[1:3], loss2[:2], rtol=1e-6, atol=0)
    assert torch.allclose(stats3[2:6], stats2[:4], rtol=1e-6, atol=0)


@pytest.mark.parametrize("C", [5, 62])
def test_mu_zero_is_todays_call_bit_for_bit(C, monkeypatch):
    """``mu = 0`` through the new argument against the positional call
    without it: the same FedAvg kernels, so the same bits."""
    from msrflute_amd.ops import fused_cnn
    c = pc.case(C, "clip")
    _, w0 = _arena(C)
    P = w0.numel()
    mr_new, _, accum_new = _mega(C, c["max_norm"], c["lr"], mu=0.0)
    stack_new = mr_new.params_stack[:3 * P].cpu()
    assert not torch.equal(stack_new[:P], w0)

    real = fused_cnn._C
    calls = []

    class _Positional:
        def __getattr__(self, name):
            return getattr(real, name)

        @staticmethod
        def cnn_round_mega(*args, mu):
            assert mu == 0.0
            calls.append(len(args))
            return real.cnn_round_mega(*args)

    monkeypatch.setattr(fused_cnn, "_C", _Positional())
    mr_old, _, accum_old = _mega(C, c["max_norm"], c["lr"], mu=0.0)
    assert calls == [26]
    assert torch.equal(mr_old.params_stack[:3 * P].cpu(), stack_new)
    assert torch.equal(accum_old, accum_new)
