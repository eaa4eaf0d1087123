"""The Shakespeare graphed mega round under DGA
(``ShakespeareMegaRound(dga=spec)``: the epoch body ends in
``_C.mega_dga_accum`` instead of ``_C.mega_pseudo_accum``, inside the
captured graph).

Shape: that of tests/test_mega_shakespeare_prox_gpu.py (T = 80, bs = 4,
K = 3 clients of 9, 4 and 6 rows: ragged, client 1 idles for two steps).
The round runs twice, captured (the default) and eagerly
(``MEGA_SHK_EAGER=1``); the two must agree bit for bit, and the tail is
held to the float64 model of tests/dga_ref64.py on the driver's own
stack, loss and stats: weights and norms to 1e-12, the accumulate to
FACTOR x floor (floor = the same tail in float32 on the CPU; rejected
unless FACTOR x floor <= 1e-3).
"""

import numpy as np
import pytest
import torch

import dga_ref64 as ref
from msrflute_amd.ops.mega_round import DGASpec
from test_mega_shakespeare_prox_gpu import (BS, CLIENT_IDS, COUNTS, LR,
                                            MAX_NORM, SEEDS, _setup)

pytestmark = pytest.mark.gpu

FACTOR = 4
BETA = 2.0


def _round(spec, eager, monkeypatch):
    from msrflute_amd.ops.mega_shakespeare import ShakespeareMegaRound
    _, arena, w0, store, ds = _setup()
    arena.data.copy_(w0)
    if eager:
        monkeypatch.setenv(ShakespeareMegaRound.EAGER_ENV, "1")
    else:
        monkeypatch.delenv(ShakespeareMegaRound.EAGER_ENV, raising=False)
    mega = ShakespeareMegaRound(arena, BS, MAX_NORM, dga=spec)
    accum = torch.zeros(arena.total, device=arena.device)
    outs = mega.run(store, ds, CLIENT_IDS, list(SEEDS), LR, arena, accum)
    torch.cuda.synchronize()
    assert outs is not None and [m["ns"] for _, m in outs] == list(COUNTS)
    assert torch.equal(arena.data, w0) and mega.calls == 1
    (g,) = mega._graphs.values()
    assert (g["graph"] is None) == eager
    K = 3
    return {"accum": accum.cpu().numpy(),
            "stack": g["flat"].detach().cpu().numpy(),
            "loss": g["loss_dev"].cpu().numpy(),
            "stats": g["stats_out"].cpu().numpy(),
            "out": g["dga_out"][:3 * K].cpu().numpy().reshape(3, K),
            "weights": [m["pl"]["weight"] for _, m in outs]}


def test_shakespeare_dga_round_captured_equals_eager_and_fp64(monkeypatch):
    _, _, w0, _, _ = _setup()
    w0 = w0.cpu().numpy()
    # a FedAvg round's stack gives the clients' pseudo-gradient norms:
    # max_grad between them, so both sides of the clip run
    probe = _round(DGASpec("train_loss", BETA, True, 1.0), True, monkeypatch)
    norms = probe["out"][1]
    max_grad = float(np.sqrt(norms.min() * norms.max()))
    # beta such that the largest exponent is -BETA
    beta = BETA / max(float(probe["loss"][k]) / COUNTS[k] for k in range(3))
    spec = DGASpec("train_loss", beta, True, max_grad)

    cap = _round(spec, False, monkeypatch)
    eag = _round(spec, True, monkeypatch)
    for name in ("stack", "loss", "stats", "accum"):
        assert np.array_equal(cap[name], eag[name]), name
    # weights and the applied float32 coefficients too; the reported f64
    # norm is folded with one atomicAdd per block, whose order is free, so
    # it repeats to f64 rounding (and c is its float32 rounding)
    assert np.array_equal(cap["out"][0], eag["out"][0])
    assert np.array_equal(cap["out"][2], eag["out"][2])
    np.testing.assert_allclose(cap["out"][1], eag["out"][1], rtol=1e-14,
                               atol=0)
    assert cap["weights"] == eag["weights"] == cap["out"][0].tolist()

    args = (w0, cap["stack"], cap["loss"], cap["stats"], COUNTS, BS,
            "train_loss", beta, True, max_grad)
    want = ref.dga_tail(*args)
    floor = ref.rel_l2(ref.dga_tail_f32(*args), want["accum"])
    assert FACTOR * floor <= 1e-3, ("misconfigured case", floor)
    err = ref.rel_l2(cap["accum"], want["accum"])
    print(f"weights {want['weight']} norms {want['norm']} max_grad "
          f"{max_grad:.4g} err {err:.3e} floor {floor:.3e}")
    np.testing.assert_allclose(cap["out"][0], want["weight"], rtol=1e-12,
                               atol=0)
    np.testing.assert_allclose(cap["out"][1], want["norm"], rtol=1e-12,
                               atol=0)
    assert (want["norm"] > max_grad).any() and (want["norm"] < max_grad).any()
    assert (want["weight"] > 0).all() and (want["weight"] < 1).all()
    assert len(set(want["weight"])) == 3
    assert err <= FACTOR * floor, (err, floor)
