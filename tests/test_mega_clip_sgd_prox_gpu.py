"""``_C.mega_clip_sgd`` with the FedProx arguments (``server``, ``mu``,
``active``, ``loss_out``) against float64.

For an active client the kernels clip, count and apply ``gp = g + mu (w -
w_server)`` and add ``0.5 mu ||w - w_server||^2`` to its loss slot; an idle
client (mask byte 0, zero gradient, ``w != w_server``) must not move at all.

Sizes, tolerance and the no-cancellation construction are those of
tests/test_mega_clip_accum_gpu.py: P on every edge of ``k_sumsq_mb``
(below one float4, P % 4 tails, one chunk, one past the seam, two seams +
3), K in {1, 3}, rtol = 1e-5 with atol = 0 and exact zeros compared
exactly.  ``w - w_server`` shares the gradient's sign pattern, so neither
``gp``, ``sum(gp)`` nor ``p - lr * gp`` cancels.  mu = 1 and ``||w -
w_server|| ~ ||g||``: both terms carry weight in every checked value.
"""

import pytest
import torch

from test_mega_clip_accum_gpu import EPS, PS, _close

pytestmark = pytest.mark.gpu

MU = 1.0
LOSS_START = 3.0


def _server(P, gen):
    """The ONE server vector all K clients share: |w_g| in [1, 2)."""
    return ((1 + torch.rand(P, generator=gen))
            * (torch.randint(0, 2, (P,), generator=gen) * 2 - 1)).float()


def _offsets(P, K, gen):
    """Per-client ``w - w_g`` of norm ~1 (elements capped at 0.375 for
    tiny P, so |w| stays above 0.6) in the gradient's sign pattern."""
    sgn = torch.ones(P)
    sgn[::3] = -1.0
    return (0.5 + torch.rand(K, P, generator=gen)) * sgn \
        * min(P ** -0.5, 0.25)


def _grads(P, K, idle, gen):
    """Gradients of norm 1 + k / 4 in the sign pattern of
    tests/test_mega_clip_accum_gpu.py (mean well above 0); exactly zero
    for an idle client."""
    g = torch.rand(K, P, generator=gen) + 0.5
    g[:, ::3] *= -0.25
    g *= (1.0 + torch.arange(K).float() / 4)[:, None] \
        / g.double().norm(dim=1).float()[:, None]
    for k in idle:
        g[k] = 0.0
    return g.float()


def _expect(p, server, g, active, max_norm, lr):
    """float64 model of one FedProx mega_clip_sgd call on float32 inputs
    ``p`` [K, P], ``server`` [P], ``g`` [K, P]."""
    p, server, g = p.double(), server.double(), g.double()
    a = active.double()[:, None]
    d = p - server[None, :]
    gp = g + MU * d * a
    norm = gp.norm(dim=1)
    scale = torch.ones_like(norm)
    if max_norm > 0:
        hit = norm > max_norm
        scale[hit] = max_norm / (norm[hit] + EPS)
    gc = gp * scale[:, None]
    stats = torch.stack([gc.sum(1), (gc * gc).sum(1)], 1).reshape(-1)
    reg = 0.5 * MU * (d * d).sum(1) * active.double()
    return p - lr * gc, gc, stats, norm, reg


def _run(P, K, regime, use_mask):
    from msrflute_amd.ops import _C
    idle = (1,) if K == 3 else ()
    active = torch.ones(K, dtype=torch.bool)
    for k in idle:
        active[k] = False
    gen = torch.Generator().manual_seed(5000 * K + P)
    server = _server(P, gen)
    p = (server[None, :] + _offsets(P, K, gen)).float()
    g = _grads(P, K, idle, gen)
    # float64 free run fixes the regime
    _, _, _, norm_free, _ = _expect(p, server, g, active, -1.0, 0.1)
    act_norms = norm_free[active]
    max_norm = {"clip": 0.5 * float(act_norms.min()),
                "free": 2.0 * float(act_norms.max()),
                "off": -1.0}[regime]

    acc = torch.full((3 * K,), 7.0, dtype=torch.float64, device="cuda")
    lr_t = torch.zeros(1, device="cuda")
    stats = torch.zeros(2 * K, device="cuda")
    loss = torch.full((K,), LOSS_START, device="cuda")
    params = p.reshape(-1).cuda()
    server_dev = server.cuda()
    mask_dev = active.cuda() if use_mask else None
    want_p = p.double()
    want_stats = torch.zeros(2 * K, dtype=torch.float64)
    want_loss = torch.full((K,), LOSS_START, dtype=torch.float64)
    for call, lr in enumerate((0.1, 0.05)):
        if call:
            g = _grads(P, K, idle, gen)
        lr_t.fill_(lr)
        grads = g.reshape(-1).cuda()
        before = params.cpu().view(K, P).clone()
        _C.mega_clip_sgd(params, grads, K, acc, max_norm, lr_t, stats,
                         server=server_dev, mu=MU, active=mask_dev,
                         loss_out=loss)
        torch.cuda.synchronize()
        want_p, want_g, st, norm, reg = _expect(
            want_p.float(), server, g, active, max_norm, float(lr_t.cpu()))
        for k in range(K):
            if active[k]:
                # the term carries weight: without it the norm is ||g||
                # (the first call's SGD step then shrinks w - w_g)
                if call == 0:
                    assert abs(float(norm[k]) - float(g[k].double().norm())) \
                        >= 0.05 * float(norm[k])
                engaged = max_norm > 0 and float(norm[k]) > max_norm
                assert engaged == (regime == "clip")
            else:
                assert float(norm[k]) == 0.0
        want_stats = want_stats + st
        want_loss = want_loss + reg
        _close(grads, want_g)          # STORE_G: the stored gradient is gc
        _close(params, want_p)
        _close(stats, want_stats)
        _close(loss, want_loss)
        got = params.cpu().view(K, P)
        for k in idle:
            assert not torch.equal(before[k], server)      # w != w_server
            assert torch.equal(got[k], before[k])          # bit-unchanged
            assert float(loss[k]) == LOSS_START            # slot untouched
        want_p = got.double()


@pytest.mark.parametrize("regime", ["clip", "free", "off"])
@pytest.mark.parametrize("P", PS)
def test_prox_three_clients_one_idle(P, regime):
    _run(P, 3, regime, use_mask=True)


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("P", PS)
def test_prox_one_client_all_active_without_mask(P, regime):
    _run(P, 1, regime, use_mask=False)


def test_mu_zero_keywords_are_todays_call():
    from msrflute_amd.ops import _C
    K, P = 3, 32769
    gen = torch.Generator().manual_seed(3)
    p = torch.randn(K * P, generator=gen)
    g = torch.randn(K * P, generator=gen)
    lr_t = torch.full((1,), 0.1, device="cuda")
    out = []
    for kw in ({}, {"server": torch.randn(P, generator=gen).cuda(),
                    "mu": 0.0, "loss_out": torch.zeros(K, device="cuda")}):
        params, grads = p.cuda(), g.cuda()
        acc = torch.zeros(2 * K, dtype=torch.float64, device="cuda")
        stats = torch.zeros(2 * K, device="cuda")
        _C.mega_clip_sgd(params, grads, K, acc, 1.0, lr_t, stats, **kw)
        torch.cuda.synchronize()
        out.append((params.cpu(), grads.cpu()))
        if kw:
            assert float(kw["loss_out"].abs().max()) == 0.0
    assert torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])
