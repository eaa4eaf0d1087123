"""FedProx flavour of tests/cnn_ref64.py: the fused CNN's local step with
the exact per-batch proximal term of ``Trainer.run_train_epoch(prox=...)``,
in float64 by default.

    gp    = g + mu * (w - w_g)          w: weights before the step
    norm  = ||gp||_2 over the whole arena (reduced in float64)
    scale, stats, SGD as in cnn_ref64, on gp
    loss  = CE(batch) + 0.5 * mu * sum (w - w_g)^2

With ``mu = 0`` every value equals ``cnn_ref64``'s bit for bit.
"""

import torch

import cnn_ref64 as ref


def step(flat, C, x, y, m2, m3, p1, p2, max_norm, lr, mu, w_g):
    """One local FedProx step on the flat weights.  Returns ``(new_flat,
    loss incl. regulariser, clipped_grad, pre_clip_norm, pre_clip_grad)``."""
    leaf = flat.detach().clone().requires_grad_(True)
    ce = ref.loss_fn(ref.split(leaf, C), x, y, m2, m3, p1, p2)
    g, = torch.autograd.grad(ce, leaf)
    d = flat.detach() - w_g
    gp = g + mu * d
    loss = ce.detach() + 0.5 * mu * (d * d).sum()
    norm = gp.double().norm()
    scale = 1.0
    if max_norm > 0 and float(norm) > max_norm:
        scale = max_norm / (float(norm) + ref.CLIP_EPS)
    gc = gp * scale
    return flat.detach() - lr * gc, loss, gc, float(norm), gp


def epoch(flat, C, xs, ys, order, bs, masks, p1, p2, max_norm, lr, mu, w_g,
          dtype=torch.float64):
    """``cnn_ref64.epoch`` with the proximal term towards ``w_g``; the same
    dict, ``loss`` including every step's regulariser."""
    w = flat.detach().to(dtype).clone()
    w_g = w_g.detach().to(dtype)
    xs = xs.to(dtype)
    loss_sum = torch.zeros((), dtype=dtype)
    stats = torch.zeros(2, dtype=dtype)
    norms, g = [], None
    n = len(order)
    for t, s in enumerate(range(0, n, bs)):
        idx = order[s:s + bs]
        m2, m3 = masks(t, len(idx))
        w, loss, g, norm, _ = step(w, C, xs[idx], ys[idx],
                                   torch.as_tensor(m2).to(dtype),
                                   torch.as_tensor(m3).to(dtype),
                                   p1, p2, max_norm, lr, mu, w_g)
        loss_sum += loss
        stats[0] += g.sum()
        stats[1] += (g * g).sum()
        norms.append(norm)
    return {"w": w, "loss": loss_sum, "stats": stats, "norms": norms,
            "grad": g}
