"""Plain torch model of the fused CNN's local training step
(csrc/fused_cnn.hip), in float64 by default.

It works on explicit tensors in the arena's order ``w1 b1 w2 b2 w3 b3 w4
b4`` and takes the dropout masks as arguments, so a test can replay a
kernel run under the kernel's own masks.  Gradients come from
``torch.autograd.grad``; clip, stats and SGD follow the kernels'
definitions:

    norm  = ||g||_2 over the whole arena (reduced in float64)
    scale = max_norm / (norm + 1e-6)  if max_norm > 0 and norm > max_norm
            1                          otherwise
    g    <- g * scale;  stats += (sum g, sum g^2);  w <- w - lr * g

With ``dtype=torch.float32`` the same code is the fp32 noise floor the
kernels are measured against.
"""

import torch
import torch.nn.functional as F

NAMES = ("w1", "b1", "w2", "b2", "w3", "b3", "w4", "b4")
CLIP_EPS = 1e-6


def shapes(C):
    return ((32, 1, 3, 3), (32,), (64, 32, 3, 3), (64,), (128, 9216),
            (128,), (C, 128), (C,))


def segments(C):
    """[(name, offset, numel)] of the flat arena."""
    out, off = [], 0
    for name, shp in zip(NAMES, shapes(C)):
        n = 1
        for s in shp:
            n *= s
        out.append((name, off, n))
        off += n
    return out


def total(C):
    name, off, n = segments(C)[-1]
    return off + n


def split(flat, C):
    """The 8 parameter tensors as views of a flat arena vector."""
    return [flat[off:off + n].view(shp)
            for (_, off, n), shp in zip(segments(C), shapes(C))]


def loss_fn(ws, x, y, m2, m3, p1, p2):
    """Mean cross-entropy of the batch ``x`` [B, 28, 28], ``y`` [B] under
    keep masks ``m2`` [B, 64, 12, 12] and ``m3`` [B, 128]."""
    w1, b1, w2, b2, w3, b3, w4, b4 = ws
    h = torch.relu(F.conv2d(x.unsqueeze(1), w1, b1))
    h = torch.relu(F.conv2d(h, w2, b2))
    h = F.max_pool2d(h, 2)
    h = h * m2 / (1.0 - p1)
    h = torch.flatten(h, 1)
    h = torch.relu(F.linear(h, w3, b3))
    h = h * m3 / (1.0 - p2)
    return F.cross_entropy(F.linear(h, w4, b4), y)


def step(flat, C, x, y, m2, m3, p1, p2, max_norm, lr):
    """One local step on the flat weights.  Returns ``(new_flat, loss,
    clipped_grad, pre_clip_norm)``."""
    leaf = flat.detach().clone().requires_grad_(True)
    loss = loss_fn(split(leaf, C), x, y, m2, m3, p1, p2)
    g, = torch.autograd.grad(loss, leaf)
    # the kernels reduce the norm in float64 whatever the gradient's type;
    # torch's own float32 norm of 1.2 M elements is off by ~1e-5, which
    # would pass into every segment of a clipped step and widen the floor
    norm = g.double().norm()
    scale = 1.0
    if max_norm > 0 and float(norm) > max_norm:
        scale = max_norm / (float(norm) + CLIP_EPS)
    g = g * scale
    return flat.detach() - lr * g, loss.detach(), g, float(norm)


def epoch(flat, C, xs, ys, order, bs, masks, p1, p2, max_norm, lr,
          dtype=torch.float64):
    """One local epoch over rows ``order`` of ``xs`` / ``ys`` in batches
    of ``bs`` (the last may be short).  ``masks(t, B)`` returns batch t's
    ``(m2, m3)`` keep masks for its B rows.  Everything is computed in
    ``dtype``.  Returns a dict: ``w`` trained weights, ``loss`` summed
    batch losses, ``stats`` (sum g, sum g^2) of the clipped gradients
    summed over batches, ``norms`` pre-clip norm per batch, ``grad`` the
    last batch's clipped gradient."""
    w = flat.detach().to(dtype).clone()
    xs = xs.to(dtype)
    loss_sum = torch.zeros((), dtype=dtype)
    stats = torch.zeros(2, dtype=dtype)
    norms, g = [], None
    n = len(order)
    for t, s in enumerate(range(0, n, bs)):
        idx = order[s:s + bs]
        m2, m3 = masks(t, len(idx))
        w, loss, g, norm = step(w, C, xs[idx], ys[idx],
                                torch.as_tensor(m2).to(dtype),
                                torch.as_tensor(m3).to(dtype),
                                p1, p2, max_norm, lr)
        loss_sum += loss
        stats[0] += g.sum()
        stats[1] += (g * g).sum()
        norms.append(norm)
    return {"w": w, "loss": loss_sum, "stats": stats, "norms": norms,
            "grad": g}


def seg_rel_err(got, want, C):
    """Per-segment relative L2 error ``||got - want|| / ||want||`` of two
    flat arena vectors, as {name: float}; ``want`` is float64."""
    out = {}
    got = got.detach().cpu().to(torch.float64)
    for name, off, n in segments(C):
        d = (got[off:off + n] - want[off:off + n]).norm()
        out[name] = float(d / want[off:off + n].norm())
    return out


def rel_err(got, want):
    """Relative error of a scalar against its float64 reference."""
    got, want = float(got), float(want)
    return abs(got - want) / abs(want)
