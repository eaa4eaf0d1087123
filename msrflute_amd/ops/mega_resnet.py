"""Cross-client MEGA round for the fed-CIFAR100 ResNet-18 (BASELINE
benchmark task 3).

The per-client path runs ~22 small MIOpen convs per batch per client —
measured 8.1x slower than ONE grouped conv covering all K clients
(tools/diag_grouped_conv.py): per-op dispatch plus grids that underfill
the 256-CU chip.  Here all K sampled clients train together:

* one [K, P] parameter stack (single autograd leaf; per-client weights
  are strided views) driven by the scaffold the Shakespeare mega round
  uses (ops/mega_round.GraphedMegaRound);
* batched compute: the super-batch is [bs, K*C, H, W] (client k owns
  channel block k) and every conv is ONE F.conv2d with groups=K over
  the K-stacked filters; normalization is GroupNorm (the benchmark
  config trains with group_norm=2), which is per-sample — so stacked
  channels keep EXACT per-client semantics with no cross-client or
  cross-batch stat pollution and no running buffers;
* per-client clip + sufficient stats + SGD and the weighted pseudo-grad
  accumulate reuse the generic K-stacked kernels (_C.mega_clip_sgd /
  _C.mega_pseudo_accum, csrc/fused_cnn.hip);
* the WHOLE local epoch is captured as one hipGraph, captured on the
  first round's REAL gather indices (capture-safety lesson from the
  Shakespeare round: degenerate capture data can bake value-dependent
  kernel choices that fault on replay);
* ragged epochs are masked by labels: inactive rows get y = -100
  (CrossEntropyLoss's default ignore_index), and since conv/GroupNorm/
  pool are all per-sample, inactive rows contribute exactly zero
  gradients — finished clients' SGD no-ops.

Only conv algorithm selection (grouped vs per-client) and float
accumulation orders differ from the per-client path.
"""

from __future__ import annotations

from typing import Optional

import torch
import torch.nn.functional as F

from .arena import ParameterArena
from .mega_round import GraphedMegaRound

_PLANES = (64, 128, 256, 512)


def _expected_names():
    names = ["net.conv1.weight", "net.n1.weight", "net.n1.bias"]
    for li in range(1, 5):
        for bi in range(2):
            p = f"net.layer{li}.{bi}."
            names += [p + "conv1.weight", p + "n1.weight", p + "n1.bias",
                      p + "conv2.weight", p + "n2.weight", p + "n2.bias"]
            if li > 1 and bi == 0:
                names += [p + "down.0.weight", p + "down.1.weight",
                          p + "down.1.bias"]
    return names + ["net.fc.weight", "net.fc.bias"]


def matches_resnet18(arena: ParameterArena) -> Optional[int]:
    """Return num_classes when the arena is the fed-CIFAR100 ResNet-18
    (2-2-2-2 BasicBlocks, 7x7 stem), else None."""
    if arena.names != _expected_names():
        return None
    if tuple(arena.shapes[0]) != (64, 3, 7, 7):
        return None
    fc = arena.shapes[-2]
    if len(fc) != 2 or fc[1] != 512:
        return None
    return int(fc[0])


class ResNetMegaRound(GraphedMegaRound):
    PAD_LABEL = -100  # CrossEntropyLoss's default ignore_index
    X_DIM = 4         # store.x is [N, C, H, W] images
    EAGER_ENV = "MEGA_RESNET_EAGER"

    def __init__(self, arena: ParameterArena, bs: int, max_grad_norm,
                 cpg: int, k_cap: int = 32, mu: float = 0.0, dga=None):
        assert cpg > 0
        super().__init__(arena, bs, max_grad_norm, k_cap, mu=mu, dga=dga)
        self.cpg = int(cpg)
        nc = matches_resnet18(arena)
        assert nc is not None
        self.NC = nc

    def _graph_key(self, K, steps, store):
        return (K, steps, self.bs)

    def _forward(self, v, x, K):
        """Grouped functional ResNet-18 over the K-stacked views;
        x [bs, K*3, H, W] -> logits [K, bs, NC]."""
        cpg = self.cpg

        def conv(h, name, stride, pad):
            w = v[name]
            return F.conv2d(h, w.reshape(-1, *w.shape[2:]), None, stride,
                            pad, 1, K)

        def gn(h, p):
            w, b = v[p + "weight"], v[p + "bias"]
            C = w.shape[1]
            return F.group_norm(h, K * max(1, C // cpg), w.reshape(-1),
                                b.reshape(-1), 1e-5)

        h = F.max_pool2d(
            F.relu(gn(conv(x, "net.conv1.weight", 2, 3), "net.n1.")), 3, 2, 1)
        for li in range(1, 5):
            for bi in range(2):
                p = f"net.layer{li}.{bi}."
                stride = 2 if (li > 1 and bi == 0) else 1
                out = F.relu(gn(conv(h, p + "conv1.weight", stride, 1),
                                p + "n1."))
                out = gn(conv(out, p + "conv2.weight", 1, 1), p + "n2.")
                if p + "down.0.weight" in v:
                    sc = gn(conv(h, p + "down.0.weight", stride, 0),
                            p + "down.1.")
                else:
                    sc = h
                h = F.relu(out + sc)
        bs = x.shape[0]
        z = F.adaptive_avg_pool2d(h, 1).reshape(bs, K, -1).permute(1, 0, 2)
        return torch.baddbmm(v["net.fc.bias"].unsqueeze(1), z,
                             v["net.fc.weight"].transpose(1, 2))

    def _step(self, flat, x, y, K, loss_dev):
        """x [bs, K*3, H, W]; y [K*bs] long with -100 on inactive rows
        (client-major).  Per-client loss = mean CE over its active rows
        (the per-client path's CrossEntropyLoss batch mean)."""
        bs = self.bs
        logits = self._forward(self._views(flat), x, K)
        ce = F.cross_entropy(logits.reshape(K * bs, self.NC), y,
                             reduction="none",
                             ignore_index=self.PAD_LABEL).view(K, bs)
        n_act = (y.view(K, bs) != self.PAD_LABEL).sum(dim=1).clamp_min(1)
        loss_k = ce.sum(dim=1) / n_act
        loss_dev += loss_k.detach()
        return loss_k.sum()

    def _gather(self, x_all, y_all, idx, mask):
        bs = self.bs
        K = idx.numel() // bs
        C, H, W = x_all.shape[1:]
        # [K*bs, C, H, W] client-major -> [bs, K*C, H, W]
        x = x_all.index_select(0, idx).view(K, bs, C, H, W) \
            .transpose(0, 1).reshape(bs, K * C, H, W)
        y = torch.where(mask, y_all.index_select(0, idx).long(),
                        torch.full((1,), self.PAD_LABEL, dtype=torch.int64,
                                   device=idx.device))
        return x, y

    def _before_capture(self):
        # exhaustive MIOpen find during warmup: grouped-conv algorithms
        # from immediate mode are fallbacks; the capture then bakes the
        # found kernels (find cost is paid once, outside the hot loop)
        torch.backends.cudnn.benchmark = True
