"""Shared scaffold of the cross-client MEGA rounds.

Every whole-round driver (the CNN kernel rounds in ops/fused_cnn.py and
core/client.py, and the two autograd rounds built on
``GraphedMegaRound``) plans a round and reports its results through the
two pure helpers here, so the shuffle-order discipline and the
lazy-stats contract each live in ONE place:

* ``plan_round``: shard lookup and eligibility (``lookup_round``, usable
  alone to validate a round without drawing) and each client's shuffle
  order — the seed's FIRST ``randperm``, the same draw the eager
  dataloader makes (tests/test_kernel_contracts_cpu.py);
* ``round_outputs``: the per-client result dicts whose ``_lazy`` triple
  the server finalizes after the round's single sync.

``GraphedMegaRound`` is the autograd flavour (Shakespeare char-LSTM,
fed-CIFAR100 ResNet-18): all K sampled clients train together on one
flat [K, P] parameter stack (a single autograd leaf; per-client weights
are strided views, so autograd accumulates a [K, P] gradient stack), the
per-client clip + sufficient stats + SGD and the weighted pseudo-gradient
accumulate are the K-stacked kernels of csrc/fused_cnn.hip, and the WHOLE
local epoch is captured as one hipGraph per shape.  Ragged epochs are
masked by labels: inactive rows get ``PAD_LABEL`` (the loss's
ignore_index), so they contribute exactly zero loss and gradient and a
finished client's SGD no-ops.  With ``mu > 0`` (FedProx) the clip kernels
add ``mu (w - w_server)`` to the gradient of the clients ACTIVE at a step
(any unmasked row) and the regulariser to their loss; a finished client,
whose weights have left the server's, gets neither and stays put.

With a ``DGASpec`` the round ends in the DGA tail (``_C.mega_dga_accum``,
or the same kernels inside ``_C.cnn_round_mega``): the softmax
aggregation weight and the clip-only local-DP rescale are formed on the
device from the loss and stats the round already holds, and the drivers
report the weights through one [K] read per round.
"""

from __future__ import annotations

import os
import time
from typing import Dict, NamedTuple, Optional, Tuple

import torch

from . import HAS_EXT, _C
from .arena import ParameterArena


# weight sources of the DGA tail -> DgaMode of csrc/launchers.h
# (== _C.DGA_MODES); "mean" is aggregate_median: mean, the rest are
# server_config.weight_train_loss under aggregate_median: softmax
DGA_MODES = {"mean": 0, "train_loss": 1, "mag_var_loss": 2,
             "mag_mean_loss": 3, "mag": 4}


class DGASpec(NamedTuple):
    """What the DGA tail needs (core.client.fused_round_dga builds it)."""
    source: str            # a key of DGA_MODES
    beta: float            # softmax_beta
    clip: bool = False     # local DP, clip-only mode
    max_grad: float = 0.0  # dp_config.max_grad

    def kwargs(self, dga_out=None):
        """The DGA argument group of the bindings."""
        kw = dict(dga_mode=DGA_MODES[self.source], dga_beta=float(self.beta),
                  dga_clip=bool(self.clip),
                  dga_max_grad=float(self.max_grad))
        if dga_out is not None:
            kw["dga_out"] = dga_out
        return kw


def lookup_round(store, user_list, client_ids, desired_max_samples=None):
    """Look the round's clients up in the device shard store.  Returns
    ``(counts, row_lo)`` — per client its sample count and first store
    row — or None when a client is unknown to the store, has no rows, or
    has more than ``desired_max_samples`` (the eager path would truncate
    its epoch there).  Touches no RNG."""
    counts, row_lo = [], []
    for cid in client_ids:
        i = store.user_pos.get(user_list[cid])
        if i is None:
            return None
        lo, hi = store.offsets[i], store.offsets[i + 1]
        n = int(hi - lo)
        if n == 0 or (desired_max_samples is not None
                      and n > desired_max_samples):
            return None
        counts.append(n)
        row_lo.append(int(lo))
    return counts, row_lo


def plan_round(store, user_list, client_ids, seeds,
               desired_max_samples=None):
    """``lookup_round`` plus each client's shuffle order.  Returns
    ``(counts, row_lo, orders)`` with ``orders[k] = randperm(counts[k])``
    drawn in client order, or None — WITHOUT any draw — when the lookup
    rejects the round."""
    found = lookup_round(store, user_list, client_ids, desired_max_samples)
    if found is None:
        return None
    counts, row_lo = found
    orders = []
    for n, seed in zip(counts, seeds):
        torch.manual_seed(seed & 0x7FFFFFFFFFFF)
        orders.append(torch.randperm(n))
    return counts, row_lo, orders


def batch_indices(counts, row_lo, orders, bs):
    """Lay a plan out as per-step gather indices: ``idx[t, k*bs + j]`` is
    the store row of client k's j-th sample of batch t, ``mask`` marks
    the slots that hold one (a client's last batch may be short, and a
    client with fewer batches than the longest idles)."""
    K = len(counts)
    steps = max((c + bs - 1) // bs for c in counts)
    idx = torch.zeros(steps, K * bs, dtype=torch.int64)
    mask = torch.zeros(steps, K * bs, dtype=torch.bool)
    for k, order in enumerate(orders):
        rows = order + row_lo[k]
        for t in range((counts[k] + bs - 1) // bs):
            chunk = rows[t * bs:(t + 1) * bs]
            idx[t, k * bs:k * bs + len(chunk)] = chunk
            mask[t, k * bs:k * bs + len(chunk)] = True
    return idx, mask


def round_outputs(client_ids, counts, bs, loss_dev, stats_dev, arena_total,
                  weights=None):
    """Per-client result dicts of a whole-round driver.  Loss and
    sufficient stats stay on the device: ``_lazy`` = (client k's summed
    batch loss, its {sum, sumsq} slice, number of gradient elements the
    stats cover).  ``weights``: the aggregation weights (host floats) when
    they are not the sample counts (DGA)."""
    now = time.time()
    if weights is None:
        weights = [float(c) for c in counts]
    outputs = []
    for k, cid in enumerate(client_ids):
        nb = (counts[k] + bs - 1) // bs
        outputs.append((cid, {
            "cs": {"setup": 0.0, "training": 0.0, "full cost": 0.0,
                   "dataloader": 0.0},
            "ns": counts[k],
            "pl": {"weight": float(weights[k]), "grad": None,
                   "pooled": True},
            "_lazy": (loss_dev[k].reshape(()),
                      stats_dev[2 * k:2 * k + 2],
                      nb * arena_total),
            "ts": now,
        }))
    return outputs


class GraphedMegaRound:
    """Base of the autograd mega rounds.  A subclass supplies the model:
    ``_step`` (forward + per-client loss), ``_gather`` (one step's batch
    in the layout the model wants), ``_graph_key``, and the class
    attributes below; optionally ``_after_backward`` / ``_before_capture``."""

    PAD_LABEL: int    # label of inactive rows == the loss's ignore_index
    X_DIM: int        # store.x.dim() of this task's shard store
    EAGER_ENV: str    # set to "1": run the epoch eagerly, never capture

    def __init__(self, arena: ParameterArena, bs: int, max_grad_norm,
                 k_cap: int = 32, mu: float = 0.0,
                 dga: Optional[DGASpec] = None):
        assert HAS_EXT and arena.device.type == "cuda"
        self.arena = arena
        self.bs = int(bs)
        # fixed per instance: the captured graphs bake them in
        self.mu = float(mu)
        self.dga = dga
        self.calls = 0  # rounds this driver ran
        self.max_norm = float(max_grad_norm) if max_grad_norm else -1.0
        self.k_cap = int(k_cap)
        self.lr_t = torch.zeros(1, dtype=torch.float32, device=arena.device)
        self._server_data = None
        self._graphs: Dict[Tuple, dict] = {}

    def supports(self, K: int) -> bool:
        return 0 < K <= self.k_cap

    def _views(self, flat):
        """Per-parameter [K, *shape] strided views into the [K, P] stack."""
        a = self.arena
        return {n: flat[:, off:off + cnt].view(-1, *a.shapes[i])
                for i, (n, off, cnt) in enumerate(
                    zip(a.names, a.offsets, a.numels))}

    # -- subclass hooks ------------------------------------------------
    def _step(self, flat, x, y, K, loss_dev):
        """Forward + loss of one batched step; adds the per-client losses
        into ``loss_dev`` and returns their sum (autograd does the
        backward)."""
        raise NotImplementedError

    def _gather(self, x_all, y_all, idx, mask):
        """The step's ``(x, y)`` for ``_step``: rows ``idx`` of the store,
        labels of ``~mask`` slots replaced by ``PAD_LABEL``."""
        raise NotImplementedError

    def _graph_key(self, K, steps, store):
        raise NotImplementedError

    def _after_backward(self, grad):
        """Fix up the [K, P] gradient stack before the clip norm sees it."""

    def _before_capture(self):
        """Runs once per shape, before the warm-up."""

    # ------------------------------------------------------------------
    def _alloc(self, K, steps, store):
        dev = self.arena.device
        P = self.arena.total
        R = K * self.bs
        g = {
            "flat": torch.zeros(K, P, device=dev, requires_grad=True),
            "idx": torch.zeros(steps, R, dtype=torch.int64, device=dev),
            "ymask": torch.zeros(steps, R, dtype=torch.bool, device=dev),
            # FedProx: client k is active at step t (has an unmasked row)
            "active": torch.zeros(steps, K, dtype=torch.bool, device=dev),
            "loss_dev": torch.zeros(K, device=dev),
            "stats_out": torch.zeros(2 * K, device=dev),
            "acc2k": torch.zeros(3 * K, dtype=torch.float64, device=dev),
            "weights": torch.zeros(K, device=dev),
            # DGA tail: sample counts in, {weight, norm, c, scratch} out
            "counts": torch.zeros(K, dtype=torch.int64, device=dev),
            "dga_out": torch.zeros(4 * K, dtype=torch.float64, device=dev),
            "accum": torch.zeros(P, device=dev),
            "graph": None,
            "captured": False,
        }
        x_all, y_all = store.x, store.y
        server = self._server_data
        mu = self.mu
        dga = self.dga

        def epoch_body():
            flat = g["flat"]
            flat.data.copy_(server.unsqueeze(0).expand(K, P))
            g["loss_dev"].zero_()
            for t in range(steps):
                x, y = self._gather(x_all, y_all, g["idx"][t],
                                    g["ymask"][t])
                if flat.grad is not None:
                    flat.grad.zero_()
                loss = self._step(flat, x, y, K, g["loss_dev"])
                loss.backward()
                self._after_backward(flat.grad)
                # mu == 0 ignores the FedProx arguments (plain clip + SGD)
                _C.mega_clip_sgd(flat.data.reshape(-1),
                                 flat.grad.reshape(-1), K, g["acc2k"],
                                 self.max_norm, self.lr_t, g["stats_out"],
                                 server=server, mu=mu, active=g["active"][t],
                                 loss_out=g["loss_dev"])
            if dga is not None:
                _C.mega_dga_accum(flat.data.reshape(-1), server, K,
                                  g["loss_dev"], g["stats_out"], g["counts"],
                                  self.bs, accum=g["accum"],
                                  **dga.kwargs(g["dga_out"]))
                return
            _C.mega_pseudo_accum(flat.grad.reshape(-1), server,
                                 flat.data.reshape(-1), g["weights"],
                                 g["accum"])

        g["body"] = epoch_body
        # the compute reads these tensors by baked pointer: pin lifetime
        g["_pins"] = (x_all, y_all, server)
        return g

    def _capture(self, g):
        """Warm up + capture the epoch.  MUST run after the round's real
        idx/ymask/lr are staged: capturing on degenerate data risks
        value-dependent kernel selection that faults on replay."""
        self._before_capture()
        if os.environ.get(self.EAGER_ENV) == "1":
            return
        # warmup (establishes flat.grad + autograd buffers), then capture;
        # nothing here writes the server arena (flat is the working copy)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):
                g["body"]()
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g["body"]()
        g["graph"] = graph
        torch.cuda.synchronize()

    def run(self, store, ds, client_ids, seeds, initial_lr: float,
            server_arena: ParameterArena, round_accum: torch.Tensor,
            desired_max_samples=None):
        """Train all of the round's clients; returns the per-client
        outputs list [(cid, meta), ...], or None (nothing touched) when
        the round is not eligible."""
        K = len(client_ids)
        if not self.supports(K) or store.x.dim() != self.X_DIM:
            return None
        plan = plan_round(store, ds.user_list, client_ids, seeds,
                          desired_max_samples)
        if plan is None:
            return None
        counts = plan[0]
        if self._server_data is None:
            self._server_data = server_arena.data
        # the captured graphs bake this pointer in
        assert self._server_data is server_arena.data
        bs = self.bs
        idx, mask = batch_indices(*plan, bs)
        steps = idx.shape[0]
        key = self._graph_key(K, steps, store)
        if key not in self._graphs:
            self._graphs[key] = self._alloc(K, steps, store)
        g = self._graphs[key]

        g["idx"].copy_(idx)
        g["ymask"].copy_(mask)
        g["active"].copy_(mask.view(steps, K, bs).any(dim=2))
        g["weights"].copy_(torch.tensor([float(c) for c in counts]))
        g["counts"].copy_(torch.tensor(counts, dtype=torch.int64))
        self.lr_t.fill_(float(initial_lr))
        if not g["captured"]:
            # first use of this shape: capture on THIS round's real data
            self._capture(g)
            g["captured"] = True
        # warmup/capture side effects land in these accumulators: zero
        # them after capture, before the replay that counts
        g["stats_out"].zero_()
        g["accum"].zero_()
        if g["graph"] is None:
            g["body"]()
        else:
            g["graph"].replay()
        # fold the epoch's accumulated weighted pseudo-gradients
        round_accum += g["accum"]
        self.calls += 1
        weights = None
        if self.dga is not None:
            # the round's one [K] read, after its launches are queued
            weights = g["dga_out"][:K].tolist()
        return round_outputs(client_ids, counts, bs, g["loss_dev"],
                             g["stats_out"], self.arena.total, weights)
