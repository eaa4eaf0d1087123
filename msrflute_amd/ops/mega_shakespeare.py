"""Cross-client MEGA round for the Shakespeare char-LSTM (BASELINE
benchmark task 4).

The per-client path runs each client's epoch on its own stream;
concurrent recurrence kernels co-schedule only ~2.5x on this stack
(tools/diag_streams.py), which left Shakespeare at ~7 rounds/s.  Here
ALL K sampled clients train together with K-stacked per-client weights:

* one flat [K, P] parameter stack (leaf tensor); every per-client weight
  is a strided view into it, so autograd accumulates a [K, P] gradient
  stack and the per-client clip + sufficient-stats + SGD is the SAME
  gfx950 kernel suite as the CNN mega round (_C.mega_clip_sgd);
* batched compute: per-client embedding via one offset index_select
  (value-independent backward — capture-safe), input/output projections
  via torch.bmm over the K-stacked weights (hipBLASLt batched GEMMs),
  and the T-step recurrences via the K-stacked recurrence kernels
  (_C.lstm_seq_fwd/_bwd — grid = all K*bs rows, each block indexing
  its client's float4-packed W_hh; the per-client FusedLSTM runs the
  same kernels at K = 1);
* the WHOLE local epoch (all batch-steps, forward + autograd backward +
  clip/SGD) is captured as ONE hipGraph keyed by (K, steps, bs, T):
  per round the host refreshes the static gather-index/label buffers
  and replays;
* ragged epochs are masked by labels: inactive rows get pad labels
  (ignore_index 0), so their CE contributions AND gradients are exactly
  zero — finished clients' SGD no-ops (the CNN mega round's trick).

``use_bf16`` (``client_config.mixed_precision: bf16``) switches both
recurrences to bf16-stored W_hh, as the per-client FusedLSTM does under
the same flag.

Per-client numerics match the per-client FusedLSTM path: same recurrence
kernel math, same per-batch mean-CE loss, same clip-then-SGD semantics;
only GEMM scheduling (bmm vs mm) and float accumulation orders differ.
The round scaffold (stack, capture, replay, outputs) is
ops/mega_round.GraphedMegaRound.
"""

from __future__ import annotations

from typing import Optional, Tuple

import torch
import torch.nn.functional as F

from .arena import ParameterArena
from .lstm import _LSTMSeq
from .mega_round import GraphedMegaRound

H = 256
# expected arena layout of the Shakespeare model
# (experiments/nlp_rnn_fedshakespeare/model.py)
_NAMES = ["net.embeddings.weight", "net.lstm.weight_ih_l0",
          "net.lstm.weight_hh_l0", "net.lstm.bias_ih_l0",
          "net.lstm.bias_hh_l0", "net.lstm.weight_ih_l1",
          "net.lstm.weight_hh_l1", "net.lstm.bias_ih_l1",
          "net.lstm.bias_hh_l1", "net.fc.weight", "net.fc.bias"]


def matches_char_lstm(arena: ParameterArena) -> Optional[Tuple[int, int]]:
    """Return (vocab, embed_dim) when the arena is the Shakespeare
    2-layer H=256 char LSTM, else None."""
    if arena.names != _NAMES:
        return None
    V, E = arena.shapes[0]
    if (tuple(arena.shapes[1]) != (4 * H, E)
            or tuple(arena.shapes[2]) != (4 * H, H)
            or tuple(arena.shapes[5]) != (4 * H, H)
            or tuple(arena.shapes[9]) != (V, H)):
        return None
    return int(V), int(E)


class ShakespeareMegaRound(GraphedMegaRound):
    PAD_LABEL = 0     # the model's CE ignore_index (the pad token)
    X_DIM = 2         # store.x is [N, T] token ids
    EAGER_ENV = "MEGA_SHK_EAGER"

    def __init__(self, arena: ParameterArena, bs: int,
                 max_grad_norm, k_cap: int = 32, use_bf16: bool = False,
                 mu: float = 0.0, dga=None):
        super().__init__(arena, bs, max_grad_norm, k_cap, mu=mu, dga=dga)
        vc = matches_char_lstm(arena)
        assert vc is not None
        self.V, self.E = vc
        # bf16-stored recurrent weights in both layers' recurrences
        # (ops/lstm._LSTMSeq); everything else in the round stays fp32
        self.use_bf16 = bool(use_bf16)

    def _graph_key(self, K, steps, store):
        return (K, steps, self.bs, store.x.shape[1], self.use_bf16)

    def _step(self, flat, x, y, K, loss_dev):
        """One batched training step's forward + loss (autograd does the
        backward); x [R, T] long, y [R, T] long (pad 0 masks)."""
        bs, V, E = self.bs, self.V, self.E
        R, T = x.shape
        v = self._views(flat)
        # per-client embedding: offset rows into the stacked table.
        # index_select, NOT F.embedding: embedding_dense_backward's
        # implementation is index-value-dependent, which is unsafe under
        # hipGraph capture (captured on round-1 data, replayed on other
        # rounds'); index_select's backward is a plain index_add with
        # value-independent kernels
        offs = (torch.arange(K, device=x.device) * V).repeat_interleave(bs)
        e = v["net.embeddings.weight"].reshape(K * V, E).index_select(
            0, (x + offs[:, None]).view(-1))
        e = e.view(K, bs * T, E)
        b0 = (v["net.lstm.bias_ih_l0"] + v["net.lstm.bias_hh_l0"])
        xp0 = torch.baddbmm(b0.unsqueeze(1), e,
                            v["net.lstm.weight_ih_l0"].transpose(1, 2))
        h0 = _LSTMSeq.apply(xp0.view(R, T, 4 * H),
                            v["net.lstm.weight_hh_l0"], bs, self.use_bf16)
        b1 = (v["net.lstm.bias_ih_l1"] + v["net.lstm.bias_hh_l1"])
        xp1 = torch.baddbmm(b1.unsqueeze(1), h0.view(K, bs * T, H),
                            v["net.lstm.weight_ih_l1"].transpose(1, 2))
        h1 = _LSTMSeq.apply(xp1.view(R, T, 4 * H),
                            v["net.lstm.weight_hh_l1"], bs, self.use_bf16)
        logits = torch.baddbmm(v["net.fc.bias"].unsqueeze(1),
                               h1.view(K, bs * T, H),
                               v["net.fc.weight"].transpose(1, 2))
        ce = F.cross_entropy(logits.reshape(-1, V), y.reshape(-1),
                             ignore_index=self.PAD_LABEL,
                             reduction="none").view(K, -1)
        n_tok = (y.view(K, -1) != self.PAD_LABEL).sum(dim=1).clamp_min(1)
        loss_k = ce.sum(dim=1) / n_tok
        loss_dev += loss_k.detach()
        return loss_k.sum()

    def _gather(self, x_all, y_all, idx, mask):
        x = x_all.index_select(0, idx).long()
        y = torch.where(mask.unsqueeze(-1),
                        y_all.index_select(0, idx).long(),
                        torch.full((1,), self.PAD_LABEL, dtype=torch.int64,
                                   device=idx.device))
        return x, y

    def _after_backward(self, grad):
        # nn.Embedding(padding_idx=0) never accumulates into the pad
        # row; the stacked index_select has no per-client padding_idx,
        # so zero those rows before the clip norm sees them
        V, E = self.V, self.E
        off = self.arena.offsets[0]  # net.embeddings.weight
        grad[:, off:off + V * E].view(-1, V, E)[:, 0, :].zero_()
