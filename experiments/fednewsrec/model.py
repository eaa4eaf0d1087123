"""fednewsrec task: attention-based news recommendation (FedNewsRec).

Reference: experiments/fednewsrec/fednewsrec_model.py (hand-rolled
multi-head attention via einsum, DocEncoder conv+attention+attentive
pooling, UserEncoder attention + GRU-tail fusion, frozen pretrained
embeddings) and model.py:47-129 (AUC/MRR/nDCG metrics).

MI355X-native divergences: multi-head attention uses
``F.scaled_dot_product_attention`` instead of 4 einsum kernels;
``model_config.fused_attention: true`` runs it as ``fused_mha``
(csrc/mha_small.hip: one launch forward and one backward on the projection
GEMMs' own [B, L, heads*d] layout; L <= 64, d <= 32, float32 on the GPU).
``model_config.fused_attention: mfma`` runs it as ``fused_mha(...,
impl="mfma")`` (csrc/mha_mfma.hip: the same range and layout, one wave per
(sequence, head) on the fp32 MFMA, nothing saved but q, k, v).
Both are off by default: ``mha_small`` is not faster than SDPA at the task's
shapes (PERF.md, "Short-sequence attention"); for the MFMA pair see PERF.md,
"Short-sequence attention on the MFMA".
``model_config.fused_pooling: true`` runs the three attentive poolings as
``fused_attentive_pool`` (csrc/attn_pool.hip: one launch forward and one
backward on the fp32 MFMA; L <= 64, D <= 512, hidden <= 256, float32 on the
GPU); off by default (PERF.md, "Attentive pooling").
``model_config.fused_conv: true`` runs the title convolution and its ReLU as
``fused_conv1d_relu`` (csrc/conv1d_seq.hip: one launch forward on the fp32
MFMA, on [B, T, E] rows as they are, no transposed views; backward, with the
embedding frozen, csrc/conv1d_bwd_w.hip's split-K weight-gradient kernel
and its fold, two launches and no library GEMM; T <= 64, channels <= 512,
kernel width <= 5, float32 on the GPU); off by default (PERF.md, "Title
convolution: backward-weights").  The embedding matrix is
random-init frozen
(no GloVe download offline — pass ``embedding_path`` to a local ``.npy``
to load real vectors); metrics are computed in torch (no sklearn/nltk);
the user encoder's GRU over the last 20 clicks is ``FusedGRU`` (H = 400:
the any-H fused recurrence, csrc/gru_seq_any.hip, one launch per
direction instead of MIOpen's per-step RNN path; same parameter names and
CPU results as ``nn.GRU``).

The task runs the eager epoch: its batches carry a (click, sample) tuple
under ``"x"``, so the trainer's probe in ``_run_train_epoch_graphed``
(``torch.is_tensor(probe.get("x"))``) turns graph capture off for it.
"""

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from msrflute_amd.core.model import BaseModel
from msrflute_amd.ops.attention import (fused_attentive_pool,
                                        fused_attentive_pool_available,
                                        fused_mha, fused_mha_available)
from msrflute_amd.ops.conv1d import (fused_conv1d_relu,
                                     fused_conv1d_relu_available)
from msrflute_amd.ops.lstm import FusedGRU
from msrflute_amd.utils import to_device

NPRATIO = 4


class AttentivePooling(nn.Module):
    """Additive attention pooling over a sequence (reference
    fednewsrec_model.py:12-42).  With ``fused`` set it is
    ``fused_attentive_pool`` on ``dense`` / ``dense2``'s own parameters where
    ``fused_attentive_pool_available`` says so; the dropout stays ahead of
    it."""

    def __init__(self, dim, hidden=200, dropout=0.2, fused=False):
        super().__init__()
        self.fused = fused
        self.drop = nn.Dropout(dropout)
        self.dense = nn.Linear(dim, hidden)
        self.dense2 = nn.Linear(hidden, 1)

    def forward(self, x):                     # [B, L, D] -> [B, D]
        x = self.drop(x)
        if self.fused and fused_attentive_pool_available(
                x.shape[1], x.shape[2], self.dense.out_features, x):
            return fused_attentive_pool(x, self.dense.weight, self.dense.bias,
                                        self.dense2.weight, self.dense2.bias)
        att = self.dense2(torch.tanh(self.dense(x))).squeeze(-1)
        att = torch.softmax(att, dim=1)
        return torch.einsum("bld,bl->bd", x, att)


class SelfAttention(nn.Module):
    """Multi-head self-attention via SDPA (reference Attention module,
    fednewsrec_model.py:44-106, was einsum-based).  With ``fused`` set it is
    ``fused_mha`` on the three projections where ``fused_mha_available``
    says so, and SDPA on head views otherwise; ``fused="mfma"`` selects
    ``impl="mfma"``, any other true value the default ``impl="lanes"``."""

    def __init__(self, dim, heads, head_dim, fused=False):
        super().__init__()
        self.fused = fused
        self.heads, self.head_dim = heads, head_dim
        out = heads * head_dim
        self.wq = nn.Linear(dim, out, bias=False)
        self.wk = nn.Linear(dim, out, bias=False)
        self.wv = nn.Linear(dim, out, bias=False)
        for w in (self.wq, self.wk, self.wv):
            nn.init.xavier_uniform_(w.weight, gain=np.sqrt(2))

    def forward(self, x):                     # [B, L, D] -> [B, L, H*Hd]
        B, L, _ = x.shape
        if self.fused and fused_mha_available(L, self.head_dim, x):
            return fused_mha(self.wq(x), self.wk(x), self.wv(x), self.heads,
                             impl="mfma" if self.fused == "mfma" else "lanes")
        q = self.wq(x).view(B, L, self.heads, self.head_dim).transpose(1, 2)
        k = self.wk(x).view(B, L, self.heads, self.head_dim).transpose(1, 2)
        v = self.wv(x).view(B, L, self.heads, self.head_dim).transpose(1, 2)
        o = F.scaled_dot_product_attention(q, k, v)
        return o.transpose(1, 2).reshape(B, L, -1)


class DocEncoder(nn.Module):
    """Title encoder: conv over words -> self-attn -> attentive pooling
    (reference fednewsrec_model.py:128-197).  With ``fused_conv`` set the
    conv and its ReLU are ``fused_conv1d_relu`` on ``conv``'s own parameters
    where ``fused_conv1d_relu_available`` says so; both dropouts stay torch
    ops around it."""

    def __init__(self, embed_dim=300, conv_dim=400, heads=20,
                 fused_conv=False):
        super().__init__()
        self.fused_conv = fused_conv
        self.drop1 = nn.Dropout(0.2)
        self.conv = nn.Conv1d(embed_dim, conv_dim, 3)
        self.drop2 = nn.Dropout(0.2)
        self.attn = SelfAttention(conv_dim, heads, conv_dim // heads)
        self.drop3 = nn.Dropout(0.2)
        self.pool = AttentivePooling(conv_dim)

    def forward(self, x):                     # [B, T, E] -> [B, D]
        x, conv = self.drop1(x), self.conv
        if self.fused_conv and fused_conv1d_relu_available(
                x.shape[1], conv.in_channels, conv.out_channels,
                conv.kernel_size[0], x):
            h = fused_conv1d_relu(x, conv.weight, conv.bias)
        else:
            h = F.relu(conv(x.transpose(1, 2)).transpose(1, 2))
        h = self.drop2(h)
        h = self.drop3(F.relu(self.attn(h)))
        return self.pool(h)


class UserEncoder(nn.Module):
    """User encoder: self-attn pooled vector fused with a GRU over the
    last 20 clicks via attentive pooling (reference
    fednewsrec_model.py:208-282)."""

    def __init__(self, dim=400, heads=20, tail=20):
        super().__init__()
        self.attn = SelfAttention(dim, heads, dim // heads)
        self.drop = nn.Dropout(0.2)
        self.pool_attn = AttentivePooling(dim)
        self.tail = tail
        self.gru = FusedGRU(dim, dim)
        self.pool_fuse = AttentivePooling(dim)

    def forward(self, news_vecs):             # [B, H, D] -> [B, D]
        v2 = self.pool_attn(self.drop(self.attn(news_vecs)))
        g, _ = self.gru(news_vecs[:, -self.tail:, :])
        v1 = g[:, -1, :]
        return self.pool_fuse(torch.stack([v1, v2], dim=1))


class FedNewsRecNet(nn.Module):
    def __init__(self, embedding_matrix, freeze_embeddings=True):
        super().__init__()
        self.embedding = nn.Embedding.from_pretrained(
            torch.as_tensor(embedding_matrix, dtype=torch.float32),
            freeze=freeze_embeddings)
        self.doc_encoder = DocEncoder(self.embedding.embedding_dim)
        self.user_encoder = UserEncoder()

    def news_encoder(self, titles):           # [.., T] ids -> [.., D]
        shape = titles.shape
        flat = titles.reshape(-1, shape[-1])
        vecs = self.doc_encoder(self.embedding(flat))
        return vecs.reshape(*shape[:-1], -1)

    def forward(self, click, sample):
        # click: [B, H, T]; sample: [B, 1+npratio, T]
        user_vec = self.user_encoder(self.news_encoder(click))
        cand_vecs = self.news_encoder(sample)
        scores = torch.einsum("bkd,bd->bk", cand_vecs, user_vec)
        return scores, user_vec


def auc_score(labels, scores):
    order = np.argsort(-scores)
    ranked = labels[order]
    n_pos, n_neg = ranked.sum(), len(ranked) - ranked.sum()
    if n_pos == 0 or n_neg == 0:
        return 0.5
    # rank-sum AUC
    ranks = np.empty(len(scores))
    ranks[np.argsort(scores)] = np.arange(1, len(scores) + 1)
    return (ranks[labels > 0].sum() - n_pos * (n_pos + 1) / 2) / (n_pos * n_neg)


def mrr_score(labels, scores):
    order = np.argsort(-scores)
    ranked = labels[order]
    rr = ranked / (np.arange(len(ranked)) + 1)
    return rr.sum() / max(ranked.sum(), 1)


def dcg_score(labels, scores, k):
    order = np.argsort(-scores)[:k]
    gains = (2 ** labels[order] - 1) / np.log2(np.arange(len(order)) + 2)
    return gains.sum()


def ndcg_score(labels, scores, k):
    ideal = dcg_score(labels, labels, k)
    return dcg_score(labels, scores, k) / ideal if ideal > 0 else 0.0


class FEDNEWS(BaseModel):
    def __init__(self, model_config):
        super().__init__()
        vocab = int(model_config.get("vocab_size", 5000))
        dim = int(model_config.get("embed_dim", 300))
        path = model_config.get("embedding_path")
        if path:
            matrix = np.load(path)
        else:
            rng = np.random.default_rng(1234)
            matrix = rng.standard_normal((vocab, dim)).astype(np.float32) * 0.1
            matrix[0] = 0.0
        self.net = FedNewsRecNet(matrix, freeze_embeddings=bool(
            model_config.get("freeze_embeddings", True)))
        for m in self.net.modules():
            if isinstance(m, SelfAttention):
                fused = model_config.get("fused_attention", False)
                m.fused = "mfma" if fused == "mfma" else bool(fused)
            if isinstance(m, AttentivePooling):
                m.fused = bool(model_config.get("fused_pooling", False))
            if isinstance(m, DocEncoder):
                m.fused_conv = bool(model_config.get("fused_conv", False))

    def loss(self, input):
        if not self.net.training:
            return torch.tensor(0.0)
        click, sample = input["x"]
        label = to_device(input["y"]).long()
        scores, _ = self.net(to_device(click).long(), to_device(sample).long())
        return F.cross_entropy(scores, label)

    def inference(self, input):
        click, cands = input["x"]
        labels = input["y"]  # [B, K] binary relevance
        click = to_device(click).long()
        cands = to_device(cands).long()
        scores, _ = self.net(click, cands)
        scores = scores.detach().cpu().numpy()
        labels = labels.cpu().numpy()
        aucs, mrrs, n5, n10 = [], [], [], []
        for i in range(len(scores)):
            aucs.append(auc_score(labels[i], scores[i]))
            mrrs.append(mrr_score(labels[i], scores[i]))
            n5.append(ndcg_score(labels[i], scores[i], 5))
            n10.append(ndcg_score(labels[i], scores[i], 10))
        bs = len(scores)
        return {
            "output": 0.0, "acc": float(np.mean(aucs)), "batch_size": bs,
            "mrr": {"value": float(np.mean(mrrs)), "higher_is_better": True},
            "ndcg@5": {"value": float(np.mean(n5)), "higher_is_better": True},
            "ndcg@10": {"value": float(np.mean(n10)),
                        "higher_is_better": True},
        }

    def set_eval(self):
        self.eval()
        self.net.eval()

    def set_train(self):
        self.train()
        self.net.train()
