"""Client logic (reference: core/client.py).

Two pieces:

* ``Client`` — the lightweight per-task handle (same constructor contract
  as the reference: client ids + config + send_gradients) with the shared
  train-dataset cache and the data-slicing helper;
* ``ClientExecutor`` — NEW: a per-rank persistent workspace holding ONE
  resident model replica + flat arena + fused optimizer that every local
  client reuses.  The reference pays per-client model construction,
  parameter copy via Python loops and a fresh optimizer object per client
  (client.py:280-344); here per-client setup is one flat arena copy (K13)
  plus an optimizer-state reset.
"""

from __future__ import annotations

import logging
import os
import time
from itertools import accumulate
from typing import Dict, Optional

import torch

from .. import ops
from ..models import make_model
from ..ops.arena import ParameterArena
from ..ops.fused_optim import make_arena_optimizer
from ..ops.mega_round import (DGASpec, lookup_round, plan_round,
                              round_outputs)
from ..strategies import select_strategy
from ..utils import (ScheduledSamplingScheduler, alpha_update, make_optimizer,
                     print_rank, to_device)
from ..utils.dataloaders_utils import get_dataset, make_train_dataloader
from .trainer import Trainer, set_component_wise_lr

# Worker-wide dataset cache (reference: client.py:45-47, 76-99)
train_dataset = None
trainset_unlab = None
trainset_unlab_rand = None


class Client:
    """Per-client handle (reference: core/client.py:49-124)."""

    def __init__(self, client_id, config, send_gradients):
        self.client_id = client_id
        self.config = config
        self.send_gradients = send_gradients

    def get_client_data(self, dataset=None):
        client_data = self.get_data(self.client_id, dataset)
        return self.client_id, client_data, self.config, self.send_gradients

    @staticmethod
    def get_train_dataset(data_path, client_train_config, task):
        """Load + cache the full train dataset once per worker
        (reference: client.py:76-99)."""
        global train_dataset, trainset_unlab, trainset_unlab_rand
        train_dataset = get_dataset(data_path, client_train_config, task, mode="train")
        if task == "semisupervision":
            trainset_unlab = get_dataset(data_path, client_train_config, task,
                                         mode="train", user_idx=-2)
            trainset_unlab_rand = get_dataset(data_path, client_train_config,
                                              task, mode="train", user_idx=-3)
        else:
            trainset_unlab = None
            trainset_unlab_rand = None
        return len(train_dataset.user_list)

    @staticmethod
    def get_data(clients, dataset):
        """Slice the cached dataset into one-or-more users' data blobs
        (reference: client.py:101-124)."""
        if dataset is None:
            datasets = ([train_dataset, trainset_unlab, trainset_unlab_rand]
                        if trainset_unlab is not None else [train_dataset])
        else:
            datasets = [dataset]
        data_with_labels = getattr(datasets[0], "user_data_label", None) is not None
        strcts = []
        for ds in datasets:
            s = {"users": [], "num_samples": [], "user_data": {}}
            if data_with_labels:
                s["user_data_label"] = {}
            for client in clients:
                user = ds.user_list[client]
                s["users"].append(user)
                s["num_samples"].append(ds.num_samples[client])
                s["user_data"][user] = ds.user_data[user]
                if data_with_labels:
                    s["user_data_label"][user] = ds.user_data_label[user]
            strcts.append(s)
        return strcts


class ClientExecutor:
    """Per-rank persistent client-training workspace."""

    def __init__(self, config, task, data_path, server_arena: ParameterArena,
                 model_path: Optional[str] = None):
        self.config = config
        self.task = task
        self.data_path = data_path
        self.server_arena = server_arena
        self.model_path = model_path or config.get("model_path")
        self.model_config = config["model_config"]
        self.client_config = config["client_config"]
        self.server_config = config["server_config"]

        # resident client model replica + arena
        self.model = make_model(self.model_config)
        self.arena = ParameterArena(self.model, bind_grads=True)
        if self.client_config.get("mixed_precision", "") == "bf16":
            # client training streams the LSTM recurrent weights as bf16
            # (fp32 masters and arithmetic; evaluation stays fp32)
            from ..ops.lstm import FusedLSTM
            for m in self.model.modules():
                if isinstance(m, FusedLSTM):
                    m.bf16_recurrent = True
        # reusable fused optimizer (reset per client)
        opt_cfg = dict(self.client_config["optimizer_config"])
        opt_cfg.setdefault("lr", self.server_config.get("initial_lr_client", 1.0))
        self._fused_opt = make_arena_optimizer(opt_cfg, self.arena)
        self._torch_opt_cfg = opt_cfg

        strategy_cls = select_strategy(config["strategy"])
        self.client_strategy = strategy_cls("client", config, self.model_path)
        self.send_dicts = self.server_config.get("send_dicts", False)
        self.perf_acc = {}  # cumulative phase timings (bench diagnostics)

        # Device-resident client shard cache (SURVEY.md §7.1 divergence 3):
        # a client's packed (x, y) tensors live in HBM after first use, so
        # repeat sampling of a client costs zero host->device traffic and
        # zero Dataset re-construction.  288 GB/GPU holds every reference
        # dataset's full shard set; budget-capped for safety.
        self._shard_cache: Dict[str, object] = {}
        self._shard_cache_bytes = 0
        self._shard_cache_budget = int(self.client_config.get(
            "shard_cache_gb", 64)) << 30
        self._shard_store = None       # whole-dataset device pack
        self._shard_store_tried = False

        # hipGraph fast path for the per-batch client step (ops/graphs.py);
        # enabled on GPU for plain-SGD clients unless disabled by config
        # Fully-fused hand-written kernel path for the flagship CNN
        # (ops/fused_cnn.py): engaged when the arena layout matches and the
        # client optimizer is plain SGD (momentum/wd 0).
        self.fused_cnn = None
        opt_c = dict(self.client_config["optimizer_config"])
        if (torch.cuda.is_available() and ops.HAS_EXT
                and self.client_config.get("use_fused_cnn", True)
                and opt_c.get("type", "sgd") == "sgd"
                and float(opt_c.get("momentum", 0.0)) == 0.0
                and float(opt_c.get("weight_decay", 0.0)) == 0.0):
            from ..ops.fused_cnn import FusedCNNEpoch, matches_cnn_femnist
            C = matches_cnn_femnist(self.arena)
            bs_cfg = int(self.client_config["data_config"]["train"]
                         .get("batch_size", 20))
            if C is not None and bs_cfg <= 32:
                drops = [m.p for m in self.model.modules()
                         if isinstance(m, torch.nn.Dropout)]
                self.fused_cnn = FusedCNNEpoch(
                    self.arena, C,
                    bs=int(self.client_config["data_config"]["train"]
                           .get("batch_size", 20)),
                    p1=drops[0] if len(drops) > 0 else 0.25,
                    p2=drops[1] if len(drops) > 1 else 0.5,
                    max_grad_norm=self.client_config["data_config"]["train"]
                    .get("max_grad_norm"),
                    use_bf16=self.client_config.get(
                        "mixed_precision", "") == "bf16")

        # MIOpen RNN kernels segfault under hipGraph capture (hipblaslt
        # assert -> SIGSEGV, observed with the fedshakespeare LSTM), so
        # models containing RNN modules always run the eager path.
        has_rnn = any(isinstance(m, torch.nn.RNNBase)
                      for m in self.model.modules())
        self.graph_cache = None
        if (torch.cuda.is_available() and not has_rnn
                and self.fused_cnn is None  # fused path supersedes graphs
                and self.client_config.get("use_hip_graphs", True)):
            from ..ops.graphs import GraphCache
            cache = GraphCache(
                self.model, self.arena,
                dict(self.client_config["optimizer_config"]),
                self.client_config["data_config"]["train"].get("max_grad_norm"))
            if cache.supports():
                self.graph_cache = cache

    # ------------------------------------------------------------------
    def _get_shard_store(self, data_config):
        """Lazily pack the whole train set into device HBM (one pinned H2D)
        when the task uses the generic array machinery; None otherwise."""
        if self._shard_store_tried:
            return self._shard_store
        self._shard_store_tried = True
        import msrflute_amd.core.client as client_mod
        from ..models import get_exp_dataloader
        from ..models.generic_data import ArrayDataLoader, DeviceShardStore
        ds = client_mod.train_dataset
        try:
            dl_cls = get_exp_dataloader(self.task) if self.task else None
        except Exception:
            dl_cls = None
        eligible = (
            ds is not None
            and getattr(ds, "user_data_label", None) is not None
            and dl_cls is not None and issubclass(dl_cls, ArrayDataLoader)
            and not getattr(ds, "_want_transform", False)
            and self.client_config.get("cache_client_shards", True))
        if eligible:
            try:
                x_shape = tuple(getattr(ds, "x_shape", None) or ())
                self._shard_store = DeviceShardStore(
                    ds, x_shape, device=self.arena.device,
                    budget_bytes=int(self.client_config.get(
                        "shard_cache_gb", 128)) << 30)
                print_rank(
                    f"packed {len(ds.user_list)} client shards into device "
                    f"memory ({self._shard_store.x.numel() * 4 >> 20} MiB)")
            except MemoryError as e:
                print_rank(f"shard store disabled: {e}")
        return self._shard_store

    def _make_optimizer(self, initial_lr):
        if self._fused_opt is not None:
            self._fused_opt.reset_state()
            if initial_lr > 0:
                self._fused_opt.param_groups[0]["lr"] = initial_lr
            return self._fused_opt
        cfg = dict(self._torch_opt_cfg)
        if initial_lr > 0:
            cfg["lr"] = initial_lr
        return make_optimizer(cfg, self.model)

    def process_round(self, client: Client, initial_lr: float, iteration: int,
                      round_seed: int = 0) -> Dict:
        """Run one client's local training (reference: client.py:226-511)."""
        config = self.config
        client_config = self.client_config
        data_config = client_config["data_config"]["train"]
        privacy_metrics_config = config.get("privacy_metrics_config", None)
        begin = time.time()
        client_stats = {}

        client_id, data_strcts, _, send_gradients = client.get_client_data()
        data_strct = data_strcts[0]
        user = data_strct["users"][0]

        # Per-client seed discipline: a client's
        # local-SGD trajectory (shuffle order, dropout) is a function of
        # (round, client) only — independent of which rank runs it — so the
        # aggregated round result is world-size-invariant up to fp
        # reduction order.
        torch.manual_seed(round_seed & 0x7FFFFFFFFFFF)

        t_dl = time.time()
        train_dataloader = self._shard_cache.get(user)
        if train_dataloader is None and torch.cuda.is_available():
            store = self._get_shard_store(data_config)
            if store is not None:
                train_dataloader = store.loader_for(
                    user, data_config.get("batch_size", 40))
                if train_dataloader is not None:
                    self._shard_cache[user] = train_dataloader
        if train_dataloader is None:
            train_dataloader = make_train_dataloader(
                data_config, self.data_path, task=self.task, clientx=0,
                data_strct=data_strct)
            if hasattr(train_dataloader, "to_device"):
                train_dataloader.to_device()
            if (torch.cuda.is_available()
                    and hasattr(train_dataloader, "dataset")
                    and getattr(train_dataloader.dataset, "x", None) is not None
                    and torch.is_tensor(train_dataloader.dataset.x)
                    and train_dataloader.dataset.x.is_cuda
                    and self._shard_cache_bytes < self._shard_cache_budget):
                ds = train_dataloader.dataset
                nbytes = ds.x.numel() * ds.x.element_size()
                if ds.y is not None and torch.is_tensor(ds.y):
                    nbytes += ds.y.numel() * ds.y.element_size()
                self._shard_cache[user] = train_dataloader
                self._shard_cache_bytes += nbytes
        client_stats["dataloader"] = time.time() - t_dl

        # one flat copy-in instead of the reference's per-tensor clone loop
        # (client.py:294-301, K13)
        self.arena.copy_data_(self.server_arena.data)
        self.arena.zero_grad()

        trainer_config = client_config.get("trainer_config", {})
        if "updatable_names" in trainer_config:
            set_component_wise_lr(self.model, client_config["optimizer_config"],
                                  trainer_config["updatable_names"])

        optimizer = self._make_optimizer(initial_lr)

        ss_scheduler = None
        if client_config.get("ss_config") is not None:
            ss_scheduler = ScheduledSamplingScheduler(model=self.model,
                                                      **client_config["ss_config"])

        trainer = Trainer(
            model=self.model,
            optimizer=optimizer,
            ss_scheduler=ss_scheduler,
            train_dataloader=train_dataloader,
            # graph path engaged inside run_train_epoch when applicable

            server_replay_config=client_config,
            max_grad_norm=data_config.get("max_grad_norm", None),
            anneal_config=client_config.get("annealing_config", None),
            num_skips_threshold=client_config.get("num_skips_threshold", -1),
            ignore_subtask=client_config["ignore_subtask"],
            arena=self.arena,
        )
        trainer.graph_cache = self.graph_cache
        trainer.fused_cnn = self.fused_cnn
        trainer.round_seed = round_seed & 0x7FFFFFFFFFFF

        desired_max_samples = data_config.get("desired_max_samples", None)
        apply_privacy_metrics = bool(privacy_metrics_config
                                     and privacy_metrics_config["apply_metrics"])
        # FedAvg weights are num_samples (host-known), so the per-client
        # loss/stats host syncs can be deferred and batched round-level
        trainer.lazy_stats = (
            config["strategy"] == "FedAvg" and not apply_privacy_metrics
            and self.arena.device.type == "cuda"
            and not getattr(self.client_strategy, "stats_on_smooth_grad", False)
            and self.server_config.get("type") != "personalization")

        client_stats["setup"] = time.time() - begin
        begin_training = time.time()

        self.model.train()

        algo_payload = None
        strategy_algo = config["strategy"]
        if strategy_algo == "FedLabels":
            datasets = [get_dataset(self.data_path, config, self.task,
                                    mode="train", test_only=False,
                                    data_strct=data_strcts[i], user_idx=0)
                        for i in range(3)]
            algo_payload = {"strategy": "FedLabels", "data": datasets,
                            "iter": iteration,
                            "config": client_config.get("semisupervision")}
        elif strategy_algo == "FedProx":
            algo_payload = {"strategy": "FedProx",
                            "mu": client_config.get("mu", 0.001)}

        train_loss, num_samples, algo_computation = trainer.train_desired_samples(
            desired_max_samples=desired_max_samples,
            apply_privacy_metrics=apply_privacy_metrics,
            algo_payload=algo_payload)

        trainer.train_loss = train_loss
        trainer.num_samples = num_samples
        trainer.algo_computation = algo_computation

        # pseudo-gradient g = w_server − w_trained (K1; reference client.py:380-383)
        if not self.send_dicts:
            ops.pseudo_grad(self.arena.grad, self.server_arena.data,
                            self.arena.data, 1.0)

        payload = self.client_strategy.generate_client_payload(trainer) \
            if send_gradients else None

        if self.server_config.get("type") == "personalization":
            self._personalization_round(client, data_strct, data_config,
                                        client_config, trainer, initial_lr,
                                        user, desired_max_samples)

        client_stats["training"] = time.time() - begin_training
        client_stats["full cost"] = time.time() - begin
        for k, v in client_stats.items():
            self.perf_acc[k] = self.perf_acc.get(k, 0.0) + v
        self.perf_acc["clients"] = self.perf_acc.get("clients", 0) + 1

        if train_loss is None and trainer.loss_dev is not None:
            # deferred host sync: the server finalizes these in one batch
            client_output = {
                "cs": client_stats, "ns": num_samples, "pl": payload,
                "_lazy": (trainer.loss_dev, trainer.stats_dev,
                          trainer.counter),
            }
        else:
            client_output = {
                "cs": client_stats,
                "tl": train_loss,
                "mg": trainer.sufficient_stats["mag"],
                "vg": trainer.sufficient_stats["var"],
                "ng": trainer.sufficient_stats["mean"],
                "rg": trainer.sufficient_stats["norm"],
                "ns": num_samples,
                "pl": payload,
            }

        if apply_privacy_metrics:
            self._apply_privacy_metrics(client_output, trainer,
                                        privacy_metrics_config)

        client_output["ts"] = time.time()
        return client_output

    # ------------------------------------------------------------------
    def _personalization_round(self, client, data_strct, data_config,
                               client_config, trainer, initial_lr, user,
                               desired_max_samples):
        """Per-user local model + convex-interpolation alpha update
        (reference: client.py:387-443)."""
        alpha = client_config.get("convex_model_interp", 0.75)
        local_model = make_model(self.config["model_config"])
        train_dataloader = make_train_dataloader(
            data_config, self.data_path, task=self.task, clientx=0,
            data_strct=data_strct)
        local_optimizer = make_optimizer(dict(client_config["optimizer_config"]),
                                         local_model)
        local_trainer = Trainer(
            model=local_model, optimizer=local_optimizer, ss_scheduler=None,
            train_dataloader=train_dataloader, server_replay_config=client_config,
            max_grad_norm=data_config.get("max_grad_norm", None),
            anneal_config=client_config.get("annealing_config", None),
            ignore_subtask=client_config["ignore_subtask"])

        local_model_name = os.path.join(self.model_path, f"{user}_model.tar")
        local_alpha_name = os.path.join(self.model_path, f"{user}_alpha")
        if os.path.exists(local_model_name):
            local_trainer.load(local_model_name, update_lr_scheduler=False,
                               update_ss_scheduler=False)
        if os.path.exists(local_alpha_name):
            alpha = torch.load(local_alpha_name, weights_only=False)

        original_local_model = local_trainer.get_model()
        local_model.train()
        train_loss, num_samples, _ = local_trainer.train_desired_samples(
            desired_max_samples=desired_max_samples, apply_privacy_metrics=False)
        print_rank(f"user {user}: LOCAL training loss={train_loss}",
                   loglevel=logging.DEBUG)
        local_trainer.save(model_path=self.model_path, config=self.config,
                           token=user)
        for p, orig in zip(local_trainer.model.parameters(),
                           original_local_model.parameters()):
            p.grad = to_device(orig.data) - p.data
        alpha = alpha_update(local_trainer.model, trainer.model, alpha, initial_lr)
        torch.save(alpha, local_alpha_name)

    # ------------------------------------------------------------------
    def _apply_privacy_metrics(self, client_output, trainer,
                               privacy_metrics_config):
        """Token-extraction + leakage attacks; may zero the client's weight
        (reference: client.py:466-508)."""
        from ..extensions.privacy import metrics as privacy_metrics

        privacy_stats = {"Dropped clients": 0}
        batches = trainer.cached_batches
        trainer.cached_batches = []
        gradients = self.arena.grad  # already flat

        if privacy_metrics_config.get("apply_indices_extraction", False):
            allowed_word_rank = privacy_metrics_config.get("allowed_word_rank", 9000)
            embed_dim = self.model_config["embed_dim"]
            vocab_size = self.model_config["vocab_size"]
            overlap, indices = privacy_metrics.extract_indices_from_embeddings(
                gradients, batches, embed_dim, vocab_size)
            max_overlap = privacy_metrics_config.get("max_allowed_overlap", None)
            if max_overlap is not None and overlap > max_overlap:
                print_rank(f"Removing client: extracted {overlap*100}% words, "
                           f"max allowed {max_overlap*100}%")
                client_output["wt"] = 0.0
                privacy_stats["Dropped clients"] = 1
            privacy_stats["Extracted indices percentage"] = overlap
            privacy_stats[f"Words percentage above {allowed_word_rank} word rank"] = \
                float((indices > allowed_word_rank).mean()) if len(indices) > 0 else 0

        if privacy_metrics_config.get("apply_leakage_metric", False):
            import numpy as np
            orig_params = {n: self.server_arena.data[
                self.server_arena.offsets[i]:self.server_arena.offsets[i]
                + self.server_arena.numels[i]].view(self.server_arena.shapes[i])
                for i, n in enumerate(self.server_arena.names)}
            # practical_epsilon_leakage needs a full state dict
            sd = {k: v.clone() for k, v in self.model.state_dict().items()}
            for n, p in orig_params.items():
                if n in sd:
                    sd[n] = p.clone()
            max_ratio = float(np.exp(privacy_metrics_config["max_leakage"]))
            leakage = privacy_metrics.practical_epsilon_leakage(
                sd, self.model, batches,
                privacy_metrics_config.get("is_leakage_weighted", False),
                max_ratio,
                privacy_metrics_config.get("attacker_optimizer_config"))
            max_leakage = privacy_metrics_config.get("max_allowed_leakage", None)
            if max_leakage is not None and leakage > max_leakage:
                print_rank(f"Removing client: leakage {leakage} > {max_leakage}")
                client_output["wt"] = 0.0
                privacy_stats["Dropped clients"] = 1
            privacy_stats["Practical epsilon (Max leakage)"] = leakage

        client_output["ps"] = privacy_stats

def convex_inference(model_global, model_personal, alpha):
    """Personalized logit interpolation accuracy
    (reference: utils/utils.py:598-603)."""
    import numpy as np
    targets = torch.tensor(model_global["labels"])
    probs = alpha * model_personal["probabilities"] + \
        (1 - alpha) * model_global["probabilities"]
    preds = torch.argmax(torch.tensor(np.asarray(probs)), dim=1)
    return torch.mean((preds == targets).float()).item()


class ClientPool:
    """P client executors on P HIP streams: clients within a round train
    CONCURRENTLY on the GPU (the round is a weighted sum — order-free).

    Each executor owns a model replica, arena, graph cache and a round
    accumulator; its stream serializes its own clients.  Weighted
    pseudo-gradients accumulate stream-locally; ``flush()`` joins the
    streams and adds the P accumulators into the server grad arena.  This
    is the MI355X-native replacement for the reference's process-per-GPU
    worker pool: concurrency lives on streams inside one
    rank instead of extra processes.
    """

    def __init__(self, config, task, data_path, server_arena, model_path=None,
                 n_parallel=4):
        self.server_arena = server_arena
        self.executors = [ClientExecutor(config, task, data_path,
                                         server_arena, model_path)
                          for _ in range(max(1, int(n_parallel)))]
        self.streams = [torch.cuda.Stream() for _ in self.executors]
        self.round_accums = [server_arena.new_buffer() for _ in self.executors]
        self._rr = 0
        self._streams_dirty = False
        # whole-round drivers, built on first use: None = not probed yet,
        # False = not this model (stop probing), else the driver
        self._mega = None          # ops.fused_cnn.MegaRound
        self._mega_lstm = None     # ops.mega_shakespeare.ShakespeareMegaRound
        self._mega_resnet = None   # ops.mega_resnet.ResNetMegaRound

    # properties the server reads off the executor
    @property
    def client_strategy(self):
        return self.executors[0].client_strategy

    @property
    def perf_acc(self):
        merged = {}
        for ex in self.executors:
            for k, v in ex.perf_acc.items():
                merged[k] = merged.get(k, 0) + v
        return merged

    def process_round(self, client, initial_lr, iteration, round_seed=0):
        k = self._rr % len(self.executors)
        self._rr += 1
        ex, st = self.executors[k], self.streams[k]
        # share the packed shard store across replicas (one copy in HBM)
        prim = self.executors[0]
        if ex is not prim and prim._shard_store_tried and not ex._shard_store_tried:
            ex._shard_store = prim._shard_store
            ex._shard_store_tried = True
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            out = ex.process_round(client, initial_lr, iteration, round_seed)
            payload = out.get("pl")
            if payload is not None and payload.get("grad") is not None \
                    and payload["weight"] != 0.0:
                ops.axpy(self.round_accums[k], payload["grad"], 1.0)
                payload["grad"] = None
                payload["pooled"] = True
        self._streams_dirty = True
        return out

    def flush(self, target_grad):
        """Join client streams and fold the P accumulators into the server
        grad arena.  Must run before the round's lazy-stats finalize."""
        if not self._streams_dirty:
            return
        cur = torch.cuda.current_stream()
        for st in self.streams:
            cur.wait_stream(st)
        for acc in self.round_accums:
            ops.axpy(target_grad, acc, 1.0)
            acc.zero_()
        self._streams_dirty = False

    # ------------------------------------------------------------------
    def run_fused_round_batch(self, client_ids, initial_lr, iteration,
                              seeds):
        """Train the round's clients with a whole-round driver, tried in
        order: Shakespeare mega round, ResNet mega round, CNN mega round,
        one _C.cnn_round per executor (on its stream) covering its chunk
        of the clients.  Returns outputs or None if no driver is eligible
        (caller falls back to the per-client path).  Eligibility is
        validated UP FRONT so no partial state is mutated on the
        fallback path."""
        prim = self.executors[0]
        cc = prim.client_config
        data_cfg = cc["data_config"]["train"]
        pm = prim.config.get("privacy_metrics_config", None)
        mu = fused_round_mu(prim.config["strategy"], cc, prim.model_config,
                            bool(pm and pm["apply_metrics"]))
        # DGA runs on the cross-client mega rounds only (its tail forms the
        # aggregation weights on the device); mu is then FedAvg's
        dga = fused_round_dga(prim.config) if mu is None else None
        if mu is None and dga is None:
            return None
        if dga is not None:
            mu = 0.0
            if len(client_ids) > 32:   # the tail's K limit (DGA_MAX_K)
                return None
        out = self._try_graphed_mega("_mega_lstm", True, _build_mega_lstm,
                                     data_cfg, client_ids, initial_lr, seeds,
                                     precisions=("bf16",), mu=mu, dga=dga)
        if out is None:
            # OPT-IN: measured SLOWER than the per-client epoch-graph path
            # on ROCm 7.2 — MIOpen decomposes groups=K convs into K
            # per-group kernels (no batching win) and grouped bwd-weight
            # falls to multi-ms CK batched-GEMM fallbacks (PERF.md,
            # profiles/).  The formulation itself is exact
            # (tests/test_mega_cpu.py, f64) and flips on wholesale when a
            # ROCm release makes grouped conv competitive.
            out = self._try_graphed_mega(
                "_mega_resnet", cc.get("use_mega_round_resnet", False),
                _build_mega_resnet, data_cfg, client_ids, initial_lr, seeds,
                mu=mu, dga=dga)
        if out is not None:
            return out
        fc = prim.fused_cnn
        if fc is None:
            return None
        store = prim._get_shard_store(data_cfg)
        if store is None or store.x[0].numel() != 784:
            return None
        ds = train_dataset
        if ds is None:
            return None
        dms = data_cfg.get("desired_max_samples", None)
        if lookup_round(store, ds.user_list, client_ids, dms) is None:
            return None

        # cross-client MEGA round: one launch set per batch-step covering
        # all K clients
        if cc.get("use_mega_round", True):
            if self._mega is None:
                from ..ops.fused_cnn import MegaRound
                self._mega = MegaRound(prim.arena, fc.C, fc.bs, fc.p1, fc.p2,
                                       data_cfg.get("max_grad_norm"),
                                       use_bf16=fc.use_bf16, mu=mu, dga=dga)
            if self._mega.supports(len(client_ids)):
                out = self._mega.run(store, ds, client_ids, seeds, initial_lr,
                                     self.server_arena, self.round_accums[0],
                                     dms)
                if out is not None:
                    self._mega_round_done(len(client_ids))
                    return out
        if dga is not None:
            return None  # _C.cnn_round weights by sample count: the pool

        # per-executor fused rounds: each chunk's shuffle orders are drawn
        # right before its launch, so the host work of chunk k+1 overlaps
        # the GPU work of chunk k
        for ex in self.executors[1:]:
            if not ex._shard_store_tried:
                ex._shard_store = store
                ex._shard_store_tried = True
        P = len(self.executors)
        outputs = []
        for k in range(P):
            chunk, schunk = client_ids[k::P], seeds[k::P]
            if not chunk:
                continue
            ex, st = self.executors[k], self.streams[k]
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                plan = plan_round(store, ds.user_list, chunk, schunk, dms)
                outputs.extend(_fused_round_impl(
                    ex, store, plan, chunk, schunk, initial_lr,
                    self.round_accums[k], mu))
            self._streams_dirty = True
        return outputs

    def _try_graphed_mega(self, attr, enabled, build, data_cfg, client_ids,
                          initial_lr, seeds, precisions=(), mu=0.0, dga=None):
        """One graph-captured cross-client round
        (ops/mega_round.GraphedMegaRound) when the model being trained is
        the one ``build(prim, data_cfg, mu, dga)`` recognises (it returns the
        driver, or None for any other model); the driver is kept in
        ``self.<attr>``.  ``precisions`` lists the ``mixed_precision``
        values the driver implements besides fp32.  Returns outputs or
        None if not this task / ineligible."""
        prim = self.executors[0]
        cc = prim.client_config
        if getattr(self, attr) is False or not enabled:
            return None
        if not cc.get("use_mega_round", True):
            return None
        mp = cc.get("mixed_precision")
        if mp and mp not in precisions:
            return None  # the graphed rounds are fp32 unless they say so
        if prim.arena is None or prim.arena.device.type != "cuda":
            return None
        opt_cfg = cc.get("optimizer_config", {})
        if (opt_cfg.get("type", "sgd") != "sgd"
                or opt_cfg.get("momentum", 0) or opt_cfg.get("weight_decay", 0)
                or opt_cfg.get("nesterov", False)):
            return None
        if getattr(self, attr) is None:
            mega = build(prim, data_cfg, mu, dga) if ops.HAS_EXT else None
            setattr(self, attr, mega or False)
        mega = getattr(self, attr)
        if mega is False or not mega.supports(len(client_ids)):
            return None
        store = prim._get_shard_store(data_cfg)
        if store is None or train_dataset is None:
            return None
        out = mega.run(store, train_dataset, client_ids, seeds, initial_lr,
                       self.server_arena, self.round_accums[0],
                       data_cfg.get("desired_max_samples", None))
        if out is not None:
            self._mega_round_done(len(client_ids))
        return out

    def _mega_round_done(self, n_clients):
        """A cross-client round ran on the current stream into
        ``round_accums[0]``."""
        self._streams_dirty = True
        prim = self.executors[0]
        prim.perf_acc["clients"] = prim.perf_acc.get("clients", 0) + n_clients


def _build_mega_lstm(prim, data_cfg, mu=0.0, dga=None):
    """The Shakespeare char-LSTM mega round (ops/mega_shakespeare.py), or
    None if ``prim`` trains another model."""
    from ..ops.mega_shakespeare import ShakespeareMegaRound, matches_char_lstm
    if matches_char_lstm(prim.arena) is None:
        return None
    return ShakespeareMegaRound(
        prim.arena, data_cfg.get("batch_size", 4),
        data_cfg.get("max_grad_norm"),
        use_bf16=prim.client_config.get("mixed_precision", "") == "bf16",
        mu=mu, dga=dga)


def _build_mega_resnet(prim, data_cfg, mu=0.0, dga=None):
    """The fed-CIFAR100 ResNet-18 mega round (ops/mega_resnet.py), or None
    if ``prim`` trains another model (or one without GroupNorm)."""
    from ..ops.mega_resnet import ResNetMegaRound, matches_resnet18
    cpg = int(prim.model_config.get("group_norm", 0) or 0)
    if cpg <= 0 or matches_resnet18(prim.arena) is None:
        return None
    return ResNetMegaRound(prim.arena, data_cfg.get("batch_size", 20),
                           data_cfg.get("max_grad_norm"), cpg, mu=mu,
                           dga=dga)


def fused_round_mu(strategy, client_config, model_config=None,
                   apply_privacy_metrics=False):
    """THE gate of the whole-round drivers (pure: config in, decision
    out).  Returns None when the round must take the per-client path,
    else the proximal coefficient the drivers train with: 0.0 for FedAvg,
    ``client_config["mu"]`` (default 0.001, as in ``process_round``) for
    FedProx.

    The drivers train full shards with SGD (plus FedProx's exact
    per-batch proximal term) and aggregate every layer's gradient with
    weights = sample counts; fall back whenever the eager path would
    behave differently: another strategy (DGA, FedLabels), privacy
    metrics, a frozen layer (its pseudo-grad segment must be zeroed,
    fedavg.py:58) or a num_skips_threshold (clients can be zero-weighted
    mid-epoch).  desired_max_samples is checked per client against shard
    sizes by lookup_round (the eager path truncates each client's epoch
    there)."""
    if strategy not in ("FedAvg", "FedProx") or apply_privacy_metrics:
        return None
    if (model_config or {}).get("freeze_layer", None):
        return None
    if int(client_config.get("num_skips_threshold", -1)) >= 0:
        return None
    if strategy == "FedAvg":
        return 0.0
    return float(client_config.get("mu", 0.001))


def fused_round_dga(config):
    """The DGA gate of the cross-client mega rounds (pure: config in,
    decision out), next to ``fused_round_mu``.  Returns the ``DGASpec`` the
    drivers end the round with, or None when the round must take the
    per-client path (the stream pool).

    The DGA tail forms ``exp(-beta * tw)`` with ``filter_weight`` and the
    clip-only local-DP rescale on the device and nothing else, so the gate
    accepts only when ``DGA.generate_client_payload`` would do nothing
    more: fast aggregation without RL or staleness (the pool's own
    conditions), no privacy metrics, frozen layer, num_skips_threshold or
    smoothed-gradient stats, no update quantization (it needs a quantile
    sort) and local DP either off or clip-only (eps < 0; the noised mode
    draws host RNG)."""
    if config.get("strategy") != "DGA":
        return None
    sc = config.get("server_config") or {}
    cc = config.get("client_config") or {}
    if (not sc.get("fast_aggregation", True) or sc.get("wantRL", False)
            or float(sc.get("stale_prob", 0.0) or 0.0) != 0.0
            or config.get("dump_norm_stats", False)
            or sc.get("type") == "personalization"):
        return None
    pm = config.get("privacy_metrics_config", None)
    if pm and pm.get("apply_metrics", False):
        return None
    if (config.get("model_config") or {}).get("freeze_layer", None):
        return None
    if int(cc.get("num_skips_threshold", -1)) >= 0:
        return None
    if cc.get("stats_on_smooth_grad", False):
        return None
    if cc.get("quant_thresh", None) is not None:
        return None
    median = sc.get("aggregate_median")
    if median == "softmax":
        source = sc.get("weight_train_loss", "train_loss")
        if source not in ("train_loss", "mag_var_loss", "mag_mean_loss"):
            source = "mag"  # generate_client_payload's else branch
        beta = float(sc["softmax_beta"])
    elif median == "mean":
        source, beta = "mean", 0.0
    else:
        return None
    dp = config.get("dp_config", None)
    clip, max_grad = False, 0.0
    if dp is not None and dp.get("enable_local_dp", False):
        if not float(dp["eps"]) < 0:
            return None
        clip, max_grad = True, float(dp["max_grad"])
        if not max_grad > 0:
            return None
    return DGASpec(source, beta, clip, max_grad)


def _fused_round_impl(ex, store, plan, client_ids, seeds, initial_lr,
                      round_accum, mu=0.0):
    """One _C.cnn_round call training ``client_ids`` on ``ex`` as planned
    (plan_round): copy-in, fused epoch, weighted pseudo-grad, accumulate
    into ``round_accum``.  Returns the per-client outputs."""
    fc = ex.fused_cnn
    counts, row_bases, orders = plan
    K = len(client_ids)
    off = sum(counts)
    order_offs = [0] + list(accumulate(counts))[:-1]
    if getattr(ex, "_order_pin", None) is None or ex._order_pin.numel() < off:
        ex._order_pin = torch.empty(max(off, 1024),
                                    dtype=torch.int64).pin_memory()
        ex._order_pin_ev = None
    if ex._order_pin_ev is not None:
        # previous round's non_blocking H2D of this buffer may still be
        # queued; overwriting the pinned staging before it lands would
        # corrupt that round's shuffle orders
        ex._order_pin_ev.synchronize()
    ex._order_pin[:off].copy_(torch.cat(orders))
    orders_dev = ex._order_pin[:off].to(ex.arena.device, non_blocking=True)
    ex._order_pin_ev = torch.cuda.Event()
    ex._order_pin_ev.record()
    if getattr(ex, "_round_stats", None) is None or \
            ex._round_stats.numel() < 2 * K:
        ex._round_stats = torch.zeros(2 * max(K, 8), device=ex.arena.device)
        ex._round_loss = torch.zeros(max(K, 8), device=ex.arena.device)
    ex._round_stats[: 2 * K].zero_()
    ex._round_loss[:K].zero_()
    fc.lr_t.fill_(float(initial_lr))
    ops._C.cnn_round(
        store.x.reshape(len(store.y), -1), store.y, orders_dev,
        torch.tensor(row_bases, dtype=torch.int64),
        torch.tensor(order_offs, dtype=torch.int64),
        torch.tensor(counts, dtype=torch.int64),
        torch.tensor(counts, dtype=torch.float32),  # FedAvg: num_samples
        torch.tensor([s & 0x7FFFFFFFFFFF for s in seeds], dtype=torch.int64),
        fc.bs, fc.C, ex.server_arena.data, ex.arena.data, ex.arena.grad,
        round_accum, fc.work_f, fc.work_i, fc.work_b, fc.work_d,
        fc.lr_t, fc.max_norm, fc.p1, fc.p2,
        ex._round_stats, ex._round_loss, fc.use_bf16, mu=mu)
    ex.perf_acc["clients"] = ex.perf_acc.get("clients", 0) + K
    return round_outputs(client_ids, counts, fc.bs, ex._round_loss,
                         ex._round_stats, ex.arena.total)
