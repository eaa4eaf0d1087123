"""The cross-client mega round (``MegaRound.run`` ->
``launch_cnn_round_mega``) with dropout ON against float64.

The existing mega tests compare it with the per-client round, which
launches the same kernels; here every client is replayed independently in
tests/cnn_ref64.py from the server weights, under the oracle masks of its
own seed and client-local indices, and compared per client and per
parameter segment.

Shape: K = 3 clients, bs = 4, counts (9, 4, 1) -> three steps; client 0
ends on a 1-row batch, client 1 idles after step 0, client 2 is a single
row and then idles.  The clients sit at non-contiguous, descending store
rows, ``round_accum`` starts non-zero, and one seed is wider than the 47
bits the driver keeps.  ``MegaRound.run`` is driven through a minimal
stand-in store, so the meta packing, the seed mask and ``weights =
counts`` are covered too.

Bound: as in tests/test_cnn_dropout_gpu.py — ``FACTOR`` times the largest
per-segment relative L2 error, over the three clients, of the same replay
in torch float32, and the case is rejected unless that is <= 1e-3.
"""

import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import cnn_ref64 as ref
import philox_oracle as po

pytestmark = pytest.mark.gpu

BS, P1, P2, LR = 4, 0.25, 0.5, 0.1
FACTOR = 4.0                      # as in tests/test_cnn_dropout_gpu.py
SEED_MASK = 0x7FFFFFFFFFFF
COUNTS = (9, 4, 1)
SEEDS = (11, (1 << 40) + 7, (1 << 50) + (1 << 33) + 9)  # last: > 47 bits
# store rows per user; the round's clients are users a, b, c
USERS = [("pad0", 2), ("c", 1), ("pad1", 2), ("b", 4), ("pad2", 3),
         ("a", 9), ("pad3", 3)]
CLIENT_IDS = [5, 3, 1]            # indices into the user list: a, b, c
ACCUM_SCALE = 1e-3                # start values of round_accum


@functools.lru_cache(maxsize=None)
def _arena(C):
    from msrflute_amd.models import make_model
    from msrflute_amd.ops.arena import ParameterArena
    torch.manual_seed(4)
    model = make_model({"model_type": "CNN",
                        "model_folder": "experiments/cv_cnn_femnist/model.py",
                        "num_classes": C})
    arena = ParameterArena(model, bind_grads=True)
    return arena, arena.data.cpu().clone()


@functools.lru_cache(maxsize=None)
def _store(C):
    n = sum(c for _, c in USERS)
    g = torch.Generator().manual_seed(70 + C)
    x = torch.randn(n, 28, 28, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    offsets = [0]
    for _, c in USERS:
        offsets.append(offsets[-1] + c)
    names = [u for u, _ in USERS]
    store = SimpleNamespace(x=x.cuda(), y=y.cuda(), offsets=offsets,
                            user_pos={u: i for i, u in enumerate(names)})
    ds = SimpleNamespace(user_list=names)
    row_bases = [offsets[i] for i in CLIENT_IDS]
    assert row_bases == [12, 5, 2]
    return store, ds, x, y, row_bases


def _orders(counts, seeds):
    out = []
    for n, s in zip(counts, seeds):
        torch.manual_seed(s & SEED_MASK)
        out.append(torch.randperm(n))
    return out


def _mega(C, max_norm, lr, client_sel=(0, 1, 2)):
    """Run the mega round for the selected clients; returns (driver,
    round_accum start, round_accum)."""
    from msrflute_amd.ops.fused_cnn import MegaRound
    arena, w0 = _arena(C)
    arena.data.copy_(w0)
    store, ds, _, _, _ = _store(C)
    mr = MegaRound(arena, C, BS, P1, P2, max_norm)
    g = torch.Generator().manual_seed(9)
    start = (ACCUM_SCALE * torch.randn(arena.total, generator=g))
    accum = start.cuda()
    outs = mr.run(store, ds, [CLIENT_IDS[k] for k in client_sel],
                  [SEEDS[k] for k in client_sel], lr, arena, accum)
    torch.cuda.synchronize()
    assert outs is not None and len(outs) == len(client_sel)
    for k, (cid, meta) in zip(client_sel, outs):
        assert cid == CLIENT_IDS[k] and meta["ns"] == COUNTS[k]
        assert meta["pl"]["weight"] == float(COUNTS[k])
    assert torch.equal(arena.data.cpu(), w0)   # the server arena is read only
    return mr, start, accum.cpu()


@functools.lru_cache(maxsize=None)
def _case(C, regime):
    _, w0 = _arena(C)
    _, _, x, y, row_bases = _store(C)
    orders = _orders(COUNTS, SEEDS)
    x64 = x.double()

    def replay(k, max_norm, lr, dtype=torch.float64):
        masks = po.epoch_masks(SEEDS[k] & SEED_MASK, P1, P2)
        return ref.epoch(w0, C, x64, y, orders[k] + row_bases[k], BS, masks,
                         P1, P2, max_norm, lr, dtype=dtype)

    free = [replay(k, -1.0, LR) for k in range(3)]
    norms = [n for r in free for n in r["norms"]]
    if regime == "clip":
        max_norm, lr = 0.25 * min(norms), 4 * LR
    else:
        max_norm, lr = 4.0 * max(norms), LR
    r64 = [replay(k, max_norm, lr) for k in range(3)]
    r32 = [replay(k, max_norm, lr, dtype=torch.float32) for k in range(3)]
    engaged = [n > max_norm for r in r64 for n in r["norms"]]
    assert [len(r["norms"]) for r in r64] == [3, 1, 1]
    assert all(engaged) if regime == "clip" else not any(engaged), \
        ([r["norms"] for r in r64], max_norm)
    upd64 = [r["w"] - w0.double() for r in r64]
    floors = [ref.seg_rel_err(r32[k]["w"] - w0, upd64[k], C)
              for k in range(3)]
    floor = max(max(f.values()) for f in floors)
    assert FACTOR * floor <= 1e-3, ("misconfigured case", floors)
    return {"max_norm": max_norm, "lr": lr, "r64": r64, "upd64": upd64,
            "floor": floor, "floors": floors}


def _check(what, errs, floor):
    bound = FACTOR * floor
    for name, e in errs.items():
        print(f"{what:>14} {name:>6}: err {e:.3e}  floor {floor:.3e}  "
              f"ratio {e / floor:.2f}")
    worst = max(errs, key=errs.get)
    assert errs[worst] <= bound, (what, worst, errs[worst], bound)


@pytest.mark.parametrize("regime", ["clip", "free"])
@pytest.mark.parametrize("C", [5, 62])
def test_mega_round_matches_fp64(C, regime):
    c = _case(C, regime)
    _, w0 = _arena(C)
    P = w0.numel()
    print("floors", [{k: f"{v:.2e}" for k, v in f.items()}
                     for f in c["floors"]])
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

    # masks left by the last step (t = 2): only client 0's row 0 is active
    G = 3 * BS
    wb = mr.work_b.cpu().numpy()
    seed0 = SEEDS[0] & SEED_MASK
    assert np.array_equal(wb[G * 9216:G * 9216 + 9216],
                          po.pool_mask(seed0, 2, 1, P1).reshape(-1))
    assert np.array_equal(wb[2 * G * 9216:2 * G * 9216 + 128],
                          po.fc1_mask(seed0, 2, 1, P2).reshape(-1))


@pytest.mark.parametrize("C", [5, 62])
def test_finished_clients_stay_bit_unchanged(C):
    """Clients 1 and 2 finish at step 0.  A round of those two alone runs
    ONE step; the three-step round must leave their weights, loss and
    stats at exactly that step-0 result."""
    c = _case(C, "free")
    _, w0 = _arena(C)
    P = w0.numel()
    mr3, _, _ = _mega(C, c["max_norm"], c["lr"])
    stack3 = mr3.params_stack[:3 * P].cpu().view(3, P)
    loss3, stats3 = mr3.loss_out.cpu(), mr3.stats_out.cpu()
    mr2, _, _ = _mega(C, c["max_norm"], c["lr"], client_sel=(1, 2))
    stack2 = mr2.params_stack[:2 * P].cpu().view(2, P)
    assert not torch.equal(stack2[0], w0) and not torch.equal(stack2[1], w0)
    assert torch.equal(stack3[1], stack2[0])
    assert torch.equal(stack3[2], stack2[1])
    # loss and stats are folded with atomics (rows of a batch, chunks of
    # the arena) whose order is free, so they repeat to rounding, not to
    # the bit; the single-row client's loss is one add and is exact
    assert torch.equal(loss3[2], mr2.loss_out.cpu()[1])
    assert torch.allclose(loss3[1:3], mr2.loss_out.cpu()[:2], rtol=1e-6,
                          atol=0)
    assert torch.allclose(stats3[2:6], mr2.stats_out.cpu()[:4], rtol=1e-6,
                          atol=0)
    # masks of step 0, all rows of both clients active or oracle-keyed
    G = 2 * BS
    wb = mr2.work_b.cpu().numpy()
    m2 = wb[G * 9216:2 * G * 9216].reshape(2, BS * 9216)
    m3 = wb[2 * G * 9216:2 * G * 9216 + G * 128].reshape(2, BS * 128)
    for slot, k in enumerate((1, 2)):
        rows = min(COUNTS[k], BS)
        seed = SEEDS[k] & SEED_MASK
        assert np.array_equal(m2[slot, :rows * 9216],
                              po.pool_mask(seed, 0, rows, P1).reshape(-1))
        assert np.array_equal(m3[slot, :rows * 128],
                              po.fc1_mask(seed, 0, rows, P2).reshape(-1))
