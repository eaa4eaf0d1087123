"""The FedProx case shared by tests/test_mega_cnn_prox_gpu.py and
tests/test_cnn_epoch_prox_gpu.py: the shape of
tests/test_mega_cnn_reference_gpu.py (its arena, seeds, client ids, bs,
dropout rates and ``round_accum`` start) with counts (9, 6, 1), replayed
per client in tests/cnn_prox_ref64.py.

Three steps: client 0 trains 4 + 4 + 1 rows; client 1 trains 4 + 2 rows
and then IDLES with ``w != w_g``; client 2 is a single row and idles from
step 1.  (A one-step client has ``w == w_g`` at its only step and does not
exercise the proximal term, which is why client 1 takes two.)

mu = 1, not a production value: at mu = 1e-3 the term is ~1e-4 of the
gradient, too close to the bound for a missing term to be caught.

Everything here runs on the CPU; ``case`` asserts, on the float64 side
alone, that the case can tell FedProx from FedAvg:

* every batch is clipped in "clip" and none in "free";
* bound = FACTOR x floor <= 1e-3, floor = the same replay in float32;
* in every segment of clients 0 and 1 the float64 FedProx update differs
  from the float64 mu = 0 update by >= 50 x the bound;
* for both the reported loss differs by >= 1e-2 relative.
"""

import functools
from types import SimpleNamespace

import torch

import cnn_prox_ref64 as pref
import cnn_ref64 as ref
import philox_oracle as po
from test_mega_cnn_reference_gpu import (BS, CLIENT_IDS, FACTOR, LR, P1, P2,
                                         SEED_MASK, SEEDS, _arena, _orders)

MU = 1.0
COUNTS = (9, 6, 1)
STEPS = (3, 2, 1)
USERS = [("pad0", 2), ("c", 1), ("pad1", 2), ("b", 6), ("pad2", 3),
         ("a", 9), ("pad3", 3)]
SEPARATION = 50.0


@functools.lru_cache(maxsize=None)
def data(C):
    """(x, y, offsets, names, row_bases) of the store, on the CPU."""
    n = sum(c for _, c in USERS)
    g = torch.Generator().manual_seed(70 + C)
    x = torch.randn(n, 28, 28, generator=g)
    y = torch.randint(0, C, (n,), generator=g)
    offsets = [0]
    for _, c in USERS:
        offsets.append(offsets[-1] + c)
    names = [u for u, _ in USERS]
    row_bases = [offsets[i] for i in CLIENT_IDS]
    assert row_bases == [14, 5, 2]
    return x, y, offsets, names, row_bases


@functools.lru_cache(maxsize=None)
def store(C):
    """The minimal stand-in device store and dataset ``MegaRound.run``
    needs."""
    x, y, offsets, names, _ = data(C)
    st = SimpleNamespace(x=x.cuda(), y=y.cuda(), offsets=offsets,
                         user_pos={u: i for i, u in enumerate(names)})
    return st, SimpleNamespace(user_list=names)


@functools.lru_cache(maxsize=None)
def case(C, regime):
    _, w0 = _arena(C)
    x, y, _, _, row_bases = data(C)
    orders = _orders(COUNTS, SEEDS)
    x64 = x.double()

    def replay(k, max_norm, lr, mu=MU, dtype=torch.float64):
        masks = po.epoch_masks(SEEDS[k] & SEED_MASK, P1, P2)
        return pref.epoch(w0, C, x64, y, orders[k] + row_bases[k], BS, masks,
                          P1, P2, max_norm, lr, mu, w0, dtype=dtype)

    free = [replay(k, -1.0, LR) for k in range(3)]
    norms = [n for r in free for n in r["norms"]]
    if regime == "clip":
        max_norm, lr = 0.25 * min(norms), 4 * LR
    else:
        max_norm, lr = 4.0 * max(norms), LR
    r64 = [replay(k, max_norm, lr) for k in range(3)]
    r32 = [replay(k, max_norm, lr, dtype=torch.float32) for k in range(3)]
    avg = [replay(k, max_norm, lr, mu=0.0) for k in range(3)]
    engaged = [n > max_norm for r in r64 for n in r["norms"]]
    assert [len(r["norms"]) for r in r64] == list(STEPS)
    assert all(engaged) if regime == "clip" else not any(engaged), \
        ([r["norms"] for r in r64], max_norm)
    upd64 = [r["w"] - w0.double() for r in r64]
    floors = [ref.seg_rel_err(r32[k]["w"] - w0, upd64[k], C)
              for k in range(3)]
    floor = max(max(f.values()) for f in floors)
    bound = FACTOR * floor
    assert bound <= 1e-3, ("misconfigured case", floors)
    # the case tells FedProx from FedAvg (clients 0 and 1; client 2 takes
    # one step at w == w_g, where the two coincide)
    sep = [ref.seg_rel_err(avg[k]["w"] - w0.double(), upd64[k], C)
           for k in range(2)]
    loss_sep = [ref.rel_err(avg[k]["loss"], r64[k]["loss"]) for k in range(2)]
    assert min(min(s.values()) for s in sep) >= SEPARATION * bound, \
        (sep, bound)
    assert min(loss_sep) >= 1e-2, loss_sep
    assert torch.equal(avg[2]["w"], r64[2]["w"])
    return {"max_norm": max_norm, "lr": lr, "r64": r64, "upd64": upd64,
            "floor": floor, "floors": floors, "orders": orders,
            "sep": min(min(s.values()) for s in sep),
            "loss_sep": min(loss_sep)}
