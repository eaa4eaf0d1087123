"""tests/cnn_prox_ref64.py on the CPU: with ``mu = 0`` it is
tests/cnn_ref64.py bit for bit, and with ``mu > 0`` its pre-clip gradient
is the gradient of the explicit FedProx objective
``CE + (mu / 2) ||w - w_g||^2``."""

import pytest
import torch

import cnn_prox_ref64 as pref
import cnn_ref64 as ref

C, BS = 5, 4


@pytest.fixture(scope="module")
def case():
    g = torch.Generator().manual_seed(5)
    flat = 0.05 * torch.randn(ref.total(C), generator=g, dtype=torch.float64)
    xs = torch.randn(8, 28, 28, generator=g, dtype=torch.float64)
    ys = torch.randint(0, C, (8,), generator=g)
    order = torch.tensor([6, 1, 7, 3, 0, 5, 2, 4])    # 2 steps of bs = 4
    mg = torch.Generator().manual_seed(6)
    m2 = [(torch.rand(BS, 64, 12, 12, generator=mg) >= 0.25).double()
          for _ in range(2)]
    m3 = [(torch.rand(BS, 128, generator=mg) >= 0.5).double()
          for _ in range(2)]

    def masks(t, rows):
        return m2[t][:rows], m3[t][:rows]

    return flat, xs, ys, order, masks


@pytest.mark.parametrize("max_norm", [-1.0, 0.05])
def test_mu_zero_is_cnn_ref64_bit_for_bit(case, max_norm):
    flat, xs, ys, order, masks = case
    a = ref.epoch(flat, C, xs, ys, order, BS, masks, 0.25, 0.5, max_norm, 0.1)
    b = pref.epoch(flat, C, xs, ys, order, BS, masks, 0.25, 0.5, max_norm,
                   0.1, 0.0, flat)
    assert len(a["norms"]) == 2
    if max_norm > 0:
        assert all(n > max_norm for n in a["norms"])
    assert torch.equal(a["w"], b["w"])
    assert torch.equal(a["loss"], b["loss"])
    assert torch.equal(a["stats"], b["stats"])
    assert torch.equal(a["grad"], b["grad"])
    assert a["norms"] == b["norms"]


def test_prox_gradient_is_autograd_of_explicit_objective(case):
    flat, xs, ys, order, masks = case
    mu, lr = 1.0, 0.1
    w_g = flat
    w = flat.clone()
    for t in range(2):
        idx = order[t * BS:(t + 1) * BS]
        m2, m3 = masks(t, BS)
        leaf = w.clone().requires_grad_(True)
        obj = ref.loss_fn(ref.split(leaf, C), xs[idx], ys[idx], m2, m3,
                          0.25, 0.5) \
            + 0.5 * mu * (leaf - w_g).square().sum()
        want, = torch.autograd.grad(obj, leaf)
        w_new, loss, gc, norm, gp = pref.step(w, C, xs[idx], ys[idx], m2, m3,
                                              0.25, 0.5, -1.0, lr, mu, w_g)
        for name, off, n in ref.segments(C):
            d = (gp[off:off + n] - want[off:off + n]).norm()
            assert float(d) <= 1e-12 * float(want[off:off + n].norm()), name
        obj = float(obj.detach())
        assert abs(float(loss) - obj) <= 1e-12 * abs(obj)
        assert abs(norm - float(want.norm())) <= 1e-12 * norm
        assert torch.equal(gc, gp)              # clip not engaged
        assert torch.equal(w_new, w - lr * gp)
        # w == w_g at a client's first step: the term acts from step 1 on
        assert torch.equal(w, w_g) == (t == 0)
        w = w_new


def test_prox_changes_the_second_step_only(case):
    flat, xs, ys, order, masks = case
    a = pref.epoch(flat, C, xs, ys, order, BS, masks, 0.25, 0.5, -1.0, 0.1,
                   0.0, flat)
    b = pref.epoch(flat, C, xs, ys, order, BS, masks, 0.25, 0.5, -1.0, 0.1,
                   1.0, flat)
    assert a["norms"][0] == b["norms"][0]
    assert a["norms"][1] != b["norms"][1]
    assert float(b["loss"]) > float(a["loss"])
