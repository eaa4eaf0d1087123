"""tests/cnn_ref64.py against the task's own model
(experiments/cv_cnn_femnist/model.py) cast to double: with all-ones masks
and p = 0 in the scale the two must agree to 1e-12 on loss and gradients,
and the clip / stats / SGD arithmetic must follow its definition."""

import importlib.util
import os

import pytest
import torch

import cnn_ref64 as ref

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
C, B = 5, 3


def _net():
    spec = importlib.util.spec_from_file_location(
        "cv_cnn_femnist_model",
        os.path.join(REPO, "experiments", "cv_cnn_femnist", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    torch.manual_seed(0)
    return mod.FEMNISTNet(C).double().eval()  # eval: dropout is identity


@pytest.fixture(scope="module")
def case():
    net = _net()
    flat = torch.cat([p.detach().reshape(-1) for p in net.parameters()])
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, 28, 28, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (B,), generator=g)
    return net, flat, x, y


def test_layout_matches_model(case):
    net, flat, _, _ = case
    assert [tuple(p.shape) for p in net.parameters()] == list(ref.shapes(C))
    assert flat.numel() == ref.total(C)
    assert [n for n, _, _ in ref.segments(C)] == list(ref.NAMES)


def test_loss_and_grads_match_model_in_double(case):
    net, flat, x, y = case
    loss_m = torch.nn.functional.cross_entropy(net(x), y)
    grads_m = torch.autograd.grad(loss_m, list(net.parameters()))
    g_m = torch.cat([g.reshape(-1) for g in grads_m])
    loss_m = loss_m.detach()

    ones2 = torch.ones(B, 64, 12, 12, dtype=torch.float64)
    ones3 = torch.ones(B, 128, dtype=torch.float64)
    w, loss, g, norm = ref.step(flat, C, x, y, ones2, ones3, 0.0, 0.0,
                                -1.0, 0.1)
    assert abs(float(loss) - float(loss_m)) <= 1e-12 * abs(float(loss_m))
    for name, off, n in ref.segments(C):
        d = (g[off:off + n] - g_m[off:off + n]).norm()
        assert float(d) <= 1e-12 * float(g_m[off:off + n].norm()), name
    assert abs(norm - float(g_m.norm())) <= 1e-12 * norm
    assert torch.equal(w, flat - 0.1 * g)


def test_masks_scale_and_gate(case):
    _, flat, x, y = case
    g = torch.Generator().manual_seed(2)
    m2 = (torch.rand(B, 64, 12, 12, generator=g) >= 0.25).double()
    m3 = (torch.rand(B, 128, generator=g) >= 0.5).double()
    leaf = flat.clone().requires_grad_(True)
    ws = ref.split(leaf, C)
    loss = ref.loss_fn(ws, x, y, m2, m3, 0.25, 0.5)
    # by hand: the same network with the scaled masks multiplied in
    F = torch.nn.functional
    h = torch.relu(F.conv2d(x.unsqueeze(1), ws[0], ws[1]))
    h = F.max_pool2d(torch.relu(F.conv2d(h, ws[2], ws[3])), 2)
    h = torch.flatten(h * (m2 * (4.0 / 3.0)), 1)
    h = torch.relu(F.linear(h, ws[4], ws[5])) * (m3 * 2.0)
    want = F.cross_entropy(F.linear(h, ws[6], ws[7]), y)
    assert abs(float(loss.detach()) - float(want.detach())) \
        <= 1e-12 * abs(float(want.detach()))
    # a dropped fc1 unit gets no gradient from the rows that dropped it
    gw3, = torch.autograd.grad(loss, ws[4])
    dead = m3.sum(0) == 0
    if dead.any():
        assert float(gw3[dead].abs().max()) == 0.0


def test_clip_stats_sgd_definition(case):
    _, flat, x, y = case
    ones2 = torch.ones(B, 64, 12, 12, dtype=torch.float64)
    ones3 = torch.ones(B, 128, dtype=torch.float64)
    _, _, g_raw, norm = ref.step(flat, C, x, y, ones2, ones3, 0.0, 0.0,
                                 -1.0, 0.1)
    # engaged: max_norm below the norm
    mn = 0.25 * norm
    w, _, g, norm2 = ref.step(flat, C, x, y, ones2, ones3, 0.0, 0.0, mn, 0.5)
    assert norm2 == norm
    scale = mn / (norm + 1e-6)
    assert torch.allclose(g, g_raw * scale, rtol=1e-15, atol=0)
    assert torch.equal(w, flat - 0.5 * g)
    # not engaged: max_norm above the norm, and max_norm <= 0
    for mn in (4 * norm, norm, -1.0, 0.0):
        _, _, g, _ = ref.step(flat, C, x, y, ones2, ones3, 0.0, 0.0, mn, 0.5)
        assert torch.equal(g, g_raw)


def test_epoch_accumulates_over_ragged_batches(case):
    _, flat, _, _ = case
    g = torch.Generator().manual_seed(3)
    xs = torch.randn(5, 28, 28, generator=g, dtype=torch.float64)
    ys = torch.randint(0, C, (5,), generator=g)
    order = torch.tensor([4, 0, 2, 1, 3])
    seen = []

    def masks(t, rows):
        seen.append((t, rows))
        return (torch.ones(rows, 64, 12, 12), torch.ones(rows, 128))

    out = ref.epoch(flat, C, xs, ys, order, 2, masks, 0.0, 0.0, -1.0, 0.1)
    assert seen == [(0, 2), (1, 2), (2, 1)]
    w, loss, stats = flat, 0.0, torch.zeros(2, dtype=torch.float64)
    for s in (0, 2, 4):
        idx = order[s:s + 2]
        m = masks(0, len(idx))
        w, l, gg, _ = ref.step(w, C, xs[idx], ys[idx], m[0].double(),
                               m[1].double(), 0.0, 0.0, -1.0, 0.1)
        loss += float(l)
        stats += torch.stack([gg.sum(), (gg * gg).sum()])
    assert torch.equal(out["w"], w) and torch.equal(out["grad"], gg)
    assert abs(float(out["loss"]) - loss) < 1e-14
    assert torch.allclose(out["stats"], stats, rtol=1e-14, atol=0)
    assert len(out["norms"]) == 3
    # float32 mode really computes in float32
    out32 = ref.epoch(flat, C, xs, ys, order, 2, masks, 0.0, 0.0, -1.0, 0.1,
                      dtype=torch.float32)
    assert out32["w"].dtype == torch.float32
    errs = ref.seg_rel_err(out32["w"] - flat.float(), out["w"] - flat, C)
    assert 0 < max(errs.values()) < 1e-3
