"""``_C.mega_dga_accum`` (the DGA tail: softmax weights, clip-only local
DP and the accumulate, all on the device) against the float64 model of
tests/dga_ref64.py.

Sizes are those of tests/test_mega_clip_accum_gpu.py: P below one float4
(1, 3), a P % 4 tail (5, 1023), exactly one 32768-element chunk of the
norm pass, one element past the seam (32769) and two seams plus a tail of
3 (65539); with K = 3 the client bases k * P are unaligned for odd P.

Bounds:
* ``dga_out`` weights and norms: 1e-12 relative against the model fed the
  same float32 inputs (device exp / sqrt in f64 are within a few ulp, the
  norm's f64 tree differs from numpy's in summation order only);
* the ``round_accum`` delta: relative L2 error <= FACTOR x floor, where
  floor is the same tail in float32 on the CPU against float64, and a case
  is rejected as misconfigured unless FACTOR x floor <= 1e-3.
``max_grad`` comes from the reference norms (0.25 x the smallest, 4 x the
largest) and each client's side of the clip is asserted.
"""

import numpy as np
import pytest
import torch

import dga_ref64 as ref
from msrflute_amd.ops.mega_round import DGA_MODES, DGASpec

pytestmark = pytest.mark.gpu

PS = [1, 3, 5, 1023, 32768, 32769, 65539]
COUNTS = [9, 4, 1]
BS = 4
BETA = 1.5
FACTOR = 4
RTOL64 = 1e-12
SOURCES = ("train_loss", "mag_var_loss", "mag_mean_loss", "mag", "mean")


def _inputs(P, K, seed=0):
    """server > params (pseudo-gradients in (0.01, 1.01) x a per-client
    size), start > 0: every sum is of like signs, no expected value is a
    cancellation.  Stats give mean^2 << sumsq / n."""
    gen = np.random.default_rng(1000 * K + P + seed)
    server = (1 + gen.random(P)).astype(np.float32)
    size = np.array([1.0, 0.5, 0.25])[:K, None]
    params = (server[None, :]
              - size * (0.01 + gen.random((K, P)))).astype(np.float32)
    start = (0.5 + gen.random(P)).astype(np.float32)
    counts = COUNTS[:K]
    n = np.array([-(-c // BS) * P for c in counts], dtype=np.float64)
    loss = (np.array(counts) * (0.2 + gen.random(K))).astype(np.float32)
    stats = np.zeros(2 * K, dtype=np.float32)
    stats[0::2] = 0.1 * n * (0.5 + gen.random(K))
    stats[1::2] = n * (1 + gen.random(K))
    return server, params, start, counts, loss, stats


def _run(server, params, start, counts, loss, stats, spec):
    """One kernel call; returns (accum float32, dga_out [3, K] float64)."""
    from msrflute_amd.ops import _C
    K, P = params.shape
    accum = torch.from_numpy(start).cuda()
    out = torch.full((4 * K,), float("nan"), dtype=torch.float64,
                     device="cuda")
    _C.mega_dga_accum(torch.from_numpy(params).reshape(-1).cuda(),
                      torch.from_numpy(server).cuda(), K,
                      torch.from_numpy(loss).cuda(),
                      torch.from_numpy(stats).cuda(),
                      torch.tensor(counts, dtype=torch.int64).cuda(), BS,
                      accum=accum, **spec.kwargs(out))
    torch.cuda.synchronize()
    return accum.cpu().numpy(), out[:3 * K].view(3, K).cpu().numpy()


def _close64(got, want):
    zero = want == 0
    assert (got[zero] == 0).all()
    err = np.abs(got[~zero] - want[~zero]) / np.abs(want[~zero])
    assert err.size == 0 or err.max() <= RTOL64, err.max()


def _check(inp, source, clip, max_grad, what):
    server, params, start, counts, loss, stats = inp
    args = (server, params, loss, stats, counts, BS, source, BETA, clip,
            max_grad)
    want = ref.dga_tail(*args, accum=start)
    delta64 = want["accum"] - start.astype(np.float64)
    floor = ref.rel_l2(
        ref.dga_tail_f32(*args, accum=start).astype(np.float64) - start,
        delta64)
    assert FACTOR * floor <= 1e-3, ("misconfigured case", floor)
    spec = DGASpec(source, BETA, clip, max_grad)
    acc, out = _run(server, params, start, counts, loss, stats, spec)
    err = ref.rel_l2(acc.astype(np.float64) - start, delta64)
    print(f"{what} {source:>13}: err {err:.3e} floor {floor:.3e} "
          f"ratio {err / floor if floor else float('inf'):.2f}")
    _close64(out[0], want["weight"])
    _close64(out[1], want["norm"])
    # c is reported as applied, rounded to float32: one float32 ulp
    assert (np.abs(out[2] - want["c"]) <= 2.0 ** -23 * want["c"]).all()
    assert err <= FACTOR * floor, (err, floor)
    # deterministic: k ascends inside one thread.  (The reported f64 norm
    # is folded with one atomicAdd per chunk, in free order: it repeats to
    # f64 rounding, and the coefficient applied is its float32 rounding.)
    acc2, out2 = _run(server, params, start, counts, loss, stats, spec)
    assert np.array_equal(acc, acc2)
    assert np.array_equal(out[0], out2[0]) and np.array_equal(out[2], out2[2])
    np.testing.assert_allclose(out2[1], out[1], rtol=1e-14, atol=0)
    return want


def test_modes_match_the_extension():
    from msrflute_amd.ops import _C
    assert dict(_C.DGA_MODES) == DGA_MODES


@pytest.mark.parametrize("regime", ["no_dp", "all_clipped", "none_clipped"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("P", PS)
def test_tail_against_float64(P, K, regime):
    inp = _inputs(P, K)
    server, params, start, counts, loss, stats = inp
    norms = ref.dga_tail(server, params, loss, stats, counts, BS, "mean",
                         BETA, True, 1.0)["norm"]
    clip = regime != "no_dp"
    max_grad = {"no_dp": 0.0, "all_clipped": 0.25 * norms.min(),
                "none_clipped": 4 * norms.max()}[regime]
    for source in SOURCES:
        want = _check(inp, source, clip, float(max_grad), f"P={P} K={K}")
        if regime == "all_clipped":
            assert (want["norm"] > max_grad).all()
            assert (want["c"] < want["weight"]).all()
        elif regime == "none_clipped":
            assert (want["norm"] < max_grad).all() and (want["norm"] > 0).all()
            # unclipped: c is the weight's float32 rounding
            assert (want["c"] == want["weight"].astype(np.float32)).all()
        else:
            assert (want["norm"] == 0).all()


@pytest.mark.parametrize("P", [5, 32769])
def test_mixed_clip_sides(P):
    """max_grad between the clients' norms: one call clips some clients
    and leaves others."""
    inp = _inputs(P, 3)
    server, params, start, counts, loss, stats = inp
    norms = ref.dga_tail(server, params, loss, stats, counts, BS, "mean",
                         BETA, True, 1.0)["norm"]
    max_grad = float(np.sqrt(norms.min() * norms.max()))
    want = _check(inp, "train_loss", True, max_grad, f"P={P} mixed")
    assert (want["norm"] > max_grad).any() and (want["norm"] < max_grad).any()


@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("P", [3, 32769])
def test_all_weights_zero_leaves_the_accumulator_bit_unchanged(P, clip):
    server, params, start, counts, loss, stats = _inputs(P, 3)
    start[::2] *= -1
    start[:1] = -0.0          # a bit pattern that "+ 0.0" would change
    loss[:] = float("nan")
    acc, out = _run(server, params, start, counts, loss, stats,
                    DGASpec("train_loss", BETA, clip, 0.5))
    assert (out[0] == 0).all() and (out[2] == 0).all()
    assert np.array_equal(acc.view(np.uint32), start.view(np.uint32))


@pytest.mark.parametrize("P", [5, 32769])
def test_overflowing_loss_gets_min_weight_nan_is_dropped(P):
    inp = _inputs(P, 3)
    server, params, start, counts, loss, stats = inp
    loss[0] = -2000.0 * counts[0]    # exp(+3000) overflows: MIN_WEIGHT
    loss[1] = float("nan")           # dropped
    want = _check(inp, "train_loss", False, 0.0, f"P={P} overflow")
    _, out = _run(server, params, start, counts, loss, stats,
                  DGASpec("train_loss", BETA, False, 0.0))
    assert out[0][0] == ref.MIN_WEIGHT == 1e-7
    assert out[0][1] == 0.0 and 0 < out[0][2] < 1
    assert want["weight"][0] == 1e-7


def test_above_100_is_capped_and_infinite_argument_is_dropped():
    inp = _inputs(1023, 3)
    server, params, start, counts, loss, stats = inp
    loss[0] = -5.0 * counts[0]       # e^7.5 = 1808 -> 100
    loss[1] = float("-inf")          # exp(+inf) = inf: filter_weight -> 0
    want = _check(inp, "train_loss", False, 0.0, "cap")
    assert want["weight"][0] == 100.0 and want["weight"][1] == 0.0
