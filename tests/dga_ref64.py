"""numpy float64 model of the DGA tail (k_dga_normsq_mb + k_dga_accum_mb,
csrc/fused_cnn.hip): the training weight ``tw``, the softmax weight with
its overflow / NaN / above-100 branches, the clip-only local-DP rescale
and the accumulate.  tests/test_dga_ref64_cpu.py ties it to
``DGA.generate_client_payload`` + ``accumulate_flat_grad``; the GPU tests
compare the kernels against it.

Inputs are the float32 values the kernels read, widened to float64.  The
two float32 roundings the kernels make on purpose are modelled: the
pseudo-gradient ``w_g - w_k`` is one float32 subtraction, and with
``f32_coef`` (the device) the coefficient ``c_k = weight_k * dp_k`` is
rounded to float32 before it multiplies.
"""

import math

import numpy as np

MIN_WEIGHT = 1e-7
SOURCES = ("train_loss", "mag_var_loss", "mag_mean_loss", "mag")


def training_weight(source, loss, s, q, count, bs, P):
    """``tw`` of one client: what generate_client_payload reads off the
    trainer, from the round's summed loss and {sum, sumsq} stats."""
    loss, s, q = float(loss), float(s), float(q)
    n = max(-(-int(count) // int(bs)) * int(P), 1)
    if source == "train_loss":
        return loss / max(int(count), 1)
    mean = s / n
    if source == "mag_var_loss":
        return max(q / n - mean * mean, 0.0)
    if source == "mag_mean_loss":
        return mean
    return math.sqrt(max(q / n, 0.0))


def softmax_weight(beta, tw):
    """exp(-beta * tw) -> MIN_WEIGHT on overflow -> filter_weight."""
    try:
        w = math.exp(-float(beta) * tw)
    except OverflowError:
        w = MIN_WEIGHT
    if math.isnan(w) or math.isinf(w):
        return 0.0
    return min(w, 100.0)


def rel_l2(got, want):
    """Relative L2 error of ``got`` against the float64 ``want``."""
    got = np.asarray(got, dtype=np.float64).reshape(-1)
    want = np.asarray(want, dtype=np.float64).reshape(-1)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def dga_tail_f32(server, params, loss, stats, counts, bs, source, beta,
                 clip=False, max_grad=0.0, accum=None):
    """The same tail with every operation in float32 (numpy on the CPU):
    the noise floor the kernels' accumulate is held to.  Returns the
    float32 ``accum``."""
    f = np.float32
    server = np.asarray(server, dtype=f)
    params = np.asarray(params, dtype=f)
    K, P = params.shape
    d = server[None, :] - params
    out = np.zeros(P, dtype=f) if accum is None else np.array(accum, dtype=f)
    with np.errstate(all="ignore"):
        for k in range(K):
            w = f(1.0)
            if source != "mean":
                n = f(max(-(-int(counts[k]) // int(bs)) * P, 1))
                s, q = f(stats[2 * k]), f(stats[2 * k + 1])
                mean = s / n
                if source == "train_loss":
                    tw = f(loss[k]) / f(max(int(counts[k]), 1))
                elif source == "mag_var_loss":
                    tw = max(q / n - mean * mean, f(0))
                elif source == "mag_mean_loss":
                    tw = mean
                else:
                    tw = np.sqrt(max(q / n, f(0)))
                arg = f(-beta) * tw
                w = np.exp(arg)
                if np.isinf(w) and not np.isinf(arg):
                    w = f(MIN_WEIGHT)
                if np.isnan(w) or np.isinf(w):
                    w = f(0)
                w = min(w, f(100))
            if clip:
                norm = np.sqrt(np.sum(d[k] * d[k], dtype=f))
                if norm > f(max_grad):
                    w = w * (f(max_grad) / norm)
            if w != 0:
                out = out + f(w) * d[k]
    return out


def dga_tail(server, params, loss, stats, counts, bs, source, beta,
             clip=False, max_grad=0.0, accum=None, f32_coef=True):
    """The whole tail.  ``server`` [P] and ``params`` [K, P] float32,
    ``loss`` [K] and ``stats`` [2K] float32, ``source`` one of SOURCES or
    "mean".  Returns float64 ``weight`` [K], ``norm`` [K] (0 without
    clip), ``c`` [K] and ``accum`` [P] (``accum`` in + the weighted sum; a
    client with c == 0 adds nothing)."""
    server = np.asarray(server, dtype=np.float32)
    params = np.asarray(params, dtype=np.float32)
    K, P = params.shape
    d = (server[None, :] - params).astype(np.float64)  # one f32 rounding
    weight = np.ones(K)
    norm = np.zeros(K)
    c = np.zeros(K)
    out = (np.zeros(P) if accum is None
           else np.asarray(accum, dtype=np.float64).copy())
    for k in range(K):
        if source != "mean":
            tw = training_weight(source, loss[k], stats[2 * k],
                                 stats[2 * k + 1], counts[k], bs, P)
            weight[k] = softmax_weight(beta, tw)
        dp = 1.0
        if clip:
            norm[k] = math.sqrt(float(np.sum(d[k] * d[k])))
            if norm[k] > max_grad:
                dp = max_grad / norm[k]
        c[k] = weight[k] * dp
        if f32_coef:
            c[k] = float(np.float32(c[k]))
        if c[k] != 0.0:
            out += c[k] * d[k]
    return {"weight": weight, "norm": norm, "c": c, "accum": out}
