#!/usr/bin/env python3
"""Self-attention segment timing (PERF.md, "Short-sequence attention on the
MFMA"): fednewsrec's ``SelfAttention(400, 20, 20)``, forward + backward with
a gradient for ``x``, at ``[880, 28, 400]`` (titles) and ``[16, 50, 400]``
(click histories).

Three paths in one process, alternating, on one set of weights:

* ``sdpa``: ``F.scaled_dot_product_attention`` on head views;
* ``lanes``: ``fused_mha(..., impl="lanes")`` (csrc/mha_small.hip);
* ``mfma``: ``fused_mha(..., impl="mfma")`` (csrc/mha_mfma.hip).

Every shape is warmed; five windows of about 100 calls per path, each ending
in a device synchronise; lowest - highest microseconds per call, and the
largest output and input-gradient difference between the paths.
``--profile`` runs 20 calls per path after the warm-up and nothing else, for
a kernel trace.

    python tools/bench_mha.py
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_mha.py \\
        --profile
"""

import argparse
import importlib.util
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

DIM, HEADS, HEAD_DIM = 400, 20, 20
SHAPES = ((880, 28), (16, 50))
PATHS = {"sdpa": False, "lanes": True, "mfma": "mfma"}


def _model_module():
    spec = importlib.util.spec_from_file_location(
        "fednewsrec_model_bench_mha",
        os.path.join(REPO, "experiments", "fednewsrec", "model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Segment:
    def __init__(self, attn, n, L):
        torch.manual_seed(n)
        self.attn = attn
        self.x = torch.randn(n, L, DIM, device="cuda", requires_grad=True)
        self.dy = torch.randn(n, L, DIM, device="cuda")

    def step(self, fused):
        self.attn.fused = fused
        for p in list(self.attn.parameters()) + [self.x]:
            p.grad = None
        out = self.attn(self.x)
        out.backward(self.dy)
        return out

    def results(self, fused):
        out = self.step(fused).detach()
        return {"y": out.clone(), "dx": self.x.grad.clone()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mha.py needs a GPU")

    torch.manual_seed(400)
    attn = _model_module().SelfAttention(DIM, HEADS, HEAD_DIM).cuda()
    for n, L in SHAPES:
        seg = Segment(attn, n, L)
        for fused in PATHS.values():
            for _ in range(20):
                seg.step(fused)
        torch.cuda.synchronize()
        if args.profile:
            for fused in PATHS.values():
                for _ in range(20):
                    seg.step(fused)
                torch.cuda.synchronize()
            continue
        res = {name: seg.results(fused) for name, fused in PATHS.items()}
        times = {name: [] for name in PATHS}
        for _ in range(args.windows):
            for name, fused in PATHS.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    seg.step(fused)
                torch.cuda.synchronize()
                times[name].append(
                    (time.perf_counter() - t0) / args.calls * 1e6)
        print(f"[{n}, {L}, {DIM}]")
        for name, ts in times.items():
            print(f"  {name:6s} {min(ts):8.1f} - {max(ts):8.1f} us")
        for name in ("lanes", "mfma"):
            diffs = ", ".join(
                f"{k} {(res[name][k] - v).abs().max().item():.2e} "
                f"(to {v.abs().max().item():.3g})"
                for k, v in res["sdpa"].items())
            print(f"  {name} - sdpa: {diffs}")
        sys.stdout.flush()


if __name__ == "__main__":
    main()
