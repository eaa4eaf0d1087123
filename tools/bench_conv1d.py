#!/usr/bin/env python3
"""Title-convolution segment timing (PERF.md, "Title convolution:
backward-weights"): ``Dropout(0)`` -> conv -> ReLU -> ``nn.Linear(400, 400)``,
forward + backward, at ``[880, 30, 300]`` and ``[80, 30, 300]``, with and
without a gradient for ``x``.

Three paths in one process, alternating:

* ``torch``: ``nn.Conv1d`` on transposed views, then ``F.relu``;
* ``library-dW``: the fused forward with the weight gradient as three
  library GEMMs over ``dz_pad``, the backward ``fused_conv1d_relu`` had
  before csrc/conv1d_bwd_w.hip (kept here as the yardstick for that kernel);
* ``fused``: ``fused_conv1d_relu`` as shipped.

Every shape is warmed; five windows of about 100 calls per path, each ending
in a device synchronise; lowest - highest microseconds per call, and the
largest output difference between the paths.  ``--profile`` runs 20 calls
per path after the warm-up and nothing else, for a kernel trace.

    python tools/bench_conv1d.py
    rocprofv3 --kernel-trace --stats -d out -- python tools/bench_conv1d.py \\
        --profile --n 880
"""

import argparse
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402
from torch import nn  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from msrflute_amd.ops import _C  # noqa: E402
from msrflute_amd.ops.attention import _aligned  # noqa: E402
from msrflute_amd.ops.conv1d import _conv1d_pack, fused_conv1d_relu  # noqa: E402

T, CIN, COUT, KW = 30, 300, 400, 3


class _LibraryDW(torch.autograd.Function):
    """The fused forward and backward-data with dW, db as library work."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        x, wp = _aligned(x), _conv1d_pack(weight)
        y = _C.conv1d_relu_fwd(x, wp, _aligned(bias.detach()))
        ctx.save_for_backward(x, y, wp)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, y, wp = ctx.saved_tensors
        dx, dz = _C.conv1d_relu_bwd(y, wp, _aligned(dy),
                                    ctx.needs_input_grad[0])
        dz, xf = dz.flatten(0, 1), x.flatten(0, 1)
        R = xf.shape[0]
        dw = torch.stack([dz[:R - k].t() @ xf[k:]
                          for k in range(wp.shape[0])], dim=2)
        return (dx if ctx.needs_input_grad[0] else None), dw, dz.sum(0)


def _torch_conv(x, w, b):
    return F.relu(F.conv1d(x.transpose(1, 2), w, b)).transpose(1, 2)


PATHS = {"torch": _torch_conv, "library-dW": _LibraryDW.apply,
         "fused": fused_conv1d_relu}


class Segment:
    def __init__(self, n, need_dx):
        torch.manual_seed(n)
        self.x = torch.randn(n, T, CIN, device="cuda", requires_grad=need_dx)
        self.dy = torch.randn(n, T - KW + 1, COUT, device="cuda")
        self.conv = nn.Conv1d(CIN, COUT, KW).cuda()
        self.lin = nn.Linear(COUT, COUT).cuda()
        self.drop = nn.Dropout(0.0)
        self.params = [self.conv.weight, self.conv.bias, self.lin.weight,
                       self.lin.bias]

    def step(self, op):
        for p in self.params + [self.x]:
            p.grad = None
        out = self.lin(op(self.drop(self.x), self.conv.weight,
                          self.conv.bias))
        out.backward(self.dy)
        return out

    def results(self, op):
        out = self.step(op).detach()
        named = {"out": out, "dWconv": self.conv.weight.grad,
                 "dbconv": self.conv.bias.grad, "dWlin": self.lin.weight.grad}
        if self.x.grad is not None:
            named["dx"] = self.x.grad
        return {k: v.clone() for k, v in named.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="*", default=[880, 80])
    ap.add_argument("--calls", type=int, default=100)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--profile", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_conv1d.py needs a GPU")

    for n in args.n:
        for need_dx in (False, True):
            seg = Segment(n, need_dx)
            for op in PATHS.values():
                for _ in range(20):
                    seg.step(op)
            torch.cuda.synchronize()
            if args.profile:
                for op in PATHS.values():
                    for _ in range(20):
                        seg.step(op)
                    torch.cuda.synchronize()
                continue
            res = {name: seg.results(op) for name, op in PATHS.items()}
            times = {name: [] for name in PATHS}
            for _ in range(args.windows):
                for name, op in PATHS.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        seg.step(op)
                    torch.cuda.synchronize()
                    times[name].append(
                        (time.perf_counter() - t0) / args.calls * 1e6)
            print(f"[{n}, {T}, {CIN}] x.requires_grad={need_dx}")
            for name, ts in times.items():
                print(f"  {name:11s} {min(ts):8.1f} - {max(ts):8.1f} us")
            for name in ("library-dW", "fused"):
                diffs = ", ".join(
                    f"{k} {(res[name][k] - v).abs().max().item():.2e} "
                    f"(to {v.abs().max().item():.3g})"
                    for k, v in res["torch"].items())
                print(f"  {name} - torch: {diffs}")
            sys.stdout.flush()


if __name__ == "__main__":
    main()
