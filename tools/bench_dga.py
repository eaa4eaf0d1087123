#!/usr/bin/env python3
"""DGA rounds/s at the benchmark's shape: ``bench.py``'s workload and
timing loop with ``strategy: DGA``, softmax aggregation on the train loss
and, optionally, local DP in clip-only mode (PERF.md).

bench.py itself stays the FedAvg headline; this runs its ``main`` over a
config that differs in the DGA keys only, and takes bench.py's arguments:

    python tools/bench_dga.py --gpus 1 --steps 300 --warmup 20
    BENCH_DGA_CLIP=1 python tools/bench_dga.py ...       # + local-DP clip
    BENCH_DGA_MEGA=0 python tools/bench_dga.py ...       # stream-pool path

``BENCH_DGA_MEGA=0`` sets ``use_mega_round: false``, the per-client
stream-pool path DGA took before it ran on the mega round; run both in
one session to compare.  ``BENCH_DGA_MAX_GRAD`` (default 0.5) and
``BENCH_DGA_BETA`` (default 1.0) set the clip and the softmax.

The result line is bench.py's; a second line names what it was measured
under.
"""

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

CLIP = os.environ.get("BENCH_DGA_CLIP", "0") == "1"
MEGA = os.environ.get("BENCH_DGA_MEGA", "1") == "1"
MAX_GRAD = float(os.environ.get("BENCH_DGA_MAX_GRAD", "0.5"))
BETA = float(os.environ.get("BENCH_DGA_BETA", "1.0"))


def main():
    fedavg_config = bench.build_config

    def build_config(args):
        cfg = fedavg_config(args)
        cfg["strategy"] = "DGA"
        cfg["server_config"]["aggregate_median"] = "softmax"
        cfg["server_config"]["weight_train_loss"] = "train_loss"
        cfg["server_config"]["softmax_beta"] = BETA
        cfg["client_config"]["use_mega_round"] = MEGA
        if CLIP:
            cfg["dp_config"] = {"enable_local_dp": True, "eps": -1.0,
                                "max_grad": MAX_GRAD, "max_weight": 1.0}
        from msrflute_amd.core.client import fused_round_dga
        assert fused_round_dga(cfg) is not None, "the DGA gate rejected it"
        return cfg

    bench.build_config = build_config
    bench.main()
    print(json.dumps({"strategy": "DGA", "softmax_beta": BETA,
                      "local_dp_clip": CLIP,
                      "max_grad": MAX_GRAD if CLIP else None,
                      "use_mega_round": MEGA}))


if __name__ == "__main__":
    main()
