#!/usr/bin/env python3
"""FedProx rounds/s at the benchmark's shape: ``bench.py``'s workload and
timing loop with ``strategy: FedProx`` and ``client_config.mu`` (PERF.md).

bench.py itself stays the FedAvg headline; this runs its ``main`` over a
config that differs in those two keys only, and takes bench.py's
arguments:

    python tools/bench_fedprox.py --gpus 1 --steps 300 --warmup 20
    BENCH_MU=0.01 python tools/bench_fedprox.py ...

The result line is bench.py's; a second line names the strategy and mu it
was measured under.
"""

import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402

MU = float(os.environ.get("BENCH_MU", "0.001"))


def main():
    fedavg_config = bench.build_config

    def build_config(args):
        cfg = fedavg_config(args)
        cfg["strategy"] = "FedProx"
        cfg["client_config"]["mu"] = MU
        return cfg

    bench.build_config = build_config
    bench.main()
    print(json.dumps({"strategy": "FedProx", "mu": MU}))


if __name__ == "__main__":
    main()
