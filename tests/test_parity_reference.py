"""Head-to-head behavior parity against the UNMODIFIED reference
(msrflute/FLUTE) on CPU/gloo.

Runs this engine's e2e_trainer via torch.distributed.run (2 procs, gloo)
on the synthetic LR-MNIST shards and the shared initial checkpoint that
the reference was run on, and asserts the per-round training-loss series,
the final test accuracy and the final checkpoint weights agree with the
reference's to fp tolerance.  The reference's side of the comparison is
the recorded result of that run (tests/golden/parity_lr_mnist/: metric
series + final weights), so the test needs no reference checkout.
Harness: tools/parity/run_parity.py — `--record-golden` re-records the
reference results where a reference checkout is present (its deps
cerberus/easydict/azureml/wget satisfied by the minimal shims in
tools/parity/shims/).
"""

import os
import subprocess
import sys

REPO = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(REPO, "tests", "golden", "parity_lr_mnist")


def test_reference_headtohead_parity(tmp_path):
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "tools", "parity",
                                      "run_parity.py"),
         "--workdir", str(tmp_path / "parity"), "--rounds", "6",
         "--golden", GOLDEN],
        cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"parity FAIL:\n{r.stdout[-4000:]}\n{r.stderr[-2000:]}"
    assert "**PARITY: PASS**" in r.stdout
