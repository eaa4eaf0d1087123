"""``strategy: FedProx`` end to end on the CNN task: the server's gate
(``core.client.fused_round_mu``) must send the round to the mega driver
with ``client_config.mu``, and the result must match the per-client route
(``process_round`` -> ``Trainer.run_train_epoch(prox=...)`` -> the fused CNN
epoch with the term) to the relative 1e-5 that
tests/test_mega_round_gpu.py holds the two routes to under FedAvg.  The
worker is that file's, with the strategy switched (mu = 1: a production mu
would hide a dropped term inside the tolerance); a FedAvg run of the same
rounds must differ by >= 10 x the tolerance, or the comparison says
nothing about the term.
"""

import os
import subprocess
import sys

import pytest

from test_mega_round_gpu import REPO, WORKER as FEDAVG_WORKER

pytestmark = pytest.mark.gpu

TAIL = r"""
w_ref, l_ref = run(mega=False)
w_mega, l_mega = run(mega=True)
w_avg, l_avg = run(mega=True, strategy="FedAvg")
rel = float((w_ref - w_mega).norm() / w_ref.norm())
sep = float((w_avg - w_mega).norm() / w_mega.norm())
print("rel weight diff:", rel, "losses:", l_ref, l_mega,
      "FedAvg differs by:", sep, l_avg)
assert sep >= 1e-4, sep
assert rel < 1e-5, rel
assert abs(l_ref - l_mega) / abs(l_ref) < 1e-4, (l_ref, l_mega)
print("FEDPROX_OK")
"""


def _worker():
    src = FEDAVG_WORKER
    for old, new in [
            ("def run(mega, samples=45):",
             "def run(mega, strategy=\"FedProx\", samples=45):"),
            ("\"strategy\": \"FedAvg\",", "\"strategy\": strategy,"),
            ("\"use_mega_round\": mega,",
             "\"use_mega_round\": mega, \"use_fused_round\": mega, "
             "\"mu\": 1.0,"),
            ("            \"mega round did not engage\"\n",
             "            \"mega round did not engage\"\n"
             "        assert server.executor._mega.mu == "
             "(1.0 if strategy == \"FedProx\" else 0.0)\n")]:
        assert src.count(old) == 1, old
        src = src.replace(old, new)
    head, sep, _ = src.partition("w_ref, l_ref = run(mega=False)")
    assert sep
    return head + TAIL


def test_fedprox_mega_round_matches_per_client_route(tmp_path):
    env = dict(os.environ)
    env.update(REPO=REPO, PYTHONPATH=REPO, OUT=str(tmp_path))
    r = subprocess.run([sys.executable, "-c", _worker()], env=env,
                       capture_output=True, text=True, timeout=600,
                       cwd=REPO)
    print(r.stdout[-1500:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "FEDPROX_OK" in r.stdout
