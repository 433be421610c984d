"""The device's plan, reports and stage states written as the log of a descheduling run: byte-identical to the
oracle's log, which the reference's own scripts/analysis.py read into tests/golden/desched_log_golden.json
(tests/test_desched_log_contract.py).  Covers ksim.desched.run(..., stages=True) for cosSim and fragOnePod.
Needs a gfx950 device.
"""
import hashlib
import json
import os

import pytest

import desched_log_case as case
import ksim.analysis as A

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "desched_log_golden.json")) as f:
    GOLD = json.load(f)


@pytest.mark.parametrize("policy", case.POLICIES)
def test_gpu_staged_log_equals_golden(policy, tmp_path):
    log = tmp_path / "gpu.log"
    victims, budget = case.engine_log(log, policy)
    want = GOLD["policies"][policy]
    assert (victims, budget) == (want["victims"], want["budget"])
    with open(log) as f:
        got = A.parse_log_full(f.readlines())
    assert {k: float(v) for k, v in got["row"].items()} == want["row"]
    assert hashlib.sha256(log.read_bytes()).hexdigest() == want["log_sha256"]
