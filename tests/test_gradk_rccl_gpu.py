"""topk gradient compression through a real RCCL communicator on the one-GPU box: a 1-rank
group with the communication forced, one scenario per child process
(tests/topk_one_rank_worker.py), so a communicator never outlives its test."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from dist_helpers import free_port

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _run(scenario, timeout=240):
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()), PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-u", str(ROOT / "tests" / "topk_one_rank_worker.py"),
                        scenario], env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads(lines[-1])
    assert res.get("ok"), res
    return res


def test_rccl_resnet_ddp_topk_equals_codec_by_hand():
    res = _run("resnet_topk")
    assert res["buckets"] >= 2 and res["launched"] == res["expect_launched"]
    # K = 32 of every 2048: 1/42.7 for full blocks, a little less with each bucket's last block
    assert 40 < res["fp32_bytes"] / res["bytes_per_step"] < 42.7
    assert 0 < res["nonzero_share"] <= 32 / 2048 + 1e-3


def test_rccl_lenet_fused_step_topk_in_hipgraph():
    res = _run("lenet_graph_topk")
    assert res["eager_launched"] == 5 * res["buckets"]


def test_rccl_grad_aggregator_topk():
    res = _run("aggregator_topk")
    assert res["comm_time"] > 0 and res["allreduce_bytes"] == res["fp32_bytes"]
    assert 40 < res["fp32_bytes"] / res["bytes_per_call"] < 42.7
