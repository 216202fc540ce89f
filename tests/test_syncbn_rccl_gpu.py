"""Synchronized BatchNorm through RCCL on the one-GPU box: a 1-rank communicator with the
multi-rank path forced (tests/syncbn_rccl_worker.py, the pattern of tests/test_rccl_gpu.py)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from dist_helpers import free_port

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def test_rccl_one_rank_forced_sync_bn():
    """The native gradient keeps the project's bound against the fp32 torch path
    (rn <= 1.5 * rc + 0.05, rc = bf16 autocast), every layer issues its two collectives per step
    on the dedicated group, and DDP launches as many buckets as without SyncBN."""
    env = dict(os.environ, RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1",
               MASTER_PORT=str(free_port()), PYTHONPATH=str(ROOT))
    r = subprocess.run([sys.executable, "-u", str(ROOT / "tests" / "syncbn_rccl_worker.py")],
                       env=env, capture_output=True, text=True, timeout=240)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert r.returncode == 0 and lines, (r.returncode, r.stdout[-3000:], r.stderr[-3000:])
    res = json.loads(lines[-1])
    assert res.get("ok"), res
    assert res["collectives"] == 2 * 40 and res["finite"]
    assert res["launched"] == res["launched_plain"] > 0
