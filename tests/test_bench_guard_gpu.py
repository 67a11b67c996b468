"""bench.py's end-of-run guard on the GPU: a 2-rank rehearsal of the headline run (both ranks on
cuda:0, hipIpc one-shot FedAvg) passes the digest check, and the same run with the last rank
skipping one round's FedAvg (its peer's barrier times out) fails it -- exit 3, no throughput line.
VERDICT r3 "next round" 1(a)."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

from tests.helpers import free_port

pytestmark = [pytest.mark.gpu, pytest.mark.slow]
ROOT = Path(__file__).resolve().parent.parent


def _run(tmp_path, *extra, world=2):
    out = tmp_path / "b.json"
    env = dict(os.environ, FEDMI_BENCH_REHEARSE="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes", "1", "--nproc-per-node", str(world),
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), str(ROOT / "bench.py"),
           "--gpus", str(world), "--steps", "3", "--warmup", "1", "--allreduce", "oneshot", "--full",
           "--ckpt-dir", str(tmp_path / "ck"), "--json-out", str(out), *extra]
    p = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=100)
    js = json.loads(out.read_text()) if out.exists() else None
    return p, js


def test_guard_passes_a_correct_run(tmp_path):
    p, js = _run(tmp_path)
    assert p.returncode == 0, p.stderr[-2000:]
    c = js["consistency"]
    assert c["ok"] and c["ranks"] == 2 and c["distinct_digests"] == 1 and c["transport_errors"] == [0, 0]
    assert js["value"] > 0 and '"value"' in p.stdout


def test_guard_fires_on_a_skipped_allreduce(tmp_path):
    p, js = _run(tmp_path, "--inject-fault", "skip-allreduce", "--peer-timeout-ms", "1500")
    assert p.returncode != 0
    assert "CONSISTENCY CHECK FAILED" in p.stderr
    assert js is not None and js["value"] is None and not js["consistency"]["ok"]
    assert '"value"' not in p.stdout            # no throughput line for a diverged run
