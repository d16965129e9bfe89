"""ResNet-50 with every BatchNormalization synchronized, two replica processes sharing the box's GPU
(scripts/bench_resnet50.py --sync-bn at 64x64): all the fusion groups that feed batch_norm_train run
synchronized -- conv-epilogue statistics, BN -> ReLU, BN -> Add -> ReLU, the conv-epilogue backward
sums, and (TDL_FUSE_BN_INPUT_MIN_PIXELS=0 forces it at this size) the deferred BN2 -> ReLU apply --
inside the captured whole-step graph, and the replicas end bit-identical."""
import json
import math
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_resnet50_two_replicas_synchronized_bn():
    env = dict(os.environ, PYTHONPATH=ROOT, TDL_SHARE_GPU="1", TDL_FUSE_BN_INPUT_MIN_PIXELS="0", TDL_BN_DEBUG="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "TF_CONFIG", "TDL_LAUNCHED", "MASTER_ADDR",
              "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "scripts/bench_resnet50.py", "--image", "64", "--conv-search", "0", "--gpus", "2",
                        "--batch", "16", "--steps", "3", "--warmup", "3", "--sync-bn"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "capture failed" not in r.stderr, r.stderr[-3000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    c = d["config"]
    assert d["n_gpus"] == 2 and c["replicas_identical"] and c["allreduce"].startswith("xgmi"), c
    assert c["buckets"]["overlapped_with_backward"], c
    assert c["sync_bn"]["layers"] == 53 and c["sync_bn"]["exchanges_per_step"] == 106, c
    assert len(c["sync_bn"]["exchange_elements"]) == 6, c  # C = 64 ... 2048, none the size of a bucket
    assert math.isfinite(c["final_loss"]) and c["final_loss"] < 2 * math.log(1000), c
    # which forms ran synchronized (TDL_BN_DEBUG names each once): statistics from a conv epilogue, the
    # deferred apply, and backward sums from a conv's input-gradient epilogue
    assert "'sync-fwd'" in r.stderr and "'stats-fused', 'apply-deferred'" in r.stderr, r.stderr[-3000:]
    assert "'sync-bwd'" in r.stderr and "'sums-fused'" in r.stderr, r.stderr[-3000:]
    assert "('fwd'" not in r.stderr and "('bwd'" not in r.stderr  # no layer took the unsynchronized path
