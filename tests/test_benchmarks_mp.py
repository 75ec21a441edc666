"""Benchmark tools run end to end on the CPU plane (parity: scripts/tests/run-fake-trainer.sh,
run-allreduce-benchmark.sh, kungfu-bench-p2p) and tracing output."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT, kungfu_run


@pytest.mark.parametrize("fuse", [False, True])
def test_fake_trainer_cpu(fuse):
    args = ["-m", "kungfu_amd.benchmarks.fake_trainer", "--model", "resnet18", "--steps", "2", "--epochs", "1"]
    r = kungfu_run(2, args + (["--fuse"] if fuse else []), timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "RESULT:" in r.stdout and '"np":2' in r.stdout, r.stdout[-2000:]


def test_allreduce_benchmark_cpu():
    r = kungfu_run(2, ["-m", "kungfu_amd.benchmarks", "--model", "resnet18", "--steps", "2", "--warmup-steps", "1"],
                   timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "RESULT:" in r.stdout and "GiB/s" in r.stdout


def test_p2p_benchmark_cpu():
    r = kungfu_run(3, ["-m", "kungfu_amd.benchmarks.p2p", "--model", "resnet18", "--steps", "2", "--epochs", "1"],
                   timeout=240)
    assert r.returncode == 0, r.stdout[-3000:]
    assert "RESULT:" in r.stdout


def test_trace_report_native_and_python():
    code = ("import torch, kungfu_amd as kf\n"
            "from kungfu_amd.utils import trace\n"
            "kf.init()\n"
            "m = torch.nn.Linear(4, 4)\n"
            "o = kf.optimizers.SynchronousSGDOptimizer(torch.optim.SGD(m.parameters(), lr=0.1))\n"
            "m(torch.randn(2, 4)).sum().backward(); o.step()\n"
            "with trace.scope('user::scope'): pass\n"
            "kf.ops.all_reduce(torch.ones(3))\n")
    env = dict(os.environ, KUNGFU_CONFIG_ENABLE_TRACE="true", PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    for name in ["optimizer::apply", "user::scope", "session::all_reduce"]:
        assert "[trace] " + name in r.stdout, r.stdout


def test_bench_model_baselines():
    """bench.py's per-model metric and per-GPU baseline (BASELINE.md sync panels at
    global batch 4096 on 16 x V100): ResNet-50 is the headline and the default."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location(
        "kf_bench", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.MODEL_BASELINES["resnet50"] == (b.METRIC, 5507.0 / 16)
    assert abs(b.MODEL_BASELINES["vgg16"][1] - 208.1) < 0.1
    assert abs(b.MODEL_BASELINES["inception_v3"][1] - 464.1) < 0.1
    assert all("SynchronousSGD" in m for m, _ in b.MODEL_BASELINES.values())


def _bench_cpu(extra):
    import json

    e = {k: v for k, v in os.environ.items()
         if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KUNGFU_SELF_SPEC")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--device", "cpu", "--model", "resnet18", "--batch", "2", "--image-size", "32"] + extra,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=240, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_bench_plain_run_dumps_reproducible_outputs(tmp_path):
    """A plain run times exactly --steps steps, reports ms_per_step and leaves the after-run checks
    to --full; --dump-outputs writes the last step's loss, the timed losses and the updated
    parameters / buffers as float32 .npy files, identical from run to run (seeded inputs)."""
    import numpy as np

    runs = []
    for name in ("a", "b"):
        res = _bench_cpu(["--dump-outputs", str(tmp_path / name)])
        assert res["steps"] == 3 and len(res["config"]["losses"]) == 3 and res["ms_per_step"] > 0
        assert res["full"] is False
        v = res["verify"]
        assert v["replicas_consistent"] is None and v["replica_checksum"] is None and v["comm_probe"] is None
        assert all(p.suffix == ".npy" for p in (tmp_path / name).iterdir())
        runs.append({p.stem: np.load(p) for p in sorted((tmp_path / name).iterdir())})
    a, b = runs
    assert sorted(a) == ["buffers", "loss", "losses", "params"]
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for k in a:
        assert a[k].dtype == np.float32 and np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k
    assert a["losses"].shape == (3,) and a["loss"][0] == a["losses"][-1]
    assert np.allclose(a["losses"], res["config"]["losses"], atol=1e-4)
    assert a["params"].size > 0 and a["params"].std() > 0


def test_bench_full_verifies_replicas():
    res = _bench_cpu(["--full"])
    assert res["full"] is True and res["verify"]["replicas_consistent"] is True
    assert len(res["verify"]["replica_checksum"]) == 2
