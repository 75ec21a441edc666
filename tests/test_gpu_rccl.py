"""Multi-rank RCCL on ONE GPU: KUNGFU_RCCL_COLOCATE=1 gives
each rank its own RCCL host identity, so 2-3 ranks sharing the card form a real RCCL
communicator over RCCL's socket transport.  Bandwidth is meaningless; what runs is the
real thing: unique-id bootstrap, non-blocking init, ncclAvg buckets issued from the
autograd thread in the auto-learned order, the watchdog, and communicator rebuild after
an elastic resize."""
import json
import os
import re
import subprocess
import sys

import pytest
import torch

from conftest import ROOT, free_port_block, kungfu_run, worker

pytestmark = pytest.mark.gpu
needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")
COLO = {"KUNGFU_FORCE_DEVICE": "0", "KUNGFU_RCCL_COLOCATE": "1", "NCCL_SOCKET_IFNAME": "lo"}


@needs_gpu
@pytest.mark.parametrize("np_", [2, 3])
def test_rccl_colocated_collectives(np_):
    r = kungfu_run(np_, [worker("rccl_colo.py")], timeout=240, extra=["-allow-xgmi"], env=COLO)
    assert r.returncode == 0, r.stdout[-5000:]
    assert r.stdout.count("RCCL_COLO_OK") == np_, r.stdout[-5000:]


@needs_gpu
@pytest.mark.parametrize("plane,dtype", [("rccl", "f32"), ("rccl", "bf16"), ("host", "f32")])
def test_ssgd_matches_single_process_global_batch(plane, dtype):
    env = dict(COLO) if plane == "rccl" else {"KUNGFU_FORCE_DEVICE": "0", "KUNGFU_GPU_DATAPLANE": "host"}
    r = kungfu_run(2, [worker("ssgd_exact.py"), dtype], timeout=300, extra=["-allow-xgmi"], env=env)
    assert r.returncode == 0, r.stdout[-5000:]
    oks = re.findall(r"SSGD_EXACT_OK rank=\d np=2 plane=(\w+)", r.stdout)
    assert oks == [plane, plane], r.stdout[-5000:]


@needs_gpu
def test_rccl_watchdog_names_stalled_bucket():
    r = kungfu_run(2, [worker("rccl_stall.py")], timeout=240, extra=["-allow-xgmi"],
                   env=dict(COLO, KUNGFU_RCCL_TIMEOUT_S="6"))
    out = r.stdout
    assert r.returncode != 0, out[-4000:]
    assert "STALL_NOT_DETECTED rank=0" not in out, out[-4000:]
    assert "kungfu rccl watchdog" in out and "bucket" in out and "has not completed" in out, out[-4000:]


def _bench(env, extra=(), expect_rc=0, gpus=2, batch=16, timeout=600):
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KUNGFU_SELF_SPEC"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "3", "--warmup",
                        "2", "--batch", str(batch), "--full"] + list(extra), cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=timeout)
    if expect_rc != 0:
        assert r.returncode != 0, r.stdout[-5000:]
        return r.stdout
    assert r.returncode == 0, r.stdout[-5000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-5000:]
    return json.loads(lines[0])


@needs_gpu
@pytest.mark.parametrize("plane", ["rccl", "host"])
def test_bench_self_launch_two_ranks(plane):
    """``bench.py --gpus 2`` with no launcher env spawns its 2 ranks itself; the JSON proves
    2 communicating ranks on the named plane and identical replicas."""
    env = dict(COLO) if plane == "rccl" else {"KUNGFU_FORCE_DEVICE": "0", "KUNGFU_GPU_DATAPLANE": "host"}
    res = _bench(env)
    v = res["verify"]
    assert res["n_gpus"] == 2 and res["config"]["parallelism"] == "dp2", res
    assert v["comm_ranks"] == 2 and v["comm_plane"] == plane, v
    assert v["replicas_consistent"] is True, v
    if plane == "rccl":
        assert v["rccl_watchdog"]["ops_watched"] > 0 and v["rccl_watchdog"]["pending"] == 0, v
    pf = v["preflight"]
    assert pf["ok"] is True and pf["errors"] == [], pf
    # one device shared by both ranks: the P2P matrix says so; the value / IPC checks ran
    assert all(str(x).startswith("n/a") for row in pf["p2p"].values() for x in row.values()), pf["p2p"]
    assert all(b and b > 0 for b in pf["allreduce_busbw_gbs"].values()), pf
    assert all(b and b > 0 for b in pf["ipc_pull_gbs"].values()), pf


@needs_gpu
def test_bench_preflight_detects_corrupt_ipc_slot():
    """VERDICT r3 #1a: rank 1 corrupts its exported IPC buffer; rank 0's pull of it fails the
    pre-flight on every rank, exit non-zero within seconds, naming the pair 0 <- 1."""
    import time

    t0 = time.time()
    out = _bench(dict(COLO, KUNGFU_PREFLIGHT_CORRUPT="1"), expect_rc=1)
    assert "pre-flight failed" in out and "IPC pull 0 <- 1 failed" in out, out[-4000:]
    assert time.time() - t0 < 240


@needs_gpu
def test_bench_preflight_stall_skips_ipc_on_every_rank():
    """rank 1 reports its pre-flight all-reduce as stalled (test hook: no stuck kernel);
    every rank then skips the IPC check (its device work would queue behind a real stuck
    collective) and the pre-flight fails, naming rank 1, instead of hanging."""
    out = _bench(dict(COLO, KUNGFU_PREFLIGHT_CORRUPT="1", KUNGFU_PREFLIGHT_CORRUPT_WHAT="stall"), expect_rc=1)
    assert "pre-flight failed" in out and "all-reduce check failed on rank 1" in out, out[-4000:]
    assert "IPC pull" not in out, out[-4000:]


@needs_gpu
def test_elastic_resize_rebuilds_rccl_communicator():
    """kungfu-run -w, 1 -> 2 -> 1 peers with the RCCL plane: the communicator is torn down
    and re-created for every cluster version (parity: KungfuResetNcclHelper,
    srcs/cpp/src/tensorflow/ops/gpu/scheduler.cpp:54-68) and replicas stay identical."""
    base = free_port_block(16)
    cfg = base + 15
    r = kungfu_run(1, [worker("elastic_train.py"), "--schedule", "1:2,2:3,1:2", "--max-step", "7",
                       "--optimizer", "ssgd", "--device", "cuda", "--model", "resnet18", "--global-batch", "16"],
                   timeout=400, port_base=base, env=COLO,
                   extra=["-w", "-allow-xgmi", "-builtin-config-port", str(cfg), "-config-server",
                          "http://127.0.0.1:%d/config" % cfg, "-H", "127.0.0.1:4"])
    assert r.returncode == 0, r.stdout[-5000:]
    steps = re.findall(r"STEP (\d+) np=(\d+) rank=(\d+) loss=(\S+) h=(\w+)", r.stdout)
    by = {}
    for st, np_, rk, loss, h in steps:
        by.setdefault(int(st), []).append((int(np_), h))
    assert sorted(by) == list(range(7)), r.stdout[-3000:]
    for st, rows in by.items():
        assert len(rows) == rows[0][0], (st, rows)
        assert len({h for _, h in rows}) == 1, (st, rows)
    assert any(rows[0][0] == 2 for rows in by.values())
    assert "plane=rccl" in r.stdout, r.stdout[-3000:]


@needs_gpu
@pytest.mark.parametrize("plane", ["host", "rccl"])
def test_monitored_ssgd_adapts_on_gpu(plane):
    """S-SGD(monitor, adapt) on the GPU bucket engine: strategy throughputs
    from the bucket all-reduces (device events on the RCCL plane), an injected slowdown
    flips the strategy on both ranks at the same step."""
    env = dict(COLO) if plane == "rccl" else {"KUNGFU_FORCE_DEVICE": "0", "KUNGFU_GPU_DATAPLANE": "host"}
    r = kungfu_run(2, [worker("adapt_ssgd.py"), "cuda"], timeout=240, extra=["-allow-xgmi"], env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    assert r.stdout.count("ADAPT_OK") == 2, r.stdout[-4000:]


@needs_gpu
@pytest.mark.parametrize("plane", ["host", "rccl"])
def test_bench_elastic_bert_gns(plane):
    """Config 5 (BERT-base + gradient noise scale + resize) as one command on one GPU:
    1 -> 2 ranks; the RCCL run differs from the host-staged one only in the plane."""
    env = dict(COLO) if plane == "rccl" else {"KUNGFU_FORCE_DEVICE": "0", "KUNGFU_GPU_DATAPLANE": "host"}
    e = dict(os.environ, PYTHONPATH=ROOT, **env)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KUNGFU_SELF_SPEC"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "bert_base", "--optimizer", "gns",
                        "--elastic", "1:3,2:4", "--batch", "8"], cwd=ROOT, env=e, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-5000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stderr[-5000:]
    res = json.loads(lines[0])
    assert [p["np"] for p in res["phases"]] == [1, 2], res["phases"]
    assert res["all_phases_consistent"] is True, res["phases"]
    gns = res["phases"][1]["gradient_noise_scale"]
    assert gns is not None and gns == gns, res["phases"]
    print(json.dumps(res))


@needs_gpu
@pytest.mark.parametrize("dtype", ["f32", "bf16"])
def test_hierarchical_bucket_engine_two_fake_hosts_rccl(dtype):
    """Hierarchical S-SGD on the GPU with 2 "hosts" x 2 ranks (conftest.run_fake_hosts):
    per bucket a local RCCL reduce, the host all-reduce among the local roots on the
    cross-host thread, a local RCCL broadcast on the second local communicator -- equal to
    one process on the global batch.  bf16: the wire buffer is cast back into the f32
    gradient on the cross-host stage's stream, after the broadcast."""
    from conftest import run_fake_hosts

    rcs, text = run_fake_hosts([worker("ssgd_exact.py"), dtype, "cuda", "hier"], env=COLO, timeout=300)
    assert all(rc == 0 for rc in rcs), text[-5000:]
    assert text.count("SSGD_EXACT_OK") == 4 and "hier=True" in text, text[-5000:]


@needs_gpu
def test_bench_two_ranks_whole_step_graph():
    """bench.py --graph 1 with 2 colocated RCCL ranks (multi-rank steps default to eager): each rank captures its whole step
    with the comm stream as the capture's origin (bucket all-reduces inside the graph), the ranks
    agree on the capture, replays exchange gradients (every rank draws its own batch, yet the
    replicas end identical)."""
    res = _bench(dict(COLO), extra=["--graph", "1", "--steps", "4", "--warmup", "4"])
    v = res["verify"]
    hg = res["config"]["hip_graph"]
    assert hg["captured"] is True and hg["replays"] >= 4 and not hg["disabled"], hg
    assert hg["segments"] > 2, hg  # segmented N-rank capture (KUNGFU_GRAPH_SEGMENTED=1, default)
    assert v["comm_ranks"] == 2 and v["replicas_consistent"] is True, v


@needs_gpu
def test_bench_two_ranks_graph_disabled_falls_back_to_eager():
    """KUNGFU_GRAPH_MULTIRANK=0: capture refused identically on every rank, eager training."""
    res = _bench(dict(COLO, KUNGFU_GRAPH_MULTIRANK="0"), extra=["--graph", "1", "--steps", "4", "--warmup", "4"])
    v = res["verify"]
    hg = res["config"]["hip_graph"]
    assert hg["captured"] is False and hg["disabled"] is True and hg["replays"] == 0, hg
    assert v["comm_ranks"] == 2 and v["replicas_consistent"] is True, v


@needs_gpu
def test_rccl_collectives_replay_inside_hipgraph():
    """RCCL collectives captured on the capture's own stream (sum, two in a row, ncclAvg) replay
    with correct values, and the process exits cleanly with the graphs alive at shutdown
    (kungfu_amd.finalize releases tracked graphs before destroying the communicator -- without
    that, the communicator's finalize waited on the graph's RCCL resources until the deadline)."""
    r = kungfu_run(2, [worker("rccl_graph.py"), "one,two,avg"], timeout=180, extra=["-allow-xgmi"], env=COLO)
    assert r.returncode == 0, r.stdout[-5000:]
    assert r.stdout.count("RCCL_GRAPH_OK") == 2, r.stdout[-5000:]


@needs_gpu
def test_bench_two_ranks_cta_budget():
    """VERDICT r3 #1b: an explicit RCCL CTA budget (ncclConfig_t.minCTAs / maxCTAs) reaches the
    communicator and is reported in verify.rccl_ctas."""
    res = _bench(dict(COLO, KUNGFU_RCCL_MIN_CTAS="2", KUNGFU_RCCL_MAX_CTAS="8"))
    v = res["verify"]
    assert v["rccl_ctas"] == [2, 8] and v["replicas_consistent"] is True, v


@needs_gpu
def test_bench_eight_colocated_ranks():
    """the N = 8 code path of bench.py before the first real 8-GPU run -- 8 RCCL
    ranks colocated on one device (socket transport): torchrun self-launch, uid bootstrap, the 8-rank
    pre-flight (P2P "n/a", 64 MiB all-reduce value check, IPC pull ring), bucket order learned from
    rank 0, the watchdog, the default N-rank capture (graph segments with eager collectives), the
    per-bucket comm probe and replica checksums; ResNet-50, batch 8 per rank."""
    res = _bench(dict(COLO), gpus=8, batch=8, timeout=900, extra=["--warmup", "4"])
    v = res["verify"]
    assert res["n_gpus"] == 8 and res["config"]["parallelism"] == "dp8", res
    assert v["comm_ranks"] == 8 and v["comm_plane"] == "rccl" and v["replicas_consistent"] is True, v
    pf = v["preflight"]
    assert pf["ok"] is True and pf["ranks"] == 8 and len(pf["devices"]) == 8, pf
    assert all(str(x).startswith("n/a") for row in pf["p2p"].values() for x in row.values()), pf["p2p"]
    assert all(b and b > 0 for b in pf["ipc_pull_gbs"].values()), pf
    assert v["rccl_watchdog"]["ops_watched"] > 0 and v["rccl_watchdog"]["pending"] == 0, v
    assert v["rccl_ctas"] == [16, 64], v["rccl_ctas"]
    hg = res["config"]["hip_graph"]
    assert hg["captured"] is True and hg["segments"] > 2 and hg["replays"] >= 3, hg
    nb = res["config"]["comm"]["buckets"]
    assert len(v["comm_per_bucket_ms"]) == nb and all(t > 0 for t in v["comm_per_bucket_ms"]), v
    assert v["exposed_comm_ms"] is not None and v["exposed_comm_ms"] >= 0, v


@needs_gpu
def test_bench_elastic_bert_gns_four_to_eight_ranks():
    """config 5 at its real sizes -- BERT-base + gradient noise scale, elastic
    4 -> 8 ranks (kungfu-run -w, config server), every rank colocated on one device over RCCL's
    socket transport; both phases keep identical replicas and the 8-rank phase reports a finite
    noise scale."""
    e = dict(os.environ, PYTHONPATH=ROOT, **COLO)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "KUNGFU_SELF_SPEC"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--model", "bert_base", "--optimizer", "gns",
                        "--elastic", "4:3,8:3", "--batch", "4", "--seq-len", "64"], cwd=ROOT, env=e,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-5000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stderr[-5000:]
    res = json.loads(lines[0])
    assert [p["np"] for p in res["phases"]] == [4, 8], res["phases"]
    assert res["all_phases_consistent"] is True, res["phases"]
    gns = res["phases"][1]["gradient_noise_scale"]
    assert gns is not None and gns == gns and abs(gns) != float("inf"), res["phases"]
    assert [(z["from"], z["to"]) for z in res["resizes"]] == [(4, 8)], res["resizes"]
