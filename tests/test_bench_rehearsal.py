"""bench.py's multi-rank flow (queue session on torchrun's store, links between every pair of
ranks, timing windows, barriers, drain, EOS, teardown) rehearsed on the CPU with
torch.distributed.run and a tiny detector -- the driver's launch shape, including 8 ranks with and
without --producers 4 (BASELINE config 3).  Host rings in shared memory stand in for HBM rings
written over xGMI; everything else is the code the 8-GPU run executes."""
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("nproc,route,producers", [(2, "balanced", 0), (4, "spread", 0), (4, "balanced", 2),
                                                   (8, "balanced", 0), (8, "balanced", 4), (2, "balanced", 1)])
def test_bench_multirank_cpu(native, nproc, route, producers):
    env = dict(os.environ)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    port = random.randint(30000, 45000)
    # config-3 shapes (producers < ranks): a lone producer's consumer-only rank covers a 4-step
    # window from its read-ahead alone, and the consumer vs producer rate comparison needs a window
    # long against the queue slack -- 48 steps
    steps = 48 if producers else 4
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
           "--gpus", str(nproc), "--steps", str(steps), "--warmup", "2", "--batch", "4", "--detector", "tiny_epix",
           "--device", "cpu", "--queue-size", str(16 * nproc), "--chunk", "4", "--route", route,
           "--producers", str(producers), "--full"]   # --full: the cross window asserted below
    if producers:
        # config 3 shape: the consumers only take frames (the CPU golden peak finder would be the
        # bottleneck of a CPU rehearsal, not the queue), so the node must consume at the producers' rate
        cmd += ["--consumer", "none"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["n_ranks"] == nproc and d["n_gpus"] == 0 and d["steps"] == steps and d["value"] > 0
    assert d["config"]["global_batch"] == 4 * nproc
    assert d["config"]["producer_ranks"] == (producers or nproc)
    x = d["extra"]["xgmi_phase"]
    assert x is not None and x["route"] == "remote_only" and x["frames_per_s"] > 0
    assert d["extra"]["validation"] == "ok", d["extra"]["validation"]
    n_p = producers or nproc
    assert len(x["bytes_sent_per_rank"]) == nproc
    # frames cross ranks in the cross window (from most producers), consumer-only ranks send nothing
    assert sum(x["bytes_sent_per_rank"]) > 0, x
    assert sum(b > 0 for b in x["bytes_sent_per_rank"][:n_p]) >= max(1, n_p // 2), x
    # remote_only: a producer never keeps a frame for its own consumer while a remote one is linked
    # (the cross window must really cross; bench.py exits 4 below 0.9)
    assert x["cross_gpu_fraction"] >= 0.9, x
    assert all(b == 0 for b in x["bytes_sent_per_rank"][n_p:]), x
    if producers:
        # BASELINE config 3 shape: consumer-only ranks get every frame they consume
        # from another process, and the node consumes at the producers' rate -- to within the queue
        # slack: production inside the window also refills the queue (queue_size 16 frames per rank
        # against 192 consumed per rank in the window, i.e. up to ~8 %), and 8 ranks share 8 CPUs
        share = d["extra"]["recv_cross_per_consumed_per_rank"]
        assert all(v >= 0.9 for v in share[n_p:]), share
        assert all(c > 0 for c in d["extra"]["consumed_per_rank"]), d["extra"]["consumed_per_rank"]
        assert d["extra"]["consumer_frames_per_s"] >= 0.90 * d["extra"]["production_frames_per_s"], d["extra"]
    # the steady-state gate replaced the fixed pre-roll (collective decision,
    # bounded), and the line carries per-rank topology evidence of every link
    g = d["extra"]["steady_gate"]
    assert g is not None and g["iterations"] >= 2 and g["tol"] == 0.03, g
    assert g["converged"] or g["seconds"] >= 10.0, g
    t = d["extra"]["topology"]
    assert len(t["device_per_rank"]) == nproc and len(t["outgoing_links_per_rank"]) == nproc
    for r, links in enumerate(t["outgoing_links_per_rank"]):
        want = (nproc - 1) if r < n_p else 0
        assert len(links) == want, (r, links)
        for lk in links:
            assert set(lk) == {"peer", "consumer_device", "attached", "kernel_copy", "peer_access", "link_type", "hops"}
            assert lk["attached"] and lk["consumer_device"] == -1 and not lk["kernel_copy"]   # host rings (CPU)


@pytest.mark.parametrize("nproc", [2, 8])
def test_bench_self_launch_cpu(native, nproc):
    """The driver's plain command, ``python bench.py --gpus N ...`` with NO launcher around it
    (VERDICT r5 missing #1): bench.py starts its N ranks itself as child processes, rank 0 prints
    exactly one JSON line and the job exits 0."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT",
                        "TORCHELASTIC_RUN_ID", "OMPI_COMM_WORLD_RANK", "PMI_RANK", "SLURM_PROCID")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "4", "--warmup", "2",
           "--batch", "4", "--detector", "tiny_epix", "--device", "cpu", "--queue-size", str(16 * nproc),
           "--chunk", "4", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd="/tmp")
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    assert d["n_ranks"] == nproc and d["config"]["launch"] == "self-launched children"
    assert d["extra"]["validation"] == "ok" and d["extra"]["xgmi_phase"]["frames_per_s"] > 0
    assert "self-launched" in r.stderr


def test_bench_self_launch_failure_propagates(native):
    """A rank that fails makes the self-launched job fail (worst child rc), without hanging."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--device", "cpu", "--detector",
           "tiny_epix", "--producers", "5"]   # invalid on every rank -> rc 2
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300, cwd="/tmp")
    assert r.returncode == 2, (r.returncode, r.stderr[-2000:])


def test_bench_self_launch_ranks_die_with_the_launcher(native):
    """A self-launched job whose parent is killed (a caller's timeout) leaves no rank running."""
    import signal
    import time

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "100000", "--warmup", "2",
           "--batch", "4", "--detector", "tiny_epix", "--device", "cpu", "--queue-size", "32", "--chunk", "4"]
    p = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, cwd="/tmp")
    pids = []
    t0 = time.time()
    while time.time() - t0 < 60 and not pids:   # the parent announces its ranks' pids on stderr
        line = p.stderr.readline()
        if "self-launched" in line:
            pids = [int(x) for x in line.split("pids [")[1].split("]")[0].split(",")]
    assert len(pids) == 2, "no self-launch line"
    time.sleep(3.0)
    p.send_signal(signal.SIGKILL)   # the parent dies without a chance to clean up
    p.wait(30)

    def alive(pid):
        try:
            os.kill(pid, 0)
        except ProcessLookupError:
            return False
        with open(f"/proc/{pid}/stat") as f:   # a zombie waiting for its reaper counts as gone
            return f.read().split(")")[-1].split()[0] != "Z"

    t1 = time.time()
    while time.time() - t1 < 20 and any(alive(x) for x in pids):
        time.sleep(0.2)
    assert not any(alive(x) for x in pids), pids
