"""``psana-ray-producer --local --mode raw --consumer_task dark`` on the GPU writes, array for array,
the file the same command writes on a CPU session (and the golden model's accumulators)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _env():
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    return env


def test_local_raw_dark_gpu_equals_cpu_session(native, cuda_device, tmp_path):
    from psana_ray_amd import dark, mkrun
    from psana_ray_amd.models import get_detector
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import open_source

    n = 150                                            # more than two 64-frame batches
    assert mkrun.main(["--data_dir", str(tmp_path), "--exp", "darkexp", "--run", "6", "--detector_name", "tiny_epix",
                       "--num_events", str(n), "--dark", "--format", "praw"]) == 0
    files = {}
    for device in ("cpu", "cuda:0"):
        files[device] = str(tmp_path / f"{device[:3]}.npz")
        r = subprocess.run([sys.executable, "-m", "psana_ray_amd.producer", "--exp", "darkexp", "--run", "6",
                            "--detector_name", "tiny_epix", "--data_dir", str(tmp_path), "--mode", "raw", "--local",
                            "--consumer_task", "dark", "--out_dark", files[device], "--device", device,
                            "--timeout", "60"], env=_env(), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        assert f"dark statistics of {n} frames" in r.stderr, r.stderr[-3000:]
    cpu, gpu = dark.DarkStats.load(files["cpu"]), dark.DarkStats.load(files["cuda:0"])
    assert gpu.key() == cpu.key() and gpu.frames == cpu.frames == n
    for k in ("cnt", "sum", "sq"):
        assert np.array_equal(getattr(gpu, k), getattr(cpu, k)), k
    src = open_source("darkexp", 6, "tiny_epix", data_dir=str(tmp_path))
    frames = []
    while True:
        evs = src.next_events(32)
        if not evs:
            break
        frames.extend(np.array(e.raw, np.uint16, copy=True) for e in evs)
    x = torch.from_numpy(np.stack(frames).view(np.int16)).view(torch.uint16)
    cnt, s, q = reference.dark_accumulate_reference(x, get_detector("tiny_epix").kernel_kind, 0, 65535)
    assert np.array_equal(gpu.cnt, cnt.to(torch.int64).numpy()) and np.array_equal(gpu.sum, s.numpy())
    assert np.array_equal(gpu.sq, q.numpy())
