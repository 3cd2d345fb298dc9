"""bench.py's plain run, --full and --dump-outputs: a plain run measures the headline alone, and
--dump-outputs writes what the last timed step computed -- checked against the golden models."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_full_and_dump_are_off_by_default():
    import bench

    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    b = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert b.full is True and b.dump_outputs == "somewhere"


@pytest.mark.gpu
def test_dump_outputs_is_the_last_steps_result_gpu(native, cuda_device, tmp_path):
    """3 timed steps of 8 epix10k2M frames over a pool of 8: the dump holds every pool frame once, in
    pool order, as float arrays below 64 MB; the sampled calibrated pixels equal the golden model
    bit for bit and the peak counts equal the golden peak finder's."""
    import torch

    from psana_ray_amd.config import PeakFinderParams
    from psana_ray_amd.models import Mode
    from psana_ray_amd.ops import reference
    from psana_ray_amd.producer import build_calibrator
    from psana_ray_amd.source import SyntheticRun

    out = tmp_path / "dump"
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "8",
           "--chunk", "8", "--pool-frames", "8", "--queue-size", "32", "--gate-tol", "0", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
    # a plain run: nothing but the headline
    assert d["extra"]["full"] is False and d["extra"]["xgmi_phase"] is None
    arrays = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    assert set(arrays) == {"calib_frames_sample", "sample_pixel_index", "frame_pool_index", "frame_producer_rank",
                           "peaks", "peak_counts", "peak_summary"}
    assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert d["extra"]["dumped_outputs_rank0"]["frames"] == 8
    assert np.array_equal(arrays["frame_pool_index"], np.arange(8.0))
    idx = arrays["sample_pixel_index"].astype(np.int64)
    assert idx.shape == (1 << 17,) and np.all(np.diff(idx) > 0)
    # the same seeded inputs as the run's
    src = SyntheticRun("synthetic", 0, "epix10k2M", rank=0, size=1, pool_frames=8, gen_device=str(cuda_device))
    cal = build_calibrator(src, cuda_device, Mode.calib, None, "auto")
    params = PeakFinderParams()
    peaks, counts = arrays["peaks"], arrays["peak_counts"].astype(np.int64)
    assert peaks.shape == (8, params.max_peaks, 8) and arrays["peak_summary"].shape == (8, 2)
    for j in (0, 5):
        ref = reference.calibrate_reference(torch.from_numpy(src.pool[j:j + 1].astype(np.int32)), src.consts, None, cal.cm)
        assert np.array_equal(ref.reshape(-1).numpy()[idx], arrays["calib_frames_sample"][j]), f"pool frame {j}"
        ref_peaks, _ = reference.peakfind_reference(ref.reshape(1, *cal.out_shape), params)
        n = int(counts[j])
        assert n == ref_peaks[0].shape[0] and n > 0
        got = peaks[j, :n, :3].astype(np.int64)
        exp = ref_peaks[0][:, :3].to(torch.int64).numpy()
        assert np.array_equal(got, exp[np.lexsort(exp.T[::-1])])   # the dump's records are sorted
        assert not peaks[j, n:].any()
