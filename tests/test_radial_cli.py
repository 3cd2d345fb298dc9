"""``psana-ray-consumer --task radial`` / ``psana-ray-producer --consumer_task radial`` as separate
processes: two consumers' accumulators merge to the golden accumulator, bit for bit."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


def _producer(addr, n_cons, extra, rank=0, size=1):
    return subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", "7", "--detector_name",
         "tiny_epix", "--calib", "--ray_address", addr, "--num_consumers", str(n_cons), "--queue_size", "6",
         "--device", "cpu", "--common_mode", "off", "--timeout", "60", *extra],
        env=_env({"RANK": str(rank), "WORLD_SIZE": str(size), "LOCAL_RANK": "0"}), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)


def _consumer(addr, cid, extra, device="cpu"):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", str(cid), "--ray_address", addr,
                             "--device", device, "--timeout", "60", "--task", "radial", "--metrics_interval", "0", *extra],
                            env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def test_two_consumers_merge_to_the_golden_accumulator_cpu(native, tmp_path):
    from psana_ray_amd import radial
    from psana_ray_amd.models import RadialBinning, make_geometry
    from psana_ray_amd.models.radial import DEFAULT_FRAC_BITS, DEFAULT_VMAX, DEFAULT_VMIN
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    n_events, nbins = 12, 24
    outs_npz = [str(tmp_path / f"c{c}.npz") for c in range(2)]
    prod = _producer(addr, 2, ["--num_events", str(n_events)])
    # no --detector_name: the detector comes from the session metadata
    cons = [_consumer(addr, c, ["--nbins", str(nbins), "--out", outs_npz[c]]) for c in range(2)]
    outs = []
    try:
        for p in [prod] + cons:
            out, _ = p.communicate(timeout=180)
            outs.append((p.returncode, out))
    finally:
        for p in [prod] + cons:
            if p.poll() is None:
                p.kill()
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    assert all("detector=tiny_epix" in out and "layout=calib" in out for _, out in outs[1:]), outs[1][1][-2000:]
    m = radial.merge(outs_npz)
    src = SyntheticRun("synthetic", 7, "tiny_epix", rank=0, size=1)   # pool generated as the producer process generates it
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    frames = reference.calibrate_reference(raw, src.consts, None, None)
    rb = RadialBinning.from_geometry(make_geometry(src.spec), "calib", nbins)
    sums, counts, prof = reference.radial_profile_reference(frames, rb.bins, nbins, DEFAULT_VMIN, DEFAULT_VMAX,
                                                            DEFAULT_FRAC_BITS)
    assert m["frames"] == n_events and int(counts.sum()) > 0
    assert m["run_sum"].dtype == np.int64 and np.array_equal(m["run_sum"], sums.sum(0).numpy())
    assert np.array_equal(m["run_count"], counts.to(torch.int64).sum(0).numpy())
    want_mean = radial.mean_profile(sums.sum(0).numpy(), counts.to(torch.int64).sum(0).numpy(), DEFAULT_FRAC_BITS)
    assert np.array_equal(m["mean_profile"].view(np.int32), want_mean.view(np.int32))
    # per-frame profiles: every event exactly once over the two files, each bitwise the golden one
    assert sorted(m["idx"].tolist()) == list(range(n_events))
    assert np.array_equal(m["profiles"].view(np.int32), prof.numpy()[m["idx"]].view(np.int32))
    assert np.array_equal(m["centers"], rb.centers) and m["params"]["nbins"] == nbins


@pytest.mark.parametrize("device", ["cpu", pytest.param("cuda:0", marks=pytest.mark.gpu)])
def test_calibrate_on_read_queue_is_calibrated_then_integrated(native, tmp_path, device):
    """A --calibrate_on_read queue carries RAW frames: the consumer calibrates (image mode, common mode)
    and integrates with the image-layout bin map; the accumulator equals the golden one bitwise."""
    from psana_ray_amd.config import resolve_common_mode
    from psana_ray_amd.models import RadialBinning, make_geometry
    from psana_ray_amd.models.radial import DEFAULT_FRAC_BITS, DEFAULT_VMAX, DEFAULT_VMIN
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    n_events, nbins = 6, 16
    out_npz = str(tmp_path / "c.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", "8", "--detector_name",
         "tiny_epix", "--num_events", str(n_events), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
         "--device", device, "--common_mode", "default", "--calibrate_on_read", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)
    cons = _consumer(addr, 0, ["--nbins", str(nbins), "--out", out_npz], device=device)
    try:
        pout, _ = prod.communicate(timeout=180)
        cout, _ = cons.communicate(timeout=180)
    finally:
        for p in (prod, cons):
            if p.poll() is None:
                p.kill()
    assert prod.returncode == 0, pout[-3000:]
    assert cons.returncode == 0 and "layout=image" in cout, cout[-3000:]
    src = SyntheticRun("synthetic", 8, "tiny_epix", rank=0, size=1)   # pool generated as the producer process generates it
    geo = make_geometry(src.spec)
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    cal = reference.calibrate_reference(raw, src.consts, None, resolve_common_mode("default", src.spec))
    img = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)
    rb = RadialBinning.from_geometry(geo, "image", nbins)
    sums, counts, _ = reference.radial_profile_reference(img, rb.bins, nbins, DEFAULT_VMIN, DEFAULT_VMAX,
                                                         DEFAULT_FRAC_BITS)
    with np.load(out_npz) as z:
        assert int(z["frames"]) == n_events
        assert np.array_equal(z["run_sum"], sums.sum(0).numpy())
        assert np.array_equal(z["run_count"], counts.to(torch.int64).sum(0).numpy())


def test_panel_sharded_session_is_refused_cpu(native):
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    prods = [_producer(addr, 1, ["--num_events", "4", "--panel_shards", "2"], rank=r, size=2) for r in range(2)]
    cons = _consumer(addr, 0, [])
    try:
        out, _ = cons.communicate(timeout=120)
    finally:
        for p in prods + [cons]:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    assert cons.returncode == 2, out[-3000:]
    lines = [l for l in out.splitlines() if "--task radial" in l]
    assert len(lines) == 1 and "panel shards" in lines[0] and "Traceback" not in out, out[-3000:]


@pytest.mark.gpu
def test_producer_local_gpu_radial(cuda_device):
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", "1",
                        "--detector_name", "epix10k2M", "--calib", "--common_mode", "default", "--local",
                        "--consumer_task", "radial", "--num_events", "64"], env=_env(), capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "produced 64 frames" in r.stderr
    assert "co-located consumer processed 64 frames, radial accumulator of 64 frames" in r.stderr
