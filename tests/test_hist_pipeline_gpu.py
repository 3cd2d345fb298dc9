"""pipeline.PixelHistConsumer on a FrameRing (alternating streams, one accumulator each, added on the
device) and ``psana-ray-consumer --task hist`` over HIP IPC -- against the golden model."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import hist as H
from psana_ray_amd.ops import reference
from psana_ray_amd.pipeline import PixelHistConsumer
from psana_ray_amd.source import SyntheticRun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = "tiny_epix"
POOL = 4


@functools.lru_cache(maxsize=None)
def _golden_pool(layout):
    """Calibrated frames [POOL, ...] from the golden model (calib, or assembled images); frame g of a run
    is pool[g % POOL]."""
    from psana_ray_amd.models import make_geometry

    src = SyntheticRun("synthetic", 4, DET, n_events=POOL, pool_frames=POOL, seed=3, gen_device="cpu")
    cal = reference.calibrate_reference(torch.from_numpy(src.pool.astype(np.int32)), src.consts, None, None)
    if layout == "image":
        geo = make_geometry(src.spec)
        cal = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)
    return cal


def _want(frames, lo=-32.0, hi=96.0, nbins=64):
    return reference.pixel_hist_reference(frames.reshape(frames.shape[0], -1), lo, hi, nbins).numpy()


def _feed(cons, ep, frames, batch):
    """Commit ``frames`` into ring slots batch by batch and poll each batch; returns the poll sizes."""
    polls = []
    for a in range(0, frames.shape[0], batch):
        part = frames[a:a + batch]
        slots = [ep.acquire(timeout=5.0) for _ in range(part.shape[0])]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(part[j])
            ep.commit(s, 0, a + j, a + j, None)
        polls.append(cons.poll(timeout=5.0))
    return polls


def _cpu_reference_path(frames, shape, batch, **kw):
    """The consumer's own CPU ``_reference`` path over the same batches."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing(shape, torch.float32, "cpu", 2, 2))
    try:
        cons = PixelHistConsumer(ep, shape, batch=batch, **kw)
        for a in range(0, frames.shape[0], batch):
            cons.process_frames(list(frames[a:a + batch]))
        return cons.stats()
    finally:
        ep.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout,kw", [("calib", {}), ("image", dict(lo=-20.5, hi=300.0, nbins=37))])
def test_three_batches_last_partial_over_alternating_streams(native, cuda_device, layout, kw):
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(layout)
    n_events, batch = 21, 8
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = PixelHistConsumer(ep, shape, detector=DET, layout=layout, batch=batch, **kw)
    assert len(cons._acc) == len(cons.streams) >= 2
    assert cons.acc_bytes == len(cons.streams) * cons.n * cons.nbins * 4
    assert _feed(cons, ep, frames, batch) == [8, 8, 5]
    st = cons.stats()
    want = _want(frames, **kw)
    assert st.hist.dtype == np.int32 and np.array_equal(st.hist, want) and st.frames == n_events
    assert (st.detector, st.layout, st.shape, st.nbins) == (DET, layout, shape, kw.get("nbins", 64))
    assert 0 < int(st.hist.sum()) <= n_events * cons.n
    # every stream's accumulator took part: none holds all samples
    per_acc = [int(a.sum(dtype=torch.int64).cpu()) for a in cons._acc]
    assert sum(per_acc) == int(want.sum()) and max(per_acc) < sum(per_acc)
    # the consumer's own CPU path gives the same words
    cpu = _cpu_reference_path(frames, shape, batch, detector=DET, layout=layout, **kw)
    assert np.array_equal(cpu.hist, st.hist) and cpu.frames == st.frames
    # process_frames (frames that are not queue items) lands in the same run; synchronize() twice is stable
    cons.process_frames([pool[i].to(cuda_device) for i in range(4)])
    st2 = cons.stats()
    assert np.array_equal(st2.hist, _want(torch.cat([frames, pool[:4]]), **kw)) and st2.frames == cons.frames == 25
    assert np.array_equal(cons.synchronize(), st2.hist)
    ep.close()


@pytest.mark.gpu
def test_calibrate_on_read_ring_and_refusals(native, cuda_device):
    """A --calibrate_on_read queue carries RAW uint16 frames: the consumer is built with check_ring=False and
    takes the calibrated frames through process_frames, several batches with a short last one."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool("calib")
    shape = tuple(pool.shape[1:])
    ep = QueueEndpoint(FrameRing(shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        PixelHistConsumer(ep, shape)
    cons = PixelHistConsumer(ep, shape, detector=DET, batch=8, check_ring=False, nbins=256)
    frames = torch.stack([pool[g % POOL] for g in range(19)])
    for a in range(0, 19, 8):
        cons.process_frames([f.to(cuda_device) for f in frames[a:a + 8]])
    st = cons.stats()
    assert st.frames == 19 and np.array_equal(st.hist, _want(frames, nbins=256))
    assert np.array_equal(_cpu_reference_path(frames, shape, 8, nbins=256).hist, st.hist)
    ep.close()
    ep = QueueEndpoint(FrameRing((2, 32, 40), torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="queue frames"):
        PixelHistConsumer(ep, shape)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    for kw in (dict(lo=1.0, hi=0.0), dict(nbins=0), dict(nbins=1025), dict(hi=float("inf"))):
        with pytest.raises(ValueError):
            PixelHistConsumer(ep, shape, **kw)
    # the frame bound: refused before any lease or launch
    cons = PixelHistConsumer(ep, shape, batch=4)
    x = [torch.ones(shape, dtype=torch.float32, device=cuda_device) for _ in range(4)]
    cons.frames = 2 ** 31 - 1 - 3
    with pytest.raises(ValueError, match="past 2147483647"):
        cons.process_frames(x)
    cons.frames = 2 ** 31 - 1
    with pytest.raises(ValueError, match="past 2147483647"):
        cons.poll(timeout=0.0)
    cons.frames = 0
    assert int(cons.synchronize().sum()) == 0
    ep.close()


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_task_hist(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer and ``psana-ray-consumer 0 --task hist --out`` as two GPU processes,
    three batches: the file loads, holds the frames sent and equals the golden model."""
    n_events, run = 20, 12
    src = SyntheticRun("synthetic", run, DET, rank=0, size=1)   # pool generated as the producer process generates it
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    pool = reference.calibrate_reference(raw, src.consts, None, None)
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "hist.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         DET, "--calib", "--common_mode", "off", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "hist", "--out", out, "--batch", "8",
                             "--metrics_interval", "0"],
                            env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    try:
        pout, _ = prod.communicate(timeout=180)
        cout, _ = cons.communicate(timeout=180)
    finally:
        for p in (prod, cons):
            if p.poll() is None:
                p.kill()
                p.communicate()
    assert prod.returncode == 0, pout[-3000:]
    assert cons.returncode == 0, cout[-3000:]
    st = H.PixelHist.load(out)
    frames = torch.stack([pool[g % k] for g in range(n_events)])
    assert st.frames == n_events and st.detector == DET and st.layout == "calib"
    assert np.array_equal(st.hist, _want(frames))
    assert f"hist: frames={n_events} " in cout and "accumulator_bytes=" in cout, cout[-2000:]
