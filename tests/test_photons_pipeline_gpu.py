"""pipeline.PhotonConsumer on a FrameRing (alternating streams, one accumulator set each, added on the
device; per-frame rows copied to the host stream-ordered) and ``psana-ray-consumer --task photons`` over HIP
IPC -- against the golden model."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import photons as PH
from psana_ray_amd.ops import reference
from psana_ray_amd.pipeline import PhotonConsumer
from psana_ray_amd.source import SyntheticRun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = "tiny_epix"
POOL = 4
ADU = 20.0


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


def _want(frames, shape, mask=None, roi=None, n_roi=None, **par):
    return reference.photon_count_reference(frames.reshape(frames.shape[0], -1), shape,
                                            dict(adu_per_photon=ADU, **par), mask, roi, n_roi)


def _same(st, want, n_events):
    assert st.frames == n_events
    for k in ("cnt", "psum", "occ", "pk", "tot"):
        g, w = getattr(st, k), getattr(want, k).numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), k


def _feed(cons, ep, frames, batch):
    """Commit ``frames`` into ring slots batch by batch and poll each batch; returns the poll sizes."""
    polls = []
    for a in range(0, frames.shape[0], batch):
        part = frames[a:a + batch]
        slots = [ep.acquire(timeout=5.0) for _ in range(part.shape[0])]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(part[j])
            ep.commit(s, 0, a + j, 100 + a + j, None if (a + j) % 2 else 9.5)
        polls.append(cons.poll(timeout=5.0))
    return polls


def _cpu_reference_path(frames, shape, batch, **kw):
    """The consumer's own CPU ``_reference`` path over the same batches."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing(shape, torch.float32, "cpu", 2, 2))
    try:
        cons = PhotonConsumer(ep, shape, ADU, batch=batch, **kw)
        for a in range(0, frames.shape[0], batch):
            cons.process_frames(list(frames[a:a + batch]), [(0, g, 100 + g) for g in range(a, min(a + batch, len(frames)))])
        return cons.stats()
    finally:
        ep.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["calib", "image"])
def test_three_batches_last_partial_over_alternating_streams(native, cuda_device, layout):
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(layout)
    n_events, batch = 21, 8
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    n = int(np.prod(shape))
    rng = np.random.default_rng(2)
    kw = {}
    if layout == "calib":   # the image runs without maps, the calib layout with a mask and three ROIs
        kw = dict(mask=(rng.random(n) < 0.9).astype(np.uint8), roi=rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n),
                  thr_seed=0.45, thr_total=0.8, vmax=3000.0)
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = PhotonConsumer(ep, shape, ADU, detector=DET, layout=layout, batch=batch, **kw)
    assert len(cons._acc) == len(cons.streams) >= 2 and cons.n_roi == (3 if kw else 1)
    assert _feed(cons, ep, frames, batch) == [8, 8, 5]
    st = cons.stats()
    want = _want(frames, shape, **kw)
    _same(st, want, n_events)
    assert (st.detector, st.layout, st.shape, st.n_roi) == (DET, layout, shape, cons.n_roi)
    assert st.gevt.tolist() == list(range(100, 121)) and st.idx.tolist() == list(range(21)) and set(st.rank) == {0}
    assert np.array_equal(np.isnan(st.photon_energy), np.arange(21) % 2 == 1) and st.photon_energy[0] == 9.5
    assert 0 < int(st.psum.sum()) and int(st.tot.sum()) <= int(st.psum.sum())
    # every stream's accumulator set took part: none holds all photons
    per_acc = [int(a[1].sum().cpu()) for a in cons._acc]
    assert sum(per_acc) == int(want.psum.sum()) and max(per_acc) < sum(per_acc)
    # the consumer's own CPU path gives the same words
    cpu = _cpu_reference_path(frames, shape, batch, detector=DET, layout=layout, **kw)
    _same(cpu, want, n_events)
    assert cpu.roi_sha256 == st.roi_sha256 and np.array_equal(cpu.roi_npix, st.roi_npix)
    # process_frames (frames that are not queue items) lands in the same run; stats() twice is stable
    cons.process_frames([pool[i].to(cuda_device) for i in range(4)], [(1, i, 500 + i, 7.0) for i in range(4)])
    st2 = cons.stats()
    _same(st2, _want(torch.cat([frames, pool[:4]]), shape, **kw), 25)
    assert st2.gevt[-4:].tolist() == [500, 501, 502, 503] and st2.rank[-4:].tolist() == [1] * 4
    st3 = cons.stats()
    assert np.array_equal(st3.psum, st2.psum) and np.array_equal(st3.pk, st2.pk)
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
        PhotonConsumer(ep, shape, ADU)
    cons = PhotonConsumer(ep, shape, ADU, detector=DET, batch=8, check_ring=False)
    frames = torch.stack([pool[g % POOL] for g in range(19)])
    for a in range(0, 19, 8):
        cons.process_frames([f.to(cuda_device) for f in frames[a:a + 8]], [(0, g, g) for g in range(a, min(a + 8, 19))])
    st = cons.stats()
    _same(st, _want(frames, shape), 19)
    assert st.gevt.tolist() == list(range(19)) and bool(np.isnan(st.photon_energy).all())
    ep.close()
    ep = QueueEndpoint(FrameRing((2, 32, 40), torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="queue frames"):
        PhotonConsumer(ep, shape, ADU)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    n = int(np.prod(shape))
    for kw in (dict(adu_per_photon=0.0), dict(adu_per_photon=None), dict(vmax=255.0 * ADU), dict(thr_seed=0.0),
               dict(thr_seed=0.95), dict(thr_total=2.0), dict(mask=np.ones(n - 1, np.uint8)),
               dict(roi=np.full(n, 8, np.uint8)), dict(roi=np.zeros(n, np.uint8), n_roi=9), dict(n_roi=2)):
        with pytest.raises(ValueError):
            PhotonConsumer(ep, shape, **{**dict(adu_per_photon=ADU), **kw})
    with pytest.raises(ValueError):
        PhotonConsumer(ep, (n,), ADU)
    # the frame bound: refused before any lease or launch
    cons = PhotonConsumer(ep, shape, ADU, batch=4)
    x = [torch.ones(shape, dtype=torch.float32, device=cuda_device) for _ in range(4)]
    cons.frames = 2 ** 31 - 1 - 3
    with pytest.raises(ValueError, match="past 2147483647"):
        cons.process_frames(x, [(0, i, i) for i in range(4)])
    cons.frames = 2 ** 31 - 1
    with pytest.raises(ValueError, match="past 2147483647"):
        cons.poll(timeout=0.0)
    cons.frames = 0
    with pytest.raises(ValueError, match="batch of at most"):
        cons.process_frames(x + x, [(0, i, i) for i in range(8)])
    assert int(cons.synchronize()["psum"].sum()) == 0 and not cons.results
    ep.close()


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_task_photons(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer and ``psana-ray-consumer 0 --task photons --out`` as two GPU processes,
    three batches: the file loads, holds the frames sent and equals the golden model."""
    n_events, run = 20, 13
    src = SyntheticRun("synthetic", run, DET, rank=0, size=1)   # pool generated as the producer process generates it
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    pool = reference.calibrate_reference(raw, src.consts, None, None)
    shape = tuple(pool.shape[1:])
    roi = np.zeros(shape, np.uint8)
    roi[1] = 1
    roi[:, :2] = 255
    roi_path = str(tmp_path / "roi.npy")
    np.save(roi_path, roi)
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "photons.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         DET, "--calib", "--common_mode", "off", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "photons", "--adu_per_photon", str(ADU),
                             "--photon_roi", roi_path, "--out", out, "--batch", "8", "--metrics_interval", "0"],
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
    st = PH.PhotonStats.load(out)
    frames = torch.stack([pool[g % k] for g in range(n_events)])
    assert st.detector == DET and st.layout == "calib" and st.n_roi == 2
    _same(st, _want(frames, shape, roi=roi.reshape(-1), n_roi=2), n_events)
    assert sorted(st.gevt.tolist()) == list(range(n_events))
    assert f"photons: frames={n_events} " in cout and "rois=2" in cout, cout[-2000:]
