"""pipeline.RoiConsumer on a FrameRing (alternating streams, per-frame rows copied to the host stream-ordered):
the slot path, the tensor path and the consumer's CPU path against the golden model, and ``psana-ray-consumer
--task roi`` on a ``--calibrate_on_read`` session over HIP IPC."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import roi as RO
from psana_ray_amd.ops import reference
from psana_ray_amd.pipeline import RoiConsumer
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
        cal = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)[:, 0]   # 2-D frames
    return cal


def _want(frames, shape, rects, vmin, vmax, S, mask, proj):
    rows, px, py = reference.roi_stats_reference(frames.reshape(frames.shape[0], -1), shape, rects, vmin, vmax, S, mask, proj)
    rows = rows.numpy()
    qmax, imax = reference.roi_key_decode(rows[:, :, 4])
    return {"npix": rows[:, :, 0].astype(np.int32), "sum": rows[:, :, 1], "sy": rows[:, :, 2], "sx": rows[:, :, 3],
            "qmax": qmax, "imax": imax, "proj_x": px.numpy(), "proj_y": py.numpy()}


def _same(st, want, n_events):
    assert st.frames == n_events
    for k, w in want.items():
        g = st._arr(k)
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), k


def _feed(cons, ep, frames, batch):
    """Commit ``frames`` into ring slots batch by batch and poll each batch; returns the poll sizes."""
    polls = []
    for a in range(0, frames.shape[0], batch):
        part = frames[a:a + batch]
        slots = [ep.acquire(timeout=5.0) for _ in range(part.shape[0])]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(part[j].reshape(ep.ring.frame_shape))
            ep.commit(s, 0, a + j, 100 + a + j, None if (a + j) % 2 else 9.5)
        polls.append(cons.poll(timeout=5.0))
    return polls


def _cpu_reference_path(frames, shape, rects, batch, **kw):
    """The consumer's own CPU ``_reference`` path over the same batches."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing(shape, torch.float32, "cpu", 2, 2))
    try:
        cons = RoiConsumer(ep, shape, rects, batch=batch, **kw)
        for a in range(0, frames.shape[0], batch):
            cons.process_frames(list(frames[a:a + batch]),
                                [(0, g, 100 + g, None if g % 2 else 9.5) for g in range(a, min(a + batch, len(frames)))])
        return cons.stats()
    finally:
        ep.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["calib", "image"])
def test_three_batches_slot_path_tensor_path_and_cpu_path(native, cuda_device, layout):
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(layout)
    n_events, batch = 21, 8
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    n = int(np.prod(shape))
    H, W = shape[-2:]
    rng = np.random.default_rng(2)
    if layout == "calib":   # 3-D frames: a mask, both projections, a narrow window
        rects = [(1, 4, 20, 8, 40), (0, 0, H, 0, W), (1, H - 1, H, W - 1, W), (0, 10, 11, 3, 30), (0, 0, H, 0, W)]
        kw = dict(mask=(rng.random(n) < 0.9).astype(np.uint8), proj="both", vmin=-8.0, vmax=1024.0, frac_bits=4)
    else:                   # 2-D frames: rectangles without a panel, the defaults, one projection
        rects = [(3, H - 2, 1, W), (0, H, 0, W), (H - 1, H, W - 1, W)]
        kw = dict(proj="y")
    full = [r if len(r) == 5 else (0, *r) for r in rects]
    par = (kw.get("vmin", -2.0 ** 20), kw.get("vmax", 2.0 ** 20), kw.get("frac_bits", 2), kw.get("mask"), kw["proj"])
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = RoiConsumer(ep, shape, rects, detector=DET, layout=layout, batch=batch, **kw)
    assert len(cons.streams) >= 2 and cons.n_roi == len(rects) and cons.rects.tolist() == [list(r) for r in full]
    assert cons.row_bytes == RO.RoiSet(full, shape).row_bytes(kw["proj"])
    assert _feed(cons, ep, frames, batch) == [8, 8, 5]
    st = cons.stats()
    want = _want(frames, shape, full, *par)
    _same(st, want, n_events)
    assert (st.detector, st.layout, st.shape, st.proj, st.R) == (DET, layout, shape, kw["proj"], len(rects))
    # rows in processing order, with the slots' headers
    assert st.gevt.tolist() == list(range(100, 121)) and st.idx.tolist() == list(range(21)) and set(st.rank) == {0}
    assert np.array_equal(np.isnan(st.photon_energy), np.arange(21) % 2 == 1) and st.photon_energy[0] == 9.5
    assert 0 < int(st.npix.sum()) and (st.proj_x.shape[1] > 0) == (kw["proj"] == "both") and st.proj_y.shape[1] > 0
    # the consumer's own CPU path gives the same file
    cpu = _cpu_reference_path(frames, shape, rects, batch, detector=DET, layout=layout, **kw)
    _same(cpu, want, n_events)
    assert cpu.key() == st.key() and all(cpu._arr(k).tobytes() == st._arr(k).tobytes() for k in RO.PER_FRAME)
    # the tensor path (frames that are not queue items) lands in the same run; stats() twice is stable
    cons.process_frames([pool[i].to(cuda_device) for i in range(4)], [(1, i, 500 + i, 7.0) for i in range(4)])
    st2 = cons.stats()
    _same(st2, _want(torch.cat([frames, pool[:4]]), shape, full, *par), 25)
    assert st2.gevt[-4:].tolist() == [500, 501, 502, 503] and st2.rank[-4:].tolist() == [1] * 4
    assert st2.photon_energy[-4:].tolist() == [7.0] * 4
    for k in want:   # what the slot path gave these frames, the tensor path gives again
        assert np.array_equal(st2._arr(k)[-4:], st._arr(k)[:4]), k
    st3 = cons.stats()
    assert all(st3._arr(k).tobytes() == st2._arr(k).tobytes() for k in RO.PER_FRAME)
    ep.close()


@pytest.mark.gpu
def test_raw_ring_and_refusals(native, cuda_device):
    """A --calibrate_on_read queue carries RAW uint16 frames: the consumer is built with check_ring=False and
    takes the calibrated frames through process_frames, several batches with a short last one."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool("calib")
    shape = tuple(pool.shape[1:])
    rects = [(1, 4, 20, 8, 40), (0, 0, 32, 0, 48)]
    ep = QueueEndpoint(FrameRing(shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        RoiConsumer(ep, shape, rects)
    cons = RoiConsumer(ep, shape, rects, detector=DET, batch=8, proj="x", check_ring=False)
    frames = torch.stack([pool[g % POOL] for g in range(19)])
    for a in range(0, 19, 8):
        cons.process_frames([f.to(cuda_device) for f in frames[a:a + 8]], [(0, g, g) for g in range(a, min(a + 8, 19))])
    st = cons.stats()
    _same(st, _want(frames, shape, rects, -2.0 ** 20, 2.0 ** 20, 2, None, "x"), 19)
    assert st.gevt.tolist() == list(range(19)) and bool(np.isnan(st.photon_energy).all())
    ep.close()
    ep = QueueEndpoint(FrameRing((2, 32, 40), torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="queue frames"):
        RoiConsumer(ep, shape, rects)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    n = int(np.prod(shape))
    for kw in (dict(rects=[]), dict(rects=[(2, 0, 1, 0, 1)]), dict(rects=[(0, 0, 33, 0, 1)]), dict(rects=[(0, 1, 0, 1)]),
               dict(vmin=1.0, vmax=0.0), dict(frac_bits=17), dict(vmax=2.0 ** 31, frac_bits=0), dict(proj="z"),
               dict(mask=np.ones(n - 1, np.uint8)), dict(rects=RO.RoiSet(rects, (2, 32, 49)))):
        with pytest.raises(ValueError):
            RoiConsumer(ep, shape, **{**dict(rects=rects), **kw})
    cons = RoiConsumer(ep, shape, rects, batch=4)
    x = [torch.ones(shape, dtype=torch.float32, device=cuda_device) for _ in range(4)]
    with pytest.raises(ValueError, match="batch of at most"):
        cons.process_frames(x + x, [(0, i, i) for i in range(8)])
    assert cons.synchronize() == 0 and not cons.results and cons.stats().frames == 0
    ep.close()


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_calibrate_on_read(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer with --calibrate_on_read (RAW frames in the queue) and ``psana-ray-consumer 0
    --task roi --out`` as two GPU processes: the consumer calibrates (image mode, common mode), then takes the
    rectangles of the 2-D image; the file equals the golden model."""
    from psana_ray_amd.config import resolve_common_mode
    from psana_ray_amd.models import make_geometry

    n_events, run = 20, 13
    src = SyntheticRun("synthetic", run, DET, rank=0, size=1)   # pool generated as the producer process generates it
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    geo = make_geometry(src.spec)
    cal = reference.calibrate_reference(raw, src.consts, None, resolve_common_mode("default", src.spec))
    pool = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)[:, 0]
    H, W = pool.shape[1:]
    rects2 = [(3, H - 2, 1, W), (0, H, 0, W), (H - 1, H, W - 1, W)]
    specs = [a for (y0, y1, x0, x1) in rects2 for a in ("--roi", f"{y0}:{y1},{x0}:{x1}")]
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "roi.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         DET, "--common_mode", "default", "--calibrate_on_read", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "roi", *specs, "--roi_proj", "both", "--roi_vmin",
                             "-50", "--roi_vmax", "400", "--out", out, "--batch", "8", "--metrics_interval", "0"],
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
    st = RO.RoiFrames.load(out)
    frames = torch.stack([pool[g % k] for g in range(n_events)])
    assert st.detector == DET and st.layout == "image" and st.shape == (H, W) and st.R == 3
    assert st.gevt.tolist() == list(range(n_events))
    _same(st, _want(frames, (H, W), [(0, *r) for r in rects2], -50.0, 400.0, 2, None, "both"), n_events)
    assert "row_bytes=" in cout
