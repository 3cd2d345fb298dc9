"""pipeline.PowderConsumer on a FrameRing (alternating streams, one accumulator set each), the
on-device hit filter, and ``psana-ray-consumer --task powder`` over HIP IPC -- against the golden models."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import powder
from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.ops import reference
from psana_ray_amd.source import SyntheticRun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DET = "tiny_epix"
POOL = 4
# the hit-filter case: tiny_epix, synthetic seed 11, thr_peak 40 (checked by test_hit_filter_choice_has_margin)
HIT_SEED, HIT_THR_PEAK, HIT_SON = 11, 40.0, 5.0
ARRAYS = ("frames", "cnt", "sum", "sq", "above", "qmax")


@functools.lru_cache(maxsize=None)
def _golden_pool(seed):
    """Calibrated frames [POOL, P, H, W] from the golden model; frame g of a run is pool[g % POOL]."""
    src = SyntheticRun("synthetic", 4, DET, n_events=POOL, pool_frames=POOL, seed=seed, gen_device="cpu")
    return reference.calibrate_reference(torch.from_numpy(src.pool.astype(np.int32)), src.consts, None, None)


def _peak_counts(frames, params):
    return [int(p.shape[0]) for p in reference.peakfind_reference(frames, params)[0]]


def _moved_counts(frames, params):
    """Reference peak counts with thr_peak and son_min both lowered (-0.01, -1 %) and both raised: a
    pixel can only gain peaks under the first and lose them under the second, so counts that agree
    under both hold for every threshold in between -- orders of magnitude more room than the float32
    rounding of the kernel's peak statistics needs."""
    return [_peak_counts(frames, PeakFinderParams(thr_peak=params.thr_peak + dt, son_min=params.son_min * ds,
                                                  radius=params.radius, max_peaks=params.max_peaks))
            for dt, ds in ((-0.01, 0.99), (0.01, 1.01))]


def _hit_case():
    params = PeakFinderParams(thr_peak=HIT_THR_PEAK, son_min=HIT_SON)
    counts = _peak_counts(_golden_pool(HIT_SEED), params)
    return params, counts, sorted(counts)[POOL // 2]


def _want(frames, counts=None, min_peaks=0, **kw):
    """Golden accumulators of ``frames`` [n, ...] as numpy arrays with the dtypes of PowderStats."""
    n = frames.shape[0]
    keys = None if counts is None else torch.tensor(counts, dtype=torch.int32)
    nfr, cnt, s, sq, qmax, above = reference.powder_accumulate_reference(
        frames.reshape(n, -1), kw.get("vmin", -2.0 ** 20), kw.get("vmax", 2.0 ** 20), kw.get("S", 2),
        kw.get("thr", 20.0), keys=keys, key_min=min_peaks)
    return {"frames": nfr.numpy(), "cnt": cnt.numpy().astype(np.int64), "sum": s.numpy(), "sq": sq.numpy(),
            "above": above.numpy().astype(np.int64), "qmax": qmax.numpy()}


def _same(st, want):
    for k in ARRAYS:
        got = getattr(st, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k]), k


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


def test_hit_filter_choice_has_margin():
    """CPU check of the hit-filter case: the reference peak counts of its frames do not change when
    thr_peak moves by +-0.01 and son_min by +-1 %, and the chosen N separates the frames."""
    params, counts, n_min = _hit_case()
    assert _moved_counts(_golden_pool(HIT_SEED), params) == [counts, counts]
    assert min(counts) < n_min <= max(counts), counts


@pytest.mark.gpu
def test_three_batches_last_partial_over_alternating_streams(native, cuda_device):
    from psana_ray_amd.pipeline import PowderConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(3)
    n_events, batch = 21, 8
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = PowderConsumer(ep, shape, detector=DET, layout="calib", batch=batch, thr_above=15.0)
    assert len(cons._acc) == len(cons.streams) >= 2 and cons.nc == 1 and cons.max_frames == 524287
    assert _feed(cons, ep, frames, batch) == [8, 8, 5]
    st = cons.stats()
    _same(st, _want(frames, thr=15.0))
    assert (st.detector, st.layout, st.shape, st.min_peaks, st.peak_params) == (DET, "calib", shape, 0, {})
    # every stream's set took part: no single set holds all frames
    per_set = [int(acc[0].cpu()[0]) for acc in cons._acc]
    assert sum(per_set) == n_events and max(per_set) < n_events
    # process_frames (frames that are not queue items) lands in the same run
    extra = [pool[i].to(cuda_device) for i in range(4)]
    cons.process_frames(extra)
    st2 = cons.stats()
    _same(st2, _want(torch.cat([frames, pool[:4]]), thr=15.0))
    assert cons.frames == 25
    ep.close()


@pytest.mark.gpu
def test_hit_filter_on_the_device(native, cuda_device):
    """min_peaks: the classes are those the REFERENCE peak counts give."""
    from psana_ray_amd.pipeline import PowderConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    params, counts, n_min = _hit_case()
    pool = _golden_pool(HIT_SEED)
    n_events, batch = 21, 8
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = PowderConsumer(ep, shape, min_peaks=n_min, peak_params=params, detector=DET, layout="calib", batch=batch)
    assert cons.nc == 2
    assert _feed(cons, ep, frames, batch) == [8, 8, 5]
    st = cons.stats()
    all_counts = [counts[g % POOL] for g in range(n_events)]
    hits = sum(c >= n_min for c in all_counts)
    assert 0 < hits < n_events and st.frames.tolist() == [n_events - hits, hits]
    _same(st, _want(frames, all_counts, n_min))
    assert st.min_peaks == n_min and st.peak_params == {"thr_peak": HIT_THR_PEAK, "son_min": HIT_SON, "radius": 1.0}
    ep.close()


@pytest.mark.gpu
def test_consumer_refuses_other_rings_and_a_full_run(native, cuda_device):
    from psana_ray_amd.pipeline import PowderConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    shape = (2, 32, 48)
    ep = QueueEndpoint(FrameRing(shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        PowderConsumer(ep, shape)
    PowderConsumer(ep, shape, check_ring=False)            # calibrate-on-read: the ring is raw
    ep.close()
    ep = QueueEndpoint(FrameRing((2, 32, 40), torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="queue frames"):
        PowderConsumer(ep, shape)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    for kw in (dict(vmin=1.0, vmax=0.0), dict(frac_bits=17), dict(frac_bits=11), dict(min_peaks=-1),
               dict(vmax=float("inf"))):
        with pytest.raises(ValueError):
            PowderConsumer(ep, shape, **kw)
    # Q = 2^30: a run of 7 frames; the consumer refuses the 8th before any launch
    cons = PowderConsumer(ep, shape, vmin=-3.0, vmax=2.0 ** 20, frac_bits=10, batch=4)
    assert cons.max_frames == 7
    x = [torch.ones(shape, dtype=torch.float32, device=cuda_device) for _ in range(4)]
    cons.process_frames(x)
    with pytest.raises(ValueError, match="max_frames = 7"):
        cons.process_frames(x)
    cons.process_frames(x[:3])
    with pytest.raises(ValueError, match="max_frames = 7"):
        cons.poll(timeout=0.0)
    st = cons.stats()
    assert st.frames.tolist() == [7] and bool((st.cnt == 7).all()) and bool((st.sum == 7 * 1024).all())
    ep.close()


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_task_powder_with_min_peaks(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer and ``psana-ray-consumer 0 --task powder --min_peaks N --out`` as two
    GPU processes, three batches: the file equals the golden model with the classes of the reference peak
    counts.  N is the count nearest the median at which no frame of this run is on an edge."""
    n_events, run = 20, 12
    src = SyntheticRun("synthetic", run, DET, rank=0, size=1)   # pool generated as the producer process generates it
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    pool = reference.calibrate_reference(raw, src.consts, None, None)
    params = PeakFinderParams()
    counts = _peak_counts(pool, params)
    moved = _moved_counts(pool, params)
    cands = sorted(set(counts), key=lambda c: abs(c - sorted(counts)[k // 2]))
    stable = [c for c in cands if min(counts) < c and all([x >= c for x in mv] == [x >= c for x in counts] for mv in moved)]
    assert stable, (counts, moved)
    n_min = stable[0]
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "powder.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         DET, "--calib", "--common_mode", "off", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "powder", "--min_peaks", str(n_min), "--out", out,
                             "--batch", "8", "--metrics_interval", "0"],
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
    st = powder.PowderStats.load(out)
    frames = torch.stack([pool[g % k] for g in range(n_events)])
    all_counts = [counts[g % k] for g in range(n_events)]
    hits = sum(c >= n_min for c in all_counts)
    assert 0 < hits < n_events
    _same(st, _want(frames, all_counts, n_min))
    assert st.detector == DET and st.layout == "calib" and st.min_peaks == n_min
    assert "powder: max_frames=524287 " in cout and f"powder: frames={n_events - hits}+{hits} " in cout, cout[-2000:]
