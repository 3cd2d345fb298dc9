"""pipeline.SparseFrameConsumer fed by a ProducerPipeline through a local endpoint, the on-device hit
filter, and ``psana-ray-consumer --task sparse`` over HIP IPC -- against the golden models."""
import functools
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import sparse
from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.models import Calibrator, Mode
from psana_ray_amd.ops import reference
from psana_ray_amd.source import SyntheticRun

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL = 4
# the hit-filter case: tiny_epix, synthetic seed 11, thr_peak 40 (checked by test_hit_filter_choice_has_margin)
HIT_SEED, HIT_THR_PEAK, HIT_SON = 11, 40.0, 5.0


def _source(det, n_events, seed):
    # the pool is generated on the CPU so that the CPU check below sees the frames the GPU test sees
    return SyntheticRun("synthetic", 4, det, n_events=n_events, pool_frames=POOL, seed=seed,
                        pinned=torch.cuda.is_available(), gen_device="cpu")


@functools.lru_cache(maxsize=None)
def _golden_pool(det, seed):
    """The pool's calibrated frames [POOL, P, H, W] from the golden model (event k carries pool[k % POOL])."""
    src = SyntheticRun("synthetic", 4, det, n_events=POOL, pool_frames=POOL, seed=seed, gen_device="cpu")
    raw = torch.from_numpy(src.pool.astype(np.int32))
    return reference.calibrate_reference(raw, src.consts, None, None)


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


def _run_consumer(det, n_events, batch, device, seed=3, **kw):
    """Produce n_events frames into a local ring, then drain it with a SparseFrameConsumer."""
    from psana_ray_amd.pipeline import ProducerPipeline, SparseFrameConsumer
    from psana_ray_amd.queue import EndOfStream, FrameRing, QueueEndpoint

    src = _source(det, n_events, seed)
    cal = Calibrator(src.consts, device, Mode.calib)
    ring = FrameRing(cal.out_shape, cal.out_dtype, device, n_events, n_events)
    ep = QueueEndpoint(ring)
    assert ProducerPipeline(src, cal, ep, chunk=min(8, n_events)).run() == n_events
    cons = SparseFrameConsumer(ep, cal.out_shape, detector=det, layout="calib", batch=batch, **kw)
    polls = []
    while True:
        try:
            k = cons.poll(timeout=5.0)
        except EndOfStream:
            break
        if k:
            polls.append(k)
    cons.synchronize()
    out = sparse.concat(cons.take_results())
    m = cons.metrics()
    ep.close()
    return out, polls, m, cons


def _check(sf, det, seed, n_events, thr, vmax, cap, counts=None, min_peaks=0):
    """Every frame exactly once; stored frames' to_dense == where(keep, golden frame, 0) bit for bit."""
    pool = _golden_pool(det, seed)
    assert sorted(sf.gevt.tolist()) == list(range(n_events)) and len(sf) == n_events
    n_over = n_skip = 0
    for i in range(n_events):
        g = int(sf.gevt[i])
        x = pool[g % POOL].numpy()
        keep = (x >= np.float32(thr)) & (x <= np.float32(vmax))
        if counts is not None and counts[g % POOL] < min_peaks:
            assert sf.flags[i] == sparse.FLAG_SKIPPED and sf.nnz[i] == 0 and sf.frame(i)[0].size == 0, g
            n_skip += 1
            continue
        assert sf.nnz[i] == keep.sum(), g
        if keep.sum() > cap:
            assert sf.flags[i] == sparse.FLAG_OVERFLOW and sf.frame(i)[0].size == 0, g
            n_over += 1
            continue
        assert sf.flags[i] == 0
        assert np.array_equal(sf.to_dense(i).view(np.int32), np.where(keep, x, np.float32(0)).view(np.int32)), g
    return n_over, n_skip


@pytest.mark.gpu
@pytest.mark.parametrize("det, batch, n_events, cap", [("tiny_epix", 8, 21, 450), ("epix10k2M", 8, 19, None)])
def test_three_batches_last_partial(native, cuda_device, det, batch, n_events, cap):
    sf, polls, m, cons = _run_consumer(det, n_events, batch, cuda_device, cap=cap)
    assert polls == [batch, batch, n_events - 2 * batch]
    assert sf.thr == 20.0 and sf.vmax == 2.0 ** 20 and sf.cap == (cap or cons.n // 16) and sf.shape == cons.shape
    n_over, _ = _check(sf, det, 3, n_events, 20.0, 2.0 ** 20, sf.cap)
    assert m == {"frames_consumed": n_events, "frames_stored": n_events - n_over, "frames_skipped": 0,
                 "frames_overflowed": n_over, "pixels_stored": int(sf.offs[-1])}
    assert int(sf.offs[-1]) > 0 and (det != "tiny_epix" or 0 < n_over < n_events)
    assert np.array_equal(sf.rank, np.zeros(n_events, np.int64)) and np.array_equal(sf.idx, sf.gevt)
    assert not np.isnan(sf.photon_energy).any()


def _hit_case():
    params = PeakFinderParams(thr_peak=HIT_THR_PEAK, son_min=HIT_SON)
    counts = _peak_counts(_golden_pool("tiny_epix", HIT_SEED), params)
    return params, counts, sorted(counts)[POOL // 2]


def test_hit_filter_choice_has_margin():
    """CPU check of the hit-filter case: the reference peak counts of its frames do not change when
    thr_peak moves by +-0.01 and son_min by +-1 %, and the chosen N separates the frames."""
    params, counts, n_min = _hit_case()
    assert _moved_counts(_golden_pool("tiny_epix", HIT_SEED), params) == [counts, counts]
    assert min(counts) < n_min <= max(counts), counts


def test_cpu_endpoint_runs_the_golden_model():
    """The same consumer on a CPU endpoint (golden models for both stages), hit filter included."""
    params, counts, n_min = _hit_case()
    sf, polls, m, _ = _run_consumer("tiny_epix", 11, 4, torch.device("cpu"), seed=HIT_SEED, cap=450, min_peaks=n_min,
                                    peak_params=params)
    assert sum(polls) == 11
    n_over, n_skip = _check(sf, "tiny_epix", HIT_SEED, 11, 20.0, 2.0 ** 20, 450, counts, n_min)
    assert 0 < n_skip < 11 and m["frames_skipped"] == n_skip and m["frames_overflowed"] == n_over
    assert sf.min_peaks == n_min and sf.peak_params == {"thr_peak": HIT_THR_PEAK, "son_min": HIT_SON, "radius": 1.0}


@pytest.mark.gpu
def test_hit_filter_on_the_device(native, cuda_device):
    """min_peaks: the stored set is the frames whose REFERENCE peak count is at least N."""
    params, counts, n_min = _hit_case()
    n_events = 21
    sf, polls, m, _ = _run_consumer("tiny_epix", n_events, 8, cuda_device, seed=HIT_SEED, cap=3072, min_peaks=n_min,
                                    peak_params=params)
    assert polls == [8, 8, 5]
    n_over, n_skip = _check(sf, "tiny_epix", HIT_SEED, n_events, 20.0, 2.0 ** 20, 3072, counts, n_min)
    want_skip = sum(counts[g % POOL] < n_min for g in range(n_events))
    assert n_over == 0 and n_skip == want_skip and 0 < want_skip < n_events
    assert m["frames_skipped"] == want_skip and m["frames_stored"] == n_events - want_skip
    stored = sorted(int(g) for g, f in zip(sf.gevt, sf.flags) if f == 0)
    assert stored == [g for g in range(n_events) if counts[g % POOL] >= n_min]


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_task_sparse_with_min_peaks(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer and ``psana-ray-consumer 0 --task sparse --min_peaks N --out`` as two
    GPU processes, three batches: the file's frames match the golden model, the skipped ones are those
    below N peaks.  N is the count nearest the median at which no frame of this run is on an edge."""
    n_events, run, det = 20, 12, "tiny_epix"
    src = SyntheticRun("synthetic", run, det, rank=0, size=1)   # pool generated as the producer process generates it
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    frames = reference.calibrate_reference(raw, src.consts, None, None)
    params = PeakFinderParams()
    counts = _peak_counts(frames, params)
    moved = _moved_counts(frames, params)
    cands = sorted(set(counts), key=lambda c: abs(c - sorted(counts)[k // 2]))
    stable = [c for c in cands if min(counts) < c and all([x >= c for x in mv] == [x >= c for x in counts] for mv in moved)]
    assert stable, (counts, moved)
    n_min = stable[0]
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "hits.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         det, "--calib", "--common_mode", "off", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "sparse", "--min_peaks", str(n_min), "--out", out,
                             "--batch", "8", "--sparse_cap", "3072", "--metrics_interval", "0"],
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
    sf = sparse.merge([out])
    assert sf.detector == det and sf.layout == "calib" and sf.min_peaks == n_min and sf.cap == 3072
    assert sf.gevt.tolist() == list(range(n_events))
    n_skip = 0
    for g in range(n_events):
        x = frames[g % k].numpy()
        if counts[g % k] < n_min:
            assert sf.flags[g] == sparse.FLAG_SKIPPED and sf.nnz[g] == 0
            n_skip += 1
            continue
        keep = (x >= np.float32(20.0)) & (x <= np.float32(2.0 ** 20))
        assert sf.flags[g] == 0 and sf.nnz[g] == keep.sum() > 0
        assert np.array_equal(sf.to_dense(g).view(np.int32), np.where(keep, x, np.float32(0)).view(np.int32)), g
    assert 0 < n_skip < n_events
    assert f"sparse: frames={n_events} stored={n_events - n_skip} skipped={n_skip} overflowed=0" in cout, cout[-2000:]
