"""pipeline.RoibinConsumer on the GPU through a local endpoint, on the ring-slot path and the tensor path, and
``psana-ray-consumer --task roibin`` over HIP IPC -- against the golden models.

The frames are exact small integers with isolated spikes on a locally constant background: the ring noise of every
spike is 0, so its signal-over-noise is far from son_min and the peak finder's choice does not hang on rounding."""
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from psana_ray_amd import roibin
from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.ops import reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPE = (2, 32, 48)
SPIKES = [0, 1, 3, 5, 2, 0, 4, 1, 6, 3, 2]      # spikes per frame; min_peaks = 2 skips five of the eleven
KW = dict(bin=2, step=0.5, vmin=-64.0, vmax=4096.0, radius=3)
ARRAYS = ("rank", "idx", "gevt", "photon_energy", "npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "rec", "box",
          "koffs", "codes")


def _frames():
    """[F, P, H, W]: integers 0 .. 7, constant 2 within 4 pixels of a spike, spikes of 50 .. 90 on a grid of 10 pixels
    (one of them at a panel corner)."""
    rng = np.random.default_rng(17)
    P, H, W = SHAPE
    F = len(SPIKES)
    x = rng.integers(0, 8, size=(F, P, H, W)).astype(np.float32)
    cells = [(p, y, xx) for p in range(P) for y in (0, 10, 20, 31) for xx in (0, 12, 24, 36, 47)]
    centres = []
    for f, k in enumerate(SPIKES):
        pick = [cells[i] for i in rng.permutation(len(cells))[:k]]
        if f == 3:
            pick[0] = (1, 31, 47)
        for p, y, xx in pick:
            x[f, p, max(y - 4, 0):y + 5, max(xx - 4, 0):xx + 5] = 2.0
        for p, y, xx in pick:
            x[f, p, y, xx] = float(rng.integers(50, 91))
        centres.append(sorted((p * H + y) * W + xx for p, y, xx in set(pick)))
    return x, centres


def _consumer(ep, batch, min_peaks=0, mask=None):
    from psana_ray_amd.pipeline import RoibinConsumer

    return RoibinConsumer(ep, SHAPE, mask=mask, min_peaks=min_peaks, peak_params=PeakFinderParams(max_peaks=16),
                          detector="tiny_epix", layout="calib", batch=batch, **KW)


def _run(x, batch, device, path, min_peaks=0, mask=None):
    """Feed the frames batch by batch (``path``: "slots" commits them into ring slots and polls, "tensors" hands
    device tensors to process_frames); returns (merged RoibinFrames, the device records and counts, the consumer)."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    F = x.shape[0]
    ep = QueueEndpoint(FrameRing(SHAPE, torch.float32, device, 2 * batch, 2 * batch))
    cons = _consumer(ep, batch, min_peaks, mask)
    assert -(-F // batch) <= cons._nbuf          # every batch keeps its own buffer row: the records can be read back
    xd = torch.from_numpy(x).to(device)
    for a in range(0, F, batch):
        n = min(batch, F - a)
        if path == "slots":
            slots = [ep.acquire(timeout=5.0) for _ in range(n)]
            for j, s in enumerate(slots):
                ep.slot_tensor(s).copy_(xd[a + j])
                ep.commit(s, 0, a + j, 100 + a + j, None if (a + j) % 2 else 9.5)
            assert cons.poll(timeout=5.0) == n
        else:
            cons.process_frames([xd[a + j] for j in range(n)],
                                [(0, a + j, 100 + a + j, None if (a + j) % 2 else 9.5) for j in range(n)])
    cons.synchronize()
    out = roibin.concat(cons.take_results())
    peaks = torch.cat([cons._pf.peaks[b, :min(batch, F - b * batch)] for b in range(-(-F // batch))]).cpu()
    counts = torch.cat([cons._pf.counts[b, :min(batch, F - b * batch)] for b in range(-(-F // batch))]).cpu()
    ep.close()
    return out, peaks, counts, cons


@pytest.mark.parametrize("path", ["slots", "tensors"])
def test_consumer_equals_the_golden_models(native, cuda_device, path):
    x, centres = _frames()
    F = x.shape[0]
    mask = np.ones(SHAPE, np.uint8)
    mask[0, 3:6, 7:20] = 0
    rf, peaks, counts, cons = _run(x, 4, cuda_device, path, min_peaks=2, mask=mask)
    assert rf.gevt.tolist() == [100 + i for i in range(F)] and rf.idx.tolist() == list(range(F))
    assert np.array_equal(np.isnan(rf.photon_energy), np.arange(F) % 2 == 1)
    # the peak finder found the spikes: the centres of the golden peak finder, which are the spikes put in
    found, _ = reference.peakfind_reference(torch.from_numpy(x), PeakFinderParams(max_peaks=16))
    P, H, W = SHAPE
    for f in range(F):
        want = sorted(int((r[0] * H + r[1]) * W + r[2]) for r in found[f].tolist())
        assert want == centres[f] and int(counts[f]) == len(want)
        got = sorted(int((r[0] * H + r[1]) * W + r[2]) for r in peaks[f, :int(counts[f])].tolist())
        assert got == want
        if SPIKES[f] >= 2:
            assert rf.boxes(f)[0].tolist() == want
    # the whole result: the golden model on the records read back from the device
    g = reference.roibin_reference(torch.from_numpy(x), SHAPE, peaks, counts, cons.params, mask=mask.reshape(-1))
    for k in ("npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "codes"):
        assert np.array_equal(getattr(rf, k), getattr(g, k).numpy()), k
    assert rf.rec.tobytes() == g.rec.numpy().tobytes() and rf.box.tobytes() == g.box.numpy().tobytes()
    skipped = [s < 2 for s in SPIKES]
    assert ((rf.flags & roibin.FLAG_SKIPPED) != 0).tolist() == skipped and rf.codes.shape[0] == F - sum(skipped)
    assert cons.metrics() == {"frames_consumed": F, "frames_kept": F - sum(skipped), "frames_skipped": sum(skipped),
                              "frames_overflowed": 0, "boxes": int(rf.offs[-1]), "saturated": 0}
    # a kept frame reconstructs: the boxes bit for bit, the corner box NaN-filled outside the panel
    d = rf.to_dense(3)
    c, _rec, box = rf.boxes(3)
    assert int(c[-1]) == (1 * H + 31) * W + 47 and np.isnan(box[-1][4:, :]).all() and np.isnan(box[-1][:, 4:]).all()
    assert np.array_equal(box[-1][:4, :4], x[3, 1, 28:, 44:]) and np.array_equal(d[1, 28:, 44:], x[3, 1, 28:, 44:])


def test_batch_split_does_not_change_the_file(native, cuda_device):
    x, _ = _frames()
    a = _run(x, 4, cuda_device, "slots", min_peaks=1)[0]
    b = _run(x, 7, cuda_device, "slots", min_peaks=1)[0]
    c = _run(x, 3, cuda_device, "tensors", min_peaks=1)[0]
    assert a.params() == b.params() == c.params()
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes() == getattr(c, k).tobytes(), k
    assert 0 < int((a.flags & roibin.FLAG_SKIPPED != 0).sum()) < len(a)


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


def test_two_processes_over_hip_ipc_task_roibin(native, cuda_device, tmp_path):
    """A synthetic tiny_epix producer and ``psana-ray-consumer 0 --device cuda:0 --task roibin --out`` as two GPU
    processes: the final line states what the file holds, and every kept frame's codes are the golden model's."""
    n_events, run, det = 20, 12, "tiny_epix"
    addr = f"127.0.0.1:{random.randint(30000, 45000)}"
    out = str(tmp_path / "rb.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(run), "--detector_name",
         det, "--calib", "--common_mode", "off", "--num_events", str(n_events), "--ray_address", addr,
         "--num_consumers", "1", "--queue_size", "16", "--device", "cuda:0", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", addr, "--device",
                             "cuda:0", "--timeout", "60", "--task", "roibin", "--rb_bin", "4", "--rb_step", "0.25",
                             "--rb_box", "2", "--out", out, "--batch", "8", "--metrics_interval", "0"],
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
    rf = roibin.merge([out])
    assert (rf.detector, rf.layout, rf.bin, rf.step, rf.radius, rf.min_peaks) == (det, "calib", 4, 0.25, 2, 0)
    assert rf.gevt.tolist() == list(range(n_events)) and rf.codes.shape == (n_events, 2, 8, 12)
    assert re.search(r"roibin: bin=4 step=0.25 .* codes=8x12 frame_bytes=384 batch=8", cout), cout[-2000:]
    assert (f"roibin: frames={n_events} kept={n_events} skipped=0 boxes={int(rf.offs[-1])} overflowed=0 "
            f"saturated={int(rf.nsat.sum())}") in cout, cout[-2000:]
    assert int(rf.offs[-1]) > 0
    # the codes do not depend on the peak finder: the golden model on the golden frames
    from psana_ray_amd.source import SyntheticRun

    src = SyntheticRun("synthetic", run, det, rank=0, size=1)
    k = min(n_events, src.pool_frames)
    raw = torch.from_numpy(np.stack([src.pool[i] for i in range(k)]).astype(np.int32))
    frames = reference.calibrate_reference(raw, src.consts, None, None)
    g = reference.roibin_reference(frames, SHAPE, torch.zeros((k, 4, 8)), torch.zeros(k, dtype=torch.int32), bin=4,
                                   step=0.25, radius=2, max_peaks=4)
    for i in range(n_events):
        assert np.array_equal(rf.frame_codes(i), g.codes[i % k].numpy()), i
        c, rec, box = rf.boxes(i)
        for j in range(len(c)):          # every box is the frame around its centre, bit for bit
            p, y, x = (int(v) for v in np.unravel_index(int(c[j]), SHAPE))
            assert (int(rec[j, 0]), int(rec[j, 1]), int(rec[j, 2])) == (p, y, x)
            assert box[j, 2, 2] == frames[i % k, p, y, x]
