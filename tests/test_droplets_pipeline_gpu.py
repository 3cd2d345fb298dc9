"""pipeline.DropletConsumer on a FrameRing: 13 tiny_epix frames in batches of 3 (polls [3, 3, 3, 3, 1]) over
alternating streams, through ring slots, through tensors and behind a calibrate-on-read ring -- every kept word
against the golden model, the ring slots released, two frames forced to overflow."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd import droplets as DR
from psana_ray_amd.ops import reference
from psana_ray_amd.pipeline import DropletConsumer
from psana_ray_amd.source import SyntheticRun

pytestmark = pytest.mark.gpu

DET = "tiny_epix"
POOL = 4
N_EVENTS, BATCH = 13, 3
PAR = dict(thr_low=15.0, thr_seed=30.0, frac_bits=3)
COLS = ("label", "npix", "adu", "sy", "sx", "qmax")


@functools.lru_cache(maxsize=None)
def _frames():
    """13 calibrated frames [2, 32, 48] from the golden model; frame 5 is active everywhere (bit 2), frame 7
    a checkerboard (more droplets than cap: bit 0)."""
    src = SyntheticRun("synthetic", 4, DET, n_events=POOL, pool_frames=POOL, seed=3, gen_device="cpu")
    pool = reference.calibrate_reference(torch.from_numpy(src.pool.astype(np.int32)), src.consts, None, None)
    x = torch.stack([pool[g % POOL] for g in range(N_EVENTS)]).clone()
    x[5] = 50.0
    yy, xx = np.indices(tuple(x.shape[2:]))
    x[7] = torch.from_numpy(np.where((yy + xx) % 2 == 0, 40.0, 0.0).astype(np.float32))
    return x


@functools.lru_cache(maxsize=None)
def _want(masked):
    x = _frames()
    shape = tuple(x.shape[1:])
    n = int(np.prod(shape))
    mask = _mask(n) if masked else None
    per = [reference.droplet_reference(x[a:a + BATCH].reshape(-1, n), shape, PAR, mask, 2048, 48)
           for a in range(0, N_EVENTS, BATCH)]
    return per


def _mask(n):
    return (np.random.default_rng(2).random(n) < 0.9).astype(np.uint8)


def _same(results, masked, gevt0=100):
    want = _want(masked)
    assert len(results) == len(want)
    g = 0
    for df, w in zip(results, want):
        F = w.nact.numel()
        assert len(df) == F and df.gevt.tolist() == list(range(gevt0 + g, gevt0 + g + F))
        for k in ("nact", "ndrop", "flags", "offs", *COLS):
            got, ref = getattr(df, k), getattr(w, k).numpy()
            assert got.dtype == ref.dtype and np.array_equal(got, ref), (k, g)
        g += F
    flags = np.concatenate([df.flags for df in results])
    assert flags[5] == DR.FLAG_PIX_OVERFLOW and flags[7] == DR.FLAG_OVERFLOW and int((flags != 0).sum()) == 2
    assert sum(int(df.offs[-1]) for df in results) > 100


def _feed(cons, ep, frames, batch):
    polls = []
    for a in range(0, frames.shape[0], batch):
        part = frames[a:a + batch]
        slots = [ep.acquire(timeout=5.0) for _ in range(part.shape[0])]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(part[j])
            ep.commit(s, 0, a + j, 100 + a + j, None if (a + j) % 2 else 9.5)
        polls.append(cons.poll(timeout=5.0))
    return polls


@pytest.mark.parametrize("masked", [False, True])
def test_ring_slots_then_tensors(native, cuda_device, masked):
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    x = _frames()
    shape = tuple(x.shape[1:])
    n = int(np.prod(shape))
    mask = _mask(n) if masked else None
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))   # 4 slots for 13 frames: they must come back
    cons = DropletConsumer(ep, shape, **PAR, pix_cap=2048, cap=48, mask=mask, detector=DET, batch=BATCH)
    assert len(cons._scratch) == len(cons.streams) >= 2 and cons.batch == BATCH
    assert cons.scratch_bytes == cons._scratch[0].numel() >= 52 * 2048 * BATCH
    assert _feed(cons, ep, x, BATCH) == [3, 3, 3, 3, 1]
    res = list(cons.synchronize())
    _same(res, masked)
    assert cons.metrics() == {"frames_consumed": 13, "frames_stored": 11, "frames_overflowed": 2,
                              "droplets_stored": sum(int(d.offs[-1]) for d in res)}
    pe = np.concatenate([d.photon_energy for d in res])
    assert np.array_equal(np.isnan(pe), np.arange(13) % 2 == 1) and pe[0] == 9.5
    assert res[0].mask_sha256 == DR.mask_hash(shape, mask) and (res[0].mask_sha256 != "") == masked
    # every slot is free again
    slots = [ep.acquire(timeout=5.0) for _ in range(4)]
    assert len(set(slots)) == 4
    ep.close()
    # the tensor path over the same batches, on a fresh consumer; then the consumer's CPU path
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    cons = DropletConsumer(ep, shape, **PAR, pix_cap=2048, cap=48, mask=mask, detector=DET, batch=BATCH)
    for a in range(0, N_EVENTS, BATCH):
        cons.process_frames([f.to(cuda_device) for f in x[a:a + BATCH]],
                            [(0, g, 100 + g) for g in range(a, min(a + BATCH, N_EVENTS))])
    _same(list(cons.synchronize()), masked)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, "cpu", 2, 2))
    cpu = DropletConsumer(ep, shape, **PAR, pix_cap=2048, cap=48, mask=mask, detector=DET, batch=BATCH)
    for a in range(0, N_EVENTS, BATCH):
        cpu.process_frames(list(x[a:a + BATCH]), [(0, g, 100 + g) for g in range(a, min(a + BATCH, N_EVENTS))])
    _same(cpu.synchronize(), masked)
    ep.close()


def test_tensor_path_keeps_every_batch(native, cuda_device):
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    x = _frames()
    shape = tuple(x.shape[1:])
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    cons = DropletConsumer(ep, shape, **PAR, pix_cap=2048, cap=48, detector=DET, batch=BATCH)
    for a in range(0, N_EVENTS, BATCH):
        cons.process_frames([f.to(cuda_device) for f in x[a:a + BATCH]],
                            [(0, g, 100 + g) for g in range(a, min(a + BATCH, N_EVENTS))])
    _same(list(cons.synchronize()), False)
    assert cons.synchronize() is cons.results and len(cons.take_results()) == 5 and not cons.results
    ep.close()


def test_calibrate_on_read_ring_and_refusals(native, cuda_device):
    """A --calibrate_on_read queue carries RAW uint16 frames: the consumer is built with check_ring=False and takes
    the calibrated frames through process_frames."""
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    x = _frames()
    shape = tuple(x.shape[1:])
    n = int(np.prod(shape))
    ep = QueueEndpoint(FrameRing(shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        DropletConsumer(ep, shape, 15.0)
    cons = DropletConsumer(ep, shape, **PAR, pix_cap=2048, cap=48, detector=DET, batch=BATCH, check_ring=False)
    for a in range(0, N_EVENTS, BATCH):
        cons.process_frames([f.to(cuda_device) for f in x[a:a + BATCH]],
                            [(0, g, g) for g in range(a, min(a + BATCH, N_EVENTS))])
    res = list(cons.synchronize())
    _same(res, False, gevt0=0)
    assert bool(np.isnan(np.concatenate([d.photon_energy for d in res])).all())
    with pytest.raises(ValueError, match="batch of at most"):
        cons.process_frames([x[0].to(cuda_device)] * 4, [(0, i, i) for i in range(4)])
    ep.close()
    ep = QueueEndpoint(FrameRing((2, 32, 40), torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="queue frames"):
        DropletConsumer(ep, shape, 15.0)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    for kw in (dict(thr_low=0.0), dict(thr_low=None), dict(thr_seed=5.0), dict(vmax=10.0), dict(frac_bits=17),
               dict(pix_cap=0), dict(cap=0), dict(cap=2 ** 31), dict(mask=np.ones(n - 1, np.uint8)),
               dict(mask=np.ones(n, np.int32))):
        with pytest.raises(ValueError):
            DropletConsumer(ep, shape, **{**dict(thr_low=15.0), **kw})
    with pytest.raises(ValueError):
        DropletConsumer(ep, (n,), 15.0)
    # a batch that does not fit the HBM share is lowered, not refused
    small = DropletConsumer(ep, shape, 15.0, batch=16, hbm_budget=300 * 1024)
    assert 1 <= small.batch < 16
    small.process_frames([x[0].to(cuda_device)], [(0, 0, 0)])
    one = small.synchronize()[0]
    assert int(one.nact[0]) == int(((x[0] >= 15.0) & (x[0] <= 2.0 ** 20)).sum())
    e = small.empty()
    assert len(e) == 0 and e.params() == one.params()
    ep.close()
