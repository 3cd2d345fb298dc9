"""pipeline.CubeConsumer on a FrameRing (alternating streams, one accumulator set each; the bins from the
slot headers) and through process_frames -- against the golden model."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd import cube
from psana_ray_amd.ops import reference
from psana_ray_amd.source import SyntheticRun

DET = "tiny_epix"
POOL = 4
ARRAYS = ("frames", "cnt", "sum", "sq")
EDGES = (9000.0, 9100.0, 4)


@functools.lru_cache(maxsize=None)
def _golden_pool(seed):
    """Calibrated frames [POOL, P, H, W] from the golden model; frame g of a run is pool[g % POOL]."""
    src = SyntheticRun("synthetic", 4, DET, n_events=POOL, pool_frames=POOL, seed=seed, gen_device="cpu")
    return reference.calibrate_reference(torch.from_numpy(src.pool.astype(np.int32)), src.consts, None, None)


def _energy(g):
    """Every fourth event carries no photon energy; the others walk over the edges and a little outside."""
    return None if g % 4 == 3 else 8990.0 + 7.0 * g


def _want(frames, bins, B, **kw):
    n = frames.shape[0]
    nfr, cnt, s, sq = reference.cube_accumulate_reference(frames.reshape(n, -1), bins, B, kw.get("vmin", -2.0 ** 20),
                                                          kw.get("vmax", 2.0 ** 20), kw.get("S", 2))
    return {"frames": nfr.numpy(), "cnt": cnt.numpy(), "sum": s.numpy(), "sq": sq.numpy()}


def _same(st, want):
    for k in ARRAYS:
        got = getattr(st, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k]), k


def _feed(cons, ep, frames, batch, first=0):
    """Commit ``frames`` into ring slots batch by batch and poll each batch; returns the poll sizes."""
    polls = []
    for a in range(0, frames.shape[0], batch):
        part = frames[a:a + batch]
        slots = [ep.acquire(timeout=5.0) for _ in range(part.shape[0])]
        for j, s in enumerate(slots):
            g = first + a + j
            ep.slot_tensor(s).copy_(part[j])
            ep.commit(s, 0, g, g, _energy(g))
        polls.append(cons.poll(timeout=5.0))
    return polls


def test_sizing_function():
    sb = cube.accumulator_set_bytes(4, 3072)
    assert sb == 4 * 3072 * 20
    assert cube.accumulator_sets_that_fit(sb, 2, 2 * sb) == 2
    assert cube.accumulator_sets_that_fit(sb, 2, 2 * sb - 1) == 1
    assert cube.accumulator_sets_that_fit(sb, 2, sb) == 1
    with pytest.raises(ValueError, match="does not fit"):
        cube.accumulator_sets_that_fit(sb, 2, sb - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("one_stream", [False, True])
def test_slots_then_tensors_with_every_fourth_energy_missing(native, cuda_device, one_stream):
    """13 frames in batches of 3 through the ring-slot path, then 3 through the tensor path.  With the sets
    declared not to fit (a budget of one set) the consumer runs on one stream and gives the same run."""
    from psana_ray_amd.pipeline import CubeConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(3)
    n_events, batch = 13, 3
    frames = torch.stack([pool[g % POOL] for g in range(n_events)])
    shape = tuple(pool.shape[1:])
    binning = cube.CubeBinning.linspace(*EDGES)
    sb = cube.accumulator_set_bytes(binning.nbins, int(np.prod(shape)))
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = CubeConsumer(ep, shape, binning, detector=DET, layout="calib", batch=batch,
                        acc_budget=sb if one_stream else None)
    assert cons.set_bytes == sb and cons.max_frames == 524287
    assert len(cons._acc) == len(cons.streams) and (len(cons.streams) == 1) == one_stream
    assert _feed(cons, ep, frames, batch) == [3, 3, 3, 3, 1]
    energies = [_energy(g) for g in range(n_events + 3)]
    bins = binning.bin_of(energies)
    assert -1 in bins[:n_events].tolist() and len(set(bins[:n_events].tolist())) >= 4
    st = cons.stats()
    _same(st, _want(frames, bins[:n_events], binning.nbins))
    assert (st.detector, st.layout, st.shape, st.by, st.nbins) == (DET, "calib", shape, "photon_energy", 4)
    assert st.edges.tobytes() == np.linspace(*EDGES[:2], EDGES[2] + 1).tobytes() and st.table_sha256 == ""
    assert st.dropped == int((bins[:n_events] < 0).sum()) and int(st.frames.sum()) + st.dropped == n_events
    if not one_stream:   # every stream's set took part: no single set holds all binned frames
        per_set = [int(acc[0].cpu().sum()) for acc in cons._acc]
        assert sum(per_set) == int(st.frames.sum()) and max(per_set) < sum(per_set)
    # process_frames (frames that are not queue items) lands in the same run
    extra = [pool[g % POOL].to(cuda_device) for g in range(n_events, n_events + 3)]
    cons.process_frames(extra, [(0, g, g, _energy(g)) for g in range(n_events, n_events + 3)])
    st2 = cons.stats()
    allf = torch.stack([pool[g % POOL] for g in range(n_events + 3)])
    _same(st2, _want(allf, bins, binning.nbins))
    assert cons.frames == n_events + 3
    # the per-frame rows are in order, dropped frames included
    assert st2.gevt.tolist() == list(range(n_events + 3)) and st2.idx.tolist() == list(range(n_events + 3))
    assert st2.bin.tolist() == bins.tolist() and st2.bin.dtype == np.int16
    pe = np.array([np.nan if e is None else e for e in energies])
    assert np.array_equal(st2.photon_energy, pe, equal_nan=True)
    ep.close()


@pytest.mark.gpu
def test_bins_from_a_table_and_refusals(native, cuda_device):
    from psana_ray_amd.pipeline import CubeConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    pool = _golden_pool(3)
    shape = tuple(pool.shape[1:])
    n = int(np.prod(shape))
    table = np.array([2, -1, 0, 2, 5, 5, 0, 1, 2, -1], np.int64)   # events 10 .. are outside the table
    binning = cube.CubeBinning("gevt", table=table, nbins=7)
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 16, 16))
    cons = CubeConsumer(ep, shape, binning, detector=DET, batch=8, vmin=-50.0, vmax=400.0, frac_bits=5)
    frames = torch.stack([pool[g % POOL] for g in range(12)])
    assert _feed(cons, ep, frames, 8) == [8, 4]
    st = cons.stats()
    bins = binning.bin_of(range(12))
    assert bins.tolist() == table.tolist() + [-1, -1]
    _same(st, _want(frames, bins, 7, vmin=-50.0, vmax=400.0, S=5))
    assert st.by == "gevt" and st.table_sha256 == binning.table_sha256 and st.edges.size == 0 and st.dropped == 4
    with pytest.raises(ValueError, match="does not fit"):
        CubeConsumer(ep, shape, binning, acc_budget=7 * n * 20 - 1)
    with pytest.raises(ValueError):
        CubeConsumer(ep, shape, "photon_energy")
    for kw in (dict(vmin=1.0, vmax=0.0), dict(frac_bits=17), dict(frac_bits=11), dict(vmax=float("inf"))):
        with pytest.raises(ValueError):
            CubeConsumer(ep, shape, binning, **kw)
    ep.close()
    ep = QueueEndpoint(FrameRing(shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="float32"):
        CubeConsumer(ep, shape, binning)
    CubeConsumer(ep, shape, binning, check_ring=False)            # calibrate-on-read: the ring is raw
    ep.close()
    # Q = 2^30: a run of 7 frames; the consumer refuses the 8th before any launch
    ep = QueueEndpoint(FrameRing(shape, torch.float32, cuda_device, 4, 4))
    cons = CubeConsumer(ep, shape, binning, vmin=-3.0, vmax=2.0 ** 20, frac_bits=10, batch=4)
    assert cons.max_frames == 7
    x = [torch.ones(shape, dtype=torch.float32, device=cuda_device) for _ in range(4)]
    cons.process_frames(x, [(0, g, g, None) for g in range(4)])
    with pytest.raises(ValueError, match="max_frames = 7"):
        cons.process_frames(x, [(0, g, g, None) for g in range(4, 8)])
    cons.process_frames(x[:3], [(0, g, g, None) for g in range(4, 7)])
    with pytest.raises(ValueError, match="max_frames = 7"):
        cons.poll(timeout=0.0)
    st = cons.stats()
    assert st.frames.tolist() == [2, 0, 2, 0, 0, 2, 0] and st.dropped == 1
    assert bool((st.cnt[5] == 2).all()) and bool((st.sum[5] == 2 * 1024).all())
    ep.close()
