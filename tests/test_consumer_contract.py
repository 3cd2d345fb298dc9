"""The surface the consumer engines of psana_ray_amd.pipeline share (poll / process_frames / metrics /
synchronize over pipeline._BatchConsumer and its two bases, _RunAccumulator and _PackedRows); the first
four (KINDS) each against its golden model in ops.reference: on a CPU endpoint anywhere, and on the GPU
through the ring-slot path and the tensor path in one run."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd import pipeline, sparse
from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.models import RadialBinning, get_detector, make_geometry
from psana_ray_amd.ops import reference
from psana_ray_amd.queue import EndOfStream, FrameRing, QueueEndpoint
from psana_ray_amd.source import SyntheticRun
from tests.test_sparse_pipeline_gpu import HIT_SON, HIT_THR_PEAK, _moved_counts, _peak_counts

DET = "tiny_epix"                # 2 x 32 x 48 = 3072 pixels
# 13 frames in batches of 3 are the polls [3, 3, 3, 3, 1]: five launches, so both streams run, buffer row 0
# is reused by the fifth launch (on its own stream) and the last batch is partial; EXTRA more frames then
# go through the tensor path
N, BATCH, EXTRA = 13, 3, 3
SEED = 26                        # of the synthetic frames: test_peak_counts_have_margin
PARAMS = PeakFinderParams(thr_peak=HIT_THR_PEAK, son_min=HIT_SON)
NBINS, ADU = 32, (3, 16000)
CAP = 450                        # some of the frames keep more pixels than this: they overflow
KINDS = ["peak", "radial", "dark", "sparse", "sparse_hits"]
RUN_ACCUMULATORS = [pipeline.DarkStatsConsumer, pipeline.PowderConsumer, pipeline.PixelHistConsumer,
                    pipeline.PhotonConsumer, pipeline.CubeConsumer]
PACKED_ROWS = [pipeline.SparseFrameConsumer, pipeline.DropletConsumer]
CLASSES = [pipeline.PeakFinderConsumer, pipeline.RadialProfileConsumer, pipeline.RoiConsumer,
           *RUN_ACCUMULATORS, *PACKED_ROWS]


@functools.lru_cache(maxsize=None)
def _frames():
    """(raw uint16 [N + EXTRA, P, H, W], their calibrated float32 frames from the golden model)."""
    src = SyntheticRun("synthetic", 4, DET, n_events=N + EXTRA, pool_frames=N + EXTRA, seed=SEED, gen_device="cpu")
    raw = torch.from_numpy(np.ascontiguousarray(src.pool).view(np.int16)).view(torch.uint16)
    cal = reference.calibrate_reference(torch.from_numpy(src.pool.astype(np.int32)), src.consts, None, None)
    return raw, cal.contiguous()


@functools.lru_cache(maxsize=None)
def _counts():
    return tuple(_peak_counts(_frames()[1], PARAMS))


def _min_peaks():
    return sorted(_counts())[len(_counts()) // 2]


@functools.lru_cache(maxsize=None)
def _binning():
    return RadialBinning.from_geometry(make_geometry(get_detector(DET)), "calib", NBINS)


def _energy(i):
    return None if i % 4 == 3 else 9.5 + i


def _meta(i):
    return (0, 100 + i, 7 * i, _energy(i))   # rank, idx, gevt, photon energy


@functools.lru_cache(maxsize=None)
def _golden(kind, n):
    """What ``synchronize()`` gives after the first n frames (compared in _check)."""
    raw, cal = _frames()
    if kind == "peak":
        return sum(_counts()[:n])
    if kind == "radial":
        from psana_ray_amd.models import radial as R

        s, c, _ = reference.radial_profile_reference(cal[:n], _binning().bins, NBINS, R.DEFAULT_VMIN, R.DEFAULT_VMAX,
                                                     R.DEFAULT_FRAC_BITS)
        return s.sum(0).numpy(), c.to(torch.int64).sum(0).numpy(), n
    if kind == "dark":
        c, s, q = reference.dark_accumulate_reference(raw[:n], get_detector(DET).kernel_kind, *ADU)
        return c.to(torch.int64).numpy(), s.numpy(), q.numpy(), n
    hits = kind == "sparse_hits"
    keys = torch.tensor(_counts()[:n], dtype=torch.int32) if hits else None
    nnz, flags, offs, pix, val = reference.sparsify_reference(cal[:n], sparse.DEFAULT_THR, sparse.DEFAULT_VMAX, CAP,
                                                              keys=keys, key_min=_min_peaks() if hits else 0)
    m = [_meta(i) for i in range(n)]
    return {"rank": [x[0] for x in m], "idx": [x[1] for x in m], "gevt": [x[2] for x in m],
            "photon_energy": np.array([np.nan if x[3] is None else x[3] for x in m]), "nnz": nnz.numpy(),
            "flags": flags.numpy(), "offs": offs.numpy(), "pix": pix.numpy(), "val": val.numpy()}


def _consumer(kind, ep, **kw):
    shape = get_detector(DET).frame_shape
    if kind == "peak":
        return pipeline.PeakFinderConsumer(ep, shape, PARAMS, batch=BATCH, keep_results=True, **kw)
    if kind == "radial":
        return pipeline.RadialProfileConsumer(ep, _binning(), batch=BATCH, keep_results=True, **kw)
    if kind == "dark":
        return pipeline.DarkStatsConsumer(ep, get_detector(DET), adu_lo=ADU[0], adu_hi=ADU[1], batch=BATCH, **kw)
    hits = kind == "sparse_hits"
    return pipeline.SparseFrameConsumer(ep, shape, cap=CAP, min_peaks=_min_peaks() if hits else 0, peak_params=PARAMS,
                                        detector=DET, batch=BATCH, **kw)


def _run(kind, device, max_items=None):
    """N frames committed to a local ring, then polled to the end of the stream.  Returns (endpoint,
    consumer, the non-zero poll sizes)."""
    data = _frames()[0 if kind == "dark" else 1]
    ep = QueueEndpoint(FrameRing(tuple(data.shape[1:]), data.dtype, device, 16, 16))
    for i in range(N):
        s = ep.acquire(timeout=5.0)
        ep.slot_tensor(s).copy_(data[i])
        ep.commit(s, *_meta(i))
    ep.finish()
    cons = _consumer(kind, ep)
    polls = []
    while True:
        try:
            k = cons.poll(timeout=0.0, max_items=max_items)   # every frame is committed: nothing to wait for
        except EndOfStream:
            break
        if k:
            polls.append(k)
    return ep, cons, polls


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def _check(kind, cons, n):
    """``synchronize()`` after n frames == the golden model, and so are the results that were kept."""
    got, want = cons.synchronize(), _golden(kind, n)
    assert cons.frames == n and cons.metrics()["frames_consumed"] == n
    metas = [tuple(_meta(i)[:3]) for i in range(n)]
    if kind == "peak":
        assert got == want
        assert [m for r in cons.results for m in r[-1]] == metas
        if cons.gpu:   # (peaks, counts, meta) per batch
            assert torch.cat([r[1] for r in cons.results]).tolist() == list(_counts()[:n])
        else:          # (per-frame peak lists, meta) per batch
            assert [int(p.shape[0]) for r in cons.results for p in r[0]] == list(_counts()[:n])
    elif kind == "radial":
        _same(got, want)
        assert [m for _, ms in cons.results for m in ms] == metas
        from psana_ray_amd.models import radial as R

        prof = reference.radial_profile_reference(_frames()[1][:n], _binning().bins, NBINS, R.DEFAULT_VMIN,
                                                  R.DEFAULT_VMAX, R.DEFAULT_FRAC_BITS)[2]
        assert torch.equal(torch.cat([p.cpu() for p, _ in cons.results]).view(torch.int32), prof.view(torch.int32))
    elif kind == "dark":
        _same(got, want)
    else:
        sf = sparse.concat(got)
        for name, w in want.items():
            g = getattr(sf, name)
            if name == "val":   # bit patterns
                g, w = g.view(np.int32), w.view(np.int32)
            assert np.array_equal(g, w, equal_nan=name == "photon_energy"), name   # NaN: no photon energy
        stored = int((sf.flags == 0).sum())
        assert 0 < stored < n and cons.metrics()["frames_stored"] == stored
        assert (int((sf.flags == sparse.FLAG_SKIPPED).sum()) > 0) == (kind == "sparse_hits")


def test_peak_counts_have_margin():
    """The reference peak counts of the frames (SEED) do not change when thr_peak moves by +-0.01 and
    son_min by +-1 % (test_sparse_pipeline_gpu._moved_counts), so the GPU's counts must EQUAL them;
    and the hit filter's N separates the frames."""
    counts = list(_counts())
    assert _moved_counts(_frames()[1], PARAMS) == [counts, counts]
    assert min(counts) < _min_peaks() <= max(counts) and max(counts) < PARAMS.max_peaks


def test_one_loop_for_every_consumer():
    """poll / process / sync_streams / _next exist once, in the base, and no engine has a _meta_of of its own;
    the run bound and the combine of the per-stream sets exist once, in _RunAccumulator; the two-step drain
    exists once, in _PackedRows; no other engine limits a poll."""
    base, acc, rows = pipeline._BatchConsumer, pipeline._RunAccumulator, pipeline._PackedRows
    assert len(CLASSES) == len(set(CLASSES)) == 10
    for cls in CLASSES:
        assert issubclass(cls, base)
        for name in ("poll", "process", "sync_streams", "_next", "_meta_of"):
            assert getattr(cls, name) is getattr(base, name), (cls, name)
        assert "_meta_of" not in vars(cls)
        assert issubclass(cls, acc) == (cls in RUN_ACCUMULATORS) and issubclass(cls, rows) == (cls in PACKED_ROWS)
    for name in ("_limit", "_check_bound", "synchronize"):
        assert name in vars(acc), name
        for cls in RUN_ACCUMULATORS:
            assert name not in vars(cls) and getattr(cls, name) is getattr(acc, name), (cls, name)
    for name in ("_launched", "_advance", "take_results", "synchronize"):
        assert name in vars(rows), name
        for cls in PACKED_ROWS:
            assert name not in vars(cls) and getattr(cls, name) is getattr(rows, name), (cls, name)
    for cls in CLASSES:
        if cls not in RUN_ACCUMULATORS:
            assert cls._limit is base._limit, cls


@pytest.mark.parametrize("kind", KINDS)
def test_cpu_endpoint(kind):
    ep, cons, polls = _run(kind, torch.device("cpu"))
    assert sum(polls) == N and max(polls) <= BATCH
    _check(kind, cons, N)
    ep.close()
    ep, cons, polls = _run(kind, torch.device("cpu"), max_items=2)
    assert sum(polls) == N and max(polls) <= 2 and cons.frames == N
    ep.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", KINDS)
def test_slots_then_tensors(native, cuda_device, kind):
    ep, cons, polls = _run(kind, cuda_device)
    assert polls == [3, 3, 3, 3, 1] and cons._b == 5 and len(cons.streams) == 2 and cons._nbuf == 4
    _check(kind, cons, N)
    # three more frames that are not queue items: the tensor path lands in the same totals
    data = _frames()[0 if kind == "dark" else 1]
    extra = [data[i].to(cuda_device) for i in range(N, N + EXTRA)]
    cons.process_frames(extra, [_meta(i)[:4 if kind.startswith("sparse") else 3] for i in range(N, N + EXTRA)])
    _check(kind, cons, N + EXTRA)
    ep.close()
