"""Producer and consumer pipelines (the per-rank engines behind the CLIs and ``bench.py``).

Producer (replaces psana_ray/producer.py:78-117, ``produce_data``):
    source events (pinned host pages) --hipMemcpyAsync, side stream--> raw HBM chunk buffers
    --calibration kernels, compute stream--> HBM ring slots --commit--> sharded queue
  * triple-buffered raw chunks: the H2D copy of chunk k+1 overlaps the kernels of chunk k;
    everything is ordered with HIP events, the host never waits for the device except on
    backpressure (no free slot) -- which replaces the reference's sleep-based exponential
    backoff (producer.py:105-111) with a condition-variable wait;
  * masks (bad-pixel via ``create_bad_pixel_mask()``, manual ``.npy``; truthy keeps,
    producer.py:81-82,92-95) are folded into the kernel tables once, not applied per event;
  * frames are written straight into the destination slot (no intermediate copies).

Consumer: drains this rank's shard in batches and runs the on-GPU peak finder (K-07) on a
consumer stream, releasing slots stream-ordered (BASELINE config 5); RadialProfileConsumer runs the
radial profile (K-08) the same way and keeps an exact integer run accumulator on the device;
SparseFrameConsumer writes the pixels above a threshold as (index, value) pairs (K-10), optionally only
of the frames the peak finder calls hits; PowderConsumer keeps the exact per-pixel run sums, spread and
maximum of the calibrated frames (K-11), split into misses and hits by the same device-side filter;
PixelHistConsumer keeps the exact per-pixel spectrum of the calibrated frames (K-12); PhotonConsumer counts
photons per pixel with psana's neighbour merge (K-13): run maps and the per-frame P(k) of up to 8 ROIs;
DropletConsumer writes every frame's connected clusters of pixels above a threshold as integer rows (K-14);
CubeConsumer keeps the exact per-pixel run sums of the calibrated frames per bin of a per-event scalar (K-15);
RoiConsumer keeps per frame the sum, moments, maximum and projections of up to 16 rectangles, read from the
rectangles alone (K-16).  The batch loop is written once, in _BatchConsumer.  _RunAccumulator (dark,
powder, hist, photons, cube) adds the frame bound of a run and one accumulator set per stream, with the one
combine of the sets in ``synchronize()``; _PackedRows (sparse, droplets) adds the header row, the data
columns and the two-step drain to pinned host memory, with its ordering rule.
"""
from __future__ import annotations

import collections
import logging
import threading
import time
from typing import List, Optional

import numpy as np
import torch

from .config import (CONSUMER_STREAM_KIND, CONSUMER_STREAMS, PRODUCER_STREAM_KIND, STREAM_KINDS, PeakFinderParams,
                     pipeline_shape)
from .models.calibrator import Calibrator
from .ops import _ext, kernels
from .queue.endpoint import EndOfStream, FrameItem, QueueEndpoint
from .utils.tracing import trace_range

log = logging.getLogger(__name__)


def resolve_producer_streams(where: str, compute_streams: Optional[int] = None,
                             ranks_per_gpu: Optional[int] = None) -> int:
    """Producer compute streams: ``compute_streams``, else config.pipeline_shape for raw frames
    ``where`` ("device" / "staged") on a GPU shared by ``ranks_per_gpu`` ranks (None: the launch's,
    parallel.launch.ranks_per_gpu).  ProducerPipeline, the producer CLI and bench.py all use it."""
    if compute_streams is not None:
        return int(compute_streams)
    if ranks_per_gpu is None:
        from .parallel.launch import ranks_per_gpu as _rpg

        ranks_per_gpu = _rpg()
    return pipeline_shape(where, int(ranks_per_gpu))["producer_streams"]


def resolve_consumer_batch(batch: Optional[int] = None, ranks_per_gpu: Optional[int] = None) -> int:
    """Frames per peak-finder launch: ``batch``, else config.pipeline_shape for the ranks sharing
    this GPU (PeakFinderConsumer, the producer's co-consumer, psana-ray-consumer, bench.py)."""
    if batch is not None:
        return int(batch)
    if ranks_per_gpu is None:
        from .parallel.launch import ranks_per_gpu as _rpg

        ranks_per_gpu = _rpg()
    return pipeline_shape("device", int(ranks_per_gpu))["consumer_batch"]


class ProducerPipeline:
    def __init__(self, source, calibrator: Optional[Calibrator], endpoint: QueueEndpoint, rank: int = 0,
                 chunk: int = 32, n_raw_buffers: int = 6, acquire_timeout_s: float = 1.0,
                 log_every: int = 0, copy_workgroups: int = 32, gpu_timing: bool = False,
                 compute_streams: Optional[int] = None, stream_kind: Optional[str] = None,
                 mask: Optional[np.ndarray] = None, n_upload_buffers: int = 3, gap_fill: Optional[bool] = None,
                 ranks_per_gpu: Optional[int] = None):
        """copy_workgroups: host->HBM staging by copy_h2d_kernel with that many workgroups (0 = the
        runtime's hipMemcpyAsync); gpu_timing: event-time each chunk's copy and calibration;
        compute_streams: chunks alternate over that many HIP streams (native engine), so one chunk's
        calibration fills the CUs its predecessor's tail leaves idle; stream_kind: their
        hardware-queue placement (config.STREAM_KINDS).  None: config.pipeline_shape /
        PRODUCER_STREAM_KIND for the source (raw frames already in HBM or staged) and the number of
        ranks sharing this GPU (``ranks_per_gpu``; None: parallel.launch.ranks_per_gpu()).

        gap_fill: image mode, zero the panel gaps of every frame (None: only when the ring was not
        zero-filled at creation -- ``FrameRing.zero_filled`` -- since a zeroed ring's gaps stay 0).

        Sources whose frames arrive calibrated (psana_wrapper without raw access): ``mask`` (truthy
        keeps, producer.py:92-95) is applied on the device after the upload; frames move in
        ``chunk``-frame batches through ``n_upload_buffers`` pinned staging buffers (one H2D copy per
        frame, no host synchronisation except before a staging buffer is refilled)."""
        self.source = source
        self.cal = calibrator
        self.ep = endpoint
        self.rank = rank
        self.chunk = min(chunk, kernels.MAX_FRAMES)
        self.device = endpoint.ring.device
        self.gpu = self.device.type == "cuda"
        self.acquire_timeout_s = acquire_timeout_s
        self.log_every = log_every
        self.frames = 0
        self.full_waits = 0
        self.t_first = None
        self.calibrated_source = getattr(source, "calibrated", False)
        # which calibration runs (metrics "producer.source_path"): the HIP kernels on raw frames,
        # psana's CPU calibration (psana_wrapper fallback), or the fp32 golden model (CPU rehearsal)
        self.source_path = "psana_cpu" if self.calibrated_source else ("raw_hip" if self.gpu else "raw_cpu")
        spec = getattr(source, "spec", None)
        file_source = getattr(source, "reader", None)   # RawFileRun: native RawRunReader
        # file sources: DMA straight out of the registered file mapping when possible
        zero_copy = source.zero_copy_frames() if (self.gpu and not self.calibrated_source
                                                  and hasattr(source, "zero_copy_frames")) else None
        self.zero_copy = zero_copy is not None
        use_engine = self.gpu and not self.calibrated_source and (hasattr(source, "cycled_frames")
                                                                  or file_source is not None)
        if self.gpu and not self.calibrated_source and not use_engine:
            _ext.load()
            self.h2d = torch.cuda.Stream(device=self.device)
            self.compute = torch.cuda.Stream(device=self.device)
            self.raw_bufs = torch.empty((n_raw_buffers, self.chunk, *spec.frame_shape), dtype=torch.uint16,
                                        device=self.device)
            self.buf_free = [torch.cuda.Event() for _ in range(n_raw_buffers)]
            self.buf_used = [False] * n_raw_buffers
            self.h2d_done = [torch.cuda.Event() for _ in range(n_raw_buffers)]
        self._k = 0
        self.mask = None
        if self.calibrated_source:
            self._init_upload(mask, n_upload_buffers)
        # completion log of the Python paths: (frames so far, perf_counter s) at commit -- the CPU
        # calibration is synchronous, so commit == completion (the native engine logs device events)
        self._done_log: List[tuple] = []
        self._inflight = collections.deque()
        self._reuses = hasattr(source, "n_staging")
        self.engine = None
        self.gap_fill = None        # image mode, native engine: kernels zero the panel gaps per frame
        self.stream_config = None   # (compute streams, kind) of the native engine
        if use_engine:
            # native hot loop: no Python (and no GIL) per frame or per chunk
            C = _ext.load()
            ring = endpoint.ring
            dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
            # gevt = event_rank + k * size; a panel-sharded source (source/shard.py) shards events
            # over rank GROUPS, while the headers keep this rank (its panel shard)
            plan = calibrator.plan
            n_gaps = plan.n_gap_runs
            self.gap_fill = bool(n_gaps) and (not ring.zero_filled if gap_fill is None else bool(gap_fill))
            if n_gaps and not self.gap_fill:
                plan.n_gap_runs = 0   # the engine keeps its own copy of the plan
            try:
                self.engine = C.ProducerEngine(ring.pool, ring.frame_bytes, dev_index,
                                               plan, self.chunk, n_raw_buffers,
                                               int(getattr(source, "event_rank", rank)),
                                               int(getattr(source, "size", 1)),
                                               copy_workgroups=int(copy_workgroups), gpu_timing=bool(gpu_timing))
            finally:
                plan.n_gap_runs = n_gaps
            self.engine.set_header_rank(int(rank))
            if zero_copy is not None:
                ptrs, pe = zero_copy
                self._source_map = source._map       # keep the registered mapping alive
                self.engine.set_cycled_source(ptrs, [float("nan") if v is None else float(v) for v in pe])
            elif file_source is not None:
                self.engine.set_file_source(file_source)    # file reads + staging in the native loop
            else:
                ptrs, pe = source.cycled_frames()
                self.engine.set_cycled_source([int(x) for x in ptrs],
                                              [float("nan") if v is None else float(v) for v in pe])
            where = "device" if self.engine.device_resident else "staged"
            n_cs = resolve_producer_streams(where, compute_streams, ranks_per_gpu)
            kind = PRODUCER_STREAM_KIND[where] if stream_kind is None else stream_kind
            self.engine.set_compute_streams(n_cs, STREAM_KINDS[kind])
            self.stream_config = (n_cs, kind)
            fab = getattr(endpoint, "_fabric", None)
            if fab is not None and fab.direct():
                # frames routed to other processes are calibrated straight into their consumer's
                # slot (csrc/fabric.h take_direct); cleared after the engine stopped (_run_engine)
                self.engine.set_fabric(fab)
                from .config import fabric_direct_headroom, fabric_direct_wait_s
                head = fabric_direct_headroom(ring.frame_bytes)   # the byte cap bench / the CLI sized the ring with
                if head > 0 and ring.pool.producer_budget - head >= 2 * self.chunk:
                    self.engine.set_direct_headroom(head, fabric_direct_wait_s())

    # --------------------------------------------------------------------------------
    def _acquire(self, n: int, stream) -> List[int]:
        slots = []
        while len(slots) < n:
            s = self.ep.acquire(timeout=self.acquire_timeout_s, stream=stream)
            if s is None:
                self.full_waits += 1
                if self.full_waits % 50 == 1:
                    log.info("Rank %d: Queue is full, waiting...", self.rank)  # producer.py:106
                continue
            slots.append(s)
        return slots

    def step(self) -> int:
        """Produce up to ``chunk`` frames.  Returns the number produced (0 = source exhausted)."""
        if self.t_first is None:
            self.t_first = time.perf_counter()
        if self.calibrated_source:
            return self._step_calibrated()
        if self._reuses and self.gpu:
            # the source refills pinned staging slots: keep its ring ahead of in-flight copies
            max_inflight = max(1, self.source.n_staging // self.chunk - 1)
            while len(self._inflight) >= max_inflight:
                self._inflight.popleft().synchronize()
        evs = self.source.next_events(self.chunk)
        if not evs:
            return 0
        n = len(evs)
        if self.gpu:
            C = _ext.load()
            b = self._k % len(self.raw_bufs)
            self._k += 1
            buf = self.raw_bufs[b]
            if self.buf_used[b]:
                self.h2d.wait_event(self.buf_free[b])
            self.buf_used[b] = True
            nbytes = evs[0].raw.nbytes
            C.memcpy_h2d_batch([int(buf[i].data_ptr()) for i in range(n)], [int(e.host_ptr) for e in evs], nbytes,
                               int(self.h2d.cuda_stream))
            self.h2d_done[b].record(self.h2d)
            if self._reuses:
                ev = torch.cuda.Event()
                ev.record(self.h2d)
                self._inflight.append(ev)
            slots = self._acquire(n, self.compute)
            self.compute.wait_event(self.h2d_done[b])
            outs = [self.ep.slot_tensor(s) for s in slots]
            self.cal.run([buf[i] for i in range(n)], outs, self.compute)
            self.buf_free[b].record(self.compute)
            for s, e in zip(slots, evs):
                self.ep.commit(s, self.rank, e.idx, e.gevt, e.photon_energy, self.compute)
        else:
            slots = self._acquire(n, None)
            raw = [torch.from_numpy(np.ascontiguousarray(e.raw).view(np.int16)).view(torch.uint16) for e in evs]
            outs = [self.ep.slot_tensor(s) for s in slots]
            self.cal.run(raw, outs)
            for s, e in zip(slots, evs):
                self.ep.commit(s, self.rank, e.idx, e.gevt, e.photon_energy)
        self.frames += n
        if not self.gpu:
            self._done_log.append((self.frames, time.perf_counter()))
        if self.log_every and self.frames % self.log_every < n:
            log.info("Rank %d produced: idx=%d | shape=%s | photon_energy=%s", self.rank, evs[-1].idx,
                     tuple(self.ep.ring.frame_shape), evs[-1].photon_energy)
        return n

    def _init_upload(self, mask, n_bufs: int):
        """Pinned staging for sources that deliver calibrated frames (psana_wrapper fallback path)."""
        shape = tuple(self.ep.ring.frame_shape)
        self._up_shape = shape
        self._up_bufs, self._up_done, self._up_keep = [], [], []
        if mask is not None:
            m = np.asarray(mask).astype(bool)
            if m.shape != shape:
                if m.size != int(np.prod(shape)):
                    raise ValueError(f"mask of shape {m.shape} does not match the frames {shape}")
                m = m.reshape(shape)
            self.mask = torch.from_numpy(~m).to(self.device)   # True = zero this pixel
            # the GPU path masks a whole uploaded chunk in one kernel launch (ops.kernels.mask_frames)
            self._mask_u8 = self.mask.reshape(-1).to(torch.uint8).contiguous() if self.gpu else None
        if self.gpu:
            C = _ext.load()
            nbytes = self.chunk * int(np.prod(shape)) * 4
            for _ in range(max(2, n_bufs)):
                keep = C.PinnedBuffer(nbytes)
                self._up_keep.append(keep)
                self._up_bufs.append(np.frombuffer(keep, dtype=np.float32).reshape(self.chunk, *shape))
                self._up_done.append(None)
            self._up_stream = torch.cuda.Stream(device=self.device)
        self._it = None

    def _step_calibrated(self) -> int:
        """psana path: frames arrive calibrated on the host in the producer's mode.  Up to ``chunk``
        frames are gathered into a pinned staging buffer, copied into their ring slots on a side
        stream (one H2D copy per frame), masked on the device and committed stream-ordered; the host
        waits only before it refills a staging buffer whose copies are still running."""
        if self._it is None:
            self._it = self.source.iter_events(self.source.mode) if hasattr(self.source, "mode") \
                else self.source.iter_events()
            self._idx = int(getattr(self.source, "cursor", 0))
        shape = self._up_shape
        frames, pes = [], []
        for _ in range(self.chunk):
            try:
                data, pe = next(self._it)
            except StopIteration:
                break
            data = np.asarray(data)
            if data.ndim == 2:
                data = data[None]   # producer.py:96-97
            if data.shape != shape:
                raise ValueError(f"psana frame of shape {data.shape}; the queue was built for {shape}")
            frames.append(data)
            pes.append(pe)
        n = len(frames)
        if n == 0:
            return 0
        idx0 = self._idx
        self._idx += n
        if self.gpu:
            C = _ext.load()
            b = self._k % len(self._up_bufs)
            self._k += 1
            if self._up_done[b] is not None:
                self._up_done[b].synchronize()   # this staging buffer's previous copies finished
            buf = self._up_bufs[b]
            for i, f in enumerate(frames):
                np.copyto(buf[i], f, casting="same_kind")
            st = self._up_stream
            slots = self._acquire(n, st)
            C.memcpy_h2d_batch([int(self.ep.slot_ptr(s)) for s in slots], [int(buf[i].ctypes.data) for i in range(n)],
                               int(buf[0].nbytes), int(st.cuda_stream))
            if self.mask is not None:   # np.where(mask, data, 0): one launch for the chunk
                kernels.mask_frames([self.ep.slot_tensor(s) for s in slots], self._mask_u8, st)
            ev = torch.cuda.Event()
            ev.record(st)
            self._up_done[b] = ev
            for i, s in enumerate(slots):
                self.ep.commit(s, self.rank, idx0 + i, self.rank + (idx0 + i) * int(getattr(self.source, "size", 1)),
                               pes[i], st)
        else:
            slots = self._acquire(n, None)
            for i, s in enumerate(slots):
                t = self.ep.slot_tensor(s)
                t.copy_(torch.from_numpy(np.ascontiguousarray(frames[i], dtype=np.float32)).view(t.shape))
                if self.mask is not None:
                    t.masked_fill_(self.mask.view(t.shape), 0.0)
                self.ep.commit(s, self.rank, idx0 + i, self.rank + (idx0 + i) * int(getattr(self.source, "size", 1)),
                               pes[i])
            self._done_log.append((self.frames + n, time.perf_counter()))
        self.frames += n
        return n

    @property
    def produced(self) -> int:
        """Frames whose calibration has COMPLETED (native engine: the chunk's device event; CPU: the
        commit).  ``enqueued`` counts frames committed with kernels possibly still running."""
        return int(self.engine.completed) if self.engine is not None else self.frames

    @property
    def enqueued(self) -> int:
        return int(self.engine.frames) if self.engine is not None else self.frames

    def completion_log(self, since: int = 0):
        """``(first_index, [(frames completed so far, t_seconds), ...])`` -- one entry per completed
        chunk from index ``since`` on, times on the :meth:`clock` of this producer."""
        if self.engine is not None:
            first, v = self.engine.completions(int(since))
            return int(first), [(int(f), ms * 1e-3) for f, ms in v]
        return int(since), list(self._done_log[int(since):])

    def clock(self, stream=None) -> float:
        """Now on the completion log's clock (seconds).  Native engine: device time of an event
        recorded on ``stream`` (default: current) -- the host waits for it, so a consumer stream's
        work issued before is finished at that point."""
        if self.engine is not None:
            h = _ext.stream_handle(stream) if stream is not None else int(torch.cuda.current_stream(self.device).cuda_stream)
            return float(self.engine.mark(h)) * 1e-3
        return time.perf_counter()

    def metrics(self) -> dict:
        """Cumulative counters for utils.metrics (sampled, nothing runs per frame)."""
        d = {"frames_produced": self.produced,
             "full_waits": int(self.engine.full_waits) if self.engine is not None else self.full_waits,
             "source_path": self.source_path}
        if self.engine is not None:
            st, acq, launch, commit, total = self.engine.timing()
            d.update(host_stage_s=st, host_acquire_s=acq, host_launch_s=launch, host_commit_s=commit)
            if self.engine.gpu_timing_enabled:   # gpu_timing=True: event-timed GPU stages
                h2d_ms, h2d_n, cal_ms, cal_n = self.engine.gpu_timing()
                d.update(gpu_h2d_ms_per_chunk=h2d_ms / max(1.0, h2d_n), gpu_calib_ms_per_chunk=cal_ms / max(1.0, cal_n),
                         gpu_chunks_timed=cal_n)
        return d

    def run(self, max_steps: Optional[int] = None, stop=None) -> int:
        """Produce until the source ends, ``max_steps`` events (per rank, Q-6) or ``stop`` is set."""
        if self.engine is not None:
            return self._run_engine(max_steps, stop)
        while not (stop is not None and stop.is_set()):
            if max_steps is not None and self.frames >= max_steps:
                log.info("Rank %d: Reached max_steps %d, terminating", self.rank, max_steps)
                break
            if max_steps is not None:
                self.chunk = max(1, min(self.chunk, max_steps - self.frames))
            if self.step() == 0:
                break
        if self.gpu and not self.calibrated_source:
            self.compute.synchronize()
        if self.gpu and self.calibrated_source:
            self._up_stream.synchronize()
        self.ep.finish()
        return self.frames


    def _run_engine(self, max_steps, stop) -> int:
        n_local = self.source.n_local_events() if hasattr(self.source, "n_local_events") else None
        self.t_first = time.perf_counter()
        k0 = int(getattr(self.source, "cursor", 0))   # resume cursor (source.seek / --start_event)
        self.engine.start(-1 if n_local is None else int(n_local), -1 if max_steps is None else int(max_steps), k0)
        try:
            while not self.engine.join(0.05):
                if (stop is not None and stop.is_set()) or self.ep.failed is not None:
                    self.engine.request_stop()
        finally:
            self.engine.request_stop()
            self.engine.join(-1.0)
            self.engine.set_fabric(None)   # the endpoint may close (and free the fabric) from here on
        err = self.engine.error()
        self.frames = int(self.engine.frames)
        self.full_waits = int(self.engine.full_waits)
        if max_steps is not None and self.frames >= max_steps:
            log.info("Rank %d: Reached max_steps %d, terminating", self.rank, max_steps)
        self.ep.finish()
        if err:
            raise RuntimeError(f"producer engine failed: {err}")
        self.ep._raise_if_failed()
        return self.frames


# Native streams with a hardware-queue placement, per (device, kind): created once (a native pool,
# csrc/streams.h), handed back here when their OWNER is collected and handed out again -- never
# destroyed while the process runs.  Tensors allocated on a stream keep its handle in torch's
# caching allocator after the wrapper is gone, so destroying the native stream could leave the
# allocator a dangling handle; and every CU-masked stream is a hardware queue of its own, so reuse
# also bounds their number.  No weak reference ever points at a torch stream object: torch's stream
# type does not clear weak references when it is freed, and a weakref left behind crashed the
# interpreter's final garbage collection (_PyWeakref_ClearRef, rc 139 after a passing GPU suite).
_STREAM_POOL: dict = {}
_STREAM_POOL_LOCK = threading.Lock()
# handles whose owner is still alive (token -> (key, handles)): at process exit they go back to the
# native pool too, so close_stream_pool() synchronises and destroys every CU-masked queue of ours
# (a PeakFinderConsumer alive at exit left its queues to the runtime's static teardown)
_STREAMS_IN_USE: dict = {}


def _return_streams(key, handles, token=None):
    with _STREAM_POOL_LOCK:
        if token is not None and _STREAMS_IN_USE.pop(token, None) is None:
            return   # already released at exit
        _STREAM_POOL.setdefault(key, []).extend(handles)


def _release_idle_streams(C):
    """Process exit: the idle pooled handles AND those of owners still alive go back to the native
    pool (csrc/streams.h; release synchronises each stream first)."""
    with _STREAM_POOL_LOCK:
        items = [(k, h) for k, hs in _STREAM_POOL.items() for h in hs]
        items += [(k, h) for k, hs in _STREAMS_IN_USE.values() for h in hs]
        _STREAM_POOL.clear()
        _STREAMS_IN_USE.clear()
    for (dev, kind), h in items:
        C.stream_release(dev, kind, h)


def _make_streams(device, n: int, kind: str, owner=None):
    """n torch streams with the given hardware-queue placement (config.STREAM_KINDS), from the
    process-wide pool of native streams (see _STREAM_POOL); they go back to the pool when ``owner``
    (a plain Python object) is collected."""
    if STREAM_KINDS[kind] == 0:
        return [torch.cuda.Stream(device=device) for _ in range(n)]
    import weakref

    C = _ext.load()
    dev = device.index if device.index is not None else torch.cuda.current_device()
    key = (dev, STREAM_KINDS[kind])
    out, handles = [], []
    for _ in range(n):
        with _STREAM_POOL_LOCK:
            free = _STREAM_POOL.setdefault(key, [])
            h = free.pop() if free else None
        if h is None:
            h = int(C.stream_create(dev, STREAM_KINDS[kind]))
        handles.append(h)
        out.append(torch.cuda.ExternalStream(h, device=device))
    if owner is not None:
        token = object()
        with _STREAM_POOL_LOCK:
            _STREAMS_IN_USE[token] = (key, handles)
        fin = weakref.finalize(owner, _return_streams, key, handles, token)
        fin.atexit = False
    return out


class _BatchConsumer:
    """What the consumer engines share: batches of leased ring slots -> one native call on a consumer
    stream -> stream-ordered release.  A consumer adds its buffers, ``synchronize()`` and the hooks
    at the end of this class.

    GPU: consecutive batches alternate between the consumer streams (two by default), so one launch's
    tail overlaps the next launch's streaming reads instead of idling HBM.  The orderings every
    consumer relies on are stated here once:
      * :meth:`poll` leases on the stream that :meth:`_next` then hands out, and the batch counter
        advances after a non-empty lease only (an empty poll uses no buffer row);
      * the ring slots go back stream-ordered right after the kernels that read them: whatever
        ``_launched`` issues afterwards reads the consumer's own buffers, never a ring slot;
      * the slot headers (a host read) are taken before the release.
    CPU endpoints run the golden models (ops.reference)."""

    name = ""            # the trace range of a batch is "consumer.<name>_batch", errors start "<name>: "
    wants_meta = False   # True: _launched(b, n, st, meta) runs after every launch (results are kept)
    meta_fields = 3      # 4: the meta tuples end with the photon energy (None: the event has none)
    batch_refusal = True   # process_frames refuses more than ``batch`` frames

    def __init__(self, endpoint: QueueEndpoint, batch: Optional[int], ranks_per_gpu: Optional[int], streams: int,
                 stream_kind: str):
        """batch: frames per launch; None -> config.pipeline_shape for the ranks sharing this GPU
        (``ranks_per_gpu``; None: parallel.launch.ranks_per_gpu())."""
        self.ep = endpoint
        self.device = endpoint.ring.device
        self.gpu = self.device.type == "cuda"
        self.batch = min(resolve_consumer_batch(batch, ranks_per_gpu), kernels.MAX_FRAMES)
        self.frames = 0
        self.streams = _make_streams(self.device, int(streams), stream_kind, owner=self) if self.gpu else []
        self.stream = self.streams[0] if self.gpu else None
        self._nbuf = 2 * len(self.streams)   # rows of every per-batch buffer
        self._b = 0                          # batches launched
        self._trace = f"consumer.{self.name}_batch"

    def _next(self):
        """(buffer row, stream index, stream) of the next launch.  Row b is reused by launch
        ``_b + _nbuf``, on the same stream (``_nbuf`` is a multiple of the stream count), so stream
        order alone keeps a launch from overwriting a row that an earlier one still uses."""
        b = self._b % self._nbuf
        k = self._b % len(self.streams)
        self._b += 1
        return b, k, self.streams[k]

    def poll(self, timeout: float = 0.05, max_items: Optional[int] = None) -> int:
        """Take up to ``batch`` ready frames (waiting up to ``timeout`` for the first) and process
        them.  Returns frames processed; raises EndOfStream at the end of the stream."""
        n_max = self._limit(self.batch if max_items is None else max(1, min(self.batch, max_items)))
        if not self.gpu:
            items: List[FrameItem] = []
            it = self.ep.get(timeout=timeout)
            if it is None:
                return 0
            items.append(it)
            while len(items) < n_max:
                try:
                    nxt = self.ep.get(timeout=0.0)
                except EndOfStream:
                    break
                if nxt is None:
                    break
                items.append(nxt)
            self.process(items)
            return len(items)
        # GPU: one native call to lease, one per kernel family, one to release -- no per-batch torch
        # ops and no host sync
        st = self.streams[self._b % len(self.streams)]   # the stream _next() hands out below
        slots = self.ep.get_batch(n_max, timeout, st)
        n = len(slots)
        if n == 0:
            return 0
        C = _ext.load()
        b, k, st = self._next()
        with trace_range(self._trace):
            self._launch_slots(C, slots, b, k, st)
        meta = self._meta_of(self.ep.pool.headers(slots)) if self.wants_meta else None
        self.ep.release_batch(slots, st)
        if self.wants_meta:
            with torch.cuda.stream(st):
                self._launched(b, n, st, meta)
        self.frames += n
        return n

    def process_frames(self, frames, meta=None):
        """Process ``frames`` (tensors on this consumer's device, issued on the current stream) that
        are not queue items -- e.g. frames calibrated on read.  ``meta``: their ``(rank, idx, gevt)``,
        with ``meta_fields = 4`` ``(rank, idx, gevt, photon_energy)`` (shorter tuples are padded with
        None).  GPU: returns the consumer stream the batch runs on."""
        n = len(frames)
        if n == 0:
            return None
        self._check_batch(n)
        meta = self._pad_meta(meta)
        st = None
        if self.gpu:
            b, k, st = self._next()
            st.wait_stream(torch.cuda.current_stream(self.device))   # the frames were produced / leased on it
            with torch.cuda.stream(st):
                self._launch_tensors(list(frames), b, k, st)
                if self.wants_meta:
                    self._launched(b, n, st, list(meta))
        else:
            self._reference(frames, meta)
        self.frames += n
        return st

    def process(self, items: List[FrameItem]):
        if not items:
            return
        st = self.process_frames([it.data for it in items], self._meta_of(items))
        for it in items:
            it.release(st) if self.gpu else it.release()

    def metrics(self) -> dict:
        return {"frames_consumed": self.frames}

    def sync_streams(self):
        """Host waits for every batch issued so far (all consumer streams)."""
        for st in self.streams:
            st.synchronize()

    # ------------------------------------------------------------------ meta tuples
    def _meta_of(self, recs):
        """The meta tuples (``meta_fields`` long) of queue items or slot headers."""
        if self.meta_fields == 3:
            return [(r.rank, r.idx, r.gevt) for r in recs]
        # a slot header carries NaN for "no photon energy", a queue item None
        return [(r.rank, r.idx, r.gevt, None if r.photon_energy != r.photon_energy else r.photon_energy)
                for r in recs]

    def _pad_meta(self, meta):
        """Caller-made meta tuples, padded with None to ``meta_fields``."""
        if meta is None or self.meta_fields == 3:
            return meta
        return [tuple(m) + (None,) * (self.meta_fields - len(m)) for m in meta]

    @staticmethod
    def _meta_columns(meta) -> dict:
        """4-field meta tuples as the columns every result file has (NaN: no photon energy)."""
        return {"rank": [m[0] for m in meta], "idx": [m[1] for m in meta], "gevt": [m[2] for m in meta],
                "photon_energy": [float("nan") if m[3] is None else float(m[3]) for m in meta]}

    # ------------------------------------------------------------------ helpers of the constructors and of stats()
    def _check_ring(self, endpoint: QueueEndpoint, needs: str, dtype=torch.float32, of: Optional[str] = None):
        """Raise unless the ring carries ``dtype`` frames of ``self.n`` elements.  It needs ``name``,
        ``n`` and ``shape`` only, so an engine calls it before the base constructor makes streams."""
        ring = endpoint.ring
        if ring.dtype != dtype:
            raise ValueError(f"{self.name}: the queue carries {ring.dtype} frames, {needs}")
        if int(np.prod(ring.frame_shape)) != self.n:
            raise ValueError(f"{self.name}: queue frames {tuple(ring.frame_shape)} are not the {self.n} pixels of "
                             + (of or f"a frame of {self.shape}"))

    def _keep_pinned(self, bufs, b: int, n: int, meta):
        """_launched: rows ``[b, :n]`` of the device buffers ``bufs`` (None stays None) go to fresh PINNED
        HOST tensors by asynchronous copies on the current (consumer) stream, so a long run keeps
        nothing in HBM; ``(*hosts, meta)`` joins :attr:`results`, valid after :meth:`sync_streams`."""
        kept = []
        for d in bufs:
            h = None
            if d is not None:
                h = torch.empty((n, *d.shape[2:]), dtype=d.dtype, pin_memory=True)
                h.copy_(d[b, :n], non_blocking=True)
            kept.append(h)
        self.results.append((*kept, meta))

    @staticmethod
    def _cat(parts, empty=None):
        """stats(): the kept batches (host tensors or arrays; None is skipped) as one fresh array,
        ``empty`` when there is none."""
        parts = [p.numpy() if isinstance(p, torch.Tensor) else np.asarray(p) for p in parts if p is not None]
        return np.concatenate(parts) if parts else empty

    # ------------------------------------------------------------------ what a consumer fills in
    def _limit(self, n_max: int) -> int:
        """Frames the next poll may take at most (it may raise instead)."""
        return n_max

    def _check_batch(self, n: int):
        """process_frames: raise if a batch of ``n`` frames cannot be taken."""
        if self.batch_refusal and n > self.batch:
            raise ValueError(f"{self.name}: {n} frames in a batch of at most {self.batch}")

    def _launch_slots(self, C, slots, b: int, k: int, st):
        """The native call(s) on leased ring ``slots``: buffer row b, stream k."""
        raise NotImplementedError

    def _launch_tensors(self, frames, b: int, k: int, st):
        """The same through ops.kernels on a list of tensors; ``st`` is the current stream."""
        raise NotImplementedError

    def _reference(self, frames, meta):
        """CPU: the golden model on ``frames``."""
        raise NotImplementedError

    def _launched(self, b: int, n: int, st, meta):
        """After a launch of n frames (``wants_meta``), ``st`` current: keep results.  The ring slots
        may be released already: read this consumer's buffers only."""


class _PeakBuffers:
    """The peak finder's (K-07) device buffers and its two calls, for :class:`PeakFinderConsumer`
    and :class:`_HitFilter`."""

    def __init__(self, device, params: PeakFinderParams, shape, batch: int, nbuf: int, n_streams: int):
        B = batch
        self.params, self.shape = params, tuple(shape)   # (P, H, W)
        self.peaks = torch.empty((nbuf, B, params.max_peaks, 8), dtype=torch.float32, device=device)
        # counts [B] int32 and summary [B, 2] f32 of a batch share one row; the peak finder
        # writes them whole from its self-resetting scratch (no per-batch fill)
        self._meta = torch.zeros((nbuf, 3 * B), dtype=torch.int32, device=device)
        self.counts = self._meta[:, :B]
        self.summary = self._meta[:, B:].view(torch.float32).view(nbuf, B, 2)
        # one scratch block per stream (a block must never serve two launches in flight)
        self.scratch = [torch.zeros(kernels.PF_SCRATCH_WORDS, dtype=torch.int32, device=device)
                        for _ in range(n_streams)]
        self.total = torch.zeros((), dtype=torch.int64, device=device)   # running peak total

    def launch_slots(self, C, ep, slots, b: int, k: int, st):
        """One native call: the peak finder on the ring slots with self-resetting outputs (no fill
        kernel), bumping the on-device running peak total."""
        P, H, W = self.shape
        p = self.params
        C.peakfind_slots(ep.pool, ep._slot_bytes, slots, P, H, W, float(p.thr_peak), float(p.son_min), int(p.radius),
                         int(p.max_peaks), int(self.peaks[b].data_ptr()), int(self.counts[b].data_ptr()),
                         int(self.summary[b].data_ptr()), int(self.total.data_ptr()), int(st.cuda_stream),
                         int(self.scratch[k].data_ptr()))

    def launch_tensors(self, frames, b: int, k: int, st):
        n = len(frames)
        kernels.peakfind(frames, self.shape, self.params, self.peaks[b, :n], self.counts[b, :n], self.summary[b, :n],
                         st, total=self.total, scratch=self.scratch[k])


class _HitFilter:
    """The hit filter of :class:`SparseFrameConsumer` and :class:`PowderConsumer`: with ``min_peaks > 0``
    the peak finder (K-07) runs first on the batch's stream and its per-frame counts are the ``keys``
    the consumer's kernel compares with ``min_peaks`` ON THE DEVICE -- no host round trip.  With
    ``min_peaks == 0`` there is no peak finder and no keys.  The constructor only validates (errors
    start with the owner's ``name``); :meth:`allocate` makes the device buffers once the owner knows
    its batch."""

    def __init__(self, name: str, shape, min_peaks: int, peak_params: Optional[PeakFinderParams]):
        self.min_peaks = int(min_peaks)
        if self.min_peaks < 0:
            raise ValueError(f"{name}: min_peaks must be >= 0")
        self.params = peak_params or PeakFinderParams()
        self.pf = None   # _PeakBuffers (GPU, min_peaks > 0)
        if self.min_peaks > 0:
            if len(shape) not in (2, 3):
                raise ValueError(f"{name}: the hit filter needs 2-D or 3-D frames, got {shape}")
            if self.params.radius not in (1, 2):
                raise ValueError(f"{name}: peak finder radius must be 1 or 2")
            self.shape = tuple(shape) if len(shape) == 3 else (1, *shape)   # (P, H, W)

    def allocate(self, device, batch: int, nbuf: int, n_streams: int):
        if self.min_peaks > 0:
            self.pf = _PeakBuffers(device, self.params, self.shape, batch, nbuf, n_streams)

    def peak_dict(self) -> dict:
        """The peak-finder parameters a result file records ({}: no filter)."""
        if self.min_peaks <= 0:
            return {}
        p = self.params
        return {"thr_peak": float(p.thr_peak), "son_min": float(p.son_min), "radius": float(p.radius)}

    def keys_slots(self, C, ep, slots, b: int, k: int, st) -> int:
        """Ring-slot path: launch the peak finder; the device pointer of the counts row (0: no filter)."""
        if self.pf is None:
            return 0
        self.pf.launch_slots(C, ep, slots, b, k, st)
        return int(self.pf.counts[b].data_ptr())

    def keys_tensors(self, frames, b: int, k: int, st):
        """Tensor path: launch the peak finder; the counts of the frames (None: no filter)."""
        if self.pf is None:
            return None
        self.pf.launch_tensors(frames, b, k, st)
        return self.pf.counts[b, :len(frames)]

    def keys_reference(self, x):
        """CPU: the golden model's counts of the stacked flat frames ``x`` (None: no filter)."""
        if self.min_peaks <= 0:
            return None
        from .ops import reference

        pk, _ = reference.peakfind_reference(x.reshape(x.shape[0], *self.shape), self.params)
        return torch.tensor([int(p.shape[0]) for p in pk], dtype=torch.int32)


class PeakFinderConsumer(_BatchConsumer):
    """Consumer engine: batches of leased slots -> K-07 peak finder -> stream-ordered release.

    GPU: every consumer stream has its own peak-finder scratch, so one launch's candidate-test tail
    (every workgroup tests its parked candidates after its stream of reads) overlaps the next
    launch's streaming reads."""

    name = "peakfind"
    batch_refusal = False

    def __init__(self, endpoint: QueueEndpoint, frame_shape, params: Optional[PeakFinderParams] = None,
                 batch: Optional[int] = None, keep_results: bool = False, stream_kind: str = CONSUMER_STREAM_KIND,
                 streams: int = CONSUMER_STREAMS, ranks_per_gpu: Optional[int] = None):
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.params = params or PeakFinderParams()
        self.shape = tuple(frame_shape)
        self.peaks_total = 0
        self.keep_results = self.wants_meta = keep_results
        self.results = []
        if self.gpu:
            self._pf = pf = _PeakBuffers(self.device, self.params, self.shape, self.batch, self._nbuf,
                                         len(self.streams))
            self.peaks, self.counts, self.summary, self.count_acc = pf.peaks, pf.counts, pf.summary, pf.total

    def _launch_slots(self, C, slots, b, k, st):
        self._pf.launch_slots(C, self.ep, slots, b, k, st)

    def _launch_tensors(self, frames, b, k, st):
        self._pf.launch_tensors(frames, b, k, st)

    def _launched(self, b, n, st, meta):
        self.results.append((self.peaks[b, :n].clone(), self.counts[b, :n].clone(), meta))

    def _reference(self, frames, meta):
        from .ops import reference

        peaks, _summary = reference.peakfind_reference(torch.stack([t.reshape(self.shape) for t in frames]),
                                                       self.params)
        self.peaks_total += sum(int(p.shape[0]) for p in peaks)
        if self.keep_results:
            self.results.append((peaks, meta))

    def synchronize(self):
        if self.gpu:
            self.sync_streams()
            self.peaks_total = int(self.count_acc.item())
        return self.peaks_total


class RadialProfileConsumer(_BatchConsumer):
    """Consumer engine: batches of leased slots -> K-08 radial profile (csrc/radial.hip) ->
    stream-ordered release.

    Per frame: int64 sums / int32 counts / float32 profile ``[nbins]``; per run: the integer
    accumulator ``run_sum`` / ``run_count`` / ``frames`` kept on the device (added to by both consumer
    streams with integer atomics -- exact in any order) and brought to the host by
    :meth:`synchronize`."""

    name = "radial"
    batch_refusal = False

    def __init__(self, endpoint: QueueEndpoint, binning, vmin: Optional[float] = None, vmax: Optional[float] = None,
                 frac_bits: Optional[int] = None, batch: Optional[int] = None, keep_results: bool = False,
                 stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """check_ring=False: the ring holds RAW frames that the caller calibrates before
        :meth:`process_frames` (``--calibrate_on_read``), so the ring's frame shape is not the binning's."""
        from .models import radial as _radial
        from .ops.reference import radial_bound_ok

        self.binning = binning
        self.nbins = int(binning.nbins)
        self.vmin = _radial.DEFAULT_VMIN if vmin is None else float(vmin)
        self.vmax = _radial.DEFAULT_VMAX if vmax is None else float(vmax)
        self.frac_bits = _radial.DEFAULT_FRAC_BITS if frac_bits is None else int(frac_bits)
        self.n = int(binning.bins.size)
        if check_ring and int(np.prod(endpoint.ring.frame_shape)) != self.n:
            raise ValueError(f"radial: binning of {self.n} elements ({binning.layout} layout) for queue frames "
                             f"{tuple(endpoint.ring.frame_shape)}")
        if not self.vmin <= self.vmax or not 0 <= self.frac_bits <= 60:
            raise ValueError("radial: empty value window or frac_bits outside [0, 60]")
        if not radial_bound_ok(self.n, self.vmin, self.vmax, self.frac_bits):
            raise ValueError("radial: max(|vmin|, |vmax|) * 2^frac_bits * n must stay below 2^53")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.keep_results = self.wants_meta = keep_results
        # per batch: (profiles [n, nbins] f32 on the HOST -- pinned, filled asynchronously on the GPU
        # path: read them after sync_streams() / synchronize() --, [(rank, idx, gevt), ...])
        self.results = []
        self.run_sum = np.zeros(self.nbins, np.int64)
        self.run_count = np.zeros(self.nbins, np.int64)
        self.run_frames = 0
        if self.gpu:
            B, nb = self.batch, self.nbins
            self.sums = torch.zeros((self._nbuf, B, nb), dtype=torch.int64, device=self.device)
            self.counts = torch.zeros((self._nbuf, B, nb), dtype=torch.int32, device=self.device)
            self.profile = torch.zeros((self._nbuf, B, nb), dtype=torch.float32, device=self.device)
            self.run = torch.zeros(2 * nb + 1, dtype=torch.int64, device=self.device)
            self.bins = binning.bins_tensor(self.device)
            kernels._validate_bin_map(self.bins, self.n, nb, self.device, "radial")
        else:
            self._bins_cpu = torch.from_numpy(binning.bins.astype(np.int64))

    def _launch_slots(self, C, slots, b, k, st):
        C.radial_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, int(self.bins.data_ptr()), self.nbins,
                       self.vmin, self.vmax, self.frac_bits, int(self.sums[b].data_ptr()),
                       int(self.counts[b].data_ptr()), int(self.profile[b].data_ptr()), int(self.run.data_ptr()),
                       int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        n = len(frames)
        kernels.radial_profile(frames, self.bins, self.nbins, self.sums[b, :n], self.counts[b, :n],
                               self.profile[b, :n], self.vmin, self.vmax, self.frac_bits, run=self.run, stream=st)

    def _launched(self, b, n, st, meta):
        """keep_results, GPU: the batch's profiles go to pinned host memory (64 frames x 1024 bins =
        256 KiB per batch)."""
        self._keep_pinned((self.profile,), b, n, meta)

    def _reference(self, frames, meta):
        from .ops import reference

        s, c, prof = reference.radial_profile_reference(torch.stack([t.reshape(-1) for t in frames]), self._bins_cpu,
                                                        self.nbins, self.vmin, self.vmax, self.frac_bits)
        self.run_sum += s.sum(dim=0).numpy()
        self.run_count += c.to(torch.int64).sum(dim=0).numpy()
        self.run_frames += len(frames)
        if self.keep_results:
            self.results.append((prof, list(meta)))

    def synchronize(self):
        """Wait for every batch and bring the run accumulator to the host.  Returns
        ``(run_sum int64 [nbins], run_count int64 [nbins], frames)``."""
        if self.gpu:
            self.sync_streams()
            run = self.run.cpu().numpy()
            self.run_sum, self.run_count = run[:self.nbins].copy(), run[self.nbins:2 * self.nbins].copy()
            self.run_frames = int(run[2 * self.nbins])
        return self.run_sum, self.run_count, self.run_frames

    def mean_profile(self) -> np.ndarray:
        """Run-averaged profile from the (synchronised) accumulator: float32, +0 where no pixel landed."""
        from .radial import mean_profile

        return mean_profile(self.run_sum, self.run_count, self.frac_bits)


_Field = collections.namedtuple("_Field", "name shape dev host init op", defaults=(0, "sum"))


class _RunAccumulator(_BatchConsumer):
    """What the engines with exact integer run sums share (dark, powder, hist, photons, cube): the frame
    bound of a run, and one accumulator set per consumer stream.

    Their kernels own a pixel per launch and use no global atomics on the run sums, so every stream
    has its OWN set: set k is only ever touched by launches on stream k, and two streams never
    read-modify-write the same words.  Every value is an integer, so the sets combine exactly in any
    order; a count is at most the frames of the run, which ``max_frames`` keeps inside its int32.
    A subclass sets ``max_frames`` and whatever :meth:`_fields` reads BEFORE this constructor, which
    builds
      * ``_acc``: per stream the tuple of device tensors in field order (one field: the bare tensor);
      * ``_host``: the host copy ``{name: array}`` at its initial values -- the CPU path adds the
        golden model's outputs to it (:meth:`_add`), the GPU path replaces it in :meth:`synchronize`,
        the only place where the sets meet."""

    bound_text = "{}"   # how "... would take the run past" goes on; {}: max_frames

    def __init__(self, endpoint: QueueEndpoint, batch: Optional[int], ranks_per_gpu: Optional[int], streams: int,
                 stream_kind: str):
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self._spec = tuple(self._fields())
        self._host = {f.name: np.full(f.shape, f.init, f.host) for f in self._spec}
        if self.gpu:
            sets = [tuple(torch.full(f.shape, f.init, dtype=f.dev, device=self.device) for f in self._spec)
                    for _ in self.streams]
            self._acc = sets if len(self._spec) > 1 else [s[0] for s in sets]

    def _check_bound(self, n: int):
        if self.frames + n > self.max_frames:
            raise ValueError(f"{self.name}: {self.frames} + {n} frames would take the run past "
                             + self.bound_text.format(self.max_frames))

    def _check_batch(self, n: int):
        super()._check_batch(n)
        self._check_bound(n)

    def _limit(self, n_max: int) -> int:
        self._check_bound(1)   # before any lease
        return max(1, min(n_max, self.max_frames - self.frames))

    @staticmethod
    def _fold(total, part, op: str):
        """``total += part`` or, for "max", their element-wise maximum, in place (tensors of one device)."""
        torch.maximum(total, part, out=total) if op == "max" else total.add_(part)

    def _add(self, parts):
        """CPU: the golden model's outputs (tensors in field order) join the host copy."""
        for f, part in zip(self._spec, parts):
            self._fold(torch.from_numpy(self._host[f.name]), part, f.op)

    def synchronize(self):
        """Wait for every batch, combine the per-stream sets ON THE DEVICE one field at a time (a
        temporary is freed before the next is made: at most one field of one set lives beside the
        sets) and copy the one result to the host, where it takes the field's host dtype.  Returns
        :meth:`_result`."""
        if self.gpu:
            self.sync_streams()
            sets = [a if isinstance(a, tuple) else (a,) for a in self._acc]
            host = {}
            with torch.cuda.device(self.device):
                for i, f in enumerate(self._spec):
                    total = sets[0][i]
                    if len(sets) > 1:
                        total = total.clone()
                        for s in sets[1:]:
                            self._fold(total, s[i], f.op)
                    host[f.name] = total.cpu().numpy().astype(f.host, copy=False)
                    del total
            self._host = host
        return self._result()

    # ------------------------------------------------------------------ what a run accumulator fills in
    def _fields(self):
        """The accumulator's fields, stated once: ``_Field(name, shape, device dtype, host dtype,
        initial value = 0, op = "sum" | "max")`` in the order of the kernel's arguments."""
        raise NotImplementedError

    def _result(self):
        """What :meth:`synchronize` returns: the host copy (one field: the bare array)."""
        return self._host if len(self._spec) > 1 else self._host[self._spec[0].name]


class DarkStatsConsumer(_RunAccumulator):
    """Consumer engine: batches of leased RAW uint16 slots -> K-09 dark statistics (csrc/dark.hip) ->
    stream-ordered release.

    Per run: per-pixel, per-candidate count / sum / sum of squares of the raw ADU inside the window
    ``[adu_lo, adu_hi]`` -- integers, so the result is exact in any frame order.  One accumulator set
    per consumer stream (:class:`_RunAccumulator`; the buffer row is not used)."""

    name = "dark"
    batch_refusal = False
    bound_text = "2^31 - 1 (the int32 count)"
    cnt = property(lambda self: self._host["cnt"])   # the (synchronised) run, int64 [NC, n] each
    sum = property(lambda self: self._host["sum"])
    sq = property(lambda self: self._host["sq"])

    def __init__(self, endpoint: QueueEndpoint, spec, adu_lo: int = 0, adu_hi: Optional[int] = None,
                 batch: Optional[int] = None, stream_kind: str = CONSUMER_STREAM_KIND,
                 streams: int = CONSUMER_STREAMS, ranks_per_gpu: Optional[int] = None):
        from .ops.reference import DARK_MAX_FRAMES

        self.spec = spec
        self.kind, self.adu_lo, self.adu_hi = kernels.validate_dark_window(
            spec.kernel_kind, adu_lo, 65535 if adu_hi is None else adu_hi, "dark")
        self.nc = int(spec.n_candidates)
        self.n = int(spec.npix)
        self._check_ring(endpoint, "dark statistics need raw uint16", torch.uint16, spec.name)
        self.max_frames = DARK_MAX_FRAMES
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)

    def _fields(self):
        s = (self.nc, self.n)
        return (_Field("cnt", s, torch.int32, np.int64), _Field("sum", s, torch.int64, np.int64),
                _Field("sq", s, torch.int64, np.int64))

    def _result(self):
        """``(cnt int64 [NC, n], sum int64 [NC, n], sq int64 [NC, n], frames)``."""
        return self.cnt, self.sum, self.sq, self.frames

    def _launch_slots(self, C, slots, b, k, st):
        cnt, s, q = self._acc[k]
        C.dark_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, self.kind, self.adu_lo, self.adu_hi,
                     int(cnt.data_ptr()), int(s.data_ptr()), int(q.data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        cnt, s, q = self._acc[k]
        kernels.dark_accumulate(frames, self.kind, self.adu_lo, self.adu_hi, cnt, s, q, frames_so_far=self.frames,
                                stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        self._add(reference.dark_accumulate_reference(torch.stack([t.reshape(-1) for t in frames]), self.kind,
                                                      self.adu_lo, self.adu_hi))

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.dark.DarkStats`."""
        from .dark import DarkStats

        cnt, s, q, frames = self.synchronize()
        return DarkStats(self.spec.name, self.kind, self.adu_lo, self.adu_hi, frames, cnt.copy(), s.copy(), q.copy())


class _PackedRows(_BatchConsumer):
    """What the engines with packed per-frame rows share (sparse, droplets, roibin): the rows of a
    batch's frames lie behind each other in the data columns, at most ``cap`` per frame, and reach the
    host through pinned buffers in two steps per batch -- the header row first, then exactly ``offs[n]``
    rows of every column (a row is ``_WIDTH[name]`` elements, one unless stated).  Finished batches collect in :attr:`results` as the subclass's frame
    objects (:meth:`take_results` hands them over).  The ring slots are released stream-ordered
    after the kernels, not after the copies.

    The ordering the drain keeps, stated here once:
      * a batch's header is waited for only when at least ``keep`` newer batches have been issued
        (``keep = 1`` while polling: after the NEXT batch, on the other stream, is in flight);
      * its data copy is issued on the batch's OWN stream -- behind the kernels that wrote the rows,
        ahead of the launch that reuses them (:meth:`_next`) -- for exactly ``offs[n]`` elements,
        never the full capacity; what a subclass copies besides the columns (:meth:`_extra_copies`: rows
        counted by something other than ``offs``) is issued at the same place, under the same rule;
      * it is collected one step later, when another batch is behind it;
      * :meth:`synchronize` flushes with two ``keep = 0`` passes: the first issues the last data
        copies, the second collects them.

    A subclass states ``_HDR``, the per-frame header fields ``(name, dtype name)`` -- header row b is
    ``offs`` int64 [B + 1], then every field [B], padded to 16 B -- and ``_COLS``, the data columns
    (``_WIDTH``: elements per row of a column that has more than one), sets ``cap`` and calls
    :meth:`_build_rows` once its batch is final."""

    wants_meta = True
    meta_fields = 4
    _HDR = ()
    _COLS = ()
    _WIDTH = {}

    def __init__(self, endpoint: QueueEndpoint, batch: Optional[int], ranks_per_gpu: Optional[int], streams: int,
                 stream_kind: str):
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self._WIDTH = dict(self._WIDTH)
        self.results = []      # finished batches (frame objects), oldest first
        self._pending = collections.deque()   # GPU batches in flight: dicts, oldest first
        self._lock = threading.Lock()

    def _build_rows(self, scratch_bytes: int):
        """GPU: the header rows, the data columns ``_out[name]`` [_nbuf, B * cap] and one scratch block
        per stream (a block must never serve two launches in flight)."""
        B, dev = self.batch, self.device
        self._layout, o = [], 0   # (field, dtype name, first byte, byte past its end) of a header row
        for name, dt in (("offs", "int64"),) + self._HDR:
            size = np.dtype(dt).itemsize * (B + (name == "offs"))
            self._layout.append((name, dt, o, o + size))
            o += size
        self._hdr_bytes = o
        self._hdr = torch.zeros((self._nbuf, (o + 15) // 16 * 16), dtype=torch.uint8, device=dev)
        self._hdr_host = torch.zeros(self._hdr.shape, dtype=torch.uint8, pin_memory=True)
        self._out = {k: torch.empty((self._nbuf, B * self.cap * self._WIDTH.get(k, 1)), dtype=getattr(torch, dt),
                                    device=dev) for k, dt in self._COLS}
        self._scratch = [torch.empty(scratch_bytes, dtype=torch.uint8, device=dev) for _ in self.streams]

    def _split(self, row, n: int) -> dict:
        """``{"offs": [n + 1], field: [n], ...}``: views of a header row (device tensor or numpy array)."""
        ns = torch if isinstance(row, torch.Tensor) else np
        out = {}
        for name, dt, lo, hi in self._layout:
            v = row[lo:hi]
            out[name] = (v if dt == "uint8" else v.view(getattr(ns, dt)))[:n + (name == "offs")]
        return out

    def empty(self):
        """The frame object of no frames with this consumer's parameters (what a run without frames writes)."""
        hdr = {"offs": np.zeros(1, np.int64), **{k: np.zeros(0, dt) for k, dt in self._HDR}}
        return self._frames_of([], hdr, {k: np.zeros(0, dt) for k, dt in self._COLS})

    def _collect(self, fr):
        with self._lock:
            self._count(fr)
            self.results.append(fr)

    # ------------------------------------------------------------------ the two host steps of a GPU batch
    def _launched(self, b: int, n: int, st, meta):
        """Batch just launched on ``st`` (current stream): header -> pinned host, then advance the older batches."""
        self._hdr_host[b].copy_(self._hdr[b], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(st)
        self._pending.append({"b": b, "n": n, "st": st, "meta": meta, "hdr": ev, "data": None})
        self._advance(keep=1)

    def _advance(self, keep: int):
        """Step every batch but the newest ``keep``: a batch whose header is awaited gets its data copy
        issued; a batch whose data copy was issued is collected once at least one newer batch is behind
        it (or on a flush, keep = 0)."""
        for i, p in enumerate(list(self._pending)):
            if len(self._pending) - i <= keep:
                break
            if p["data"] is None:
                p["hdr"].synchronize()
                p["head"] = {k: v.copy() for k, v in self._split(self._hdr_host[p["b"]].numpy(), p["n"]).items()}
                total = int(p["head"]["offs"][p["n"]])
                p["cols"] = {k: torch.empty(total * self._WIDTH.get(k, 1), dtype=getattr(torch, dt),
                                            pin_memory=total > 0) for k, dt in self._COLS}
                ev = torch.cuda.Event()
                with torch.cuda.stream(p["st"]):   # exactly offs[n] rows, never the full capacity
                    if total:
                        for k, h in p["cols"].items():
                            h.copy_(self._out[k][p["b"], :h.numel()], non_blocking=True)
                    p["cols"].update(self._extra_copies(p["b"], p["n"], p["head"]))
                    ev.record(p["st"])
                p["data"] = ev
        while self._pending and self._pending[0]["data"] is not None and len(self._pending) > 2 * keep:
            p = self._pending.popleft()
            p["data"].synchronize()
            self._collect(self._frames_of(p["meta"], p["head"], {k: h.numpy().copy() for k, h in p["cols"].items()}))

    def take_results(self) -> list:
        """The finished batches collected so far (oldest first); they are removed from :attr:`results`."""
        with self._lock:
            out, self.results = self.results, []
        return out

    def synchronize(self):
        """Wait for every batch and collect it.  Returns the list of finished batches not taken yet."""
        if self.gpu:
            self._advance(keep=0)
            self._advance(keep=0)   # first pass issues the last data copies, second collects them
            self.sync_streams()
        return self.results

    # ------------------------------------------------------------------ what a packed-rows consumer fills in
    def _frames_of(self, meta, hdr: dict, cols: dict):
        """The frame object of a batch: its meta tuples, header fields and data columns (host arrays by name)."""
        raise NotImplementedError

    def _count(self, fr):
        """Add a finished batch to the counters behind :meth:`metrics` (the lock is held)."""

    def _extra_copies(self, b: int, n: int, head: dict) -> dict:
        """Data step of buffer row b (the batch's stream is current, its header ``head`` is on the host): issue
        the copies of what the columns do not hold and return the pinned host tensors by name; they reach
        :meth:`_frames_of` with the columns."""
        return {}


class SparseFrameConsumer(_PackedRows):
    """Consumer engine: batches of leased slots -> K-10 zero suppression (csrc/sparse.hip) ->
    stream-ordered release.

    Per frame: the (pixel index, value) pairs with ``thr <= v <= vmax`` (and ``mask != 0``), packed in
    index order; at most ``cap`` per frame (a frame with more stores nothing and is flagged).  With
    ``min_peaks > 0`` the hit filter (:class:`_HitFilter`) decides on the device which frames are
    looked at.  The batches reach :attr:`results` as :class:`psana_ray_amd.sparse.SparseFrames` the
    way :class:`_PackedRows` states."""

    name = "sparse"
    _HDR = (("nnz", "int32"), ("flags", "uint8"))
    _COLS = (("pix", "int32"), ("val", "float32"))

    def __init__(self, endpoint: QueueEndpoint, frame_shape, thr: Optional[float] = None, vmax: Optional[float] = None,
                 cap: Optional[int] = None, mask=None, min_peaks: int = 0, peak_params: Optional[PeakFinderParams] = None,
                 detector: str = "", layout: str = "calib", batch: Optional[int] = None,
                 stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame.  check_ring=False: the ring holds RAW
        frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from . import sparse as _sparse
        from .ops.reference import validate_sparse_params

        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.shape = tuple(int(s) for s in frame_shape)
        self.n = int(np.prod(self.shape))
        if not 1 <= self.n < 2 ** 31:
            raise ValueError("sparse: frames must have 1 .. 2^31 - 1 elements")
        self.thr, self.vmax, self.cap = validate_sparse_params(
            _sparse.DEFAULT_THR if thr is None else thr, _sparse.DEFAULT_VMAX if vmax is None else vmax,
            _sparse.default_cap(self.n) if cap is None else cap, self.batch, "sparse")
        self._hits = _HitFilter("sparse", self.shape, min_peaks, peak_params)
        self.min_peaks, self.peak_params = self._hits.min_peaks, self._hits.params
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "zero suppression needs calibrated float32 ones")
        self._mask_np = None
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype != np.uint8 or m.size != self.n or (m.ndim > 1 and tuple(m.shape) != self.shape):
                raise ValueError(f"sparse: the mask must be uint8 of the frame's shape {self.shape}, got {m.dtype} "
                                 f"{tuple(m.shape)}")
            self._mask_np = np.ascontiguousarray(m.reshape(-1))
        self.frames_stored = self.frames_skipped = self.frames_overflowed = self.pixels_stored = 0
        if self.gpu:
            self._build_rows(kernels.sparsify_scratch_bytes(self.n, self.cap, self.batch))
            self._mask = None if self._mask_np is None else torch.from_numpy(self._mask_np).to(self.device)
            self._hits.allocate(self.device, self.batch, self._nbuf, len(self.streams))

    def _frames_of(self, meta, hdr, cols):
        from .sparse import SparseFrames

        return SparseFrames(self.detector, self.layout, self.shape, self.thr, self.vmax, self.cap, self.min_peaks,
                            self._hits.peak_dict(), **self._meta_columns(meta), **hdr, **cols)

    def _count(self, sf):
        from .sparse import FLAG_OVERFLOW, FLAG_SKIPPED

        self.frames_skipped += int(((sf.flags & FLAG_SKIPPED) != 0).sum())
        self.frames_overflowed += int(((sf.flags & FLAG_OVERFLOW) != 0).sum())
        self.frames_stored += int(((sf.flags & (FLAG_SKIPPED | FLAG_OVERFLOW)) == 0).sum())
        self.pixels_stored += int(sf.offs[-1])

    def _launch_slots(self, C, slots, b, k, st):
        h, o = self._split(self._hdr[b], len(slots)), self._out
        keys = self._hits.keys_slots(C, self.ep, slots, b, k, st)
        C.sparsify_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, self.thr, self.vmax, self.cap,
                         0 if self._mask is None else int(self._mask.data_ptr()), keys, self.min_peaks,
                         int(h["nnz"].data_ptr()), int(h["flags"].data_ptr()), int(h["offs"].data_ptr()),
                         int(o["pix"][b].data_ptr()), int(o["val"][b].data_ptr()),
                         int(self._scratch[k].data_ptr()), self._scratch[k].numel(), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        h, o = self._split(self._hdr[b], len(frames)), self._out
        keys = self._hits.keys_tensors(frames, b, k, st)
        kernels.sparsify([t.reshape(-1) for t in frames], self.thr, self.vmax, self.cap, h["nnz"], h["flags"],
                         h["offs"], o["pix"][b], o["val"][b], mask=self._mask, keys=keys, key_min=self.min_peaks,
                         scratch=self._scratch[k], stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        nnz, flags, offs, pix, val = reference.sparsify_reference(x, self.thr, self.vmax, self.cap, mask=self._mask_np,
                                                                  keys=self._hits.keys_reference(x),
                                                                  key_min=self.min_peaks)
        self._collect(self._frames_of(meta, {"offs": offs.numpy(), "nnz": nnz.numpy(), "flags": flags.numpy()},
                                      {"pix": pix.numpy(), "val": val.numpy()}))

    def metrics(self) -> dict:
        return {"frames_consumed": self.frames, "frames_stored": self.frames_stored,
                "frames_skipped": self.frames_skipped, "frames_overflowed": self.frames_overflowed,
                "pixels_stored": self.pixels_stored}


class PowderConsumer(_RunAccumulator):
    """Consumer engine: batches of leased slots -> K-11 powder statistics (csrc/powder.hip) ->
    stream-ordered release.

    Per run: per-pixel, per-class count / sum / sum of squares / maximum / count above ``thr_above`` of
    the quantised calibrated value inside ``[vmin, vmax]`` -- integers, so the result is exact in any
    frame order.  With ``min_peaks > 0`` the hit filter (:class:`_HitFilter`) decides on the device
    whether a frame is a hit (class 1) or a miss (class 0); with ``min_peaks == 0`` there is one class.
    One accumulator set per consumer stream (:class:`_RunAccumulator`): :meth:`synchronize` returns the
    dict of ``frames`` int64 [NC], ``cnt`` / ``sum`` / ``sq`` / ``above`` int64 [NC, n] and ``qmax``
    int32 [NC, n] (the sets' maximum)."""

    name = "powder"
    bound_text = "max_frames = {} (the int32 count and the int64 sum of squares)"

    def __init__(self, endpoint: QueueEndpoint, frame_shape, vmin: Optional[float] = None, vmax: Optional[float] = None,
                 frac_bits: Optional[int] = None, thr_above: Optional[float] = None, min_peaks: int = 0,
                 peak_params: Optional[PeakFinderParams] = None, detector: str = "", layout: str = "calib",
                 batch: Optional[int] = None, stream_kind: str = CONSUMER_STREAM_KIND,
                 streams: int = CONSUMER_STREAMS, ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame.  check_ring=False: the ring holds RAW
        frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from .ops import reference as _ref

        self.shape = tuple(int(s) for s in frame_shape)
        self.n = int(np.prod(self.shape))
        if not 1 <= self.n < 2 ** 31:
            raise ValueError("powder: frames must have 1 .. 2^31 - 1 elements")
        self.vmin, self.vmax, self.frac_bits, self.thr_above, _Q, self.max_frames = _ref.validate_powder_params(
            _ref.POWDER_VMIN if vmin is None else vmin, _ref.POWDER_VMAX if vmax is None else vmax,
            _ref.POWDER_FRAC_BITS if frac_bits is None else frac_bits,
            _ref.POWDER_THR_ABOVE if thr_above is None else thr_above, "powder")
        self._hits = _HitFilter("powder", self.shape, min_peaks, peak_params)
        self.min_peaks, self.peak_params = self._hits.min_peaks, self._hits.params
        self.nc = 2 if self.min_peaks > 0 else 1
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "powder statistics need calibrated float32 ones")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        if self.gpu:
            self._hits.allocate(self.device, self.batch, self._nbuf, len(self.streams))

    def _fields(self):
        from .ops.reference import POWDER_QMAX_NONE

        c, s = (self.nc,), (self.nc, self.n)
        return (_Field("frames", c, torch.int64, np.int64), _Field("cnt", s, torch.int32, np.int64),
                _Field("sum", s, torch.int64, np.int64), _Field("sq", s, torch.int64, np.int64),
                _Field("qmax", s, torch.int32, np.int32, POWDER_QMAX_NONE, "max"),
                _Field("above", s, torch.int32, np.int64))

    def _launch_slots(self, C, slots, b, k, st):
        nfr, cnt, s, q, qmax, above = self._acc[k]
        keys = self._hits.keys_slots(C, self.ep, slots, b, k, st)
        C.powder_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, self.vmin, self.vmax, self.frac_bits,
                       self.thr_above, self.nc, keys, self.min_peaks, int(nfr.data_ptr()), int(cnt.data_ptr()),
                       int(s.data_ptr()), int(q.data_ptr()), int(qmax.data_ptr()), int(above.data_ptr()),
                       int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        nfr, cnt, s, q, qmax, above = self._acc[k]
        keys = self._hits.keys_tensors(frames, b, k, st)
        kernels.powder_accumulate([t.reshape(-1) for t in frames], self.vmin, self.vmax, self.frac_bits,
                                  self.thr_above, nfr, cnt, s, q, qmax, above, keys=keys, key_min=self.min_peaks,
                                  frames_so_far=self.frames, stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        self._add(reference.powder_accumulate_reference(x, self.vmin, self.vmax, self.frac_bits, self.thr_above,
                                                        keys=self._hits.keys_reference(x), key_min=self.min_peaks))

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.powder.PowderStats`."""
        from .powder import PowderStats

        h = self.synchronize()
        return PowderStats(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits,
                           self.thr_above, self.min_peaks, self._hits.peak_dict(), h["frames"].copy(), h["cnt"].copy(),
                           h["sum"].copy(), h["sq"].copy(), h["above"].copy(), h["qmax"].copy())


class PixelHistConsumer(_RunAccumulator):
    """Consumer engine: batches of leased slots -> K-12 per-pixel histograms (csrc/pixhist.hip) ->
    stream-ordered release.

    Per run: how often every pixel read a value in each of ``nbins`` equal bins of ``[lo, hi]`` -- integers,
    so the result is exact in any frame order.  One accumulator int32 ``[n, nbins]`` per consumer stream
    (:class:`_RunAccumulator`): :meth:`synchronize` returns their sum, ``hist`` int32 [n, nbins]."""

    name = "hist"
    bound_text = "{} (the int32 count of a bin)"

    def __init__(self, endpoint: QueueEndpoint, frame_shape, lo: Optional[float] = None, hi: Optional[float] = None,
                 nbins: Optional[int] = None, detector: str = "", layout: str = "calib", batch: Optional[int] = None,
                 stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame.  check_ring=False: the ring holds RAW
        frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from .ops import reference as _ref

        self.shape = tuple(int(s) for s in frame_shape)
        self.n = int(np.prod(self.shape))
        self.lo, self.hi, self.nbins, self.inv_w = _ref.validate_pixel_hist_params(
            _ref.HIST_LO if lo is None else lo, _ref.HIST_HI if hi is None else hi,
            _ref.HIST_BINS if nbins is None else nbins, n=self.n, what="hist")
        self.max_frames = _ref.HIST_MAX_FRAMES
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "pixel histograms need calibrated float32 ones")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.acc_bytes = self.n * self.nbins * 4 * max(1, len(self.streams))
        log.info("hist: %d accumulator(s) of %d x %d int32 = %.1f MB in all", max(1, len(self.streams)), self.n,
                 self.nbins, self.acc_bytes / 1e6)

    def _fields(self):
        return (_Field("hist", (self.n, self.nbins), torch.int32, np.int32),)

    def _launch_slots(self, C, slots, b, k, st):
        C.pixel_hist_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, self.lo, self.hi, self.inv_w, self.nbins,
                           int(self._acc[k].data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        kernels.pixel_hist([t.reshape(-1) for t in frames], self.lo, self.hi, self.nbins, self._acc[k],
                           frames_so_far=self.frames, stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        self._add((reference.pixel_hist_reference(x, self.lo, self.hi, self.nbins),))

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.hist.PixelHist`."""
        from .hist import PixelHist

        return PixelHist(self.detector, self.layout, self.shape, self.lo, self.hi, self.nbins, self.frames,
                         self.synchronize().copy())


class PhotonConsumer(_RunAccumulator):
    """Consumer engine: batches of leased slots -> K-13 photon counting (csrc/photons.hip) ->
    stream-ordered release.

    Per run: per pixel the samples (``cnt``), the photons (``psum``) and the frames with at least one photon
    (``occ``); per frame and ROI the photon-count distribution ``pk`` [R, 8] and the photons ``tot`` [R] --
    integers, so the result is exact in any frame order.  The frames never leave the GPU: the per-frame rows
    (a few hundred bytes) go to pinned host memory stream-ordered.  One set of run maps per consumer stream
    (:class:`_RunAccumulator`): :meth:`synchronize` returns the dict of ``cnt`` int32 / ``psum`` int64 /
    ``occ`` int32 [n]."""

    name = "photons"
    wants_meta = True
    meta_fields = 4
    bound_text = "{} (the int32 counts of a pixel)"

    def __init__(self, endpoint: QueueEndpoint, frame_shape, adu_per_photon, vmax: Optional[float] = None,
                 thr_seed: Optional[float] = None, thr_total: Optional[float] = None, mask=None, roi=None,
                 n_roi: Optional[int] = None, detector: str = "", layout: str = "calib", batch: Optional[int] = None,
                 stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame, [P, H, W] or [H, W].  mask / roi: uint8 arrays of
        that many elements (keep-mask; ROI labels 0 .. R - 1, 255 = none), or None.  check_ring=False: the
        ring holds RAW frames that the caller calibrates before :meth:`process_frames`
        (``--calibrate_on_read``)."""
        from .ops import reference as _ref

        self.shape = tuple(int(s) for s in frame_shape)
        self.phw = _ref.photon_shape(self.shape, "photons")
        self.n = int(np.prod(self.phw))
        self.params = _ref.validate_photon_params(adu_per_photon, vmax, thr_seed, thr_total, what="photons")
        self._mask_np, self._roi_np, self.n_roi = _ref.validate_photon_maps(self.phw, mask, roi, n_roi, "photons")
        self.max_frames = _ref.PHOTON_MAX_FRAMES
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "photon counting needs calibrated float32 ones")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        # per batch: (pk int32 [n, R, 8], tot int64 [n, R], [(rank, idx, gevt, photon_energy), ...]); on the GPU
        # path the arrays are pinned host tensors filled asynchronously: valid after sync_streams()
        self.results = []
        if self.gpu:
            dev, n, B, R = self.device, self.n, self.batch, self.n_roi
            self._pk = torch.zeros((self._nbuf, B, R, _ref.PHOTON_PK_BINS), dtype=torch.int32, device=dev)
            self._tot = torch.zeros((self._nbuf, B, R), dtype=torch.int64, device=dev)
            self._mask = None if self._mask_np is None else torch.from_numpy(self._mask_np).to(dev)
            self._roi = None if self._roi_np is None else torch.from_numpy(self._roi_np).to(dev)
            if self._roi is not None:
                self._roi._pr_checked_roi = (n, R)   # validated on the host above

    def _fields(self):
        s = (self.n,)
        return (_Field("cnt", s, torch.int32, np.int32), _Field("psum", s, torch.int64, np.int64),
                _Field("occ", s, torch.int32, np.int32))

    def _launch_slots(self, C, slots, b, k, st):
        P, H, W = self.phw
        pp = self.params
        cnt, psum, occ = self._acc[k]
        C.photons_slots(self.ep.pool, self.ep._slot_bytes, slots, P, H, W, pp.inv, pp.vmax, pp.thr_seed, pp.thr_total,
                        0 if self._mask is None else int(self._mask.data_ptr()),
                        0 if self._roi is None else int(self._roi.data_ptr()), self.n_roi, int(cnt.data_ptr()),
                        int(psum.data_ptr()), int(occ.data_ptr()), int(self._pk[b].data_ptr()),
                        int(self._tot[b].data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        n = len(frames)
        cnt, psum, occ = self._acc[k]
        kernels.photons([t.reshape(-1) for t in frames], self.phw, self.params, cnt, psum, occ, self._pk[b, :n],
                        self._tot[b, :n], mask=self._mask, roi=self._roi, n_roi=self.n_roi,
                        frames_so_far=self.frames, stream=st)

    def _launched(self, b, n, st, meta):
        self._keep_pinned((self._pk, self._tot), b, n, meta)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        out = reference.photon_count_reference(x, self.phw, self.params, self._mask_np, self._roi_np, self.n_roi)
        self._add((out.cnt, out.psum, out.occ))
        self.results.append((out.pk, out.tot, list(meta)))

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.photons.PhotonStats`."""
        from .photons import PhotonStats

        h = self.synchronize()
        R = self.n_roi
        return PhotonStats.from_maps(self.detector, self.layout, self.shape, self.params, self._mask_np, self._roi_np,
                                     R, self.frames, h["cnt"].copy(), h["psum"].copy(), h["occ"].copy(),
                                     **self._meta_columns([m for *_, ms in self.results for m in ms]),
                                     pk=self._cat([r[0] for r in self.results], np.zeros((0, R, 8), np.int32)),
                                     tot=self._cat([r[1] for r in self.results], np.zeros((0, R), np.int64)))


class RoiConsumer(_BatchConsumer):
    """Consumer engine: batches of leased slots -> K-16 ROI statistics (csrc/roi.hip) -> stream-ordered release.

    Per frame and rectangle: the pixels inside the value window, their sum, first moments, maximum with its
    position and, when selected, the projections onto x and y -- integers, equal to the golden model word for
    word.  Only the rectangles are read.  The frames never leave the GPU: the per-frame rows (64 bytes per
    rectangle plus the projections) go to pinned host memory stream-ordered.  There is no run accumulator, so
    the streams share nothing and a run has no frame bound."""

    name = "roi"
    wants_meta = True
    meta_fields = 4

    def __init__(self, endpoint: QueueEndpoint, frame_shape, rects, vmin: Optional[float] = None,
                 vmax: Optional[float] = None, frac_bits: Optional[int] = None, proj: str = "none", mask=None,
                 detector: str = "", layout: str = "calib", batch: Optional[int] = None,
                 stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame, [P, H, W] or [H, W].  rects: a
        :class:`psana_ray_amd.roi.RoiSet`, or int rows (p, y0, y1, x0, x1) -- (y0, y1, x0, x1) for 2-D frames.
        mask: a uint8 array of a frame's elements (non-zero = keep), or None.  check_ring=False: the ring
        holds RAW frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from .ops import reference as _ref
        from .roi import RoiSet, mask_sha256

        self.shape = tuple(int(s) for s in frame_shape)
        self.phw = _ref.photon_shape(self.shape, "roi")
        self.n = int(np.prod(self.phw))
        self.roiset = rects if isinstance(rects, RoiSet) else RoiSet(rects, self.shape)
        if self.roiset.phw != self.phw:
            raise ValueError(f"roi: rectangles for frames of {self.roiset.frame_shape}, these are {self.shape}")
        self.rects = self.roiset.rects
        self.n_roi = self.roiset.R
        self.vmin, self.vmax, self.frac_bits, _Q = _ref.validate_roi_params(
            _ref.ROI_VMIN if vmin is None else vmin, _ref.ROI_VMAX if vmax is None else vmax,
            _ref.ROI_FRAC_BITS if frac_bits is None else frac_bits, self.rects, "roi")
        self.proj = "none" if proj is None else proj
        self._want_x, self._want_y = _ref.validate_roi_proj(self.proj, "roi")
        self._mask_np, _roi, _R = _ref.validate_photon_maps(self.phw, mask, None, None, "roi")
        self.mask_sha256 = mask_sha256(self.phw, self._mask_np)
        self.Lx = int(self.roiset.offx[-1]) if self._want_x else 0
        self.Ly = int(self.roiset.offy[-1]) if self._want_y else 0
        self.row_bytes = self.roiset.row_bytes(self.proj)
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "ROI statistics need calibrated float32 ones")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        # per batch: (rows int64 [n, R, 8], proj_x int64 [n, Lx], proj_y int64 [n, Ly], [(rank, idx, gevt,
        # photon_energy), ...]); on the GPU path the arrays are pinned host tensors filled asynchronously: valid
        # after sync_streams()
        self.results = []
        if self.gpu:
            dev, B, R = self.device, self.batch, self.n_roi
            self._rows = torch.zeros((self._nbuf, B, R, _ref.ROI_ROW_WORDS), dtype=torch.int64, device=dev)
            self._px = torch.zeros((self._nbuf, B, self.Lx), dtype=torch.int64, device=dev) if self._want_x else None
            self._py = torch.zeros((self._nbuf, B, self.Ly), dtype=torch.int64, device=dev) if self._want_y else None
            self._mask = None if self._mask_np is None else torch.from_numpy(self._mask_np).to(dev)
            self._plan = kernels.roi_plan(self.phw, self.rects, dev)

    def _launch_slots(self, C, slots, b, k, st):
        C.roi_slots(self.ep.pool, self.ep._slot_bytes, slots, self._plan, self.vmin, self.vmax, self.frac_bits,
                    0 if self._mask is None else int(self._mask.data_ptr()), int(self._rows[b].data_ptr()),
                    0 if self._px is None else int(self._px[b].data_ptr()),
                    0 if self._py is None else int(self._py[b].data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        n = len(frames)
        kernels.roi_stats([t.reshape(-1) for t in frames], self.phw, self.rects, self.vmin, self.vmax, self.frac_bits,
                          self._rows[b, :n], None if self._px is None else self._px[b, :n],
                          None if self._py is None else self._py[b, :n], mask=self._mask, stream=st)

    def _launched(self, b, n, st, meta):
        self._keep_pinned((self._rows, self._px, self._py), b, n, meta)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        rows, px, py = reference.roi_stats_reference(x, self.phw, self.rects, self.vmin, self.vmax, self.frac_bits,
                                                     self._mask_np, self.proj)
        self.results.append((rows, px if self._want_x else None, py if self._want_y else None, list(meta)))

    def synchronize(self) -> int:
        """Wait for every batch; returns the frames processed."""
        if self.gpu:
            self.sync_streams()
        return self.frames

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.roi.RoiFrames`, rows in processing order."""
        from .ops.reference import ROI_ROW_WORDS
        from .roi import RoiFrames

        self.synchronize()
        rows = self._cat([r[0] for r in self.results], np.zeros((0, self.n_roi, ROI_ROW_WORDS), np.int64))
        # None: nothing kept (an axis not selected, or no batch yet) -> RoiFrames makes it empty
        px, py = self._cat([r[1] for r in self.results]), self._cat([r[2] for r in self.results])
        return RoiFrames.from_rows(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits,
                                   self.proj, self.rects, self.mask_sha256, rows, px, py,
                                   **self._meta_columns([m for *_, ms in self.results for m in ms]))


class DropletConsumer(_PackedRows):
    """Consumer engine: batches of leased slots -> K-14 droplets (csrc/droplets.hip) -> stream-ordered release.

    Per frame: the 4-connected clusters of pixels with ``thr_low <= v <= vmax`` (and ``mask != 0``) that hold a
    pixel ``v >= thr_seed``, each as integers (label, npix, adu, sy, sx, qmax), label ascending; at most
    ``pix_cap`` active pixels and ``cap`` droplets per frame (a frame with more stores nothing and is flagged).
    The batches reach :attr:`results` as :class:`psana_ray_amd.droplets.DropletFrames` the way
    :class:`_PackedRows` states.  Only the first launch of a batch (K-10's scan) reads frame values, so the
    ring slots go back stream-ordered right after the native call.  A batch that would not fit the free HBM
    share is lowered, not refused."""

    name = "droplets"
    _HDR = (("nact", "int32"), ("ndrop", "int32"), ("flags", "uint8"))
    _COLS = (("label", "int32"), ("npix", "int32"), ("adu", "int64"), ("sy", "int64"), ("sx", "int64"),
             ("qmax", "int32"))

    def __init__(self, endpoint: QueueEndpoint, frame_shape, thr_low, thr_seed: Optional[float] = None,
                 vmax: Optional[float] = None, frac_bits: Optional[int] = None, pix_cap: Optional[int] = None,
                 cap: Optional[int] = None, mask=None, detector: str = "", layout: str = "calib",
                 batch: Optional[int] = None, stream_kind: str = CONSUMER_STREAM_KIND, streams: int = CONSUMER_STREAMS,
                 ranks_per_gpu: Optional[int] = None, check_ring: bool = True, hbm_budget: Optional[int] = None):
        """frame_shape: the shape of a (calibrated) frame, [P, H, W] or [H, W].  mask: uint8 keep-mask of that many
        elements, or None.  check_ring=False: the ring holds RAW frames that the caller calibrates before
        :meth:`process_frames` (``--calibrate_on_read``).  hbm_budget: bytes this consumer's scratch blocks and
        outputs may take (None: half of the free device memory divided by the ranks sharing the GPU)."""
        from . import droplets as _dr
        from .ops import reference as _ref

        self.shape = tuple(int(s) for s in frame_shape)
        self.phw = _ref.photon_shape(self.shape, "droplets")
        self.n = int(np.prod(self.phw))
        self.params = _ref.validate_droplet_params(thr_low, thr_seed, vmax, frac_bits, what="droplets")
        self._mask_np = _ref.droplet_mask(self.phw, mask, "droplets")
        self.mask_sha256 = _dr.mask_hash(self.phw, self._mask_np)
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "droplets need calibrated float32 ones")
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.pix_cap, self.cap = _ref.validate_droplet_caps(self.phw, self.params, pix_cap, cap, self.batch, "droplets")
        self.frames_stored = self.frames_overflowed = self.droplets_stored = 0
        self.scratch_bytes = 0
        if self.gpu:
            dev, ns = self.device, len(self.streams)
            if hbm_budget is None:
                if ranks_per_gpu is None:
                    from .parallel.launch import ranks_per_gpu as _rpg

                    ranks_per_gpu = _rpg()
                hbm_budget = torch.cuda.mem_get_info(dev)[0] // 2 // max(1, int(ranks_per_gpu))

            def need(B):   # scratch per stream + the output rows
                return ns * kernels.droplets_scratch_bytes(self.n, self.pix_cap, self.cap, B) \
                    + self._nbuf * B * self.cap * 36

            asked = self.batch
            while self.batch > 1 and need(self.batch) > hbm_budget:
                self.batch = (self.batch + 1) // 2
            if self.batch != asked:
                log.warning("droplets: a batch of %d frames needs %.1f MB, the HBM share is %.1f MB: batch lowered to %d",
                            asked, need(asked) / 1e6, hbm_budget / 1e6, self.batch)
            B = self.batch
            self.scratch_bytes = kernels.droplets_scratch_bytes(self.n, self.pix_cap, self.cap, B)
            log.info("droplets: %d scratch block(s) of %.1f MB (52 B per row of %d x %d active pixels), outputs %.1f MB",
                     ns, self.scratch_bytes / 1e6, B, self.pix_cap, self._nbuf * B * self.cap * 36 / 1e6)
            self._build_rows(self.scratch_bytes)
            self._mask = None if self._mask_np is None else torch.from_numpy(self._mask_np).to(dev)

    def _frames_of(self, meta, hdr, cols):
        from .droplets import DropletFrames

        return DropletFrames(self.detector, self.layout, self.phw, self.params.thr_low, self.params.thr_seed,
                             self.params.vmax, self.params.frac_bits, self.pix_cap, self.cap, self.mask_sha256,
                             **self._meta_columns(meta), **hdr, **cols)

    def _count(self, df):
        over = int((df.flags != 0).sum())
        self.frames_overflowed += over
        self.frames_stored += len(df) - over
        self.droplets_stored += int(df.offs[-1])

    def _launch_slots(self, C, slots, b, k, st):
        offs, nact, ndrop, flags = self._split(self._hdr[b], len(slots)).values()
        P, H, W = self.phw
        pp = self.params
        o = self._out
        C.droplets_slots(self.ep.pool, self.ep._slot_bytes, slots, P, H, W, pp.thr_low, pp.thr_seed, pp.vmax, pp.frac_bits,
                         self.pix_cap, self.cap, 0 if self._mask is None else int(self._mask.data_ptr()),
                         int(nact.data_ptr()), int(ndrop.data_ptr()), int(flags.data_ptr()), int(offs.data_ptr()),
                         int(o["label"][b].data_ptr()), int(o["npix"][b].data_ptr()), int(o["adu"][b].data_ptr()),
                         int(o["sy"][b].data_ptr()), int(o["sx"][b].data_ptr()), int(o["qmax"][b].data_ptr()),
                         int(self._scratch[k].data_ptr()), self._scratch[k].numel(), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        offs, nact, ndrop, flags = self._split(self._hdr[b], len(frames)).values()
        o = self._out
        kernels.droplets([t.reshape(-1) for t in frames], self.phw, self.params, self.pix_cap, self.cap, nact, ndrop, flags,
                         offs, o["label"][b], o["npix"][b], o["adu"][b], o["sy"][b], o["sx"][b], o["qmax"][b],
                         mask=self._mask, scratch=self._scratch[k], stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        x = torch.stack([t.reshape(-1) for t in frames])
        r = reference.droplet_reference(x, self.phw, self.params, self._mask_np, self.pix_cap, self.cap)
        self._collect(self._frames_of(meta, {k: getattr(r, k).numpy() for k in ("offs", "nact", "ndrop", "flags")},
                                      {k: getattr(r, k).numpy() for k, _ in self._COLS}))

    def metrics(self) -> dict:
        return {"frames_consumed": self.frames, "frames_stored": self.frames_stored,
                "frames_overflowed": self.frames_overflowed, "droplets_stored": self.droplets_stored}


class CubeConsumer(_RunAccumulator):
    """Consumer engine: batches of leased slots -> K-15 cube (csrc/cube.hip) -> stream-ordered release.

    Per run and BIN of a per-event scalar (``binning``: :class:`psana_ray_amd.cube.CubeBinning`, from the
    photon energy or from the global event number): per-pixel count / sum / sum of squares of the quantised
    calibrated value inside ``[vmin, vmax]`` -- integers, so the result is exact in any frame order.  A
    frame's bin is computed on the HOST from its slot header before the launch; a frame without a bin is
    dropped (not read).  One accumulator set per consumer stream (:class:`_RunAccumulator`):
    :meth:`synchronize` returns the dict of ``frames`` int64 [B], ``cnt`` int32 / ``sum`` int64 / ``sq``
    int64 [B, n].  When the sets of all streams do not fit ``acc_budget`` bytes (default: half of the free
    HBM) the consumer runs on one stream."""

    name = "cube"
    wants_meta = True
    meta_fields = 4
    bound_text = "max_frames = {} (the int32 count and the int64 sum of squares)"

    def __init__(self, endpoint: QueueEndpoint, frame_shape, binning, vmin: Optional[float] = None,
                 vmax: Optional[float] = None, frac_bits: Optional[int] = None, detector: str = "",
                 layout: str = "calib", batch: Optional[int] = None, stream_kind: str = CONSUMER_STREAM_KIND,
                 streams: int = CONSUMER_STREAMS, ranks_per_gpu: Optional[int] = None, check_ring: bool = True,
                 acc_budget: Optional[int] = None):
        """frame_shape: the shape of a (calibrated) frame.  check_ring=False: the ring holds RAW
        frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from . import cube as _cube
        from .ops import reference as _ref

        self.shape = tuple(int(s) for s in frame_shape)
        self.n = int(np.prod(self.shape))
        if not 1 <= self.n < 2 ** 31:
            raise ValueError("cube: frames must have 1 .. 2^31 - 1 elements")
        self.vmin, self.vmax, self.frac_bits, _thr, _Q, self.max_frames = _ref.validate_powder_params(
            _ref.POWDER_VMIN if vmin is None else vmin, _ref.POWDER_VMAX if vmax is None else vmax,
            _ref.POWDER_FRAC_BITS if frac_bits is None else frac_bits, 0.0, "cube")
        if not isinstance(binning, _cube.CubeBinning):
            raise ValueError("cube: binning must be a psana_ray_amd.cube.CubeBinning")
        self.binning = binning
        self.nbins = binning.nbins
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "the cube needs calibrated float32 ones")
        self.set_bytes = _cube.accumulator_set_bytes(self.nbins, self.n)
        dev = endpoint.ring.device
        if dev.type == "cuda":
            if acc_budget is None:
                acc_budget = torch.cuda.mem_get_info(dev)[0] // 2   # half of the free HBM
            fit = _cube.accumulator_sets_that_fit(self.set_bytes, streams, acc_budget)   # ValueError: not even one
            if fit < int(streams):
                log.info("cube: %d accumulator sets of %d bytes do not fit %d bytes: running on one stream",
                         int(streams), self.set_bytes, acc_budget)
            streams = fit
        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        log.info("cube: %d bins x %d pixels x 20 B = %d bytes per accumulator set, %d set(s), max_frames=%d",
                 self.nbins, self.n, self.set_bytes, max(1, len(self.streams)), self.max_frames)
        self.dropped = 0
        self.rows = []            # per batch: ([(rank, idx, gevt, photon_energy), ...], bins int32 [n])
        self._bins = None         # the bins of the batch being launched
        self._pending = None      # the meta of the batch process_frames hands to _launch_tensors

    def _fields(self):
        b, s = (self.nbins,), (self.nbins, self.n)
        return (_Field("frames", b, torch.int64, np.int64), _Field("cnt", s, torch.int32, np.int32),
                _Field("sum", s, torch.int64, np.int64), _Field("sq", s, torch.int64, np.int64))

    def process_frames(self, frames, meta):
        self._pending = self._pad_meta(meta)   # _launch_tensors bins the batch from it
        return super().process_frames(frames, self._pending)

    def _launch_slots(self, C, slots, b, k, st):
        # the bins come from the slot headers (a host read), before the native call
        self._bins = self.binning.bin_of_meta(self._meta_of(self.ep.pool.headers(slots)))
        nfr, cnt, s, q = self._acc[k]
        C.cube_slots(self.ep.pool, self.ep._slot_bytes, slots, self.n, self.vmin, self.vmax, self.frac_bits,
                     self.nbins, self._bins.tolist(), int(nfr.data_ptr()), int(cnt.data_ptr()), int(s.data_ptr()),
                     int(q.data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        self._bins = self.binning.bin_of_meta(self._pending)
        nfr, cnt, s, q = self._acc[k]
        kernels.cube_accumulate([t.reshape(-1) for t in frames], self._bins, self.nbins, self.vmin, self.vmax,
                                self.frac_bits, nfr, cnt, s, q, frames_so_far=self.frames, stream=st)

    def _keep_rows(self, meta, bins):
        self.dropped += int((bins < 0).sum())
        self.rows.append((list(meta), bins))

    def _launched(self, b, n, st, meta):
        self._keep_rows(meta, self._bins)

    def _reference(self, frames, meta):
        from .ops import reference

        bins = self.binning.bin_of_meta(meta)
        x = torch.stack([t.reshape(-1) for t in frames])
        self._add(reference.cube_accumulate_reference(x, bins, self.nbins, self.vmin, self.vmax, self.frac_bits))
        self._keep_rows(meta, bins)

    def stats(self):
        """The (synchronised) run as a :class:`psana_ray_amd.cube.CubeStats`."""
        from .cube import CubeStats

        h = self.synchronize()
        bins = self._cat([b for _, b in self.rows], np.zeros(0, np.int32))
        bg = self.binning
        return CubeStats(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, bg.by,
                         self.nbins, bg.edges, bg.table_sha256, h["frames"].copy(), self.dropped, h["cnt"].copy(),
                         h["sum"].copy(), h["sq"].copy(), **self._meta_columns([m for ms, _ in self.rows for m in ms]),
                         bin=bins.astype(np.int16))


class RoibinConsumer(_PackedRows):
    """Consumer engine: batches of leased slots -> K-07 peak finder -> K-17 roibin (csrc/roibin.hip) ->
    stream-ordered release.

    Per kept frame (``counts >= min_peaks``): one lossless (2R+1)^2 box per peak record, ordered by centre, and the
    frame binned ``bin`` x ``bin`` into int16 codes of ``step``.  The peak finder always runs (the boxes need its
    records); its counts gate the frames ON THE DEVICE.  The boxes travel as packed rows the way
    :class:`_PackedRows` states; the codes of the KEPT frames only follow in the same data step (a skipped frame's
    code rows are neither written nor copied).  The batches reach :attr:`results` as
    :class:`psana_ray_amd.roibin.RoibinFrames`."""

    name = "roibin"
    _HDR = (("npk", "int32"), ("nbox", "int32"), ("nbad", "int32"), ("nsat", "int32"), ("flags", "uint8"))
    _COLS = (("ctr", "int32"), ("rec", "float32"), ("box", "float32"))

    def __init__(self, endpoint: QueueEndpoint, frame_shape, bin: Optional[int] = None, step: Optional[float] = None,
                 vmin: Optional[float] = None, vmax: Optional[float] = None, radius: Optional[int] = None, mask=None,
                 min_peaks: int = 0, peak_params: Optional[PeakFinderParams] = None, detector: str = "",
                 layout: str = "calib", batch: Optional[int] = None, stream_kind: str = CONSUMER_STREAM_KIND,
                 streams: int = CONSUMER_STREAMS, ranks_per_gpu: Optional[int] = None, check_ring: bool = True):
        """frame_shape: the shape of a (calibrated) frame, [P, H, W] or [H, W].  check_ring=False: the ring holds
        RAW frames that the caller calibrates before :meth:`process_frames` (``--calibrate_on_read``)."""
        from . import roibin as _roibin
        from .ops import reference as R

        super().__init__(endpoint, batch, ranks_per_gpu, streams, stream_kind)
        self.shape = tuple(int(s) for s in frame_shape)
        self.shape3 = R.photon_shape(self.shape, "roibin")
        self.n = int(np.prod(self.shape3))
        self.peak_params = peak_params or PeakFinderParams()
        if self.peak_params.radius not in (1, 2):
            raise ValueError("roibin: peak finder radius must be 1 or 2")
        self.params = R.validate_roibin_params(
            R.ROIBIN_BIN if bin is None else bin, R.ROIBIN_STEP if step is None else step,
            R.ROIBIN_VMIN if vmin is None else vmin, R.ROIBIN_VMAX if vmax is None else vmax,
            R.ROIBIN_RADIUS if radius is None else radius, self.peak_params.max_peaks, min_peaks, "roibin")
        self.min_peaks = self.params.min_peaks
        self.cap = self.params.max_peaks
        self.code_shape = R.roibin_code_shape(self.shape3, self.params.bin)
        self.frame_bytes = R.roibin_frame_bytes(self.shape3, self.params)
        self._wn = 2 * self.params.radius + 1
        self._WIDTH.update(rec=8, box=self._wn * self._wn)
        self.detector, self.layout = str(detector), str(layout)
        if check_ring:
            self._check_ring(endpoint, "roibin needs calibrated float32 ones")
        self._mask_np = None
        if mask is not None:
            m = np.asarray(mask)
            if m.dtype != np.uint8 or m.size != self.n or (m.ndim > 1 and tuple(m.shape) != self.shape):
                raise ValueError(f"roibin: the mask must be uint8 of the frame's shape {self.shape}, got {m.dtype} "
                                 f"{tuple(m.shape)}")
            self._mask_np = np.ascontiguousarray(m.reshape(-1))
        self.mask_sha256 = _roibin.mask_sha256(self._mask_np)
        self.frames_kept = self.frames_skipped = self.frames_overflowed = self.boxes = self.saturated = 0
        if self.gpu:
            self._build_rows(0)
            self._codes = torch.empty((self._nbuf, self.batch, *self.code_shape), dtype=torch.int16, device=self.device)
            self._mask = None if self._mask_np is None else torch.from_numpy(self._mask_np).to(self.device)
            self._pf = _PeakBuffers(self.device, self.peak_params, self.shape3, self.batch, self._nbuf,
                                    len(self.streams))

    def peak_dict(self) -> dict:
        p = self.peak_params
        return {"thr_peak": float(p.thr_peak), "son_min": float(p.son_min), "radius": float(p.radius)}

    def _frames_of(self, meta, hdr, cols):
        from .roibin import FLAG_SKIPPED, RoibinFrames

        p = self.params
        kept = (np.asarray(hdr["flags"]) & FLAG_SKIPPED) == 0
        codes = cols.get("codes")
        return RoibinFrames(self.detector, self.layout, self.shape, p.bin, p.step, p.inv, p.vmin, p.vmax, p.radius,
                            p.max_peaks, p.min_peaks, self.peak_dict(), self.mask_sha256, **self._meta_columns(meta),
                            **hdr, ctr=cols["ctr"], rec=np.asarray(cols["rec"]).reshape(-1, 8),
                            box=np.asarray(cols["box"]).reshape(-1, self._wn, self._wn),
                            koffs=np.concatenate([[0], np.cumsum(kept)]).astype(np.int64),
                            codes=None if codes is None else np.asarray(codes).reshape(-1, *self.code_shape))

    def _count(self, rf):
        from .roibin import FLAG_OVERFLOW, FLAG_SKIPPED

        self.frames_skipped += int(((rf.flags & FLAG_SKIPPED) != 0).sum())
        self.frames_overflowed += int(((rf.flags & FLAG_OVERFLOW) != 0).sum())
        self.frames_kept += int(rf.koffs[-1])
        self.boxes += int(rf.offs[-1])
        self.saturated += int(rf.nsat.astype(np.int64).sum())

    def _extra_copies(self, b, n, head):
        """The code rows of the batch's KEPT frames, run by run: a skipped frame's codes never cross to the host."""
        kept = (head["flags"] & 2) == 0
        K = int(kept.sum())
        host = torch.empty((K, *self.code_shape), dtype=torch.int16, pin_memory=K > 0)
        edges = np.flatnonzero(np.diff(np.concatenate([[0], kept.astype(np.int8), [0]])))   # run starts and ends
        j = 0
        for a, e in zip(edges[::2].tolist(), edges[1::2].tolist()):
            host[j:j + e - a].copy_(self._codes[b, a:e], non_blocking=True)
            j += e - a
        return {"codes": host}

    def _launch_slots(self, C, slots, b, k, st):
        n = len(slots)
        h, o, p = self._split(self._hdr[b], n), self._out, self.params
        P, H, W = self.shape3
        self._pf.launch_slots(C, self.ep, slots, b, k, st)
        C.roibin_slots(self.ep.pool, self.ep._slot_bytes, slots, P, H, W, p.bin, p.inv, p.vmin, p.vmax, p.radius,
                       p.min_peaks, p.max_peaks, 0 if self._mask is None else int(self._mask.data_ptr()),
                       int(self._pf.peaks[b].data_ptr()), int(self._pf.counts[b].data_ptr()),
                       int(self._codes[b].data_ptr()), int(h["npk"].data_ptr()), int(h["nbox"].data_ptr()),
                       int(h["nbad"].data_ptr()), int(h["nsat"].data_ptr()), int(h["flags"].data_ptr()),
                       int(h["offs"].data_ptr()), int(o["ctr"][b].data_ptr()), int(o["rec"][b].data_ptr()),
                       int(o["box"][b].data_ptr()), int(st.cuda_stream))

    def _launch_tensors(self, frames, b, k, st):
        n = len(frames)
        h, o, p = self._split(self._hdr[b], n), self._out, self.params
        rows = n * p.max_peaks
        self._pf.launch_tensors([t.reshape(-1) for t in frames], b, k, st)
        kernels.roibin([t.reshape(-1) for t in frames], self.shape3, p, self._pf.peaks[b, :n], self._pf.counts[b, :n],
                       self._codes[b, :n], h["npk"], h["nbox"], h["nbad"], h["nsat"], h["flags"], h["offs"],
                       o["ctr"][b, :rows], o["rec"][b, :rows * 8].view(rows, 8),
                       o["box"][b, :rows * self._wn ** 2].view(rows, self._wn, self._wn), mask=self._mask, stream=st)

    def _reference(self, frames, meta):
        from .ops import reference

        p = self.params
        x = torch.stack([t.reshape(self.shape3) for t in frames]).to(torch.float32)
        found, _summary = reference.peakfind_reference(x, self.peak_params)
        peaks = torch.zeros((len(frames), p.max_peaks, 8), dtype=torch.float32)
        for f, rec in enumerate(found):
            peaks[f, :min(rec.shape[0], p.max_peaks)] = rec[:p.max_peaks]
        counts = torch.tensor([int(r.shape[0]) for r in found], dtype=torch.int32)
        g = reference.roibin_reference(x, self.shape3, peaks, counts, p, mask=self._mask_np)
        self._collect(self._frames_of(meta, {k: getattr(g, k).numpy() for k in ("offs", "npk", "nbox", "nbad", "nsat",
                                                                                "flags")},
                                      {"ctr": g.ctr.numpy(), "rec": g.rec.numpy(), "box": g.box.numpy(),
                                       "codes": g.codes.numpy()}))

    def metrics(self) -> dict:
        return {"frames_consumed": self.frames, "frames_kept": self.frames_kept, "frames_skipped": self.frames_skipped,
                "frames_overflowed": self.frames_overflowed, "boxes": self.boxes, "saturated": self.saturated}
