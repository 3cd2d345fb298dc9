"""Consumer client: ``DataReader`` (reference parity: psana_ray/data_reader.py:4-48).

Same surface as the reference -- ``DataReader(address, queue_name, ray_namespace)``,
``connect()``, ``read()``, ``close()``, context manager, ``DataReaderError`` -- with these
MI355X-native semantics:

* ``connect()`` joins the queue session at the rendezvous store (``address``; the reference's
  ``ray.init`` + ``ray.get_actor``, data_reader.py:11-24) -- at any time, before, during or after
  the producers -- gets this consumer's HBM ring shard and starts the fabric thread: every live
  producer writes frames straight into the shard (HIP IPC peer copies over xGMI; shared memory
  for host rings).
  Defaults come from ONE shared module, so they match the producer's (fixes Q-3).
* ``read()`` is non-blocking by default and returns None when nothing is ready (data_reader.py:35);
  items are the reference's ``[rank, idx, data, photon_energy]`` (4 fields, producer.py:101; the
  reference example's 3-field unpack is quirk Q-1), ``data`` a torch tensor on the consumer's
  device (``as_numpy=True`` for a host ndarray).  ``read(timeout=s)`` waits event-driven.
* end of stream is distinct from "empty" (fixes Q-2): once every producer finished and the shard
  is drained, ``read()`` raises :class:`EndOfStream` -- a ``DataReaderError`` subclass, so the
  reference's consumer loop (``except DataReaderError: break``) terminates cleanly -- and
  ``reader.done`` becomes True.
* a dead peer raises ``DataReaderError("Queue peer is dead.")`` (data_reader.py:36-37).
* ``close()`` releases only what this reader created (fixes Q-13).
* ``lease()`` / ``read_batch()`` give zero-copy access to HBM slots for GPU consumers (H-9);
  ``batches()`` yields contiguous ``[B, *frame]`` tensors for PyTorch steps (``batching.py``).

``queue_name`` / ``ray_namespace`` may also name an in-process :mod:`cpu queue
<psana_ray_amd.queue.cpu_queue>` created with ``create_queue`` (BASELINE config 1); it is used
when it exists in this process.
"""
from __future__ import annotations

import logging
from typing import List, Optional

import numpy as np
import torch

from .config import DEFAULT_PREFETCH, DEFAULT_QUEUE_NAME, DEFAULT_RAY_ADDRESS, DEFAULT_RAY_NAMESPACE
from .queue.endpoint import EndOfStream as _QueueEOS
from .queue.endpoint import FrameItem, QueuePeerError

log = logging.getLogger(__name__)


class DataReaderError(Exception):
    """Custom exception for DataReader errors (data_reader.py:46-48)."""


class EndOfStream(DataReaderError):
    """Every producer finished and this consumer's queue shard is drained."""


class DataReader:
    def __init__(self, address: str = DEFAULT_RAY_ADDRESS, queue_name: str = DEFAULT_QUEUE_NAME,
                 ray_namespace: str = DEFAULT_RAY_NAMESPACE, consumer_id: Optional[int] = None,
                 device: Optional[str] = None, as_numpy: bool = False, timeout_s: float = 300.0,
                 slots: Optional[int] = None, prefetch: Optional[int] = None):
        self.address = address
        self.queue_name = queue_name
        self.ray_namespace = ray_namespace
        self.consumer_id = consumer_id
        self.device_req = device
        self.as_numpy = as_numpy
        self.timeout_s = timeout_s
        # read-ahead bound (frames noticed-but-not-taken + grants outstanding): what a crashed reader
        # can lose; its ring is landing space for that plus the frames it leased, never queue
        # capacity (queue_size stays the producers' one logical bound)
        self.prefetch = int(prefetch) if prefetch is not None else DEFAULT_PREFETCH
        self.slots = slots          # ring slots (default: 2 x prefetch)
        self._queue = None       # the reference's actor handle slot: endpoint or in-process queue
        self._local = None
        self._sess = None
        self._done = False
        self.frames_read = 0

    # ------------------------------------------------------------------------------------
    def connect(self):
        if self._queue is not None:
            return self
        from .queue.cpu_queue import get_queue

        try:   # in-process queue (config 1)
            self._local = get_queue(self.queue_name, self.ray_namespace)
            self._queue = self._local
            return self
        except ValueError:
            pass
        try:
            self._connect_distributed()
        except Exception as e:
            print(f"Error getting queue: {e}")   # data_reader.py:22
            self.close()
            raise
        return self

    def _connect_distributed(self):
        from .parallel.rendezvous import open_store
        from .queue.endpoint import QueueEndpoint
        from .queue.ring import FrameRing, physical_slots
        from .queue.session import QueueSession, wait_meta

        store = open_store(self.address, spawn_if_absent=False, timeout_s=self.timeout_s)
        meta = wait_meta(store, self.ray_namespace, self.queue_name, self.timeout_s)
        sess = QueueSession(store, self.ray_namespace, self.queue_name, meta, "consumer")
        try:
            if meta["device_kind"] == "cuda":
                if self.device_req:
                    device = torch.device(self.device_req)
                else:
                    import os

                    n = max(1, torch.cuda.device_count())
                    lr = os.environ.get("LOCAL_RANK")
                    k = int(lr) if lr is not None else int(meta.get("n_producers", 0)) + sess.consumer_seq
                    device = torch.device(f"cuda:{k % n}")
                torch.cuda.set_device(device)
            else:
                device = torch.device("cpu")
            dtype = {"float32": torch.float32, "uint16": torch.uint16}[meta["dtype"]]
            shape = tuple(meta["frame_shape"])
            frame_bytes = int(np.prod(shape)) * (4 if meta["dtype"] == "float32" else 2)
            want = self.slots or 2 * max(1, self.prefetch)
            slots = physical_slots(want, frame_bytes, device, 0.8)
            ring = FrameRing(shape, dtype, device, 0, slots, shm_name=sess.ring_name() if device.type == "cpu" else None)
            ep = QueueEndpoint(ring, sess, is_producer=False, is_consumer=True, prefetch=self.prefetch)
            ep.start()
        except BaseException:
            sess.close("failed")
            raise
        self._sess, self._queue = sess, ep
        self._meta = meta
        self._panel_shards = meta.get("panel_shards")
        recipe = meta.get("calibrate_on_read")
        if recipe:
            self._calibrator = self._make_calibrator(recipe, device)
        self.consumer_id = sess.consumer_seq
        log.info("consumer %d joined queue %s/%s as member %d (session %d) on %s (%d slots)", sess.consumer_seq,
                 self.ray_namespace, self.queue_name, sess.mid, meta["session"], device, slots)

    @staticmethod
    def _make_calibrator(recipe: dict, device):
        """Rebuild the producer's calibration from the session recipe (--calibrate_on_read)."""
        from .config import CommonModeParams
        from .models.calibrator import Calibrator
        from .models.detector import Mode
        from .producer import load_masks
        from .source import open_source

        src = open_source(recipe["exp"], int(recipe["run"]), recipe["detector_name"], rank=0, size=1, pinned=False,
                          pool_frames=1, data_dir=recipe.get("data_dir"), mode=Mode.raw)
        if getattr(src, "calibrated", False) or not hasattr(src, "consts"):
            raise DataReaderError("calibrate_on_read: the producer's source has no calibration constants here")
        cf = recipe.get("constants")
        if cf:   # the producer ran with --constants: the same file, byte for byte, or nothing
            from .models.constants import CalibConstants, file_sha256

            try:
                digest = file_sha256(cf["path"])
            except OSError as e:
                raise DataReaderError(f"calibrate_on_read: the producer's constants file {cf['path']} cannot be "
                                      f"read here ({e})") from None
            if digest != cf["sha256"]:
                raise DataReaderError(f"calibrate_on_read: constants file {cf['path']} has sha256 {digest}, the "
                                      f"producer loaded {cf['sha256']}")
            try:
                src.consts = CalibConstants.load(cf["path"], src.consts.spec)
            except ValueError as e:
                raise DataReaderError(f"calibrate_on_read: {e}") from None
        mask = load_masks(src, recipe.get("uses_bad_pixel_mask", False), recipe.get("manual_mask_path"))
        cm = recipe.get("common_mode")
        cm = None if cm is None else CommonModeParams(int(cm[0]), float(cm[1]), float(cm[2]), int(cm[3]),
                                                      None if cm[4] is None else int(cm[4]))
        return Calibrator(src.consts, device, Mode(recipe["mode"]), mask=mask, common_mode=cm,
                          geometry=getattr(src, "geometry", None))

    @property
    def calibrator(self):
        """The consumer-side Calibrator when the producer used --calibrate_on_read, else None."""
        return getattr(self, "_calibrator", None)

    def calibrate(self, items: List[FrameItem], release: bool = True, stream=None) -> torch.Tensor:
        """Calibrate leased RAW items (``--calibrate_on_read`` queues) into a new
        ``[n, *out_shape]`` tensor on this reader's device; releases the items by default."""
        cal = self.calibrator
        if cal is None:
            raise DataReaderError("calibrate(): the queue carries calibrated frames already")
        out = torch.empty((len(items), *cal.out_shape), dtype=cal.out_dtype, device=cal.device)
        if items:
            cal.run([it.data for it in items], [out[i] for i in range(len(items))], stream)
            if release:
                for it in items:
                    it.release(stream)
        return out

    @property
    def session_meta(self):
        """The queue session's metadata as the producers published it (None: in-process queue)."""
        return getattr(self, "_meta", None)

    @property
    def panel_shards(self) -> int:
        """G when the producers split frames into panel shards (``--panel_shards``), else 1."""
        ps = getattr(self, "_panel_shards", None)
        return int(ps["n_shards"]) if ps else 1

    def panel_range(self, item) -> tuple:
        """Panels ``[lo, hi)`` of the whole detector frame that ``item`` (a FrameItem or a reference
        ``[rank, idx, data, pe]`` list) carries; the whole frame when frames are not sharded."""
        rank = item.rank if hasattr(item, "rank") else int(item[0])
        data = item.data if hasattr(item, "data") else item[2]
        n = int(data.shape[0])
        g = self.panel_shards
        return ((rank % g) * n, (rank % g + 1) * n) if g > 1 else (0, n)

    def shard_assembler(self, dtype: torch.dtype = torch.float32, max_pending: int = 256):
        """A :class:`~psana_ray_amd.batching.ShardAssembler` for this session's panel shards."""
        from .batching import ShardAssembler

        self._check()
        return ShardAssembler(self.panel_shards, self._queue.ring.frame_shape, self._queue.ring.device, dtype,
                              max_pending)

    # ------------------------------------------------------------------------------------
    @property
    def done(self) -> bool:
        return self._done

    @property
    def endpoint(self):
        return self._queue if self._local is None else None

    def _check(self):
        if self._queue is None:
            raise RuntimeError("DataReader is not connected. Call connect() first.")   # data_reader.py:33

    def lease(self, timeout: float = 0.0, stream=None) -> Optional[FrameItem]:
        """Zero-copy: the next frame as a leased HBM slot (release it, or use ``with``).  With a
        ``--calibrate_on_read`` producer the slot holds the RAW frame: see :meth:`calibrate`."""
        self._check()
        if self._local is not None:
            raise DataReaderError("lease() needs the distributed HBM queue")
        try:
            it = self._queue.get(timeout=timeout, stream=stream)
        except _QueueEOS as e:
            self._done = True
            raise EndOfStream(str(e)) from e
        except QueuePeerError as e:
            raise DataReaderError("Queue peer is dead.") from e
        if it is not None:
            self.frames_read += 1
        return it

    def read(self, timeout: float = 0.0):
        """``[rank, idx, data, photon_energy]`` or None (nothing ready within ``timeout``)."""
        self._check()
        if self._local is not None:
            item = self._local.get(timeout=timeout or None)
            if item is not None:
                self.frames_read += 1
            return item
        it = self.lease(timeout)
        if it is None:
            return None
        if self.calibrator is not None:   # raw ring: calibrate on read (capacity tier)
            data = self.calibrate([it])[0]
            rank, idx, pe = it.rank, it.idx, it.photon_energy
        else:
            rank, idx, data, pe = it.to_list(copy=True)
        if self.as_numpy:
            data = data.cpu().numpy()
        return [rank, idx, data, pe]

    def read_batch(self, max_n: int, timeout: float = 0.0) -> List[FrameItem]:
        """Up to ``max_n`` leased frames in one call (zero-copy GPU consumers)."""
        out: List[FrameItem] = []
        while len(out) < max_n:
            try:
                it = self.lease(timeout if not out else 0.0)
            except EndOfStream:
                if out:
                    break
                raise
            if it is None:
                break
            out.append(it)
        return out

    def batches(self, batch_size: int = 16, dtype: torch.dtype = torch.float32, timeout: float = 1.0,
                drop_last: bool = False, stream=None):
        """Yield :class:`~psana_ray_amd.batching.FrameBatch` es of ``batch_size`` frames (the last
        one partial unless ``drop_last``) until the end of the stream.  HBM queues: the leased
        slots are gathered into one new ``[n, *frame]`` tensor by a single HIP launch (bf16
        conversion fused for ``dtype=torch.bfloat16``) and released stream-ordered."""
        from .batching import collate_items

        self._check()
        ep = self.endpoint
        if ep is not None and ep._fabric is not None and ep._fabric.prefetch < 2 * batch_size:
            # keep one batch in flight while the previous one is collated
            ep._fabric.set_prefetch(min(2 * batch_size, ep.ring.n_slots))
        if self._local is not None:
            # in-process CPU queue (config 1): reference semantics have no end-of-stream marker
            # (a None get is "empty", Q-2), so the iteration ends after `timeout` s without a frame
            buf = []
            while True:
                item = self.read(timeout)
                if item is None:
                    if buf and not drop_last:
                        yield self._batch_from_lists(buf, dtype)
                    return
                buf.append(item)
                if len(buf) == batch_size:
                    yield self._batch_from_lists(buf, dtype)
                    buf = []
        cal = self.calibrator
        pending: List[FrameItem] = []
        while True:
            try:
                got = self.read_batch(batch_size - len(pending), timeout)
            except EndOfStream:
                if pending and not drop_last:
                    yield collate_items(pending, dtype, stream,
                                        calibrate=(lambda its: self.calibrate(its, True, stream)) if cal else None)
                elif pending:
                    for it in pending:
                        it.release(stream)
                return
            pending.extend(got)
            if len(pending) == batch_size:
                yield collate_items(pending, dtype, stream,
                                    calibrate=(lambda its: self.calibrate(its, True, stream)) if cal else None)
                pending = []

    @staticmethod
    def _batch_from_lists(items, dtype):
        from .batching import FrameBatch

        data = torch.stack([torch.as_tensor(it[2]) for it in items]).to(dtype)
        pe = [float("nan") if it[3] is None else float(it[3]) for it in items]
        r = torch.tensor([it[0] for it in items], dtype=torch.int64)
        i = torch.tensor([it[1] for it in items], dtype=torch.int64)
        return FrameBatch(data=data, rank=r, idx=i, gevt=torch.full_like(i, -1), photon_energy=torch.tensor(pe))

    def close(self):
        ep = self.endpoint
        if ep is not None:
            # leave the queue: producers stop writing into this shard (frames still in flight go to
            # other consumers) before its memory is released; other members are unaffected
            ep.close(timeout=min(30.0, self.timeout_s))
        self._queue = None
        self._local = None

    def __enter__(self):
        self.connect()
        return self

    def __exit__(self, exc_type, exc_val, exc_tb):
        self.close()
