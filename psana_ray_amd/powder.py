"""Powder statistics of a run: per-pixel sum, spread, maximum and count above a threshold of the
CALIBRATED frames, split into misses and hits.

``psana-ray-consumer --task powder`` accumulates, per pixel and frame class (0 = miss, 1 = hit; one
class without a hit filter), the count, sum, sum of squares, maximum and count above a threshold of the
quantised value ``q = round_half_even(v * 2^frac_bits)`` as INTEGERS (the K-11 numerics contract,
docs/ARCHITECTURE.md): :class:`PowderStats` is that accumulator, :func:`merge` combines several
consumers' files exactly and :func:`derive_mask` turns one into a keep-mask that ``--radial_mask`` and
``--sparse_mask`` load.

    python -m psana_ray_amd.powder merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.powder info RUN.npz
    python -m psana_ray_amd.powder export RUN.npz --out_prefix run_hits --cls 1
    python -m psana_ray_amd.powder mask RUN.npz --out mask.npy --hot_fraction 0.5
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .ops.reference import POWDER_QMAX_NONE, validate_powder_params

POWDER_FORMAT = "psana_ray_amd.powder/1"
_FIELDS = ("format", "detector", "layout", "shape", "vmin", "vmax", "frac_bits", "thr_above", "min_peaks",
           "peak_params", "frames", "cnt", "sum", "sq", "above", "qmax")


@dataclass
class PowderStats:
    """Integer accumulators of a powder run.  ``frames`` int64 ``[NC]`` (frames per class); ``cnt`` /
    ``sum`` / ``sq`` / ``above`` int64 and ``qmax`` int32, all ``[NC, n]`` with n = prod(shape): count,
    sum of q, sum of q^2, samples with v >= thr_above and the largest q of the samples of class c inside
    ``[vmin, vmax]`` (``qmax`` is INT32_MIN where there was none).  NC = 2 (miss, hit) with a hit filter
    (``min_peaks > 0``; ``peak_params`` are the peak finder's), else 1."""
    detector: str
    layout: str
    shape: tuple
    vmin: float
    vmax: float
    frac_bits: int
    thr_above: float
    min_peaks: int
    peak_params: dict
    frames: np.ndarray
    cnt: np.ndarray
    sum: np.ndarray
    sq: np.ndarray
    above: np.ndarray
    qmax: np.ndarray
    max_frames: int = field(init=False)

    def __post_init__(self):
        self.detector, self.layout = str(self.detector), str(self.layout)
        self.shape = tuple(int(s) for s in self.shape)
        self.vmin, self.vmax, self.frac_bits, self.thr_above, _Q, self.max_frames = validate_powder_params(
            self.vmin, self.vmax, self.frac_bits, self.thr_above, "powder")
        self.min_peaks = int(self.min_peaks)
        self.peak_params = {str(k): float(v) for k, v in dict(self.peak_params).items()}
        self.frames = np.ascontiguousarray(self.frames, np.int64).reshape(-1)
        nc, n = int(self.frames.size), int(np.prod(self.shape))
        if nc not in (1, 2) or nc != (2 if self.min_peaks > 0 else 1):
            raise ValueError(f"powder: {nc} classes with min_peaks = {self.min_peaks} (2 iff min_peaks > 0)")
        if (self.frames < 0).any() or int(self.frames.sum()) > self.max_frames:
            raise ValueError(f"powder: {self.frames.tolist()} frames outside 0 .. max_frames = {self.max_frames}")
        for k in ("cnt", "sum", "sq", "above"):
            setattr(self, k, np.ascontiguousarray(getattr(self, k), np.int64))
        self.qmax = np.ascontiguousarray(self.qmax, np.int32)
        for k in ("cnt", "sum", "sq", "above", "qmax"):
            if getattr(self, k).shape != (nc, n):
                raise ValueError(f"powder: {k} must be [{nc}, {n}], got {getattr(self, k).shape}")

    @property
    def nc(self) -> int:
        return int(self.frames.size)

    @property
    def n(self) -> int:
        return int(self.cnt.shape[1])

    def key(self):
        """What two accumulators must share to be merged."""
        return (self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.thr_above,
                self.min_peaks, json.dumps(self.peak_params, sort_keys=True), self.nc)

    _KEY_NAMES = ("detector", "layout", "shape", "vmin", "vmax", "frac_bits", "thr_above", "min_peaks", "peak_params",
                  "classes")

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez(f, format=np.asarray(POWDER_FORMAT), detector=np.asarray(self.detector),
                     layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                     vmin=np.float32(self.vmin), vmax=np.float32(self.vmax), frac_bits=np.int64(self.frac_bits),
                     thr_above=np.float32(self.thr_above), min_peaks=np.int64(self.min_peaks),
                     peak_params=np.asarray(json.dumps(self.peak_params, sort_keys=True)), frames=self.frames,
                     cnt=self.cnt, sum=self.sum, sq=self.sq, above=self.above, qmax=self.qmax)
        return path

    @classmethod
    def load(cls, path) -> "PowderStats":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a powder-statistics file (no {', '.join(missing)})")
            if str(z["format"]) != POWDER_FORMAT:
                raise ValueError(f"{path}: powder-statistics format {str(z['format'])!r}, expected {POWDER_FORMAT!r}")
            for k in ("frames", "cnt", "sum", "sq", "above"):
                if z[k].dtype != np.int64:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected int64")
            if z["qmax"].dtype != np.int32:
                raise ValueError(f"{path}: qmax is {z['qmax'].dtype}, expected int32")
            return cls(str(z["detector"]), str(z["layout"]), tuple(int(s) for s in z["shape"]), float(z["vmin"]),
                       float(z["vmax"]), int(z["frac_bits"]), float(z["thr_above"]), int(z["min_peaks"]),
                       json.loads(str(z["peak_params"])), z["frames"], z["cnt"], z["sum"], z["sq"], z["above"],
                       z["qmax"])

    def add(self, other: "PowderStats") -> "PowderStats":
        """Exact merge of two accumulators of the same detector, shape, parameters and classes: integer
        sums, and the larger ``qmax``."""
        if other.key() != self.key():
            diff = [n for n, a, b in zip(self._KEY_NAMES, self.key(), other.key()) if a != b]
            raise ValueError(f"powder: accumulators differ in {', '.join(diff)}")
        total = int(self.frames.sum()) + int(other.frames.sum())
        if total > self.max_frames:
            raise ValueError(f"powder: merged run of {total} frames is longer than max_frames = {self.max_frames}")
        return PowderStats(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits,
                           self.thr_above, self.min_peaks, self.peak_params, self.frames + other.frames,
                           self.cnt + other.cnt, self.sum + other.sum, self.sq + other.sq, self.above + other.above,
                           np.maximum(self.qmax, other.qmax))

    # ---------------------------------------------------------------- float64 views of the integers
    def _combined(self, c: Optional[int]):
        """(cnt, sum, sq, above, qmax) [n] of class ``c``, or of all classes together (None)."""
        if c is None:
            return (self.cnt.sum(axis=0), self.sum.sum(axis=0), self.sq.sum(axis=0), self.above.sum(axis=0),
                    self.qmax.max(axis=0))
        if not 0 <= int(c) < self.nc:
            raise ValueError(f"powder: class {c} of {self.nc}")
        c = int(c)
        return self.cnt[c], self.sum[c], self.sq[c], self.above[c], self.qmax[c]

    def mean(self, c: Optional[int] = None) -> np.ndarray:
        """float64 ``sum / cnt * 2^-S`` [n] in the frames' units, NaN where ``cnt == 0``."""
        cnt, s, _sq, _a, _m = self._combined(c)
        d = np.where(cnt > 0, cnt, 1).astype(np.float64)
        return np.where(cnt > 0, s.astype(np.float64) / d * 2.0 ** -self.frac_bits, np.nan)

    def rms(self, c: Optional[int] = None) -> np.ndarray:
        """float64 ``sqrt(max(0, sq / cnt - (sum / cnt)^2)) * 2^-S`` [n], NaN where ``cnt == 0``.  A
        pixel whose samples were all equal has rms EXACTLY 0: that is decided on the integers (the
        samples are all m iff ``sum == cnt * m`` and ``sq == m * sum``; ``|m * sum| <= cnt * Q^2`` fits
        an int64 by the run bound), not by a float64 cancellation."""
        cnt, s, sq, _a, _m = self._combined(c)
        di = np.where(cnt > 0, cnt, 1)
        d = di.astype(np.float64)
        m_int = s // di
        constant = (m_int * di == s) & (m_int * s == sq)
        m = s.astype(np.float64) / d
        var = np.maximum(0.0, sq.astype(np.float64) / d - m * m)
        return np.where(cnt > 0, np.where(constant, 0.0, np.sqrt(var)) * 2.0 ** -self.frac_bits, np.nan)

    def max(self, c: Optional[int] = None) -> np.ndarray:
        """float64 maximum projection ``qmax * 2^-S`` [n], NaN where there was no sample."""
        _cnt, _s, _sq, _a, m = self._combined(c)
        return np.where(m != POWDER_QMAX_NONE, m.astype(np.float64) * 2.0 ** -self.frac_bits, np.nan)

    def fraction_above(self, c: Optional[int] = None) -> np.ndarray:
        """float64 ``above / cnt`` [n], NaN where ``cnt == 0``."""
        cnt, _s, _sq, a, _m = self._combined(c)
        return np.where(cnt > 0, a.astype(np.float64) / np.where(cnt > 0, cnt, 1), np.nan)


def merge(paths) -> PowderStats:
    """Combine several ``--task powder --out`` files: exactly what one consumer would have accumulated
    over the same frames.  Raises ValueError for files of other parameters, detector, shape or classes,
    and for a merged run past ``powder_max_frames``."""
    paths = list(paths)
    if not paths:
        raise ValueError("powder.merge: no files")
    out = None
    for p in paths:
        st = PowderStats.load(p)
        try:
            out = st if out is None else out.add(st)
        except ValueError as e:
            raise ValueError(f"powder.merge: {p}: {e}") from None
    return out


def derive_mask(stats: PowderStats, hot_fraction: float = 0.5, min_samples: int = 1) -> np.ndarray:
    """uint8 keep-mask of the frame's shape (1 = keep), all classes together.  A pixel is 0 where it is
    HOT (``above / cnt > hot_fraction``), DEAD or shadowed (``cnt < min_samples``) or STUCK (``rms == 0``
    with ``cnt >= 2``).  Loads as ``--radial_mask`` and ``--sparse_mask``."""
    cnt, _s, _sq, above, _m = stats._combined(None)
    hot = above.astype(np.float64) > float(hot_fraction) * cnt.astype(np.float64)
    dead = cnt < int(min_samples)
    with np.errstate(invalid="ignore"):
        stuck = (cnt >= 2) & (stats.rms(None) == 0.0)
    return (~(hot | dead | stuck)).astype(np.uint8).reshape(stats.shape)


# ------------------------------------------------------------------------------------------- CLI
def _cmd_merge(a) -> int:
    try:
        st = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"powder merge: {e}", file=sys.stderr)
        return 2
    st.save(a.out)
    print(f"powder merge: {len(a.files)} files, frames={'+'.join(str(int(f)) for f in st.frames)} of "
          f"{st.detector} -> {a.out}")
    return 0


def _cmd_info(a) -> int:
    try:
        st = PowderStats.load(a.file)
    except (ValueError, OSError) as e:
        print(f"powder info: {e}", file=sys.stderr)
        return 2
    print(json.dumps({"detector": st.detector, "layout": st.layout, "shape": list(st.shape), "vmin": st.vmin,
                      "vmax": st.vmax, "frac_bits": st.frac_bits, "thr_above": st.thr_above,
                      "min_peaks": st.min_peaks, "peak_params": st.peak_params,
                      "frames": [int(f) for f in st.frames], "max_frames": st.max_frames,
                      "samples": [int(c) for c in st.cnt.sum(axis=1)],
                      "pixels_without_sample": int((st.cnt.sum(axis=0) == 0).sum())}, sort_keys=True))
    return 0


def _cmd_export(a) -> int:
    try:
        st = PowderStats.load(a.file)
        c = None if a.cls < 0 else a.cls
        for name in ("mean", "rms", "max"):
            np.save(f"{a.out_prefix}_{name}.npy", getattr(st, name)(c).reshape(st.shape))
    except (ValueError, OSError) as e:
        print(f"powder export: {e}", file=sys.stderr)
        return 2
    print(f"powder export: {a.out_prefix}_mean.npy, _rms.npy, _max.npy of "
          f"{'all classes' if c is None else f'class {c}'}, shape {st.shape}")
    return 0


def _cmd_mask(a) -> int:
    try:
        st = PowderStats.load(a.file)
        m = derive_mask(st, a.hot_fraction, a.min_samples)
        np.save(a.out, m)
    except (ValueError, OSError) as e:
        print(f"powder mask: {e}", file=sys.stderr)
        return 2
    print(f"powder mask: {int((m == 0).sum())} of {m.size} pixels masked -> {a.out}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.powder", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="combine several consumers' powder-statistics files (exact)")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    i = sub.add_parser("info", help="parameters, frames and sample counts of a file, as JSON")
    i.add_argument("file")
    i.set_defaults(fn=_cmd_info)
    e = sub.add_parser("export", help="mean / rms / max of a class as frame-shaped float64 .npy files")
    e.add_argument("file")
    e.add_argument("--out_prefix", required=True, help="writes <prefix>_mean.npy, <prefix>_rms.npy, <prefix>_max.npy")
    e.add_argument("--cls", type=int, default=-1, help="0 = misses, 1 = hits, -1 = all classes together (default)")
    e.set_defaults(fn=_cmd_export)
    k = sub.add_parser("mask", help="keep-mask (uint8 .npy) without hot, dead and stuck pixels")
    k.add_argument("file")
    k.add_argument("--out", required=True)
    k.add_argument("--hot_fraction", type=float, default=0.5)
    k.add_argument("--min_samples", type=int, default=1)
    k.set_defaults(fn=_cmd_mask)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
