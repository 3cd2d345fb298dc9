"""Dark-run statistics and the calibration constants derived from them.

A dark run (no beam, a few thousand raw frames) gives per-pixel pedestal and noise for each gain
range, and a bad-pixel status.  ``psana-ray-consumer --task dark`` accumulates, per pixel and decoded
gain candidate, the count, sum and sum of squares of the raw ADU as INTEGERS (the K-09 numerics
contract, docs/ARCHITECTURE.md): :class:`DarkStats` is that accumulator, :func:`merge` adds several
consumers' files exactly, and :func:`derive_constants` turns one dark run per gain configuration into
a :class:`CalibConstants` that ``psana-ray-producer --constants`` loads.

    python -m psana_ray_amd.dark merge A.npz B.npz --out DARK.npz
    python -m psana_ray_amd.dark derive DARK.npz --out CONSTS.npz --base CONSTS0.npz --gain_config AHL
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from .models.constants import CalibConstants
from .models.detector import EPIX_CAND_A, EPIX_CAND_B, EPIX_CONFIG_NAMES, get_detector

DARK_FORMAT = "psana_ray_amd.dark/1"
KIND_NAMES = ("epix10ka", "jungfrau", "plain")
NC_OF_KIND = (2, 3, 1)      # candidates per kernel kind
MAX_FRAMES = 2 ** 31 - 1    # frames per run: the int32 count is the only limit (65535^2 * (2^31 - 1) < 2^63)

# status bits of derive_constants
STATUS_NOISY = 1     # rms above its high limit
STATUS_QUIET = 2     # rms below its low limit (a stuck pixel has rms 0)
STATUS_OFFSET = 4    # mean outside its limits
STATUS_STARVED = 8   # fewer than min_frames samples in a covered gain range
STATUS_BITS = (STATUS_NOISY, STATUS_QUIET, STATUS_OFFSET, STATUS_STARVED)

DEFAULT_MIN_FRAMES = 50
# robust limits: median +- k * 1.4826 * MAD over the pixels of a covered range.  The spread over
# pixels of a healthy detector is roughly normal (pedestals scatter by ~100 ADU, noise by a few
# percent); 6 sigma-equivalents flags a normal pixel with probability 2e-9 -- none of a 16M-pixel
# detector -- and still catches hot, dead and offset pixels, which sit tens of sigma out.
DEFAULT_K = 6.0


@dataclass
class DarkStats:
    """Integer accumulators of a dark run: ``cnt`` / ``sum`` / ``sq`` are int64 ``[NC, npix]`` (count,
    sum of ADU, sum of ADU^2 of the samples that decoded to candidate c inside ``[adu_lo, adu_hi]``);
    ``kind`` is DetectorSpec.kernel_kind (0 epix10ka, 1 jungfrau, 2 plain); ``frames`` the frames seen."""
    detector: str
    kind: int
    adu_lo: int
    adu_hi: int
    frames: int
    cnt: np.ndarray
    sum: np.ndarray
    sq: np.ndarray

    def __post_init__(self):
        self.kind, self.adu_lo, self.adu_hi, self.frames = int(self.kind), int(self.adu_lo), int(self.adu_hi), int(self.frames)
        if self.kind not in (0, 1, 2):
            raise ValueError(f"dark: unknown gain kind {self.kind}")
        if not 0 <= self.adu_lo <= self.adu_hi <= 65535:
            raise ValueError(f"dark: ADU window [{self.adu_lo}, {self.adu_hi}] outside 0 <= lo <= hi <= 65535")
        if not 0 <= self.frames <= MAX_FRAMES:
            raise ValueError(f"dark: {self.frames} frames outside 0 .. 2^31 - 1")
        self.cnt = np.ascontiguousarray(self.cnt, np.int64)
        self.sum = np.ascontiguousarray(self.sum, np.int64)
        self.sq = np.ascontiguousarray(self.sq, np.int64)
        nc = NC_OF_KIND[self.kind]
        if self.cnt.ndim != 2 or self.cnt.shape[0] != nc or self.sum.shape != self.cnt.shape or self.sq.shape != self.cnt.shape:
            raise ValueError(f"dark: accumulators must be three [{nc}, npix] arrays, got {self.cnt.shape}, "
                             f"{self.sum.shape}, {self.sq.shape}")

    @property
    def npix(self) -> int:
        return int(self.cnt.shape[1])

    def key(self):
        """What two accumulators must share to be added."""
        return (self.detector, self.kind, self.adu_lo, self.adu_hi, self.npix)

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez(f, format=np.asarray(DARK_FORMAT), detector=np.asarray(self.detector), kind=np.int64(self.kind),
                     adu_lo=np.int64(self.adu_lo), adu_hi=np.int64(self.adu_hi), frames=np.int64(self.frames),
                     cnt=self.cnt, sum=self.sum, sq=self.sq)
        return path

    @classmethod
    def load(cls, path) -> "DarkStats":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in ("format", "detector", "kind", "adu_lo", "adu_hi", "frames", "cnt", "sum", "sq")
                       if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a dark-statistics file (no {', '.join(missing)})")
            if str(z["format"]) != DARK_FORMAT:
                raise ValueError(f"{path}: dark-statistics format {str(z['format'])!r}, expected {DARK_FORMAT!r}")
            for k in ("cnt", "sum", "sq"):
                if z[k].dtype != np.int64:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected int64")
            return cls(str(z["detector"]), int(z["kind"]), int(z["adu_lo"]), int(z["adu_hi"]), int(z["frames"]),
                       z["cnt"], z["sum"], z["sq"])

    def add(self, other: "DarkStats") -> "DarkStats":
        """Exact integer sum of two accumulators of the same detector, kind and window."""
        if other.key() != self.key():
            names = ("detector", "kind", "adu_lo", "adu_hi", "npix")
            diff = [n for n, a, b in zip(names, self.key(), other.key()) if a != b]
            raise ValueError(f"dark: accumulators differ in {', '.join(diff)}: {self.key()} vs {other.key()}")
        if self.frames + other.frames > MAX_FRAMES:
            raise ValueError("dark: merged run longer than 2^31 - 1 frames")
        return DarkStats(self.detector, self.kind, self.adu_lo, self.adu_hi, self.frames + other.frames,
                         self.cnt + other.cnt, self.sum + other.sum, self.sq + other.sq)

    def mean(self) -> np.ndarray:
        """float64 ``sum / cnt`` [NC, npix], NaN where ``cnt == 0``."""
        c = self.cnt.astype(np.float64)
        return np.where(self.cnt > 0, self.sum.astype(np.float64) / np.where(self.cnt > 0, c, 1.0), np.nan)

    def variance(self) -> np.ndarray:
        """float64 ``max(0, sq / cnt - mean^2)`` [NC, npix], NaN where ``cnt == 0``.

        Cancellation bound: ``sum`` (< 2^47) and ``cnt`` convert to float64 exactly, ``sq`` to within
        2^-53 relative; the two divisions, the square and the subtraction round once each (2^-53
        relative), all on terms no larger than ``sq / cnt = mean^2 + var``.  That is at most five
        roundings of 2^-53 each, so the absolute error of the variance is below ``VARIANCE_BOUND *
        (mean^2 + var)`` with VARIANCE_BOUND = 2^-50 -- for dark data (var << mean^2) about 2^-50 *
        mean^2: 2.4e-7 ADU^2 at the top of the 14-bit ADUs of epix10ka and jungfrau, 3.8e-6 ADU^2 at
        a plain detector's 65535.  A noise of 1 ADU rms is known to about 1e-6 ADU either way."""
        c = np.where(self.cnt > 0, self.cnt.astype(np.float64), 1.0)
        m = self.sum.astype(np.float64) / c
        v = np.maximum(0.0, self.sq.astype(np.float64) / c - m * m)
        return np.where(self.cnt > 0, v, np.nan)

    def rms(self) -> np.ndarray:
        """float64 ``sqrt(max(0, sq / cnt - mean^2))`` [NC, npix] (see :meth:`variance` for the bound)."""
        return np.sqrt(self.variance())


VARIANCE_BOUND = 2.0 ** -50   # |variance() - exact| <= VARIANCE_BOUND * (mean^2 + var)


def merge(paths) -> DarkStats:
    """Add the accumulators of several ``--task dark --out`` files: exactly what one consumer would have
    accumulated over the same frames.  Raises ValueError for files of another detector, kind or window."""
    paths = list(paths)
    if not paths:
        raise ValueError("dark.merge: no files")
    out = None
    for p in paths:
        st = DarkStats.load(p)
        try:
            out = st if out is None else out.add(st)
        except ValueError as e:
            raise ValueError(f"dark.merge: {p}: {e}") from None
    return out


def _gain_config_array(gain_config, spec) -> Optional[np.ndarray]:
    """The configuration the dark run was taken in as a per-pixel uint8 [npix] (epix10ka only)."""
    if spec.kind != "epix10ka":
        return None
    if gain_config is None:
        raise ValueError(f"derive_constants: an epix10ka dark run needs the gain configuration it was taken in "
                         f"(one of {', '.join(EPIX_CONFIG_NAMES)} or a per-pixel array)")
    if isinstance(gain_config, str):
        if gain_config not in EPIX_CONFIG_NAMES:
            raise ValueError(f"derive_constants: gain_config {gain_config!r} is not one of {', '.join(EPIX_CONFIG_NAMES)}")
        return np.full(spec.npix, EPIX_CONFIG_NAMES.index(gain_config), np.uint8)
    cfg = np.asarray(gain_config)
    if cfg.size != spec.npix or not np.issubdtype(cfg.dtype, np.integer) or cfg.min() < 0 or cfg.max() > 4:
        raise ValueError(f"derive_constants: a per-pixel gain_config must hold {spec.npix} integers in 0..4")
    return cfg.reshape(-1).astype(np.uint8)


def _robust_limits(x: np.ndarray, k: float):
    med = float(np.median(x))
    sig = 1.4826 * float(np.median(np.abs(x - med)))
    return med - k * sig, med + k * sig


def derive_constants(stats_list, base: CalibConstants, gain_config=None, min_frames: int = DEFAULT_MIN_FRAMES,
                     rms_lo: Optional[float] = None, rms_hi: Optional[float] = None,
                     mean_lo: Optional[float] = None, mean_hi: Optional[float] = None, k: float = DEFAULT_K,
                     include_base_status: bool = False):
    """Constants from dark runs: ``(CalibConstants, report)``.

    ``stats_list``: one :class:`DarkStats` (or several, one dark run per gain configuration; they fill
    their gain ranges in turn, a later one replacing an earlier one on a range both cover).
    ``gain_config``: the configuration each dark run was TAKEN in -- one of EPIX_CONFIG_NAMES or a
    per-pixel array, or a list of those, one per DarkStats; ignored for jungfrau and plain.  It maps
    candidate c of a pixel to its gain range through EPIX_CAND_A / EPIX_CAND_B (jungfrau: c is the
    range); ``base.gain_config`` is never used for that.

    A gain range is COVERED when the median over its pixels of its counts is >= ``min_frames``.  For
    a covered range, ``pedestals[g] = float32(mean)`` at pixels with ``cnt >= min_frames``; every other
    pedestal, and all of ``gains``, ``gain_config`` and ``cm_gains`` (a dark run cannot measure gains),
    come from ``base``.  ``status`` is the uint8 OR over covered ranges of 1 (rms above its high limit),
    2 (rms below its low limit, or exactly 0: stuck), 4 (mean outside its limits), 8 (``cnt <
    min_frames``; such a pixel's mean and rms are not judged).  A limit given here is absolute and
    holds for every range; one left None is robust, median -+ ``k`` * 1.4826 * MAD over the range's
    pixels with enough samples (comparisons are strict: a pixel ON a limit is good).  ``base.status``
    is OR-ed in only with ``include_base_status``.

    ``report``: ``covered`` (gain ranges), ``ranges`` (per covered range: pixels, median mean / rms,
    the limits used, flagged pixels per bit), ``flagged`` (pixels per bit over all ranges), ``bad_pixels``."""
    if isinstance(stats_list, DarkStats):
        stats_list = [stats_list]
    stats_list = list(stats_list)
    if not stats_list:
        raise ValueError("derive_constants: no dark statistics")
    spec = base.spec
    if isinstance(gain_config, (list, tuple)) and not isinstance(gain_config, str):
        if len(gain_config) != len(stats_list):
            raise ValueError(f"derive_constants: {len(gain_config)} gain configurations for {len(stats_list)} dark runs")
        cfgs = list(gain_config)
    else:
        cfgs = [gain_config] * len(stats_list)
    min_frames = int(min_frames)
    if min_frames < 2:
        raise ValueError("derive_constants: min_frames must be at least 2 (an rms needs two samples)")
    npix, G = spec.npix, spec.n_gains
    ped = np.array(base.pedestals, np.float32, copy=True)
    ped_flat = ped.reshape(G, npix)
    status = np.zeros(npix, np.uint8)
    report = {"detector": spec.name, "min_frames": min_frames, "k": float(k), "covered": [], "ranges": {}}
    for st, cfg_in in zip(stats_list, cfgs):
        if st.kind != spec.kernel_kind or st.npix != npix or st.detector != spec.name:
            raise ValueError(f"derive_constants: dark statistics of {st.detector} (kind {KIND_NAMES[st.kind]}, "
                             f"{st.npix} pixels) for base constants of {spec.name} ({spec.kind}, {npix} pixels)")
        cfg = _gain_config_array(cfg_in, spec)
        nc = st.cnt.shape[0]
        if spec.kind == "epix10ka":
            cmap = np.stack([np.asarray(EPIX_CAND_A, np.int64)[cfg], np.asarray(EPIX_CAND_B, np.int64)[cfg]])
        else:
            cmap = np.repeat(np.arange(nc, dtype=np.int64)[:, None], npix, axis=1)
        for g in range(G):
            sel = cmap == g                      # [NC, npix]: candidate c of pixel p is gain range g
            has = sel.any(axis=0)
            if not has.any():
                continue
            # several candidates of a pixel can be one range (FH: bit 14 changes nothing): integer sums
            one = DarkStats(st.detector, 2, st.adu_lo, st.adu_hi, st.frames,
                            np.where(sel, st.cnt, 0).sum(axis=0, keepdims=True),
                            np.where(sel, st.sum, 0).sum(axis=0, keepdims=True),
                            np.where(sel, st.sq, 0).sum(axis=0, keepdims=True))
            cnt = one.cnt[0]
            if float(np.median(cnt[has])) < min_frames:
                continue
            enough = has & (cnt >= min_frames)
            mean, rms = one.mean()[0], one.rms()[0]
            lim = {}
            r_lo, r_hi = _robust_limits(rms[enough], k)
            m_lo, m_hi = _robust_limits(mean[enough], k)
            lim["rms_lo"] = r_lo if rms_lo is None else float(rms_lo)
            lim["rms_hi"] = r_hi if rms_hi is None else float(rms_hi)
            lim["mean_lo"] = m_lo if mean_lo is None else float(mean_lo)
            lim["mean_hi"] = m_hi if mean_hi is None else float(mean_hi)
            bits = np.zeros(npix, np.uint8)
            bits[enough & (rms > lim["rms_hi"])] |= STATUS_NOISY
            bits[enough & ((rms < lim["rms_lo"]) | (rms == 0.0))] |= STATUS_QUIET
            bits[enough & ((mean < lim["mean_lo"]) | (mean > lim["mean_hi"]))] |= STATUS_OFFSET
            bits[has & ~enough] |= STATUS_STARVED
            status |= bits
            ped_flat[g, enough] = mean[enough].astype(np.float32)
            if g not in report["covered"]:
                report["covered"].append(g)
            report["ranges"][g] = {
                "pixels": int(has.sum()), "median_count": float(np.median(cnt[has])),
                "median_mean": float(np.median(mean[enough])), "median_rms": float(np.median(rms[enough])),
                "limits": lim, "flagged": {int(b): int(((bits & b) != 0).sum()) for b in STATUS_BITS}}
    report["covered"].sort()
    report["flagged"] = {int(b): int(((status & b) != 0).sum()) for b in STATUS_BITS}
    if include_base_status:
        status |= np.asarray(base.status, np.uint8).reshape(-1)
    report["bad_pixels"] = int((status != 0).sum())
    out = CalibConstants(spec, ped, np.array(base.gains, np.float32, copy=True), status.reshape(spec.frame_shape),
                         None if base.gain_config is None else np.array(base.gain_config, copy=True),
                         tuple(base.cm_gains))
    return out, report


# ------------------------------------------------------------------------------------------- CLI
def _cmd_merge(a) -> int:
    try:
        st = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"dark merge: {e}", file=sys.stderr)
        return 2
    st.save(a.out)
    print(f"dark merge: {len(a.files)} files, {st.frames} frames of {st.detector} -> {a.out}")
    return 0


def _cmd_derive(a) -> int:
    try:
        stats = [DarkStats.load(p) for p in a.files]
        spec = get_detector(stats[0].detector)
        if a.base is not None:
            base = CalibConstants.load(a.base, spec)
        elif a.exp is not None and a.run is not None:
            from .source import open_source

            base = open_source(a.exp, a.run, spec.name, data_dir=a.data_dir).consts
        else:
            print("dark derive: give the base constants: --base CONSTS0.npz, or --exp E --run R [--data_dir D]",
                  file=sys.stderr)
            return 2
        cfg = a.gain_config
        if cfg is not None and len(cfg) == 1:
            cfg = cfg[0]
        consts, report = derive_constants(stats, base, gain_config=cfg, min_frames=a.min_frames, rms_lo=a.rms_min,
                                          rms_hi=a.rms_max, mean_lo=a.mean_min, mean_hi=a.mean_max, k=a.k,
                                          include_base_status=a.include_base_status)
    except (ValueError, KeyError, OSError) as e:
        print(f"dark derive: {e}", file=sys.stderr)
        return 2
    except Exception as e:   # NoSourceError and the like: one line, not a traceback
        print(f"dark derive: {type(e).__name__}: {e}", file=sys.stderr)
        return 2
    consts.save(a.out)
    if a.report:
        with open(a.report, "w") as f:
            json.dump(report, f, indent=1, sort_keys=True)
    print(f"dark derive: {spec.name}: gain ranges {report['covered']} from {sum(s.frames for s in stats)} frames, "
          f"{report['bad_pixels']} bad pixels {report['flagged']} -> {a.out}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.dark", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="add several consumers' dark-statistics files (exact)")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    d = sub.add_parser("derive", help="constants (pedestals, status) from dark statistics")
    d.add_argument("files", nargs="+", help="one dark-statistics file per gain configuration")
    d.add_argument("--out", required=True, help="constants file for psana-ray-producer --constants")
    d.add_argument("--base", default=None, help="constants file everything unmeasured is copied from")
    d.add_argument("--exp", default=None, help="with --run: copy from the constants the source of this run uses")
    d.add_argument("--run", type=int, default=None)
    d.add_argument("--data_dir", default=None)
    d.add_argument("--gain_config", nargs="+", choices=EPIX_CONFIG_NAMES, default=None,
                   help="epix10ka: the configuration the dark run(s) were taken in (one, or one per file)")
    d.add_argument("--min_frames", type=int, default=DEFAULT_MIN_FRAMES)
    d.add_argument("--k", type=float, default=DEFAULT_K, help="robust limits: median +- k * 1.4826 * MAD")
    d.add_argument("--rms_min", type=float, default=None, help="absolute low rms limit (ADU)")
    d.add_argument("--rms_max", type=float, default=None, help="absolute high rms limit (ADU)")
    d.add_argument("--mean_min", type=float, default=None, help="absolute low pedestal limit (ADU)")
    d.add_argument("--mean_max", type=float, default=None, help="absolute high pedestal limit (ADU)")
    d.add_argument("--include_base_status", action="store_true", help="OR the base constants' status in")
    d.add_argument("--report", default=None, help="write the report as JSON")
    d.set_defaults(fn=_cmd_derive)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
