"""Per-pixel spectra of a run: how often every pixel of the CALIBRATED frames read every value.

``psana-ray-consumer --task hist`` counts, per pixel, the samples in each of ``nbins`` equal bins of a
window ``[lo, hi]`` as INTEGERS (the K-12 numerics contract, docs/ARCHITECTURE.md): :class:`PixelHist` is
that accumulator, :func:`merge` adds several consumers' files exactly, and :func:`derive_gain_correction`
/ :func:`apply_gain_correction` turn the one-photon peak of a flat-field or fluorescence run into gains
that ``--constants`` loads.

    python -m psana_ray_amd.hist merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.hist info RUN.npz
    python -m psana_ray_amd.hist spectrum RUN.npz --out s.npy
    python -m psana_ray_amd.hist gain RUN.npz --peak 6,12 --expected 9.5 --base BASE.npz --gain_range 0 \\
        --out consts.npz --corr_out corr.npy
"""
from __future__ import annotations

import argparse
import json
import sys
from dataclasses import dataclass, field

import numpy as np

from .ops.reference import HIST_MAX_FRAMES, validate_pixel_hist_params

HIST_FORMAT = "psana_ray_amd.hist/1"
_FIELDS = ("format", "detector", "layout", "shape", "lo", "hi", "nbins", "frames", "hist")
_ROWS = 1 << 16   # pixels per block of the float64 views (bounded temporaries)


@dataclass
class PixelHist:
    """Per-pixel histograms of a run.  ``hist`` int32 ``[n, nbins]`` with n = prod(shape), pixel-major:
    ``hist[p, b]`` is the number of frames in which pixel p read a value in bin b of the ``nbins`` equal
    bins of ``[lo, hi]`` (the last bin closed on the right); ``frames`` is the number of frames seen, so no
    bin exceeds it.  Bin k spans ``edges()[k] .. edges()[k + 1]``; the device bins with float32
    arithmetic, so a sample within a float32 rounding of an edge may sit in the neighbouring bin."""
    detector: str
    layout: str
    shape: tuple
    lo: float
    hi: float
    nbins: int
    frames: int
    hist: np.ndarray
    inv_w: float = field(init=False)

    def __post_init__(self):
        self.detector, self.layout = str(self.detector), str(self.layout)
        self.shape = tuple(int(s) for s in self.shape)
        n = int(np.prod(self.shape))
        self.frames = int(self.frames)
        self.lo, self.hi, self.nbins, self.inv_w = validate_pixel_hist_params(self.lo, self.hi, self.nbins, n=n,
                                                                              frames=max(0, self.frames), what="hist")
        if self.frames < 0:
            raise ValueError(f"hist: {self.frames} frames")
        h = np.asarray(self.hist)
        if h.dtype != np.int32:
            raise ValueError(f"hist: hist is {h.dtype}, expected int32")
        if h.shape != (n, self.nbins):
            raise ValueError(f"hist: hist must be [{n}, {self.nbins}], got {h.shape}")
        self.hist = np.ascontiguousarray(h)
        if h.size and (int(h.min()) < 0 or int(h.max()) > self.frames):
            raise ValueError(f"hist: a bin outside 0 .. frames = {self.frames}")

    @property
    def n(self) -> int:
        return int(self.hist.shape[0])

    @property
    def width(self) -> float:
        """The bin width (hi - lo) / nbins in float64."""
        return (self.hi - self.lo) / self.nbins

    def key(self):
        """What two accumulators must share to be merged."""
        return (self.detector, self.layout, self.shape, self.lo, self.hi, self.nbins)

    _KEY_NAMES = ("detector", "layout", "shape", "lo", "hi", "nbins")

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez_compressed(f, format=np.asarray(HIST_FORMAT), detector=np.asarray(self.detector),
                                layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                                lo=np.float32(self.lo), hi=np.float32(self.hi), nbins=np.int64(self.nbins),
                                frames=np.int64(self.frames), hist=self.hist)
        return path

    @classmethod
    def load(cls, path) -> "PixelHist":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a pixel-histogram file (no {', '.join(missing)})")
            if str(z["format"]) != HIST_FORMAT:
                raise ValueError(f"{path}: pixel-histogram format {str(z['format'])!r}, expected {HIST_FORMAT!r}")
            if z["frames"].dtype != np.int64:
                raise ValueError(f"{path}: frames is {z['frames'].dtype}, expected int64")
            hist = z["hist"]
            if hist.dtype != np.int32:
                raise ValueError(f"{path}: hist is {hist.dtype}, expected int32")
            return cls(str(z["detector"]), str(z["layout"]), tuple(int(s) for s in z["shape"]), float(z["lo"]),
                       float(z["hi"]), int(z["nbins"]), int(z["frames"]), hist)

    def add(self, other: "PixelHist") -> "PixelHist":
        """Exact merge of two accumulators of the same detector, layout, shape, window and nbins."""
        if other.key() != self.key():
            diff = [n for n, a, b in zip(self._KEY_NAMES, self.key(), other.key()) if a != b]
            raise ValueError(f"hist: accumulators differ in {', '.join(diff)}")
        total = self.frames + other.frames
        if total > HIST_MAX_FRAMES:
            raise ValueError(f"hist: merged run of {total} frames is longer than {HIST_MAX_FRAMES}")
        # a bin is at most its run's frames, so the int32 sum cannot wrap
        return PixelHist(self.detector, self.layout, self.shape, self.lo, self.hi, self.nbins, total,
                         self.hist + other.hist)

    # ---------------------------------------------------------------- float64 views of the integers
    def edges(self) -> np.ndarray:
        """float64 [nbins + 1]: ``lo + k * (hi - lo) / nbins``; the last is exactly ``hi``."""
        e = self.lo + np.arange(self.nbins + 1, dtype=np.float64) * self.width
        e[-1] = self.hi
        return e

    def centers(self) -> np.ndarray:
        """float64 [nbins]: ``lo + (k + 0.5) * (hi - lo) / nbins``."""
        return self.lo + (np.arange(self.nbins, dtype=np.float64) + 0.5) * self.width

    def total(self) -> np.ndarray:
        """The detector spectrum: int64 [nbins], the sum over pixels."""
        return self.hist.sum(axis=0, dtype=np.int64)

    def counts(self) -> np.ndarray:
        """int64 [n]: the samples of every pixel inside the window."""
        return self.hist.sum(axis=1, dtype=np.int64)

    def mode(self) -> np.ndarray:
        """float64 [n]: the centre of the fullest bin of every pixel; ties go to the lowest bin; NaN where
        the pixel has no sample."""
        k = np.argmax(self.hist, axis=1)   # the first of equal maxima
        return np.where(self.counts() > 0, self.centers()[k], np.nan)

    def quantile(self, q: float) -> np.ndarray:
        """float64 [n]: the q-quantile (0 <= q <= 1) of every pixel's histogram, linear inside the bin.
        With N the pixel's samples, ``C[k] = hist[0] + ... + hist[k]`` (``C[-1] = 0``) and ``t = q * N``,
        let k be the FIRST bin with ``hist[k] > 0`` and ``C[k] >= t``; the result is
        ``edges[k] + (t - C[k - 1]) / hist[k] * width``.  So q = 0 gives the left edge of the first
        non-empty bin, q = 1 the right edge of the last one, and a quantile that falls between two
        non-empty bins gives the right edge of the lower one.  NaN where N = 0."""
        q = float(q)
        if not 0.0 <= q <= 1.0:
            raise ValueError(f"hist: quantile {q} outside [0, 1]")
        out = np.full(self.n, np.nan)
        e, w = self.edges(), self.width
        for a in range(0, self.n, _ROWS):
            h = self.hist[a:a + _ROWS].astype(np.int64)
            C = np.cumsum(h, axis=1)
            N = C[:, -1]
            t = q * N.astype(np.float64)
            k = np.argmax((h > 0) & (C >= t[:, None]), axis=1)
            rows = np.arange(h.shape[0])
            hk = h[rows, k]
            below = (C[rows, k] - hk).astype(np.float64)
            v = e[k] + (t - below) / np.where(hk > 0, hk, 1) * w
            out[a:a + _ROWS] = np.where(N > 0, v, np.nan)
        return out

    def centroid(self, lo: float, hi: float, min_count: int = 1) -> np.ndarray:
        """float64 [n]: the count-weighted mean of the centres of the bins whose centre lies in
        ``[lo, hi]``; NaN where the pixel has fewer than ``min_count`` (at least 1) samples in those bins.
        A sample differs from its bin's centre by at most half a bin, and so does the centroid from the
        mean of the samples in those bins."""
        c = self.centers()
        sel = np.nonzero((c >= float(lo)) & (c <= float(hi)))[0]
        if sel.size == 0:
            raise ValueError(f"hist: no bin centre in [{lo}, {hi}]")
        need = max(1, int(min_count))
        out = np.full(self.n, np.nan)
        for a in range(0, self.n, _ROWS):
            h = self.hist[a:a + _ROWS, sel[0]:sel[-1] + 1].astype(np.int64)   # the selected bins are contiguous
            cnt = h.sum(axis=1)
            # exact integer moment about the first selected bin, then one float64 division
            m = (h * np.arange(h.shape[1], dtype=np.int64)).sum(axis=1)
            v = c[sel[0]] + m.astype(np.float64) / np.where(cnt > 0, cnt, 1) * self.width
            out[a:a + _ROWS] = np.where(cnt >= need, v, np.nan)
        return out


def merge(paths) -> PixelHist:
    """Add several ``--task hist --out`` files: exactly what one consumer would have accumulated over the
    same frames.  Raises ValueError for files of another detector, layout, shape, window or nbins, and for
    a merged run past 2^31 - 1 frames."""
    paths = list(paths)
    if not paths:
        raise ValueError("hist.merge: no files")
    out = None
    for p in paths:
        h = PixelHist.load(p)
        try:
            out = h if out is None else out.add(h)
        except ValueError as e:
            raise ValueError(f"hist.merge: {p}: {e}") from None
    return out


def derive_gain_correction(h: PixelHist, peak_lo: float, peak_hi: float, expected: float,
                           min_count: int = 1) -> np.ndarray:
    """float32 [n] ``expected / centroid(peak_lo, peak_hi, min_count)``: the factor by which a pixel's
    calibrated values must be multiplied to put its peak at ``expected``.  NaN where the centroid is NaN
    (too few samples in the peak window) or not positive."""
    expected = float(expected)
    if not np.isfinite(expected) or expected <= 0.0:
        raise ValueError(f"hist: expected peak position {expected} must be finite and positive")
    c = h.centroid(peak_lo, peak_hi, min_count)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(c > 0.0, expected / c, np.nan).astype(np.float32)


def apply_gain_correction(consts, corr, gain_range: int):
    """New :class:`~psana_ray_amd.models.constants.CalibConstants` with ``gains[gain_range] /= corr`` where
    ``corr`` is finite and positive; everything else is copied.  The calibration is ``out = v * (1 / gain)``,
    so dividing the gain by ``corr`` multiplies the calibrated value by it."""
    from .models.constants import CalibConstants

    g = int(gain_range)
    gains = np.array(consts.gains, np.float32, copy=True)
    if not 0 <= g < gains.shape[0]:
        raise ValueError(f"hist: gain_range {g} outside 0 .. {gains.shape[0] - 1}")
    corr = np.asarray(corr, np.float32)
    if corr.size != gains[g].size:
        raise ValueError(f"hist: a correction of {corr.size} pixels for constants of {gains[g].size} (the "
                         "histogram must be of calib-layout frames)")
    corr = corr.reshape(gains[g].shape)
    ok = np.isfinite(corr) & (corr > 0)
    gains[g] = np.where(ok, gains[g] / np.where(ok, corr, np.float32(1.0)), gains[g]).astype(np.float32)
    cfg = None if consts.gain_config is None else np.array(consts.gain_config, copy=True)
    return CalibConstants(consts.spec, np.array(consts.pedestals, np.float32, copy=True), gains,
                          np.array(consts.status, np.uint8, copy=True), cfg, tuple(consts.cm_gains))


# ------------------------------------------------------------------------------------------- CLI
def _cmd_merge(a) -> int:
    try:
        h = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"hist merge: {e}", file=sys.stderr)
        return 2
    h.save(a.out)
    print(f"hist merge: {len(a.files)} files, frames={h.frames} of {h.detector} -> {a.out}")
    return 0


def _cmd_info(a) -> int:
    try:
        h = PixelHist.load(a.file)
    except (ValueError, OSError) as e:
        print(f"hist info: {e}", file=sys.stderr)
        return 2
    cnt = h.counts()
    print(json.dumps({"detector": h.detector, "layout": h.layout, "shape": list(h.shape), "lo": h.lo, "hi": h.hi,
                      "nbins": h.nbins, "bin_width": h.width, "frames": h.frames, "samples": int(cnt.sum()),
                      "pixels_without_sample": int((cnt == 0).sum())}, sort_keys=True))
    return 0


def _cmd_spectrum(a) -> int:
    try:
        h = PixelHist.load(a.file)
        np.save(a.out, h.total())
    except (ValueError, OSError) as e:
        print(f"hist spectrum: {e}", file=sys.stderr)
        return 2
    print(f"hist spectrum: int64 [{h.nbins}] over {h.n} pixels and {h.frames} frames -> {a.out}")
    return 0


def _cmd_gain(a) -> int:
    from .models.constants import CalibConstants

    try:
        lo, hi = (float(x) for x in a.peak.split(","))
        h = PixelHist.load(a.file)
        base = CalibConstants.load(a.base)
        corr = derive_gain_correction(h, lo, hi, a.expected, a.min_count)
        out = apply_gain_correction(base, corr, a.gain_range)
        out.save(a.out)
        if a.corr_out:
            np.save(a.corr_out, corr.reshape(h.shape))
    except (ValueError, OSError, KeyError) as e:
        print(f"hist gain: {e}", file=sys.stderr)
        return 2
    print(f"hist gain: {int(np.isfinite(corr).sum())} of {corr.size} pixels corrected in gain range {a.gain_range} "
          f"-> {a.out}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.hist", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="add several consumers' pixel-histogram files (exact)")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    i = sub.add_parser("info", help="parameters, frames and sample counts of a file, as JSON")
    i.add_argument("file")
    i.set_defaults(fn=_cmd_info)
    s = sub.add_parser("spectrum", help="the detector spectrum (sum over pixels) as an int64 .npy")
    s.add_argument("file")
    s.add_argument("--out", required=True)
    s.set_defaults(fn=_cmd_spectrum)
    g = sub.add_parser("gain", help="gains from the centroid of a peak: new constants for --constants")
    g.add_argument("file")
    g.add_argument("--peak", required=True, help="LO,HI: the bins whose centre lies inside hold the peak (a negative LO: --peak=-4,12)")
    g.add_argument("--expected", type=float, required=True, help="where the peak belongs, in the frames' units")
    g.add_argument("--base", required=True, help="the constants the run was calibrated with (.npz)")
    g.add_argument("--gain_range", type=int, required=True, help="the gain table the run's pixels were in")
    g.add_argument("--min_count", type=int, default=1, help="samples in the peak window a pixel needs (default 1)")
    g.add_argument("--out", required=True)
    g.add_argument("--corr_out", default=None, help="also write the float32 correction, frame-shaped (.npy)")
    g.set_defaults(fn=_cmd_gain)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
