"""The cube of a run: the per-pixel mean image of the CALIBRATED frames as a function of a per-event
scalar -- photon energy, delay bin, laser on / off, scan step.

``psana-ray-consumer --task cube`` assigns every frame a bin on the host (:class:`CubeBinning`: from its
photon energy and bin edges, or from its global event number and a table the user computed) and
accumulates, per pixel and bin, the count, sum and sum of squares of the quantised value ``q =
round_half_even(v * 2^frac_bits)`` as INTEGERS (the K-15 numerics contract, docs/ARCHITECTURE.md):
:class:`CubeStats` is that accumulator with its per-frame rows, :func:`merge` combines several consumers'
files exactly.

    python -m psana_ray_amd.cube merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.cube info RUN.npz
    python -m psana_ray_amd.cube export RUN.npz --out_prefix run --ref_bin 0
"""
from __future__ import annotations

import argparse
import hashlib
import json
import math
import sys
from dataclasses import dataclass, field
from typing import Optional

import numpy as np

from .ops.reference import CUBE_BYTES_PER_PIXEL, CUBE_DROPPED, validate_cube_nbins, validate_powder_params

CUBE_FORMAT = "psana_ray_amd.cube/1"
BY = ("photon_energy", "gevt")
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "bin")
_FIELDS = ("format", "detector", "layout", "shape", "vmin", "vmax", "frac_bits", "by", "nbins", "edges",
           "table_sha256", "frames", "dropped", "cnt", "sum", "sq", *PER_FRAME)
_DTYPES = {"edges": np.float64, "frames": np.int64, "dropped": np.int64, "cnt": np.int32, "sum": np.int64,
           "sq": np.int64, "rank": np.int64, "idx": np.int64, "gevt": np.int64, "photon_energy": np.float64,
           "bin": np.int16}


class CubeBinning:
    """The bin of a frame, computed on the host in float64 / integers.

    ``by="photon_energy"``: ``edges`` float64 ``[B + 1]``, strictly increasing; a frame with energy ``pe`` goes
    to ``searchsorted(edges, pe, side="right") - 1``, ``pe == edges[B]`` to ``B - 1``; no energy (None / NaN)
    and an energy outside ``[edges[0], edges[B]]`` give -1 (dropped).

    ``by="gevt"``: ``table`` is a 1-D integer array with values -1 .. B - 1, ``B = nbins`` or ``max + 1``; a
    frame goes to ``table[gevt]``, a ``gevt`` outside the table is dropped."""

    def __init__(self, by: str, edges=None, table=None, nbins: Optional[int] = None):
        if by not in BY:
            raise ValueError(f"cube: by must be one of {', '.join(BY)}, got {by!r}")
        self.by = by
        self.edges = np.zeros(0, np.float64)
        self.table = None
        self.table_sha256 = ""
        if by == "photon_energy":
            if edges is None:
                raise ValueError("cube: binning by photon energy needs bin edges")
            if table is not None:
                raise ValueError("cube: a bin table belongs to by='gevt'")
            e = np.asarray(edges)
            if e.ndim != 1 or e.size < 2 or e.dtype.kind not in "fiu":
                raise ValueError("cube: edges must be a 1-D array of at least 2 numbers")
            e = np.ascontiguousarray(e, np.float64)
            if not np.isfinite(e).all() or not (np.diff(e) > 0).all():
                raise ValueError("cube: edges must be finite and strictly increasing")
            self.nbins = validate_cube_nbins(e.size - 1, "cube")
            if nbins is not None and int(nbins) != self.nbins:
                raise ValueError(f"cube: {e.size} edges make {self.nbins} bins, not {nbins}")
            self.edges = e
        else:
            if table is None:
                raise ValueError("cube: binning by gevt needs a bin table")
            if edges is not None:
                raise ValueError("cube: bin edges belong to by='photon_energy'")
            t = np.asarray(table)
            if t.ndim != 1 or t.size < 1 or t.dtype.kind not in "iu":
                raise ValueError("cube: the bin table must be a non-empty 1-D integer array")
            t = np.ascontiguousarray(t.astype(np.int64))
            top = int(t.max())
            if nbins is None:
                if top < 0:
                    raise ValueError("cube: the bin table drops every event; give the number of bins")
                nbins = top + 1
            self.nbins = validate_cube_nbins(nbins, "cube")
            if int(t.min()) < CUBE_DROPPED or top >= self.nbins:
                raise ValueError(f"cube: the bin table has values outside -1 .. {self.nbins - 1}")
            self.table = t
            self.table_sha256 = hashlib.sha256(t.astype("<i8").tobytes()).hexdigest()

    @classmethod
    def linspace(cls, lo: float, hi: float, n: int) -> "CubeBinning":
        """``n`` equal energy bins of ``[lo, hi]``: the edges are ``np.linspace(lo, hi, n + 1)``."""
        n = validate_cube_nbins(n, "cube")
        return cls("photon_energy", edges=np.linspace(float(lo), float(hi), n + 1))

    def bin_of(self, values) -> np.ndarray:
        """int32 bins of photon energies (``by="photon_energy"``; None / NaN = none) or global event numbers
        (``by="gevt"``)."""
        if self.by == "photon_energy":
            pe = np.array([np.nan if v is None else float(v) for v in values], np.float64).reshape(-1)
            B, e = self.nbins, self.edges
            inside = (pe >= e[0]) & (pe <= e[B])   # NaN fails both
            b = np.searchsorted(e, np.where(inside, pe, e[0]), side="right") - 1
            return np.where(inside, np.minimum(b, B - 1), CUBE_DROPPED).astype(np.int32)
        g = np.array([int(v) for v in values], np.int64).reshape(-1)
        inside = (g >= 0) & (g < self.table.size)
        return np.where(inside, self.table[np.where(inside, g, 0)], CUBE_DROPPED).astype(np.int32)

    def bin_of_meta(self, meta) -> np.ndarray:
        """int32 bins of ``(rank, idx, gevt, photon_energy)`` tuples."""
        return self.bin_of([m[3] if self.by == "photon_energy" else m[2] for m in meta])


def bin_of(values, by: str = "photon_energy", edges=None, table=None, nbins: Optional[int] = None) -> np.ndarray:
    """int32 bins of photon energies or global event numbers: ``CubeBinning(by, ...).bin_of(values)``."""
    return CubeBinning(by, edges=edges, table=table, nbins=nbins).bin_of(values)


def accumulator_set_bytes(nbins: int, n: int) -> int:
    """Bytes of one accumulator set (cnt int32, sum int64, sq int64 ``[nbins, n]``)."""
    return int(nbins) * int(n) * CUBE_BYTES_PER_PIXEL


def accumulator_sets_that_fit(set_bytes: int, streams: int, budget: int) -> int:
    """How many accumulator sets -- one per consumer stream -- a consumer keeps in ``budget`` bytes:
    ``streams`` when they all fit, 1 when only one does; ValueError when one set does not fit."""
    set_bytes, streams, budget = int(set_bytes), max(1, int(streams)), int(budget)
    if set_bytes > budget:
        raise ValueError(f"cube: one accumulator set of {set_bytes} bytes does not fit the budget of {budget} bytes "
                         "(fewer bins, or a consumer per part of the scan)")
    return streams if set_bytes * streams <= budget else 1


@dataclass
class CubeStats:
    """Integer accumulators of a cube run.  ``frames`` int64 ``[B]`` (frames per bin), ``dropped`` (frames
    without a bin); ``cnt`` int32, ``sum`` / ``sq`` int64, all ``[B, n]`` with n = prod(shape): count, sum of
    q and sum of q^2 of the samples of bin b inside ``[vmin, vmax]``.  Per frame (``[N]``, N = frames.sum() +
    dropped, dropped frames included): ``rank`` / ``idx`` / ``gevt`` int64, ``photon_energy`` float64 (NaN =
    none) and ``bin`` int16 (-1 = dropped).  ``edges`` float64 ``[B + 1]`` with ``by == "photon_energy"``
    (else empty), ``table_sha256`` with ``by == "gevt"`` (else empty)."""
    detector: str
    layout: str
    shape: tuple
    vmin: float
    vmax: float
    frac_bits: int
    by: str
    nbins: int
    edges: np.ndarray
    table_sha256: str
    frames: np.ndarray
    dropped: int
    cnt: np.ndarray
    sum: np.ndarray
    sq: np.ndarray
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    bin: np.ndarray = None
    max_frames: int = field(init=False)

    def __post_init__(self):
        self.detector, self.layout, self.by = str(self.detector), str(self.layout), str(self.by)
        self.table_sha256 = str(self.table_sha256)
        self.shape = tuple(int(s) for s in self.shape)
        self.vmin, self.vmax, self.frac_bits, _thr, _Q, self.max_frames = validate_powder_params(
            self.vmin, self.vmax, self.frac_bits, 0.0, "cube")
        if self.by not in BY:
            raise ValueError(f"cube: by = {self.by!r}")
        self.nbins = validate_cube_nbins(int(self.nbins), "cube")
        self.dropped = int(self.dropped)
        B, n = self.nbins, int(np.prod(self.shape))
        self.edges = np.ascontiguousarray(np.zeros(0) if self.edges is None else self.edges, np.float64).reshape(-1)
        if self.edges.size != (B + 1 if self.by == "photon_energy" else 0):
            raise ValueError(f"cube: {self.edges.size} edges for {B} bins by {self.by}")
        if (self.by == "gevt") != bool(self.table_sha256):
            raise ValueError("cube: a table hash is given iff the bins come from a table")
        self.frames = np.ascontiguousarray(self.frames, np.int64).reshape(-1)
        N = int(self.frames.sum()) + self.dropped
        if self.frames.shape != (B,) or (self.frames < 0).any() or self.dropped < 0 or N > self.max_frames:
            raise ValueError(f"cube: frames {self.frames.tolist()} + {self.dropped} dropped outside {B} bins of a run "
                             f"of at most max_frames = {self.max_frames}")
        shapes = {"cnt": (B, n), "sum": (B, n), "sq": (B, n), "rank": (N,), "idx": (N,), "gevt": (N,),
                  "photon_energy": (N,), "bin": (N,)}
        for k, shp in shapes.items():
            v = getattr(self, k)
            a = np.zeros(shp, _DTYPES[k]) if v is None else np.asarray(v)
            if k in PER_FRAME and a.dtype != _DTYPES[k]:
                a = a.astype(_DTYPES[k])   # lists of Python numbers
            if a.dtype != _DTYPES[k]:
                raise ValueError(f"cube: {k} is {a.dtype}, expected {np.dtype(_DTYPES[k])}")
            if a.shape != shp:
                raise ValueError(f"cube: {k} must be {list(shp)}, got {list(a.shape)}")
            setattr(self, k, np.ascontiguousarray(a))
        if N and (int(self.bin.min()) < CUBE_DROPPED or int(self.bin.max()) >= B):
            raise ValueError(f"cube: a frame's bin outside -1 .. {B - 1}")
        per_bin = np.bincount(self.bin[self.bin >= 0].astype(np.int64), minlength=B)
        if not np.array_equal(per_bin, self.frames):
            raise ValueError("cube: the per-frame rows do not add up to the frames per bin")

    @property
    def n(self) -> int:
        return int(self.cnt.shape[1])

    def key(self):
        """What two files must share to be merged (the edges bit for bit)."""
        return (self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.by, self.nbins,
                self.edges.tobytes(), self.table_sha256)

    _KEY_NAMES = ("detector", "layout", "shape", "vmin", "vmax", "frac_bits", "by", "nbins", "edges", "table_sha256")

    def _with(self, frames, dropped, cnt, s, sq, rows) -> "CubeStats":
        return CubeStats(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.by,
                         self.nbins, self.edges, self.table_sha256, frames, dropped, cnt, s, sq, **rows)

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez_compressed(f, format=np.asarray(CUBE_FORMAT), detector=np.asarray(self.detector),
                                layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                                vmin=np.float32(self.vmin), vmax=np.float32(self.vmax),
                                frac_bits=np.int64(self.frac_bits), by=np.asarray(self.by), nbins=np.int64(self.nbins),
                                edges=self.edges, table_sha256=np.asarray(self.table_sha256), frames=self.frames,
                                dropped=np.int64(self.dropped), cnt=self.cnt, sum=self.sum, sq=self.sq,
                                **{k: getattr(self, k) for k in PER_FRAME})
        return path

    @classmethod
    def load(cls, path) -> "CubeStats":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a cube file (no {', '.join(missing)})")
            if str(z["format"]) != CUBE_FORMAT:
                raise ValueError(f"{path}: cube format {str(z['format'])!r}, expected {CUBE_FORMAT!r}")
            for k, dt in _DTYPES.items():
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            return cls(str(z["detector"]), str(z["layout"]), tuple(int(s) for s in z["shape"]), float(z["vmin"]),
                       float(z["vmax"]), int(z["frac_bits"]), str(z["by"]), int(z["nbins"]), z["edges"],
                       str(z["table_sha256"]), z["frames"], int(z["dropped"]), z["cnt"], z["sum"], z["sq"],
                       **{k: z[k] for k in PER_FRAME})

    def by_gevt(self) -> "CubeStats":
        """The same run with its per-frame rows ordered by ``gevt``; ValueError for a ``gevt`` present twice."""
        order = np.argsort(self.gevt, kind="stable")
        g = self.gevt[order]
        if g.size > 1 and (g[1:] == g[:-1]).any():
            raise ValueError(f"cube: gevt {int(g[1:][g[1:] == g[:-1]][0])} is present twice")
        return self._with(self.frames, self.dropped, self.cnt, self.sum, self.sq,
                          {k: getattr(self, k)[order] for k in PER_FRAME})

    def add(self, other: "CubeStats") -> "CubeStats":
        """Exact merge of two runs of the same detector, shape, parameters and binning: the accumulators add,
        the per-frame rows of ``other`` follow this run's."""
        if other.key() != self.key():
            diff = [n for n, a, b in zip(self._KEY_NAMES, self.key(), other.key()) if a != b]
            raise ValueError(f"cube: files differ in {', '.join(diff)}")
        total = int(self.frames.sum()) + int(other.frames.sum()) + self.dropped + other.dropped
        if total > self.max_frames:
            raise ValueError(f"cube: merged run of {total} frames is longer than max_frames = {self.max_frames}")
        # a count is at most its run's frames, which the bound keeps inside an int32
        return self._with(self.frames + other.frames, self.dropped + other.dropped, self.cnt + other.cnt,
                          self.sum + other.sum, self.sq + other.sq,
                          {k: np.concatenate([getattr(self, k), getattr(other, k)]) for k in PER_FRAME})

    # ---------------------------------------------------------------- float64 views of the integers
    def _bin(self, b) -> int:
        if not 0 <= int(b) < self.nbins:
            raise ValueError(f"cube: bin {b} of {self.nbins}")
        return int(b)

    def mean(self, b: int) -> np.ndarray:
        """float64 ``sum / cnt * 2^-S`` [n] of bin ``b`` in the frames' units, NaN where ``cnt == 0``."""
        b = self._bin(b)
        cnt, s = self.cnt[b].astype(np.int64), self.sum[b]
        d = np.where(cnt > 0, cnt, 1).astype(np.float64)
        return np.where(cnt > 0, s.astype(np.float64) / d * 2.0 ** -self.frac_bits, np.nan)

    def rms(self, b: int) -> np.ndarray:
        """float64 ``sqrt(max(0, sq / cnt - (sum / cnt)^2)) * 2^-S`` [n] of bin ``b``, NaN where ``cnt == 0``.
        A pixel whose samples were all equal has rms EXACTLY 0: that is decided on the integers (the
        samples are all m iff ``sum == cnt * m`` and ``sq == m * sum``; ``|m * sum| <= cnt * Q^2`` fits an
        int64 by the run bound), not by a float64 cancellation."""
        b = self._bin(b)
        cnt, s, sq = self.cnt[b].astype(np.int64), self.sum[b], self.sq[b]
        di = np.where(cnt > 0, cnt, 1)
        d = di.astype(np.float64)
        m_int = s // di
        constant = (m_int * di == s) & (m_int * s == sq)
        m = s.astype(np.float64) / d
        var = np.maximum(0.0, sq.astype(np.float64) / d - m * m)
        return np.where(cnt > 0, np.where(constant, 0.0, np.sqrt(var)) * 2.0 ** -self.frac_bits, np.nan)

    def diff(self, b: int, ref: int) -> np.ndarray:
        """float64 ``mean(b) - mean(ref)`` [n]: the difference signal, NaN where either bin has no sample."""
        return self.mean(b) - self.mean(ref)

    def mean_energy(self) -> np.ndarray:
        """float64 ``[B]``: the mean photon energy of every bin's frames that carry one, NaN for a bin
        without such a frame.  Summed with ``math.fsum`` over the per-frame rows in ``gevt`` order, so a
        merged file gives the same bytes as one consumer's."""
        order = np.argsort(self.gevt, kind="stable")
        pe, bn = self.photon_energy[order], self.bin[order]
        out = np.full(self.nbins, np.nan)
        for b in range(self.nbins):
            v = pe[(bn == b) & ~np.isnan(pe)]
            if v.size:
                out[b] = math.fsum(v.tolist()) / v.size
        return out


def merge(paths) -> CubeStats:
    """Combine several ``--task cube --out`` files: the accumulators add to exactly what one consumer would
    have accumulated over the same frames, the per-frame rows are ordered by ``gevt``.  Raises ValueError for
    files of another detector, layout, shape, window, frac_bits, binning source, edges (bit for bit) or table
    hash, for a ``gevt`` present twice and for a merged run past ``max_frames``."""
    paths = list(paths)
    if not paths:
        raise ValueError("cube.merge: no files")
    out = None
    for p in paths:
        st = CubeStats.load(p)
        try:
            out = st if out is None else out.add(st)
        except ValueError as e:
            raise ValueError(f"cube.merge: {p}: {e}") from None
    try:
        return out.by_gevt()
    except ValueError as e:
        raise ValueError(f"cube.merge: {e}") from None


# ------------------------------------------------------------------------------------------- CLI
def _cmd_merge(a) -> int:
    try:
        st = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"cube merge: {e}", file=sys.stderr)
        return 2
    st.save(a.out)
    print(f"cube merge: {len(a.files)} files, frames={int(st.frames.sum())} binned + {st.dropped} dropped of "
          f"{st.detector} -> {a.out}")
    return 0


def _cmd_info(a) -> int:
    try:
        st = CubeStats.load(a.file)
    except (ValueError, OSError) as e:
        print(f"cube info: {e}", file=sys.stderr)
        return 2
    me = st.mean_energy()
    print(json.dumps({"detector": st.detector, "layout": st.layout, "shape": list(st.shape), "vmin": st.vmin,
                      "vmax": st.vmax, "frac_bits": st.frac_bits, "by": st.by, "nbins": st.nbins,
                      "edges": st.edges.tolist(), "table_sha256": st.table_sha256,
                      "frames": [int(f) for f in st.frames], "dropped": st.dropped, "max_frames": st.max_frames,
                      "bins_filled": int((st.frames > 0).sum()),
                      "mean_energy": [None if v != v else float(v) for v in me],
                      "samples": int(st.cnt.sum(dtype=np.int64))}, sort_keys=True))
    return 0


def _cmd_export(a) -> int:
    try:
        st = CubeStats.load(a.file)
        full = (st.nbins, *st.shape)
        mean = np.stack([st.mean(b) for b in range(st.nbins)])
        np.save(f"{a.out_prefix}_mean.npy", mean.astype(np.float32).reshape(full))
        np.save(f"{a.out_prefix}_frames.npy", st.frames)
        np.save(f"{a.out_prefix}_energy.npy", st.mean_energy())
        names = "_mean.npy, _frames.npy, _energy.npy"
        if a.ref_bin is not None:
            ref = st.mean(a.ref_bin)
            np.save(f"{a.out_prefix}_diff.npy", (mean - ref[None, :]).astype(np.float32).reshape(full))
            names += ", _diff.npy"
    except (ValueError, OSError) as e:
        print(f"cube export: {e}", file=sys.stderr)
        return 2
    print(f"cube export: {a.out_prefix}{names} of {st.nbins} bins, shape {st.shape}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.cube", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="combine several consumers' cube files (exact)")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    i = sub.add_parser("info", help="parameters, binning and frames per bin of a file, as JSON")
    i.add_argument("file")
    i.set_defaults(fn=_cmd_info)
    e = sub.add_parser("export", help="the mean image of every bin as float32 [B, *shape] .npy, frames and mean "
                                      "energy per bin")
    e.add_argument("file")
    e.add_argument("--out_prefix", required=True,
                   help="writes <prefix>_mean.npy, <prefix>_frames.npy, <prefix>_energy.npy")
    e.add_argument("--ref_bin", type=int, default=None,
                   help="also write <prefix>_diff.npy: every bin's mean minus this bin's")
    e.set_defaults(fn=_cmd_export)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
