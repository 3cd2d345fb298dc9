"""Sparse (zero-suppressed) frames: what ``psana-ray-consumer --task sparse`` writes.

A frame is kept as the (pixel index, value) pairs of its pixels with ``thr <= v <= vmax`` (the K-10
contract, docs/ARCHITECTURE.md): linear indices into the frame of ``shape``, ascending, and bit copies
of the float32 values.  :class:`SparseFrames` is a set of such frames with their event identity,
:func:`merge` joins several consumers' files into one ordered by global event id.

    python -m psana_ray_amd.sparse info  FILE.npz [...]
    python -m psana_ray_amd.sparse merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.sparse dense RUN.npz --frame 3 --out frame3.npy
"""
from __future__ import annotations

import argparse
import glob as _glob
import json
import os
import sys
from dataclasses import dataclass, field

import numpy as np

SPARSE_FORMAT = "psana_ray_amd.sparse/1"
FLAG_OVERFLOW = 1   # the frame had more than cap kept pixels: nnz is exact, nothing is stored
FLAG_SKIPPED = 2    # the frame failed the hit filter (min_peaks): it was not looked at
DEFAULT_THR = 20.0            # the peak finder's default threshold
DEFAULT_VMAX = float(2 ** 20)
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "nnz", "flags")


def default_cap(n: int) -> int:
    """Pixels per frame a consumer reserves when ``--sparse_cap`` is not given: n // 16 (6.25 %)."""
    return max(1, int(n) // 16)


@dataclass
class SparseFrames:
    """N sparse frames.  Parameters (two sets must share them to be merged): ``detector``, ``layout``
    ("calib" / "image"), ``shape`` of a dense frame, the window ``thr`` / ``vmax``, the per-frame
    capacity ``cap``, the hit filter ``min_peaks`` (0 = none) and the peak finder's parameters used for
    it (``peak_params``, a dict; empty without a filter).  Per frame: ``rank``, ``idx``, ``gevt`` int64,
    ``photon_energy`` float64 (NaN = none), ``nnz`` int32 (exact, also for an overflowed frame),
    ``flags`` uint8 (FLAG_OVERFLOW, FLAG_SKIPPED).  Data: ``offs`` int64 [N + 1], ``pix`` int32 and
    ``val`` float32 [offs[N]] -- frame i's pairs at offs[i] .. offs[i + 1]."""
    detector: str
    layout: str
    shape: tuple
    thr: float
    vmax: float
    cap: int
    min_peaks: int = 0
    peak_params: dict = field(default_factory=dict)
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    nnz: np.ndarray = None
    flags: np.ndarray = None
    offs: np.ndarray = None
    pix: np.ndarray = None
    val: np.ndarray = None

    def __post_init__(self):
        self.shape = tuple(int(s) for s in self.shape)
        self.thr, self.vmax = float(np.float32(self.thr)), float(np.float32(self.vmax))
        self.cap, self.min_peaks = int(self.cap), int(self.min_peaks)
        self.peak_params = {str(k): float(v) for k, v in dict(self.peak_params or {}).items()}
        e = np.zeros(0, np.int64)
        self.rank = np.ascontiguousarray(e if self.rank is None else self.rank, np.int64)
        self.idx = np.ascontiguousarray(e if self.idx is None else self.idx, np.int64)
        self.gevt = np.ascontiguousarray(e if self.gevt is None else self.gevt, np.int64)
        self.photon_energy = np.ascontiguousarray(np.zeros(0) if self.photon_energy is None else self.photon_energy,
                                                  np.float64)
        self.nnz = np.ascontiguousarray(e if self.nnz is None else self.nnz, np.int32)
        self.flags = np.ascontiguousarray(e if self.flags is None else self.flags, np.uint8)
        self.offs = np.ascontiguousarray(np.zeros(1, np.int64) if self.offs is None else self.offs, np.int64)
        self.pix = np.ascontiguousarray(e if self.pix is None else self.pix, np.int32)
        self.val = np.ascontiguousarray(np.zeros(0, np.float32) if self.val is None else self.val, np.float32)
        N = self.gevt.size
        if any(getattr(self, k).shape != (N,) for k in PER_FRAME) or self.offs.shape != (N + 1,):
            raise ValueError(f"sparse: per-frame arrays must have one entry per frame ({N}) and offs {N + 1}")
        if self.offs[0] != 0 or bool((np.diff(self.offs) < 0).any()) or self.pix.shape != (int(self.offs[-1]),) \
                or self.val.shape != self.pix.shape:
            raise ValueError("sparse: offs must start at 0 and ascend to the length of pix and val")
        stored = np.where(self.flags & (FLAG_OVERFLOW | FLAG_SKIPPED), 0, self.nnz.astype(np.int64))
        if not np.array_equal(np.diff(self.offs), stored):
            raise ValueError("sparse: offs disagree with nnz / flags")
        n = int(np.prod(self.shape))
        if self.pix.size and (int(self.pix.min()) < 0 or int(self.pix.max()) >= n):
            raise ValueError(f"sparse: pixel index outside the frame of {n} elements")

    def __len__(self) -> int:
        return int(self.gevt.size)

    @property
    def n(self) -> int:
        return int(np.prod(self.shape))

    def params(self) -> dict:
        """What two sets must share to be merged."""
        return {"detector": self.detector, "layout": self.layout, "shape": list(self.shape), "thr": self.thr,
                "vmax": self.vmax, "cap": self.cap, "min_peaks": self.min_peaks, "peak_params": self.peak_params}

    def frame(self, i: int):
        """``(pix int32 [k], val float32 [k])`` of frame i (views); empty for a skipped or overflowed frame."""
        i = range(len(self))[i]
        a, b = int(self.offs[i]), int(self.offs[i + 1])
        return self.pix[a:b], self.val[a:b]

    def to_dense(self, i: int) -> np.ndarray:
        """Frame i as a float32 array of ``shape``: the kept values, +0 elsewhere.  Raises ValueError for
        an overflowed frame (its pixels were not stored; a skipped frame gives zeros)."""
        i = range(len(self))[i]
        if self.flags[i] & FLAG_OVERFLOW:
            raise ValueError(f"sparse: frame {i} (gevt {int(self.gevt[i])}) overflowed its capacity "
                             f"({int(self.nnz[i])} > {self.cap} pixels): nothing was stored")
        out = np.zeros(self.n, np.float32)
        p, v = self.frame(i)
        out[p] = v
        return out.reshape(self.shape)

    def select(self, order) -> "SparseFrames":
        """The frames ``order`` (indices), in that order."""
        order = np.asarray(order, np.int64).reshape(-1)
        lens = np.diff(self.offs)[order]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = (np.concatenate([np.arange(self.offs[i], self.offs[i + 1]) for i in order])
                if order.size else np.zeros(0, np.int64)).astype(np.int64)
        return SparseFrames(**{k: getattr(self, k) for k in ("detector", "layout", "shape", "thr", "vmax", "cap",
                                                             "min_peaks", "peak_params")},
                            **{k: getattr(self, k)[order] for k in PER_FRAME}, offs=offs, pix=self.pix[take],
                            val=self.val[take])

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez(f, format=np.asarray(SPARSE_FORMAT), detector=np.asarray(self.detector),
                     layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                     thr=np.float32(self.thr), vmax=np.float32(self.vmax), cap=np.int64(self.cap),
                     min_peaks=np.int64(self.min_peaks),
                     peak_params=np.asarray(json.dumps(self.peak_params, sort_keys=True)),
                     rank=self.rank, idx=self.idx, gevt=self.gevt, photon_energy=self.photon_energy, nnz=self.nnz,
                     flags=self.flags, offs=self.offs, pix=self.pix, val=self.val)
        return path

    @classmethod
    def _load_one(cls, path) -> "SparseFrames":
        with np.load(str(path), allow_pickle=False) as z:
            keys = ("format", "detector", "layout", "shape", "thr", "vmax", "cap", "min_peaks", "peak_params",
                    *PER_FRAME, "offs", "pix", "val")
            missing = [k for k in keys if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a sparse-frames file (no {', '.join(missing)})")
            if str(z["format"]) != SPARSE_FORMAT:
                raise ValueError(f"{path}: sparse-frames format {str(z['format'])!r}, expected {SPARSE_FORMAT!r}")
            for k, dt in (("pix", np.int32), ("val", np.float32), ("offs", np.int64)):
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            return cls(str(z["detector"]), str(z["layout"]), tuple(z["shape"].tolist()), float(z["thr"]),
                       float(z["vmax"]), int(z["cap"]), int(z["min_peaks"]), json.loads(str(z["peak_params"])),
                       **{k: z[k] for k in PER_FRAME}, offs=z["offs"], pix=z["pix"], val=z["val"])

    @classmethod
    def load(cls, path) -> "SparseFrames":
        """One file, a list of files, or a glob pattern (the parts of ``--part_frames``, in name order):
        several files are concatenated in the order given."""
        paths = expand(path)
        parts = [cls._load_one(p) for p in paths]
        return parts[0] if len(parts) == 1 else concat(parts, paths)


def expand(path) -> list:
    """A path, a list of paths or a glob pattern -> the list of files (a pattern's matches sorted)."""
    if isinstance(path, (list, tuple)):
        out = [str(p) for p in path]
    else:
        path = str(path)
        out = [path] if os.path.exists(path) else sorted(_glob.glob(path))
    if not out:
        raise ValueError(f"sparse: no file matches {path!r}")
    return out


def concat(parts, names=None) -> SparseFrames:
    """The frames of several sets with the same parameters, one after the other."""
    parts = list(parts)
    if not parts:
        raise ValueError("sparse: nothing to concatenate")
    p0 = parts[0].params()
    for k, p in enumerate(parts[1:], 1):
        if p.params() != p0:
            diff = sorted(key for key in p0 if p.params()[key] != p0[key])
            who = names[k] if names else f"set {k}"
            raise ValueError(f"sparse: {who} was written with different parameters ({', '.join(diff)})")
    lens = np.concatenate([np.diff(p.offs) for p in parts]) if parts else np.zeros(0, np.int64)
    return SparseFrames(**{k: getattr(parts[0], k) for k in ("detector", "layout", "shape", "thr", "vmax", "cap",
                                                             "min_peaks", "peak_params")},
                        **{k: np.concatenate([getattr(p, k) for p in parts]) for k in PER_FRAME},
                        offs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                        pix=np.concatenate([p.pix for p in parts]), val=np.concatenate([p.val for p in parts]))


def merge(files) -> SparseFrames:
    """Join several consumers' files (paths, lists or globs) into one set ordered by ``gevt``.  Raises
    ValueError for files written with other parameters, and for a ``gevt`` present twice."""
    paths = [p for f in (files if isinstance(files, (list, tuple)) else [files]) for p in expand(f)]
    try:
        allf = concat([SparseFrames._load_one(p) for p in paths], paths)
    except ValueError as e:
        raise ValueError(f"sparse.merge: {e}") from None
    order = np.argsort(allf.gevt, kind="stable")
    g = allf.gevt[order]
    dup = g[1:][g[1:] == g[:-1]]
    if dup.size:
        raise ValueError(f"sparse.merge: gevt {int(dup[0])} is present twice ({dup.size} duplicates)")
    return allf.select(order)


def _info(sf: SparseFrames, name: str) -> str:
    stored = int(((sf.flags & (FLAG_OVERFLOW | FLAG_SKIPPED)) == 0).sum())
    return (f"{name}: frames={len(sf)} stored={stored} skipped={int((sf.flags & FLAG_SKIPPED != 0).sum())} "
            f"overflowed={int((sf.flags & FLAG_OVERFLOW != 0).sum())} pixels={int(sf.offs[-1])} "
            f"detector={sf.detector} layout={sf.layout} shape={'x'.join(map(str, sf.shape))} thr={sf.thr:g} "
            f"vmax={sf.vmax:g} cap={sf.cap} min_peaks={sf.min_peaks}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.sparse", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("info", help="one summary line per file")
    p.add_argument("files", nargs="+")
    p = sub.add_parser("merge", help="join files into one ordered by gevt")
    p.add_argument("files", nargs="+")
    p.add_argument("--out", required=True)
    p = sub.add_parser("dense", help="write one frame as a dense float32 .npy")
    p.add_argument("file")
    p.add_argument("--frame", type=int, default=None, help="position in the file")
    p.add_argument("--gevt", type=int, default=None, help="global event id (instead of --frame)")
    p.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    try:
        if a.cmd == "info":
            for f in a.files:
                for path in expand(f):
                    print(_info(SparseFrames._load_one(path), path))
        elif a.cmd == "merge":
            sf = merge(a.files)
            sf.save(a.out)
            print(_info(sf, a.out))
        else:
            sf = SparseFrames.load(a.file)
            if (a.frame is None) == (a.gevt is None):
                raise ValueError("dense: give --frame or --gevt")
            i = a.frame
            if i is None:
                hit = np.flatnonzero(sf.gevt == a.gevt)
                if hit.size != 1:
                    raise ValueError(f"dense: gevt {a.gevt} is in the file {hit.size} times")
                i = int(hit[0])
            if not -len(sf) <= i < len(sf):
                raise ValueError(f"dense: frame {i} outside the file's {len(sf)} frames")
            with open(a.out, "wb") as f:
                np.save(f, sf.to_dense(i))
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
