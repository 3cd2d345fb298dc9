"""Droplet lists: what ``psana-ray-consumer --task droplets`` writes.

A droplet is a 4-connected cluster of the pixels of one panel with ``thr_low <= v <= vmax`` that holds at
least one pixel ``v >= thr_seed`` (the K-14 contract, docs/ARCHITECTURE.md).  It is kept as integers:
``label`` (its lowest linear pixel index), ``npix``, ``adu`` = sum of q, ``sy`` / ``sx`` = sum of q * row /
q * column and ``qmax``, with q = rint(v * 2^frac_bits).  :class:`DropletFrames` is a set of frames' droplet
lists with their event identity; :func:`merge` joins several consumers' files into one ordered by global
event id.

    python -m psana_ray_amd.droplets info     FILE.npz [...]
    python -m psana_ray_amd.droplets merge    A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.droplets spectrum RUN.npz --lo 0 --hi 100 --nbins 200 --out spectrum.npy
    python -m psana_ray_amd.droplets export   RUN.npz --frame 3 --adu_per_photon 10 --out map3.npy
"""
from __future__ import annotations

import argparse
import hashlib
import sys
from dataclasses import dataclass

import numpy as np

from .sparse import expand

DROPLET_FORMAT = "psana_ray_amd.droplets/1"
FLAG_OVERFLOW = 1       # more than cap droplets: ndrop is exact, nothing is stored
FLAG_PIX_OVERFLOW = 4   # more than pix_cap active pixels: nact is exact, ndrop is 0, nothing is stored
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "nact", "ndrop", "flags")
_PF_DTYPE = {"rank": np.int64, "idx": np.int64, "gevt": np.int64, "photon_energy": np.float64, "nact": np.int32,
             "ndrop": np.int32, "flags": np.uint8}
COLUMNS = ("label", "npix", "adu", "sy", "sx", "qmax")
_COL_DTYPE = {"label": np.int32, "npix": np.int32, "adu": np.int64, "sy": np.int64, "sx": np.int64, "qmax": np.int32}
_PARAMS = ("detector", "layout", "shape", "thr_low", "thr_seed", "vmax", "frac_bits", "pix_cap", "cap", "mask_sha256")


def mask_hash(shape, mask) -> str:
    """sha256 hex of the shape and the keep-mask as the kernel sees it (non-zero = keep), "" without a mask:
    files written over other pixels do not merge."""
    if mask is None:
        return ""
    m = (np.asarray(mask).reshape(-1) != 0).astype(np.uint8)
    h = hashlib.sha256()
    h.update(np.asarray(tuple(shape), np.int64).tobytes())
    h.update(m.tobytes())
    return h.hexdigest()


@dataclass
class DropletFrames:
    """N frames' droplets.  Parameters (two sets must share them to be merged): ``detector``, ``layout``,
    ``shape`` [P, H, W] of a frame, ``thr_low`` / ``thr_seed`` / ``vmax`` (float32 values), ``frac_bits``, the
    capacities ``pix_cap`` / ``cap`` and ``mask_sha256`` ("" without a mask).  Per frame: ``rank``, ``idx``,
    ``gevt`` int64, ``photon_energy`` float64, ``nact`` / ``ndrop`` int32 (exact), ``flags`` uint8.  Data:
    ``offs`` int64 [N + 1] and the six columns -- frame i's droplets at offs[i] .. offs[i + 1], label ascending."""
    detector: str
    layout: str
    shape: tuple
    thr_low: float
    thr_seed: float
    vmax: float
    frac_bits: int
    pix_cap: int
    cap: int
    mask_sha256: str = ""
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    nact: np.ndarray = None
    ndrop: np.ndarray = None
    flags: np.ndarray = None
    offs: np.ndarray = None
    label: np.ndarray = None
    npix: np.ndarray = None
    adu: np.ndarray = None
    sy: np.ndarray = None
    sx: np.ndarray = None
    qmax: np.ndarray = None

    def __post_init__(self):
        self.shape = tuple(int(s) for s in self.shape)
        if len(self.shape) == 2:
            self.shape = (1, *self.shape)
        if len(self.shape) != 3 or min(self.shape) < 1:
            raise ValueError(f"droplets: the shape must be [P, H, W] or [H, W], got {self.shape}")
        self.thr_low, self.thr_seed, self.vmax = (float(np.float32(v)) for v in (self.thr_low, self.thr_seed, self.vmax))
        self.frac_bits, self.pix_cap, self.cap = int(self.frac_bits), int(self.pix_cap), int(self.cap)
        self.mask_sha256 = str(self.mask_sha256 or "")
        for k in PER_FRAME:
            v = getattr(self, k)
            setattr(self, k, np.ascontiguousarray(np.zeros(0) if v is None else v, _PF_DTYPE[k]))
        self.offs = np.ascontiguousarray(np.zeros(1, np.int64) if self.offs is None else self.offs, np.int64)
        for k in COLUMNS:
            v = getattr(self, k)
            setattr(self, k, np.ascontiguousarray(np.zeros(0) if v is None else v, _COL_DTYPE[k]))
        N = self.gevt.size
        if any(getattr(self, k).shape != (N,) for k in PER_FRAME) or self.offs.shape != (N + 1,):
            raise ValueError(f"droplets: per-frame arrays must have one entry per frame ({N}) and offs {N + 1}")
        if self.offs[0] != 0 or bool((np.diff(self.offs) < 0).any()) \
                or any(getattr(self, k).shape != (int(self.offs[-1]),) for k in COLUMNS):
            raise ValueError("droplets: offs must start at 0 and ascend to the length of every column")
        stored = np.where(self.flags & (FLAG_OVERFLOW | FLAG_PIX_OVERFLOW), 0, self.ndrop.astype(np.int64))
        if not np.array_equal(np.diff(self.offs), stored):
            raise ValueError("droplets: offs disagree with ndrop / flags")
        if self.label.size and (int(self.label.min()) < 0 or int(self.label.max()) >= self.n):
            raise ValueError(f"droplets: label outside the frame of {self.n} elements")

    @classmethod
    def from_lists(cls, detector, layout, shape, params, mask_sha256, rank, idx, gevt, photon_energy, nact, ndrop, flags,
                   offs, columns, pix_cap=None, cap=None) -> "DropletFrames":
        """From ``ops.reference.DropletParams`` and the outputs of one or more launches (``columns``: a dict of
        the six arrays, cut at offs[-1])."""
        n = int(np.prod(shape))
        return cls(detector, layout, shape, params.thr_low, params.thr_seed, params.vmax, params.frac_bits,
                   max(1, n // 16) if pix_cap is None else pix_cap, max(1, n // 64) if cap is None else cap,
                   mask_sha256 or "", rank, idx, gevt, photon_energy, nact, ndrop, flags, offs,
                   **{k: columns[k] for k in COLUMNS})

    def __len__(self) -> int:
        return int(self.gevt.size)

    @property
    def n(self) -> int:
        return int(np.prod(self.shape))

    def params(self) -> dict:
        """What two sets must share to be merged."""
        return {k: (list(self.shape) if k == "shape" else getattr(self, k)) for k in _PARAMS}

    def _range(self, i):
        i = range(len(self))[i]
        return int(self.offs[i]), int(self.offs[i + 1])

    def frame(self, i: int) -> dict:
        """The six columns of frame i (views); empty for an overflowed frame."""
        a, b = self._range(i)
        return {k: getattr(self, k)[a:b] for k in COLUMNS}

    def com(self, i: int):
        """``(panel int64, y float64, x float64)`` of frame i's droplets: the charge-weighted centre ``sy / adu``,
        ``sx / adu`` in panel coordinates (NaN where adu == 0) and the panel of ``label``."""
        a, b = self._range(i)
        adu = self.adu[a:b].astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            y = np.where(adu != 0, self.sy[a:b] / adu, np.nan)
            x = np.where(adu != 0, self.sx[a:b] / adu, np.nan)
        return self.label[a:b].astype(np.int64) // (self.shape[1] * self.shape[2]), y, x

    def energy(self) -> np.ndarray:
        """Every droplet's summed charge in ADU: float64 ``adu * 2^-frac_bits`` (exact below 2^53)."""
        return self.adu.astype(np.float64) * 2.0 ** -self.frac_bits

    def photons(self, adu_per_photon: float, offset: float = 0.5) -> np.ndarray:
        """``floor(energy / adu_per_photon + offset)`` per droplet, int64."""
        if not (np.isfinite(adu_per_photon) and adu_per_photon > 0):
            raise ValueError(f"droplets: adu_per_photon must be finite and positive, got {adu_per_photon}")
        return np.floor(self.energy() / float(adu_per_photon) + float(offset)).astype(np.int64)

    def spectrum(self, lo: float, hi: float, nbins: int) -> np.ndarray:
        """int64 [nbins]: droplets of the run per bin of energy over [lo, hi) (bin = floor((e - lo) * nbins /
        (hi - lo)); outside the range: not counted).  Integer counts of per-droplet values: files merged in any
        order give the same spectrum."""
        nbins = int(nbins)
        if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi and nbins >= 1):
            raise ValueError(f"droplets: spectrum needs finite lo < hi and nbins >= 1, got {lo}, {hi}, {nbins}")
        e = self.energy()
        b = np.floor((e - float(lo)) * (nbins / (float(hi) - float(lo)))).astype(np.int64)
        ok = (e >= lo) & (e < hi) & (b >= 0) & (b < nbins)
        return np.bincount(b[ok], minlength=nbins).astype(np.int64)

    def photon_map(self, i: int, adu_per_photon: float, offset: float = 0.5) -> np.ndarray:
        """int32 array of ``shape``: every droplet's photons of frame i added at its rounded centre of mass.
        Raises ValueError for an overflowed frame."""
        j = range(len(self))[i]
        if self.flags[j] & (FLAG_OVERFLOW | FLAG_PIX_OVERFLOW):
            raise ValueError(f"droplets: frame {j} (gevt {int(self.gevt[j])}) overflowed its capacity: nothing was stored")
        a, b = self._range(j)
        P, H, W = self.shape
        out = np.zeros(self.n, np.int64)
        panel, y, x = self.com(j)
        k = self.photons(adu_per_photon, offset)[a:b]
        ok = np.isfinite(y) & np.isfinite(x)
        yy = np.clip(np.rint(y[ok]).astype(np.int64), 0, H - 1)
        xx = np.clip(np.rint(x[ok]).astype(np.int64), 0, W - 1)
        np.add.at(out, panel[ok] * H * W + yy * W + xx, k[ok])
        return out.astype(np.int32).reshape(self.shape)

    def select(self, order) -> "DropletFrames":
        """The frames ``order`` (indices), in that order."""
        order = np.asarray(order, np.int64).reshape(-1)
        lens = np.diff(self.offs)[order]
        offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        take = (np.concatenate([np.arange(self.offs[i], self.offs[i + 1]) for i in order])
                if order.size else np.zeros(0, np.int64)).astype(np.int64)
        return DropletFrames(**{k: getattr(self, k) for k in _PARAMS}, **{k: getattr(self, k)[order] for k in PER_FRAME},
                             offs=offs, **{k: getattr(self, k)[take] for k in COLUMNS})

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez(f, format=np.asarray(DROPLET_FORMAT), detector=np.asarray(self.detector),
                     layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                     thr_low=np.float32(self.thr_low), thr_seed=np.float32(self.thr_seed), vmax=np.float32(self.vmax),
                     frac_bits=np.int64(self.frac_bits), pix_cap=np.int64(self.pix_cap), cap=np.int64(self.cap),
                     mask_sha256=np.asarray(self.mask_sha256), **{k: getattr(self, k) for k in PER_FRAME},
                     offs=self.offs, **{k: getattr(self, k) for k in COLUMNS})
        return path

    @classmethod
    def _load_one(cls, path) -> "DropletFrames":
        with np.load(str(path), allow_pickle=False) as z:
            keys = ("format", *_PARAMS, *PER_FRAME, "offs", *COLUMNS)
            missing = [k for k in keys if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a droplet file (no {', '.join(missing)})")
            if str(z["format"]) != DROPLET_FORMAT:
                raise ValueError(f"{path}: droplet format {str(z['format'])!r}, expected {DROPLET_FORMAT!r}")
            for k, dt in (("offs", np.int64), *_COL_DTYPE.items()):
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            return cls(str(z["detector"]), str(z["layout"]), tuple(z["shape"].tolist()), float(z["thr_low"]),
                       float(z["thr_seed"]), float(z["vmax"]), int(z["frac_bits"]), int(z["pix_cap"]), int(z["cap"]),
                       str(z["mask_sha256"]), **{k: z[k] for k in PER_FRAME}, offs=z["offs"],
                       **{k: z[k] for k in COLUMNS})

    @classmethod
    def load(cls, path) -> "DropletFrames":
        """One file, a list of files, or a glob pattern: several files are concatenated in the order given."""
        paths = expand(path)
        parts = [cls._load_one(p) for p in paths]
        return parts[0] if len(parts) == 1 else concat(parts, paths)


def concat(parts, names=None) -> DropletFrames:
    """The frames of several sets with the same parameters, one after the other."""
    parts = list(parts)
    if not parts:
        raise ValueError("droplets: nothing to concatenate")
    p0 = parts[0].params()
    for k, p in enumerate(parts[1:], 1):
        if p.params() != p0:
            diff = sorted(key for key in p0 if p.params()[key] != p0[key])
            who = names[k] if names else f"set {k}"
            raise ValueError(f"droplets: {who} was written with different parameters ({', '.join(diff)})")
    lens = np.concatenate([np.diff(p.offs) for p in parts])
    return DropletFrames(**{k: getattr(parts[0], k) for k in _PARAMS},
                         **{k: np.concatenate([getattr(p, k) for p in parts]) for k in PER_FRAME},
                         offs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                         **{k: np.concatenate([getattr(p, k) for p in parts]) for k in COLUMNS})


def merge(files) -> DropletFrames:
    """Join several consumers' files (paths, lists or globs) into one set ordered by ``gevt``.  Raises
    ValueError for files written with other parameters, detector, shape or mask, and for a ``gevt`` present
    twice."""
    paths = [p for f in (files if isinstance(files, (list, tuple)) else [files]) for p in expand(f)]
    try:
        allf = concat([DropletFrames._load_one(p) for p in paths], paths)
    except ValueError as e:
        raise ValueError(f"droplets.merge: {e}") from None
    order = np.argsort(allf.gevt, kind="stable")
    g = allf.gevt[order]
    dup = g[1:][g[1:] == g[:-1]]
    if dup.size:
        raise ValueError(f"droplets.merge: gevt {int(dup[0])} is present twice ({dup.size} duplicates)")
    return allf.select(order)


def _info(df: DropletFrames, name: str) -> str:
    over = int((df.flags & (FLAG_OVERFLOW | FLAG_PIX_OVERFLOW) != 0).sum())
    return (f"{name}: frames={len(df)} stored={len(df) - over} overflowed={over} droplets={int(df.offs[-1])} "
            f"detector={df.detector} layout={df.layout} shape={'x'.join(map(str, df.shape))} thr_low={df.thr_low:g} "
            f"thr_seed={df.thr_seed:g} vmax={df.vmax:g} frac_bits={df.frac_bits} pix_cap={df.pix_cap} cap={df.cap} "
            f"mask={df.mask_sha256[:12] or 'none'}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.droplets", description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("info", help="one summary line per file")
    p.add_argument("files", nargs="+")
    p = sub.add_parser("merge", help="join files into one ordered by gevt")
    p.add_argument("files", nargs="+")
    p.add_argument("--out", required=True)
    p = sub.add_parser("spectrum", help="int64 histogram of droplet energy over the run, as .npy")
    p.add_argument("files", nargs="+")
    p.add_argument("--lo", type=float, required=True)
    p.add_argument("--hi", type=float, required=True)
    p.add_argument("--nbins", type=int, required=True)
    p.add_argument("--out", required=True)
    p = sub.add_parser("export", help="one frame's photon map (int32, the frame's shape) as .npy")
    p.add_argument("file")
    p.add_argument("--frame", type=int, default=None, help="position in the file")
    p.add_argument("--gevt", type=int, default=None, help="global event id (instead of --frame)")
    p.add_argument("--adu_per_photon", type=float, required=True)
    p.add_argument("--out", required=True)
    a = ap.parse_args(argv)
    try:
        if a.cmd == "info":
            for f in a.files:
                for path in expand(f):
                    print(_info(DropletFrames._load_one(path), path))
        elif a.cmd == "merge":
            df = merge(a.files)
            df.save(a.out)
            print(_info(df, a.out))
        elif a.cmd == "spectrum":
            df = DropletFrames.load([p for f in a.files for p in expand(f)])
            with open(a.out, "wb") as f:
                np.save(f, df.spectrum(a.lo, a.hi, a.nbins))
        else:
            df = DropletFrames.load(a.file)
            if (a.frame is None) == (a.gevt is None):
                raise ValueError("export: give --frame or --gevt")
            i = a.frame
            if i is None:
                hit = np.flatnonzero(df.gevt == a.gevt)
                if hit.size != 1:
                    raise ValueError(f"export: gevt {a.gevt} is in the file {hit.size} times")
                i = int(hit[0])
            if not -len(df) <= i < len(df):
                raise ValueError(f"export: frame {i} outside the file's {len(df)} frames")
            with open(a.out, "wb") as f:
                np.save(f, df.photon_map(i, a.adu_per_photon))
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
