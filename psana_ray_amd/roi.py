"""Per-frame statistics of rectangular regions of interest (ROIs) of the CALIBRATED frames.

``psana-ray-consumer --task roi`` keeps, for every frame and each of up to 16 rectangles, a small record of
INTEGERS (the K-16 numerics contract, docs/ARCHITECTURE.md): the pixels inside the value window, their sum,
the first moments in y and x, the maximum with its position and, when asked for, the projections of the
rectangle onto its x and y axes -- the integrated intensity of a Bragg spot or a beam monitor as a time
series, the position of a beam, one emission spectrum per shot.  :class:`RoiSet` is the set of rectangles,
:class:`RoiFrames` the result, :func:`merge` joins several consumers' files.

    python -m psana_ray_amd.roi merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.roi info RUN.npz
    python -m psana_ray_amd.roi export RUN.npz --out_prefix run
"""
from __future__ import annotations

import argparse
import hashlib
import json
import re
import sys
from dataclasses import dataclass

import numpy as np

from .ops.reference import (ROI_ROW_WORDS, photon_shape, roi_key_decode, roi_offsets, validate_roi_params,
                            validate_roi_proj, validate_roi_rects)

ROI_FORMAT = "psana_ray_amd.roi/1"
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "npix", "sum", "sy", "sx", "qmax", "imax", "proj_x", "proj_y")
_HEADER = ("format", "detector", "layout", "shape", "vmin", "vmax", "frac_bits", "proj", "rects", "rects_sha256",
           "mask_sha256", "offx", "offy")
_FIELDS = (*_HEADER, *PER_FRAME)
_DTYPES = {"rects": np.int32, "offx": np.int64, "offy": np.int64, "rank": np.int64, "idx": np.int64, "gevt": np.int64,
           "photon_energy": np.float64, "npix": np.int32, "sum": np.int64, "sy": np.int64, "sx": np.int64,
           "qmax": np.int32, "imax": np.int32, "proj_x": np.int64, "proj_y": np.int64}
_SPEC3 = re.compile(r"^\s*(\d+)\s*,\s*(\d+)\s*:\s*(\d+)\s*,\s*(\d+)\s*:\s*(\d+)\s*$")
_SPEC2 = re.compile(r"^\s*(\d+)\s*:\s*(\d+)\s*,\s*(\d+)\s*:\s*(\d+)\s*$")


def mask_sha256(shape, mask=None) -> str:
    """A hash of the keep-mask as the kernel sees it (no mask = all kept), so files taken over other pixels do
    not merge."""
    P, H, W = photon_shape(shape, "roi")
    n = P * H * W
    if mask is None:
        keep = np.ones(n, np.uint8)
    else:
        m = np.asarray(mask)
        if m.size != n:
            raise ValueError(f"roi: mask of {m.size} elements for frames of {n}")
        keep = (m.reshape(-1) != 0).astype(np.uint8)
    h = hashlib.sha256()
    h.update(np.asarray([P, H, W], np.int64).tobytes())
    h.update(keep.tobytes())
    return h.hexdigest()


class RoiSet:
    """The rectangles of a run for frames of ``shape`` ([P, H, W], or [H, W]: one panel): ``rects`` int32
    [R, 5] rows (p, y0, y1, x0, x1), half-open, validated."""

    def __init__(self, rects, shape):
        self.frame_shape = tuple(int(s) for s in shape)
        self.phw = photon_shape(self.frame_shape, "roi")
        a = np.asarray(rects)
        if a.ndim == 2 and a.shape[1] == 4 and np.issubdtype(a.dtype, np.integer):
            if len(self.frame_shape) != 2:
                raise ValueError(f"roi: rectangles without a panel (Y0:Y1,X0:X1) need 2-D frames, these are "
                                 f"{self.frame_shape}")
            a = np.concatenate([np.zeros((a.shape[0], 1), a.dtype), a], axis=1)
        self.rects = validate_roi_rects(a, self.phw, "roi")
        self.offx, self.offy = roi_offsets(self.rects)

    @staticmethod
    def parse_spec(spec: str, ndim: int):
        """One ``P,Y0:Y1,X0:X1`` (3-D frames) or ``Y0:Y1,X0:X1`` (2-D frames) as (p, y0, y1, x0, x1)."""
        m3, m2 = _SPEC3.match(str(spec)), _SPEC2.match(str(spec))
        if m3 is None and m2 is None:
            raise ValueError(f"roi: malformed rectangle {spec!r}; expected P,Y0:Y1,X0:X1 (or Y0:Y1,X0:X1 for 2-D frames)")
        if ndim == 3 and m3 is None:
            raise ValueError(f"roi: rectangle {spec!r} names no panel, but the frames are 3-D: use P,Y0:Y1,X0:X1")
        if ndim == 2 and m2 is None:
            raise ValueError(f"roi: rectangle {spec!r} names a panel, but the frames are 2-D: use Y0:Y1,X0:X1")
        v = [int(g) for g in (m3 or m2).groups()]
        if any(t >= 2 ** 31 for t in v):
            raise ValueError(f"roi: rectangle {spec!r} is out of range")
        return tuple(v) if m3 is not None else (0, *v)

    @classmethod
    def from_specs(cls, specs, shape) -> "RoiSet":
        specs = list(specs)
        if not specs:
            raise ValueError("roi: no rectangle")
        shape = tuple(int(s) for s in shape)
        if len(shape) not in (2, 3):
            raise ValueError(f"roi: frames of shape {shape}; 2-D or 3-D frames are possible")
        rows = np.asarray([cls.parse_spec(s, len(shape)) for s in specs], np.int64)
        return cls(rows if len(shape) == 3 else rows[:, 1:], shape)

    @classmethod
    def from_file(cls, path, shape) -> "RoiSet":
        """An int ``[R, 5]`` (or ``[R, 4]`` for 2-D frames) ``.npy`` file."""
        try:
            a = np.load(str(path), allow_pickle=False)
        except (OSError, ValueError) as e:
            raise ValueError(f"roi: cannot read {path}: {e}") from None
        if a.ndim != 2 or a.shape[1] not in (4, 5) or not np.issubdtype(a.dtype, np.integer):
            raise ValueError(f"roi: {path} holds {a.dtype} {list(a.shape)}, expected an integer [R, 5] or [R, 4] array")
        return cls(a, shape)

    @property
    def R(self) -> int:
        return int(self.rects.shape[0])

    @property
    def sha256(self) -> str:
        """A hash of the rectangles as the kernel sees them."""
        h = hashlib.sha256()
        h.update(np.asarray(self.phw, np.int64).tobytes())
        h.update(np.ascontiguousarray(self.rects, np.int32).tobytes())
        return h.hexdigest()

    def row_bytes(self, proj="none") -> int:
        """What one frame's record costs on the host: the device row and the projections."""
        wx, wy = validate_roi_proj(proj, "roi")
        return self.R * ROI_ROW_WORDS * 8 + 8 * (int(self.offx[-1]) * wx + int(self.offy[-1]) * wy)


@dataclass
class RoiFrames:
    """ROI records of a run, one row per frame (``[N]``): ``rank`` / ``idx`` / ``gevt`` int64, ``photon_energy``
    float64 (NaN = none); per rectangle (``[N, R]``) ``npix`` int32, ``sum`` / ``sy`` / ``sx`` int64 (of q =
    rint(v * 2^frac_bits)), ``qmax`` / ``imax`` int32 (INT32_MIN and -1 without a sample; imax is the LOWEST
    linear frame index of the maximum); ``proj_x`` int64 [N, Lx] / ``proj_y`` int64 [N, Ly], the rectangles'
    column / row sums one after the other at ``offx`` / ``offy`` (zero columns for an axis not selected)."""
    detector: str
    layout: str
    shape: tuple
    vmin: float
    vmax: float
    frac_bits: int
    proj: str
    rects: np.ndarray
    mask_sha256: str
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    npix: np.ndarray = None
    sum_: np.ndarray = None
    sy: np.ndarray = None
    sx: np.ndarray = None
    qmax: np.ndarray = None
    imax: np.ndarray = None
    proj_x: np.ndarray = None
    proj_y: np.ndarray = None

    def __post_init__(self):
        self.detector, self.layout, self.mask_sha256 = str(self.detector), str(self.layout), str(self.mask_sha256)
        self.shape = tuple(int(s) for s in self.shape)
        self.roiset = RoiSet(self.rects, self.shape)
        self.rects = self.roiset.rects
        self.rects_sha256 = self.roiset.sha256
        self.offx, self.offy = self.roiset.offx, self.roiset.offy
        self.vmin, self.vmax, self.frac_bits, _Q = validate_roi_params(self.vmin, self.vmax, self.frac_bits,
                                                                       self.rects, "roi")
        self.proj = "none" if self.proj is None else str(self.proj)
        wx, wy = validate_roi_proj(self.proj, "roi")
        R = self.roiset.R
        g = self.gevt if self.gevt is not None else ()
        N = int(np.asarray(g).shape[0])
        Lx, Ly = int(self.offx[-1]) * wx, int(self.offy[-1]) * wy
        shapes = {"rank": (N,), "idx": (N,), "gevt": (N,), "photon_energy": (N,), "npix": (N, R), "sum": (N, R),
                  "sy": (N, R), "sx": (N, R), "qmax": (N, R), "imax": (N, R), "proj_x": (N, Lx), "proj_y": (N, Ly)}
        for k, shp in shapes.items():
            attr = "sum_" if k == "sum" else k
            v = getattr(self, attr)
            a = np.zeros(shp, _DTYPES[k]) if v is None else np.asarray(v)
            if k in ("rank", "idx", "gevt", "photon_energy") and a.dtype != _DTYPES[k]:
                a = a.astype(_DTYPES[k])   # lists of Python numbers
            if a.dtype != _DTYPES[k]:
                raise ValueError(f"roi: {k} is {a.dtype}, expected {np.dtype(_DTYPES[k])}")
            if a.shape != shp:
                raise ValueError(f"roi: {k} must be {list(shp)}, got {list(a.shape)}")
            setattr(self, attr, np.ascontiguousarray(a))

    # ---------------------------------------------------------------- construction
    @classmethod
    def from_rows(cls, detector, layout, shape, vmin, vmax, frac_bits, proj, rects, mask_sha, rows, proj_x=None,
                  proj_y=None, **meta) -> "RoiFrames":
        """Built from device rows: ``rows`` int64 [N, R, 8] (npix, sum, sy, sx, key, 0, 0, 0)."""
        rows = np.asarray(rows)
        if rows.ndim != 3 or rows.shape[2] != ROI_ROW_WORDS or rows.dtype != np.int64:
            raise ValueError(f"roi: rows must be int64 [N, R, {ROI_ROW_WORDS}], got {rows.dtype} {list(rows.shape)}")
        qmax, imax = roi_key_decode(rows[:, :, 4])
        return cls(detector, layout, shape, vmin, vmax, frac_bits, proj, rects, mask_sha,
                   npix=rows[:, :, 0].astype(np.int32), sum_=rows[:, :, 1].copy(), sy=rows[:, :, 2].copy(),
                   sx=rows[:, :, 3].copy(), qmax=qmax.reshape(rows.shape[:2]), imax=imax.reshape(rows.shape[:2]),
                   proj_x=proj_x, proj_y=proj_y, **meta)

    @property
    def frames(self) -> int:
        return int(self.gevt.shape[0])

    @property
    def R(self) -> int:
        return self.roiset.R

    def key(self):
        """What two files must share to be merged."""
        return (self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.proj,
                self.rects_sha256, self.mask_sha256)

    _KEY_NAMES = ("detector", "layout", "shape", "vmin", "vmax", "frac_bits", "proj", "rects_sha256", "mask_sha256")

    def _arr(self, k):
        return getattr(self, "sum_" if k == "sum" else k)

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez_compressed(f, format=np.asarray(ROI_FORMAT), detector=np.asarray(self.detector),
                                layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                                vmin=np.float32(self.vmin), vmax=np.float32(self.vmax),
                                frac_bits=np.int64(self.frac_bits), proj=np.asarray(self.proj), rects=self.rects,
                                rects_sha256=np.asarray(self.rects_sha256), mask_sha256=np.asarray(self.mask_sha256),
                                offx=self.offx, offy=self.offy, **{k: self._arr(k) for k in PER_FRAME})
        return path

    @classmethod
    def load(cls, path) -> "RoiFrames":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not an ROI file (no {', '.join(missing)})")
            if str(z["format"]) != ROI_FORMAT:
                raise ValueError(f"{path}: ROI format {str(z['format'])!r}, expected {ROI_FORMAT!r}")
            for k, dt in _DTYPES.items():
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            st = cls(str(z["detector"]), str(z["layout"]), tuple(int(s) for s in z["shape"]), float(z["vmin"]),
                     float(z["vmax"]), int(z["frac_bits"]), str(z["proj"]), z["rects"], str(z["mask_sha256"]),
                     **{("sum_" if k == "sum" else k): z[k] for k in PER_FRAME})
            if str(z["rects_sha256"]) != st.rects_sha256:
                raise ValueError(f"{path}: rects_sha256 does not match the rectangles")
            if not (np.array_equal(z["offx"], st.offx) and np.array_equal(z["offy"], st.offy)):
                raise ValueError(f"{path}: offx / offy do not match the rectangles")
            return st

    def select(self, order) -> "RoiFrames":
        """The same run with its rows in another order (a permutation)."""
        order = np.asarray(order, np.int64)
        if order.shape != (self.frames,) or not np.array_equal(np.sort(order), np.arange(self.frames)):
            raise ValueError("roi: select needs a permutation of the frames")
        return RoiFrames(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.proj,
                         self.rects, self.mask_sha256,
                         **{("sum_" if k == "sum" else k): self._arr(k)[order] for k in PER_FRAME})

    def add(self, other: "RoiFrames") -> "RoiFrames":
        """The rows of ``other`` after this run's."""
        if other.key() != self.key():
            diff = [n for n, a, b in zip(self._KEY_NAMES, self.key(), other.key()) if a != b]
            raise ValueError(f"roi: files differ in {', '.join(diff)}")
        return RoiFrames(self.detector, self.layout, self.shape, self.vmin, self.vmax, self.frac_bits, self.proj,
                         self.rects, self.mask_sha256,
                         **{("sum_" if k == "sum" else k): np.concatenate([self._arr(k), other._arr(k)])
                            for k in PER_FRAME})

    # ---------------------------------------------------------------- per-ROI views of the integers
    def _r(self, r: int) -> int:
        if not 0 <= int(r) < self.R:
            raise ValueError(f"roi: rectangle {r} of {self.R}")
        return int(r)

    @property
    def _unit(self) -> float:
        return 2.0 ** -self.frac_bits

    def sum(self, r: int) -> np.ndarray:
        """float64 [N]: the sum of the rectangle's values, ``sum * 2^-S``."""
        return self.sum_[:, self._r(r)].astype(np.float64) * self._unit

    def mean(self, r: int) -> np.ndarray:
        """float64 [N]: the mean value per counted pixel, NaN where none counted."""
        r = self._r(r)
        n = self.npix[:, r]
        return np.where(n > 0, self.sum_[:, r].astype(np.float64) * self._unit / np.where(n > 0, n, 1), np.nan)

    def max(self, r: int) -> np.ndarray:
        """float64 [N]: the largest value, ``qmax * 2^-S``; NaN where no pixel counted."""
        r = self._r(r)
        return np.where(self.npix[:, r] > 0, self.qmax[:, r].astype(np.float64) * self._unit, np.nan)

    def argmax(self, r: int) -> np.ndarray:
        """int64 [N, 3]: (p, y, x) of the maximum (the lowest index among equals); -1 where no pixel counted."""
        r = self._r(r)
        _P, H, W = self.roiset.phw
        i = self.imax[:, r].astype(np.int64)
        out = np.stack([i // (H * W), (i // W) % H, i % W], axis=1)
        out[i < 0] = -1
        return out

    def com(self, r: int) -> np.ndarray:
        """float64 [N, 2]: the centre of mass (y, x) = (sy / sum, sx / sum) inside the panel; NaN where sum == 0."""
        r = self._r(r)
        s = self.sum_[:, r]
        d = np.where(s != 0, s, 1).astype(np.float64)
        return np.stack([np.where(s != 0, self.sy[:, r] / d, np.nan), np.where(s != 0, self.sx[:, r] / d, np.nan)], axis=1)

    def _proj(self, r: int, axis: str) -> np.ndarray:
        r = self._r(r)
        if axis not in ("x", "y"):
            raise ValueError(f"roi: projection axis {axis!r}; x or y")
        if not validate_roi_proj(self.proj, "roi")[axis == "y"]:
            raise ValueError(f"roi: the run kept no {axis} projection (proj = {self.proj})")
        off, a = (self.offx, self.proj_x) if axis == "x" else (self.offy, self.proj_y)
        return a[:, int(off[r]):int(off[r + 1])]

    def projection(self, r: int, axis: str) -> np.ndarray:
        """float64 [N, len]: per frame the rectangle's sum over y per column (``axis`` "x") or over x per row ("y")."""
        return self._proj(r, axis).astype(np.float64) * self._unit

    def run_projection(self, r: int, axis: str) -> np.ndarray:
        """int64 [len]: the projection summed over the frames, exact (in units of 2^-S)."""
        return self._proj(r, axis).sum(axis=0, dtype=np.int64)


def merge(paths) -> RoiFrames:
    """Join several ``--task roi --out`` files: the rows ordered by ``gevt``, exactly what one consumer would have
    written for the same frames.  Raises ValueError for files of another detector, layout, shape, window,
    frac_bits, proj, rectangle hash or mask hash, and for a ``gevt`` present twice."""
    paths = list(paths)
    if not paths:
        raise ValueError("roi.merge: no files")
    out = None
    for p in paths:
        st = RoiFrames.load(p)
        try:
            out = st if out is None else out.add(st)
        except ValueError as e:
            raise ValueError(f"roi.merge: {p}: {e}") from None
    order = np.argsort(out.gevt, kind="stable")
    g = out.gevt[order]
    dup = g[1:][g[1:] == g[:-1]]
    if dup.size:
        raise ValueError(f"roi.merge: gevt {int(dup[0])} is present twice ({dup.size} duplicates)")
    return out.select(order)


# ------------------------------------------------------------------------------------------- CLI
def _summary(st: RoiFrames) -> dict:
    return {"detector": st.detector, "layout": st.layout, "shape": list(st.shape), "vmin": st.vmin, "vmax": st.vmax,
            "frac_bits": st.frac_bits, "proj": st.proj, "rois": st.R, "rects": st.rects.tolist(),
            "rects_sha256": st.rects_sha256, "mask_sha256": st.mask_sha256, "frames": st.frames,
            "row_bytes": st.roiset.row_bytes(st.proj),
            "sum_per_roi": [float(st.sum(r).sum()) for r in range(st.R)]}


def _cmd_merge(a) -> int:
    try:
        st = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"roi merge: {e}", file=sys.stderr)
        return 2
    st.save(a.out)
    print(f"roi merge: {len(a.files)} files, frames={st.frames} rois={st.R} of {st.detector} -> {a.out}")
    return 0


def _cmd_info(a) -> int:
    try:
        st = RoiFrames.load(a.file)
    except (ValueError, OSError) as e:
        print(f"roi info: {e}", file=sys.stderr)
        return 2
    print(json.dumps(_summary(st), sort_keys=True))
    return 0


def _cmd_export(a) -> int:
    try:
        st = RoiFrames.load(a.file)
        names = ["sum", "com"]
        arrs = {"sum": np.stack([st.sum(r) for r in range(st.R)], axis=1),
                "com": np.stack([st.com(r) for r in range(st.R)], axis=1)}
        for axis in ("x", "y"):
            if validate_roi_proj(st.proj, "roi")[axis == "y"]:
                for r in range(st.R):
                    arrs[f"proj_{axis}_r{r}"] = st.projection(r, axis)
                    names.append(f"proj_{axis}_r{r}")
        for name in names:
            with open(f"{a.out_prefix}_{name}.npy", "wb") as f:
                np.save(f, arrs[name])
    except (ValueError, OSError) as e:
        print(f"roi export: {e}", file=sys.stderr)
        return 2
    print(f"roi export: {', '.join(f'{a.out_prefix}_{n}.npy' for n in names)}; {st.frames} frames, {st.R} rois")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.roi", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="join several consumers' ROI files, rows by gevt")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    i = sub.add_parser("info", help="parameters, rectangles and frames of a file, as JSON")
    i.add_argument("file")
    i.set_defaults(fn=_cmd_info)
    e = sub.add_parser("export", help="sums, centres of mass and projections as float64 .npy files")
    e.add_argument("file")
    e.add_argument("--out_prefix", required=True,
                   help="writes <prefix>_sum.npy [N, R], <prefix>_com.npy [N, R, 2] and <prefix>_proj_x_r<k>.npy / "
                        "_proj_y_r<k>.npy [N, len] for the axes the run kept")
    e.set_defaults(fn=_cmd_export)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
