"""Photon counts of a run: photons per pixel of the CALIBRATED frames, and the per-frame P(k) of up to 8 ROIs.

``psana-ray-consumer --task photons`` turns every calibrated value into a number of photons the way psana's
``det.photons`` does -- whole photons by floor of ``v / adu_per_photon``, then the fractional remainders of
neighbouring pixel pairs merged (the K-13 numerics contract, docs/ARCHITECTURE.md) -- and keeps INTEGERS:
per pixel the samples, the photons and the frames with a photon; per frame and ROI the number of pixels with
1, 2, ... 7 and >= 8 photons and the photons in all.  :class:`PhotonStats` is that result, :func:`merge` adds
several consumers' files exactly.

    python -m psana_ray_amd.photons merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.photons info RUN.npz
    python -m psana_ray_amd.photons export RUN.npz --out_prefix run
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from dataclasses import dataclass

import numpy as np

from .ops.reference import (PHOTON_MAX_FRAMES, PHOTON_PK_BINS, photon_shape, validate_photon_maps,
                            validate_photon_params)

PHOTONS_FORMAT = "psana_ray_amd.photons/1"
PARAMS = ("detector", "layout", "shape", "adu_per_photon", "inv", "vmax", "thr_seed", "thr_total", "n_roi")
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "pk", "tot")
_FIELDS = ("format", *PARAMS, "roi_npix", "roi_sha256", "frames", "cnt", "psum", "occ", *PER_FRAME)
_DTYPES = {"roi_npix": np.int64, "frames": np.int64, "cnt": np.int32, "psum": np.int64, "occ": np.int32,
           "rank": np.int32, "idx": np.int64, "gevt": np.int64, "photon_energy": np.float64, "pk": np.int32,
           "tot": np.int64}


def describe_roi(shape, mask=None, roi=None, n_roi=None):
    """``(R, roi_npix int64 [R], sha256 hex)`` of a keep-mask and ROI labels for frames of ``shape``: the kept
    pixels of every ROI (what P(0) and kbar are derived from) and a hash of the two maps as the kernel sees
    them (no mask = all kept, no labels = all ROI 0), so files counted over other pixels do not merge."""
    P, H, W = photon_shape(shape)
    n = P * H * W
    mask, roi, R = validate_photon_maps((P, H, W), mask, roi, n_roi)
    keep = np.ones(n, np.uint8) if mask is None else (mask != 0).astype(np.uint8)
    lab = np.zeros(n, np.uint8) if roi is None else roi
    npix = np.array([int(((lab == r) & (keep != 0)).sum()) for r in range(R)], np.int64)
    h = hashlib.sha256()
    h.update(np.asarray([P, H, W, R], np.int64).tobytes())
    h.update(keep.tobytes())
    h.update(lab.tobytes())
    return R, npix, h.hexdigest()


@dataclass
class PhotonStats:
    """Photon counts of a run.  Per pixel (``[n]``, n = prod(shape)): ``cnt`` int32 samples inside ``(0, vmax]``
    that the mask keeps, ``psum`` int64 photons, ``occ`` int32 frames with at least one photon.  Per frame
    (``[N]``, N == frames): ``rank`` / ``idx`` / ``gevt`` / ``photon_energy`` (NaN = none), ``pk`` int32
    ``[N, R, 8]`` (kept pixels of ROI r with k == j + 1 photons; the last bin is k >= 8) and ``tot`` int64
    ``[N, R]`` (their photons).  ``roi_npix`` int64 [R] are the kept pixels of every ROI: P(0) is derived from
    it, the device does not count empty pixels."""
    detector: str
    layout: str
    shape: tuple
    adu_per_photon: float
    vmax: float
    thr_seed: float
    thr_total: float
    n_roi: int
    roi_npix: np.ndarray
    roi_sha256: str
    frames: int
    cnt: np.ndarray
    psum: np.ndarray
    occ: np.ndarray
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    pk: np.ndarray = None
    tot: np.ndarray = None

    def __post_init__(self):
        self.detector, self.layout, self.roi_sha256 = str(self.detector), str(self.layout), str(self.roi_sha256)
        self.shape = tuple(int(s) for s in self.shape)
        n = int(np.prod(photon_shape(self.shape)))
        self.frames, self.n_roi = int(self.frames), int(self.n_roi)
        if self.frames < 0:
            raise ValueError(f"photons: {self.frames} frames")
        pp = validate_photon_params(self.adu_per_photon, self.vmax, self.thr_seed, self.thr_total, frames=self.frames)
        self.adu_per_photon, self.inv, self.vmax, self.thr_seed, self.thr_total = pp
        R = self.n_roi
        if not 1 <= R <= 8:
            raise ValueError(f"photons: {R} ROIs")
        N = self.frames
        shapes = {"roi_npix": (R,), "cnt": (n,), "psum": (n,), "occ": (n,), "rank": (N,), "idx": (N,), "gevt": (N,),
                  "photon_energy": (N,), "pk": (N, R, PHOTON_PK_BINS), "tot": (N, R)}
        for k, shp in shapes.items():
            v = getattr(self, k)
            a = np.zeros(shp, _DTYPES[k]) if v is None else np.asarray(v)
            if k in ("rank", "idx", "gevt", "photon_energy") and a.dtype != _DTYPES[k]:
                a = a.astype(_DTYPES[k])   # lists of Python numbers
            if a.dtype != _DTYPES[k]:
                raise ValueError(f"photons: {k} is {a.dtype}, expected {np.dtype(_DTYPES[k])}")
            if a.shape != shp:
                raise ValueError(f"photons: {k} must be {list(shp)}, got {list(a.shape)}")
            setattr(self, k, np.ascontiguousarray(a))
        if n and (int(self.cnt.min()) < 0 or int(self.cnt.max()) > N or int(self.occ.min()) < 0
                  or bool((self.occ > self.cnt).any()) or int(self.psum.min()) < 0):
            raise ValueError(f"photons: a pixel count outside 0 .. frames = {N}")
        if int(self.roi_npix.min()) < 0 or int(self.roi_npix.sum()) > n:
            raise ValueError("photons: roi_npix outside the frame")
        if N and (int(self.pk.min()) < 0 or bool((self.pk.sum(axis=2, dtype=np.int64) > self.roi_npix).any())):
            raise ValueError("photons: a frame counts more pixels than its ROI has")

    @classmethod
    def from_maps(cls, detector, layout, shape, params, mask, roi, n_roi, frames, cnt, psum, occ, **per_frame):
        """Built from the maps themselves (``params``: ops.reference.PhotonParams)."""
        R, npix, sha = describe_roi(shape, mask, roi, n_roi)
        return cls(detector, layout, shape, params.adu_per_photon, params.vmax, params.thr_seed, params.thr_total, R,
                   npix, sha, frames, cnt, psum, occ, **per_frame)

    @property
    def n(self) -> int:
        return int(self.cnt.shape[0])

    def key(self):
        """What two files must share to be merged."""
        return (self.detector, self.layout, self.shape, self.adu_per_photon, self.vmax, self.thr_seed, self.thr_total,
                self.n_roi, self.roi_sha256)

    _KEY_NAMES = ("detector", "layout", "shape", "adu_per_photon", "vmax", "thr_seed", "thr_total", "n_roi",
                  "roi_sha256")

    def save(self, path) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            np.savez_compressed(f, format=np.asarray(PHOTONS_FORMAT), detector=np.asarray(self.detector),
                                layout=np.asarray(self.layout), shape=np.asarray(self.shape, np.int64),
                                adu_per_photon=np.float32(self.adu_per_photon), inv=np.float32(self.inv),
                                vmax=np.float32(self.vmax), thr_seed=np.float32(self.thr_seed),
                                thr_total=np.float32(self.thr_total), n_roi=np.int64(self.n_roi),
                                roi_npix=self.roi_npix, roi_sha256=np.asarray(self.roi_sha256),
                                frames=np.int64(self.frames), cnt=self.cnt, psum=self.psum, occ=self.occ,
                                **{k: getattr(self, k) for k in PER_FRAME})
        return path

    @classmethod
    def load(cls, path) -> "PhotonStats":
        with np.load(str(path), allow_pickle=False) as z:
            missing = [k for k in _FIELDS if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a photon-statistics file (no {', '.join(missing)})")
            if str(z["format"]) != PHOTONS_FORMAT:
                raise ValueError(f"{path}: photon-statistics format {str(z['format'])!r}, expected {PHOTONS_FORMAT!r}")
            for k, dt in _DTYPES.items():
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            st = cls(str(z["detector"]), str(z["layout"]), tuple(int(s) for s in z["shape"]),
                     float(z["adu_per_photon"]), float(z["vmax"]), float(z["thr_seed"]), float(z["thr_total"]),
                     int(z["n_roi"]), z["roi_npix"], str(z["roi_sha256"]), int(z["frames"]), z["cnt"], z["psum"],
                     z["occ"], **{k: z[k] for k in PER_FRAME})
            if np.float32(z["inv"]) != np.float32(st.inv):
                raise ValueError(f"{path}: inv = {float(z['inv'])!r} is not float32(1 / adu_per_photon) = {st.inv!r}")
            return st

    def select(self, order) -> "PhotonStats":
        """The same run with its per-frame rows in another order (a permutation)."""
        order = np.asarray(order, np.int64)
        if order.shape != (self.frames,) or not np.array_equal(np.sort(order), np.arange(self.frames)):
            raise ValueError("photons: select needs a permutation of the frames")
        return PhotonStats(self.detector, self.layout, self.shape, self.adu_per_photon, self.vmax, self.thr_seed,
                           self.thr_total, self.n_roi, self.roi_npix, self.roi_sha256, self.frames, self.cnt,
                           self.psum, self.occ, **{k: getattr(self, k)[order] for k in PER_FRAME})

    def add(self, other: "PhotonStats") -> "PhotonStats":
        """Exact merge: the accumulators add, the per-frame rows of ``other`` follow this run's."""
        if other.key() != self.key():
            diff = [n for n, a, b in zip(self._KEY_NAMES, self.key(), other.key()) if a != b]
            raise ValueError(f"photons: files differ in {', '.join(diff)}")
        total = self.frames + other.frames
        if total > PHOTON_MAX_FRAMES:
            raise ValueError(f"photons: merged run of {total} frames is longer than {PHOTON_MAX_FRAMES}")
        # cnt and occ are at most their run's frames, so the int32 sums cannot wrap
        return PhotonStats(self.detector, self.layout, self.shape, self.adu_per_photon, self.vmax, self.thr_seed,
                           self.thr_total, self.n_roi, self.roi_npix, self.roi_sha256, total, self.cnt + other.cnt,
                           self.psum + other.psum, self.occ + other.occ,
                           **{k: np.concatenate([getattr(self, k), getattr(other, k)]) for k in PER_FRAME})

    # ---------------------------------------------------------------- float64 views of the integers
    def mean_photons(self) -> np.ndarray:
        """float64 ``psum / cnt`` [n]: photons per sample, NaN where the pixel had no sample."""
        d = np.where(self.cnt > 0, self.cnt, 1).astype(np.float64)
        return np.where(self.cnt > 0, self.psum.astype(np.float64) / d, np.nan)

    def occupancy(self) -> np.ndarray:
        """float64 ``occ / cnt`` [n]: the fraction of samples with at least one photon, NaN without samples."""
        d = np.where(self.cnt > 0, self.cnt, 1).astype(np.float64)
        return np.where(self.cnt > 0, self.occ.astype(np.float64) / d, np.nan)

    def _roi(self, roi: int) -> int:
        if not 0 <= int(roi) < self.n_roi:
            raise ValueError(f"photons: ROI {roi} of {self.n_roi}")
        return int(roi)

    def pk_table(self, roi: int = 0) -> np.ndarray:
        """int64 ``[N, 9]``: per frame the kept pixels of the ROI with 0, 1, ... 7 and >= 8 photons; column 0
        is derived, ``roi_npix - sum_j pk``."""
        r = self._roi(roi)
        pk = self.pk[:, r, :].astype(np.int64)
        return np.concatenate([(self.roi_npix[r] - pk.sum(axis=1))[:, None], pk], axis=1)

    def kbar(self, roi: int = 0) -> np.ndarray:
        """float64 ``tot / roi_npix`` [N]: mean photons per kept pixel of the ROI, NaN for an empty ROI."""
        r = self._roi(roi)
        npix = int(self.roi_npix[r])
        return self.tot[:, r].astype(np.float64) / npix if npix else np.full(self.frames, np.nan)


def merge(paths) -> PhotonStats:
    """Combine several ``--task photons --out`` files: the accumulators add to exactly what one consumer would
    have counted over the same frames, the per-frame rows are ordered by ``gevt``.  Raises ValueError for files
    of other parameters, detector, shape or ROI hash, for a ``gevt`` present twice and for a merged run past
    2^31 - 1 frames."""
    paths = list(paths)
    if not paths:
        raise ValueError("photons.merge: no files")
    out = None
    for p in paths:
        st = PhotonStats.load(p)
        try:
            out = st if out is None else out.add(st)
        except ValueError as e:
            raise ValueError(f"photons.merge: {p}: {e}") from None
    order = np.argsort(out.gevt, kind="stable")
    g = out.gevt[order]
    dup = g[1:][g[1:] == g[:-1]]
    if dup.size:
        raise ValueError(f"photons.merge: gevt {int(dup[0])} is present twice ({dup.size} duplicates)")
    return out.select(order)


# ------------------------------------------------------------------------------------------- CLI
def _summary(st: PhotonStats) -> dict:
    return {"detector": st.detector, "layout": st.layout, "shape": list(st.shape),
            "adu_per_photon": st.adu_per_photon, "inv": st.inv, "vmax": st.vmax, "thr_seed": st.thr_seed,
            "thr_total": st.thr_total, "n_roi": st.n_roi, "roi_npix": [int(v) for v in st.roi_npix],
            "roi_sha256": st.roi_sha256, "frames": st.frames, "samples": int(st.cnt.sum(dtype=np.int64)),
            "photons": int(st.psum.sum()), "pixels_without_sample": int((st.cnt == 0).sum()),
            "photons_per_roi": [int(v) for v in st.tot.sum(axis=0)] if st.frames else [0] * st.n_roi}


def _cmd_merge(a) -> int:
    try:
        st = merge(a.files)
    except (ValueError, OSError) as e:
        print(f"photons merge: {e}", file=sys.stderr)
        return 2
    st.save(a.out)
    print(f"photons merge: {len(a.files)} files, frames={st.frames} photons={int(st.psum.sum())} of {st.detector} "
          f"-> {a.out}")
    return 0


def _cmd_info(a) -> int:
    try:
        st = PhotonStats.load(a.file)
    except (ValueError, OSError) as e:
        print(f"photons info: {e}", file=sys.stderr)
        return 2
    print(json.dumps(_summary(st), sort_keys=True))
    return 0


def _cmd_export(a) -> int:
    try:
        st = PhotonStats.load(a.file)
        for name, arr in (("mean_photons", st.mean_photons()), ("occupancy", st.occupancy())):
            with open(f"{a.out_prefix}_{name}.npy", "wb") as f:
                np.save(f, arr.reshape(st.shape))
    except (ValueError, OSError) as e:
        print(f"photons export: {e}", file=sys.stderr)
        return 2
    print(f"photons export: {a.out_prefix}_mean_photons.npy, _occupancy.npy, shape {st.shape}")
    return 0


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.photons", description=__doc__,
                                 formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    m = sub.add_parser("merge", help="add several consumers' photon-statistics files (exact), rows by gevt")
    m.add_argument("files", nargs="+")
    m.add_argument("--out", required=True)
    m.set_defaults(fn=_cmd_merge)
    i = sub.add_parser("info", help="parameters, frames and photon counts of a file, as JSON")
    i.add_argument("file")
    i.set_defaults(fn=_cmd_info)
    e = sub.add_parser("export", help="mean photons per sample and occupancy as frame-shaped float64 .npy files")
    e.add_argument("file")
    e.add_argument("--out_prefix", required=True, help="writes <prefix>_mean_photons.npy and <prefix>_occupancy.npy")
    e.set_defaults(fn=_cmd_export)
    a = ap.parse_args(argv)
    return a.fn(a)


if __name__ == "__main__":
    sys.exit(main())
