"""Roibin frames: what ``psana-ray-consumer --task roibin`` writes.

A kept frame is stored twice over (the K-17 contract, docs/ARCHITECTURE.md): a small LOSSLESS box of
(2R+1) x (2R+1) float32 pixels around every peak the peak finder reported, and the whole frame binned
B x B into int16 codes (``code * step`` is the block mean to within ``step / 2``; -32768 = no pixel of the
block counted).  :class:`RoibinFrames` is a set of such frames with their event identity, :func:`merge`
joins several consumers' files into one ordered by global event id.  The files are plain ``.npz`` (no
pickle); the only entropy coding is what ``np.savez_compressed`` gives.

    python -m psana_ray_amd.roibin info  FILE.npz [...]
    python -m psana_ray_amd.roibin merge A.npz B.npz --out RUN.npz
    python -m psana_ray_amd.roibin dense RUN.npz --gevt 3 --out frame3.npy
"""
from __future__ import annotations

import argparse
import hashlib
import json
import sys
from dataclasses import dataclass, field

import numpy as np

from .sparse import expand as _expand

ROIBIN_FORMAT = "psana_ray_amd.roibin/1"
FLAG_OVERFLOW = 1   # the finder met more than max_peaks peaks: which it kept is arbitrary, so no boxes
FLAG_SKIPPED = 2    # the frame failed the hit filter (min_peaks): it was neither read nor written
FLAG_BAD = 4        # a record was not a pixel of the frame (counted in nbad)
CODE_NONE = -32768
RUN_LEVEL = ("detector", "layout", "shape", "bin", "step", "inv", "vmin", "vmax", "radius", "max_peaks", "min_peaks",
             "peak_params", "mask_sha256")
PER_FRAME = ("rank", "idx", "gevt", "photon_energy", "npk", "nbox", "nbad", "nsat", "flags")
_PF_DTYPE = {"rank": np.int64, "idx": np.int64, "gevt": np.int64, "photon_energy": np.float64, "npk": np.int32,
             "nbox": np.int32, "nbad": np.int32, "nsat": np.int32, "flags": np.uint8}


def mask_sha256(mask) -> str:
    """The hash two files must share to be merged: sha256 of the keep-mask's bytes as uint8, "" without a mask."""
    if mask is None:
        return ""
    return hashlib.sha256(np.ascontiguousarray(np.asarray(mask) != 0, np.uint8).tobytes()).hexdigest()


def code_shape(shape, bin) -> tuple:
    """(P, Hb, Wb) of the codes of frames of ``shape`` ([P, H, W], or [H, W] as one panel)."""
    s = tuple(int(v) for v in shape)
    P, H, W = (1, *s) if len(s) == 2 else s
    B = int(bin)
    return P, -(-H // B), -(-W // B)


@dataclass
class RoibinFrames:
    """N roibin frames.  Run level (two sets must share it to be merged): ``detector``, ``layout``, ``shape`` of a
    dense frame, ``bin``, ``step``, ``inv`` (float32(1 / step), the scale the codes were made with), the window
    ``vmin`` / ``vmax``, the box ``radius``, ``max_peaks``, the hit filter ``min_peaks``, the peak finder's
    ``peak_params`` (a dict) and ``mask_sha256`` ("" = no mask).  Per frame: ``rank``, ``idx``, ``gevt`` int64,
    ``photon_energy`` float64, ``npk`` / ``nbox`` / ``nbad`` / ``nsat`` int32, ``flags`` uint8.  Boxes: ``offs``
    int64 [N + 1], ``ctr`` int32 [K], ``rec`` float32 [K, 8], ``box`` float32 [K, 2R+1, 2R+1] -- frame i's at
    offs[i] .. offs[i + 1], centres ascending.  Codes: ``koffs`` int64 [N + 1] (the exclusive scan of kept) and
    ``codes`` int16 [kept, P, Hb, Wb], the kept frames only."""
    detector: str
    layout: str
    shape: tuple
    bin: int
    step: float
    inv: float
    vmin: float
    vmax: float
    radius: int
    max_peaks: int
    min_peaks: int = 0
    peak_params: dict = field(default_factory=dict)
    mask_sha256: str = ""
    rank: np.ndarray = None
    idx: np.ndarray = None
    gevt: np.ndarray = None
    photon_energy: np.ndarray = None
    npk: np.ndarray = None
    nbox: np.ndarray = None
    nbad: np.ndarray = None
    nsat: np.ndarray = None
    flags: np.ndarray = None
    offs: np.ndarray = None
    ctr: np.ndarray = None
    rec: np.ndarray = None
    box: np.ndarray = None
    koffs: np.ndarray = None
    codes: np.ndarray = None

    def __post_init__(self):
        self.shape = tuple(int(s) for s in self.shape)
        if len(self.shape) not in (2, 3) or min(self.shape) < 1:
            raise ValueError(f"roibin: the shape must be [P, H, W] or [H, W], got {self.shape}")
        self.bin, self.radius = int(self.bin), int(self.radius)
        self.max_peaks, self.min_peaks = int(self.max_peaks), int(self.min_peaks)
        for k in ("step", "inv", "vmin", "vmax"):
            setattr(self, k, float(np.float32(getattr(self, k))))
        self.peak_params = {str(k): float(v) for k, v in dict(self.peak_params or {}).items()}
        self.mask_sha256 = str(self.mask_sha256)
        for k in PER_FRAME:
            v = getattr(self, k)
            setattr(self, k, np.ascontiguousarray(np.zeros(0, _PF_DTYPE[k]) if v is None else v, _PF_DTYPE[k]))
        Wn = 2 * self.radius + 1
        cs = code_shape(self.shape, self.bin)
        self.offs = np.ascontiguousarray(np.zeros(1, np.int64) if self.offs is None else self.offs, np.int64)
        self.koffs = np.ascontiguousarray(np.zeros(1, np.int64) if self.koffs is None else self.koffs, np.int64)
        self.ctr = np.ascontiguousarray(np.zeros(0, np.int32) if self.ctr is None else self.ctr, np.int32)
        self.rec = np.ascontiguousarray(np.zeros((0, 8), np.float32) if self.rec is None else self.rec, np.float32)
        self.box = np.ascontiguousarray(np.zeros((0, Wn, Wn), np.float32) if self.box is None else self.box, np.float32)
        self.codes = np.ascontiguousarray(np.zeros((0, *cs), np.int16) if self.codes is None else self.codes, np.int16)
        N = self.gevt.size
        if any(getattr(self, k).shape != (N,) for k in PER_FRAME) or self.offs.shape != (N + 1,) \
                or self.koffs.shape != (N + 1,):
            raise ValueError(f"roibin: per-frame arrays must have one entry per frame ({N}), offs and koffs {N + 1}")
        K = int(self.offs[-1])
        if self.offs[0] != 0 or not np.array_equal(np.diff(self.offs), self.nbox.astype(np.int64)) \
                or self.ctr.shape != (K,) or self.rec.shape != (K, 8) or self.box.shape != (K, Wn, Wn):
            raise ValueError("roibin: offs must be the exclusive scan of nbox, the length of ctr, rec and box")
        kept = (self.flags & FLAG_SKIPPED) == 0
        if self.koffs[0] != 0 or not np.array_equal(np.diff(self.koffs), kept.astype(np.int64)) \
                or self.codes.shape != (int(self.koffs[-1]), *cs):
            raise ValueError("roibin: koffs must be the exclusive scan of the kept frames, codes [kept, P, Hb, Wb]")
        if self.ctr.size and (int(self.ctr.min()) < 0 or int(self.ctr.max()) >= self.n):
            raise ValueError(f"roibin: a box centre outside the frame of {self.n} elements")

    def __len__(self) -> int:
        return int(self.gevt.size)

    @property
    def n(self) -> int:
        return int(np.prod(self.shape))

    def params(self) -> dict:
        """What two sets must share to be merged."""
        d = {k: getattr(self, k) for k in RUN_LEVEL}
        d["shape"] = list(self.shape)
        return d

    def boxes(self, i: int):
        """``(ctr int32 [k], rec float32 [k, 8], box float32 [k, 2R+1, 2R+1])`` of frame i (views)."""
        i = range(len(self))[i]
        a, b = int(self.offs[i]), int(self.offs[i + 1])
        return self.ctr[a:b], self.rec[a:b], self.box[a:b]

    def frame_codes(self, i: int) -> np.ndarray:
        """The codes int16 [P, Hb, Wb] of frame i (a view); ValueError for a skipped frame."""
        i = range(len(self))[i]
        if self.flags[i] & FLAG_SKIPPED:
            raise ValueError(f"roibin: frame {i} (gevt {int(self.gevt[i])}) was skipped by the hit filter "
                             f"({int(self.npk[i])} < {self.min_peaks} peaks): nothing was stored")
        return self.codes[int(self.koffs[i])]

    def to_dense(self, i: int) -> np.ndarray:
        """Frame i as a float32 array of ``shape``: every pixel float32(code) * step of its block (NaN for a block
        without a counting pixel), then the boxes copied over it bit for bit (cells outside the panel are left
        out).  ValueError for a skipped frame."""
        i = range(len(self))[i]
        codes = self.frame_codes(i)
        B, R = self.bin, self.radius
        s3 = (1, *self.shape) if len(self.shape) == 2 else self.shape
        P, H, W = s3
        val = codes.astype(np.float32) * np.float32(self.step)
        val[codes == CODE_NONE] = np.nan
        out = np.repeat(np.repeat(val, B, axis=1), B, axis=2)[:, :H, :W].copy()
        ob = out.view(np.uint32)
        ctr, _rec, box = self.boxes(i)
        bb = box.view(np.uint32)
        for j, c in enumerate(ctr.tolist()):
            p, y, x = c // (H * W), (c // W) % H, c % W
            y0, y1, x0, x1 = max(y - R, 0), min(y + R + 1, H), max(x - R, 0), min(x + R + 1, W)
            ob[p, y0:y1, x0:x1] = bb[j, y0 - (y - R):y1 - (y - R), x0 - (x - R):x1 - (x - R)]
        return out.reshape(self.shape)

    def select(self, order) -> "RoibinFrames":
        """The frames ``order`` (indices), in that order."""
        order = np.asarray(order, np.int64).reshape(-1)
        lens = np.diff(self.offs)[order]
        take = (np.concatenate([np.arange(self.offs[i], self.offs[i + 1]) for i in order])
                if order.size else np.zeros(0, np.int64)).astype(np.int64)
        kept = np.diff(self.koffs)[order]
        ktake = self.koffs[order][kept != 0]
        return RoibinFrames(**{k: getattr(self, k) for k in RUN_LEVEL},
                            **{k: getattr(self, k)[order] for k in PER_FRAME},
                            offs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64), ctr=self.ctr[take],
                            rec=self.rec[take], box=self.box[take],
                            koffs=np.concatenate([[0], np.cumsum(kept)]).astype(np.int64), codes=self.codes[ktake])

    def save(self, path, compressed: bool = False) -> str:
        path = str(path)
        with open(path, "wb") as f:   # a file object: numpy appends no suffix
            (np.savez_compressed if compressed else np.savez)(
                f, format=np.asarray(ROIBIN_FORMAT), detector=np.asarray(self.detector), layout=np.asarray(self.layout),
                shape=np.asarray(self.shape, np.int64), bin=np.int64(self.bin), step=np.float32(self.step),
                inv=np.float32(self.inv), vmin=np.float32(self.vmin), vmax=np.float32(self.vmax),
                radius=np.int64(self.radius), max_peaks=np.int64(self.max_peaks), min_peaks=np.int64(self.min_peaks),
                peak_params=np.asarray(json.dumps(self.peak_params, sort_keys=True)),
                mask_sha256=np.asarray(self.mask_sha256), **{k: getattr(self, k) for k in PER_FRAME}, offs=self.offs,
                ctr=self.ctr, rec=self.rec, box=self.box, koffs=self.koffs, codes=self.codes)
        return path

    @classmethod
    def _load_one(cls, path) -> "RoibinFrames":
        with np.load(str(path), allow_pickle=False) as z:
            keys = ("format", *RUN_LEVEL, *PER_FRAME, "offs", "ctr", "rec", "box", "koffs", "codes")
            missing = [k for k in keys if k not in z.files]
            if missing:
                raise ValueError(f"{path}: not a roibin-frames file (no {', '.join(missing)})")
            if str(z["format"]) != ROIBIN_FORMAT:
                raise ValueError(f"{path}: roibin-frames format {str(z['format'])!r}, expected {ROIBIN_FORMAT!r}")
            for k, dt in (("ctr", np.int32), ("rec", np.float32), ("box", np.float32), ("codes", np.int16),
                          ("offs", np.int64), ("koffs", np.int64)):
                if z[k].dtype != dt:
                    raise ValueError(f"{path}: {k} is {z[k].dtype}, expected {np.dtype(dt)}")
            return cls(str(z["detector"]), str(z["layout"]), tuple(z["shape"].tolist()), int(z["bin"]), float(z["step"]),
                       float(z["inv"]), float(z["vmin"]), float(z["vmax"]), int(z["radius"]), int(z["max_peaks"]),
                       int(z["min_peaks"]), json.loads(str(z["peak_params"])), str(z["mask_sha256"]),
                       **{k: z[k] for k in PER_FRAME}, offs=z["offs"], ctr=z["ctr"], rec=z["rec"], box=z["box"],
                       koffs=z["koffs"], codes=z["codes"])

    @classmethod
    def load(cls, path) -> "RoibinFrames":
        """One file, a list of files, or a glob pattern (the parts of ``--part_frames``, in name order): several
        files are concatenated in the order given."""
        paths = expand(path)
        parts = [cls._load_one(p) for p in paths]
        return parts[0] if len(parts) == 1 else concat(parts, paths)


def expand(path) -> list:
    """A path, a list of paths or a glob pattern -> the list of files (a pattern's matches sorted)."""
    try:
        return _expand(path)
    except ValueError:
        raise ValueError(f"roibin: no file matches {path!r}") from None


def concat(parts, names=None) -> RoibinFrames:
    """The frames of several sets with the same run-level fields, one after the other."""
    parts = list(parts)
    if not parts:
        raise ValueError("roibin: nothing to concatenate")
    p0 = parts[0].params()
    for k, p in enumerate(parts[1:], 1):
        if p.params() != p0:
            diff = sorted(key for key in p0 if p.params()[key] != p0[key])
            who = names[k] if names else f"set {k}"
            raise ValueError(f"roibin: {who} was written with different parameters ({', '.join(diff)})")
    lens = np.concatenate([np.diff(p.offs) for p in parts])
    kept = np.concatenate([np.diff(p.koffs) for p in parts])
    return RoibinFrames(**{k: getattr(parts[0], k) for k in RUN_LEVEL},
                        **{k: np.concatenate([getattr(p, k) for p in parts]) for k in PER_FRAME},
                        offs=np.concatenate([[0], np.cumsum(lens)]).astype(np.int64),
                        koffs=np.concatenate([[0], np.cumsum(kept)]).astype(np.int64),
                        **{k: np.concatenate([getattr(p, k) for p in parts]) for k in ("ctr", "rec", "box", "codes")})


def merge(files) -> RoibinFrames:
    """Join several consumers' files (paths, lists or globs) into one set ordered by ``gevt``.  Raises ValueError
    for files with another detector, layout, shape, parameter or mask hash, and for a ``gevt`` present twice."""
    paths = [p for f in (files if isinstance(files, (list, tuple)) else [files]) for p in expand(f)]
    try:
        allf = concat([RoibinFrames._load_one(p) for p in paths], paths)
    except ValueError as e:
        raise ValueError(f"roibin.merge: {e}") from None
    order = np.argsort(allf.gevt, kind="stable")
    g = allf.gevt[order]
    dup = g[1:][g[1:] == g[:-1]]
    if dup.size:
        raise ValueError(f"roibin.merge: gevt {int(dup[0])} is present twice ({dup.size} duplicates)")
    return allf.select(order)


def _info(rf: RoibinFrames, name: str) -> str:
    P, Hb, Wb = code_shape(rf.shape, rf.bin)
    return (f"{name}: frames={len(rf)} kept={int(rf.koffs[-1])} skipped={int((rf.flags & FLAG_SKIPPED != 0).sum())} "
            f"boxes={int(rf.offs[-1])} overflowed={int((rf.flags & FLAG_OVERFLOW != 0).sum())} "
            f"saturated={int(rf.nsat.astype(np.int64).sum())} detector={rf.detector} layout={rf.layout} "
            f"shape={'x'.join(map(str, rf.shape))} bin={rf.bin} step={rf.step:g} codes={Hb}x{Wb} radius={rf.radius} "
            f"max_peaks={rf.max_peaks} min_peaks={rf.min_peaks} mask={rf.mask_sha256[:12] or 'none'}")


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m psana_ray_amd.roibin", description=__doc__.split("\n\n")[0])
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
                    print(_info(RoibinFrames._load_one(path), path))
        elif a.cmd == "merge":
            rf = merge(a.files)
            rf.save(a.out)
            print(_info(rf, a.out))
        else:
            rf = RoibinFrames.load(a.file)
            if (a.frame is None) == (a.gevt is None):
                raise ValueError("dense: give --frame or --gevt")
            i = a.frame
            if i is None:
                hit = np.flatnonzero(rf.gevt == a.gevt)
                if hit.size != 1:
                    raise ValueError(f"dense: gevt {a.gevt} is in the file {hit.size} times")
                i = int(hit[0])
            if not -len(rf) <= i < len(rf):
                raise ValueError(f"dense: frame {i} outside the file's {len(rf)} frames")
            with open(a.out, "wb") as f:
                np.save(f, rf.to_dense(i))
    except (ValueError, OSError) as e:
        print(f"error: {e}", file=sys.stderr)
        return 2
    return 0


if __name__ == "__main__":
    sys.exit(main())
