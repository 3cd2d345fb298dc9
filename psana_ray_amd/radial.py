"""Radial-profile accumulators of ``psana-ray-consumer --task radial``: the ``.npz`` a consumer
writes, and :func:`merge`, which adds several consumers' files.

The accumulators are integers (the K-08 numerics contract, docs/ARCHITECTURE.md), so adding the
files of N consumers gives exactly -- bit for bit -- what one consumer would have accumulated over
the same frames, in any order.
"""
from __future__ import annotations

import json
from typing import Iterable, Optional

import numpy as np


def mean_profile(run_sum, run_count, frac_bits: int) -> np.ndarray:
    """float32(double(run_sum) * 2^-S / double(run_count)), +0 where run_count == 0."""
    s = np.asarray(run_sum, np.int64).astype(np.float64)
    c = np.asarray(run_count, np.int64).astype(np.float64)
    return np.where(c > 0, s * 2.0 ** -int(frac_bits) / np.where(c > 0, c, 1.0), 0.0).astype(np.float32)


def accumulator_params(binning, vmin: float, vmax: float, frac_bits: int) -> dict:
    """The parameters two accumulators must share to be added: the binning and the quantisation."""
    p = dict(binning.params())
    p.update(vmin=float(np.float32(vmin)), vmax=float(np.float32(vmax)), frac_bits=int(frac_bits))
    return p


def save(path: str, binning, vmin: float, vmax: float, frac_bits: int, run_sum, run_count, frames: int,
         records: Optional[Iterable] = None):
    """Write one consumer's accumulator.  ``records``: per batch ``(profiles [n, nbins], [(rank, idx,
    gevt), ...])`` (kept per-frame profiles)."""
    recs = list(records or [])
    meta = [m for _, ms in recs for m in ms]
    prof = (np.concatenate([np.asarray(p, np.float32).reshape(-1, binning.nbins) for p, _ in recs])
            if recs else np.zeros((0, binning.nbins), np.float32))
    np.savez(path, centers=np.asarray(binning.centers, np.float64), pixels_per_bin=np.asarray(binning.pixels_per_bin),
             run_sum=np.asarray(run_sum, np.int64), run_count=np.asarray(run_count, np.int64),
             frames=np.int64(frames), mean_profile=mean_profile(run_sum, run_count, frac_bits),
             rank=np.array([m[0] for m in meta], np.int64), idx=np.array([m[1] for m in meta], np.int64),
             gevt=np.array([m[2] for m in meta], np.int64), profiles=prof,
             params=np.array(json.dumps(accumulator_params(binning, vmin, vmax, frac_bits), sort_keys=True)))


def load_params(z) -> dict:
    return json.loads(str(z["params"]))


def merge(paths) -> dict:
    """Add the accumulators of several ``--task radial --out`` files.  Returns a dict with
    ``centers``, ``run_sum``, ``run_count``, ``frames``, ``mean_profile``, ``params`` and the
    concatenated per-frame ``rank`` / ``idx`` / ``gevt`` / ``profiles``.  Raises ValueError when the
    files' binning or quantisation parameters differ (their sums would not be comparable)."""
    paths = list(paths)
    if not paths:
        raise ValueError("radial.merge: no files")
    out = None
    for p in paths:
        with np.load(p, allow_pickle=False) as z:
            params = load_params(z)
            if out is None:
                out = {"params": params, "centers": z["centers"].copy(), "run_sum": z["run_sum"].astype(np.int64),
                       "run_count": z["run_count"].astype(np.int64), "frames": int(z["frames"]),
                       "rank": [z["rank"]], "idx": [z["idx"]], "gevt": [z["gevt"]], "profiles": [z["profiles"]]}
                continue
            if params != out["params"]:
                diff = sorted(k for k in set(params) | set(out["params"]) if params.get(k) != out["params"].get(k))
                raise ValueError(f"radial.merge: {p} was accumulated with different parameters ({', '.join(diff)})")
            out["run_sum"] = out["run_sum"] + z["run_sum"].astype(np.int64)
            out["run_count"] = out["run_count"] + z["run_count"].astype(np.int64)
            out["frames"] += int(z["frames"])
            for k in ("rank", "idx", "gevt", "profiles"):
                out[k].append(z[k])
    for k in ("rank", "idx", "gevt", "profiles"):
        out[k] = np.concatenate(out[k])
    out["mean_profile"] = mean_profile(out["run_sum"], out["run_count"], out["params"]["frac_bits"])
    return out
