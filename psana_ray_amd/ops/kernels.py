"""Validated torch-facing wrappers of the gfx950 HIP kernels (K-01..K-05, K-07..K-17).

Every wrapper checks device / dtype / shape / contiguity / alignment on the host BEFORE the
launch (a mis-shaped launch of a hand-written kernel can fault the GPU), splits batches into
launches of at most ``MAX_FRAMES`` frames, and launches on the given torch stream.
"""
from __future__ import annotations

import operator
from typing import Optional, Sequence

import torch

from . import _ext

MAX_FRAMES = 64
# int32 words of the peak finder's self-resetting scratch (csrc/peakfind.hip PfScratch)
# peak-finder scratch block per consumer stream (csrc/kernels.h kPfScratchBytes): self-resetting
# counters (1 KiB header) + every workgroup's candidate spill list for hit-rich frames (16 MiB)
PF_SCRATCH_WORDS = (1024 + 4096 * 1024 * 4) // 4


def _ptr(t: torch.Tensor) -> int:
    return int(t.data_ptr())


def _check_frames(frames: Sequence[torch.Tensor], dtype, numel: int, device, what: str):
    for t in frames:
        if t.device != device:
            raise ValueError(f"{what}: tensor on {t.device}, expected {device}")
        if t.dtype != dtype:
            raise ValueError(f"{what}: dtype {t.dtype}, expected {dtype}")
        if t.numel() != numel:
            raise ValueError(f"{what}: {t.numel()} elements, expected {numel}")
        if not t.is_contiguous():
            raise ValueError(f"{what}: tensor must be contiguous")
        if t.data_ptr() % 16:
            raise ValueError(f"{what}: tensor must be 16-byte aligned")


def _validate_index_map(idx: torch.Tensor, npix: int, what: str):
    """One-time (cached on the tensor) host check that the gather map stays inside the frame."""
    if getattr(idx, "_pr_checked_npix", None) == npix:
        return
    if idx.dtype != torch.int32 or not idx.is_contiguous() or idx.data_ptr() % 16:
        raise ValueError(f"{what}: idx must be a contiguous, 16-B aligned int32 tensor")
    if idx.numel() and (int(idx.max()) >= npix or int(idx.min()) < -1):
        raise ValueError(f"{what}: index map points outside the frame")
    idx._pr_checked_npix = npix


def _chunks(n: int):
    for i in range(0, n, MAX_FRAMES):
        yield i, min(n, i + MAX_FRAMES)


def calib_basic(raw: Sequence[torch.Tensor], out: Sequence[torch.Tensor], ped: torch.Tensor, gf: torch.Tensor,
                kind: int, stream: Optional[torch.cuda.Stream] = None):
    C = _ext.load()
    npix = ped.shape[1]
    dev = ped.device
    _check_frames(raw, torch.uint16, npix, dev, "calib_basic raw")
    _check_frames(out, torch.float32, npix, dev, "calib_basic out")
    if len(raw) != len(out):
        raise ValueError("calib_basic: raw/out length mismatch")
    s = _ext.stream_handle(stream)
    for a, b in _chunks(len(raw)):
        C.calib_basic([_ptr(t) for t in raw[a:b]], [_ptr(t) for t in out[a:b]], _ptr(ped), _ptr(gf), npix, kind, s)


def calib_image(raw, out, ped, gf, kind, idx: torch.Tensor, stream=None):
    C = _ext.load()
    npix = ped.shape[1]
    dev = ped.device
    nout = idx.numel()
    _check_frames(raw, torch.uint16, npix, dev, "calib_image raw")
    _check_frames(out, torch.float32, nout, dev, "calib_image out")
    if idx.device != dev:
        raise ValueError("calib_image: idx must be on the kernel device")
    _validate_index_map(idx, npix, "calib_image")
    s = _ext.stream_handle(stream)
    for a, b in _chunks(len(raw)):
        C.calib_image([_ptr(t) for t in raw[a:b]], [_ptr(t) for t in out[a:b]], _ptr(ped), _ptr(gf), npix, kind,
                      _ptr(idx), nout, s)


def calib_cm(raw, out, ped, gf, elig, kind, spec, cm, stream=None, ped_sg=None):
    """``ped_sg``: optional signed pedestal tables (CalibConstants.cm_signed_pedestals); the production
    shapes then read the eligibility from their sign bits instead of ``elig``."""
    C = _ext.load()
    npix = ped.shape[1]
    dev = ped.device
    _check_frames(raw, torch.uint16, npix, dev, "calib_cm raw")
    _check_frames(out, torch.float32, npix, dev, "calib_cm out")
    stride = {1: 1, 2: 2, 3: 4}[ped.shape[0]]
    if elig.dtype != torch.uint8 or elig.numel() != (npix // 8) * stride:
        raise ValueError("calib_cm: elig must be the uint8 eligibility bit-planes [npix / 8, stride] "
                         "(CalibConstants.device_tables)")
    if ped_sg is not None and (ped_sg.dtype != torch.float32 or ped_sg.shape != ped.shape or ped_sg.device != dev
                               or not ped_sg.is_contiguous()):
        raise ValueError("calib_cm: ped_sg must be a contiguous float32 table shaped like ped on its device")
    bank = cm.bank_cols or spec.bank_cols
    if C.cm_tile_cols(spec.asic_rows, spec.asic_cols, int(bank), 0, int(kind)) == 0:
        raise ValueError(f"common mode: no full-height stripe of the {spec.asic_rows}x{spec.asic_cols} ASIC "
                         f"(bank {bank}) fits in 160 KiB of LDS")
    s = _ext.stream_handle(stream)
    for a, b in _chunks(len(raw)):
        C.calib_cm([_ptr(t) for t in raw[a:b]], [_ptr(t) for t in out[a:b]], _ptr(ped), _ptr(gf), _ptr(elig), kind,
                   spec.n_panels, spec.panel_rows, spec.panel_cols, spec.asic_rows, spec.asic_cols,
                   float(cm.thr), float(cm.maxcorr), int(cm.npix_min), int(cm.flags), int(bank), s,
                   0 if ped_sg is None else _ptr(ped_sg))


def assemble(frames, out, idx: torch.Tensor, npix: int, omask: Optional[torch.Tensor] = None, stream=None):
    C = _ext.load()
    dev = idx.device
    nout = idx.numel()
    _check_frames(frames, torch.float32, npix, dev, "assemble in")
    _check_frames(out, torch.float32, nout, dev, "assemble out")
    _validate_index_map(idx, npix, "assemble")
    if omask is not None and (omask.dtype != torch.uint8 or omask.numel() != nout or omask.device != dev):
        raise ValueError("assemble: omask must be uint8[nout] on the kernel device")
    s = _ext.stream_handle(stream)
    for a, b in _chunks(len(frames)):
        C.assemble([_ptr(t) for t in frames[a:b]], [_ptr(t) for t in out[a:b]], _ptr(idx), nout,
                   0 if omask is None else _ptr(omask), s)


def peakfind(frames: Sequence[torch.Tensor], shape, params, peaks: torch.Tensor, counts: torch.Tensor,
             summary: torch.Tensor, stream=None, total: Optional[torch.Tensor] = None,
             scratch: Optional[torch.Tensor] = None):
    """frames: F tensors of ``shape`` = (P, H, W) f32.  Outputs: peaks [F, max_peaks, 8] f32,
    counts [F] int32, summary [F, 2] f32.  ``total`` (int64 scalar on the device, optional) is
    incremented by the number of peak records written.

    ``scratch``: a zero-initialised int32 tensor of PF_SCRATCH_WORDS on the frames' device, reused
    by every call on one stream.  The kernel then accumulates there and its last workgroup writes
    counts / summary whole and re-zeroes the scratch -- no fill kernel per call.  Without it, counts
    and summary are zeroed here on the stream first."""
    C = _ext.load()
    P, H, W = shape
    F = len(frames)
    if F == 0:
        return
    dev = frames[0].device
    _check_frames(frames, torch.float32, P * H * W, dev, "peakfind in")
    if peaks.shape != (F, params.max_peaks, 8) or peaks.dtype != torch.float32:
        raise ValueError("peakfind: peaks must be float32 [F, max_peaks, 8]")
    if counts.shape != (F,) or counts.dtype != torch.int32:
        raise ValueError("peakfind: counts must be int32 [F]")
    if summary.shape != (F, 2) or summary.dtype != torch.float32:
        raise ValueError("peakfind: summary must be float32 [F, 2]")
    if params.radius not in (1, 2):
        raise ValueError("peakfind: radius must be 1 or 2")
    if total is not None and (total.dtype != torch.int64 or total.numel() != 1 or total.device != dev):
        raise ValueError("peakfind: total must be an int64 scalar on the frames' device")
    if C.PF_SCRATCH_BYTES != 4 * PF_SCRATCH_WORDS:   # the kernel's spill lists would overrun the block
        raise RuntimeError(f"peakfind: PF_SCRATCH_WORDS {PF_SCRATCH_WORDS} disagrees with the extension's "
                           f"kPfScratchBytes {C.PF_SCRATCH_BYTES}")
    if scratch is not None and (scratch.dtype != torch.int32 or scratch.numel() < PF_SCRATCH_WORDS
                                or scratch.device != dev or not scratch.is_contiguous()):
        raise ValueError(f"peakfind: scratch must be a contiguous int32 [{PF_SCRATCH_WORDS}] tensor on the frames' device")
    s = _ext.stream_handle(stream)
    if scratch is None:
        with torch.cuda.stream(stream) if stream is not None else torch.cuda.stream(torch.cuda.current_stream()):
            counts.zero_()
            summary.zero_()
    for a, b in _chunks(F):
        C.peakfind([_ptr(t) for t in frames[a:b]], P, H, W, float(params.thr_peak), float(params.son_min),
                   int(params.radius), int(params.max_peaks), _ptr(peaks[a]), _ptr(counts[a:]), _ptr(summary[a]), s,
                   0 if total is None else _ptr(total), 0 if scratch is None else _ptr(scratch))


def _validate_bin_map(bins: torch.Tensor, n: int, nbins: int, dev, what: str):
    """The bin map's shape / dtype / placement, and a one-time (cached on the tensor) check that every
    entry is < nbins or 0xFFFF."""
    if bins.dtype != torch.uint16 or bins.dim() != 1 or not bins.is_contiguous() or bins.data_ptr() % 16:
        raise ValueError(f"{what}: bins must be a contiguous, 16-B aligned 1-D uint16 tensor")
    if bins.device != dev:
        raise ValueError(f"{what}: bins on {bins.device}, expected {dev}")
    if bins.numel() != n:
        raise ValueError(f"{what}: bin map of {bins.numel()} entries for frames of {n} elements")
    if getattr(bins, "_pr_checked_nbins", None) == nbins:
        return
    b = bins.view(torch.int16).to(torch.int32) & 0xFFFF
    if bool(((b >= nbins) & (b != 0xFFFF)).any()):
        raise ValueError(f"{what}: bin map entry >= nbins ({nbins}) that is not 0xFFFF")
    bins._pr_checked_nbins = nbins


def radial_profile(frames: Sequence[torch.Tensor], bins: torch.Tensor, nbins: int, sums: torch.Tensor,
                   counts: torch.Tensor, profile: torch.Tensor, vmin: float, vmax: float, frac_bits: int,
                   run: Optional[torch.Tensor] = None, stream=None):
    """K-08 radial profile (csrc/radial.hip; contract: ops.reference.radial_profile_reference).
    frames: F float32 tensors of n elements (any layout); bins: uint16 [n] on their device, 0xFFFF =
    excluded, every other entry < nbins.  Outputs (overwritten): sums int64 [F, nbins], counts int32
    [F, nbins], profile float32 [F, nbins].  ``run`` (optional): int64 [2 * nbins + 1] on the device --
    run_sum, run_count, frames -- to which the batch is ADDED (integer atomics: exact, and safe from
    several streams at once).  Everything is checked here, before any launch."""
    from .reference import radial_bound_ok

    F = len(frames)
    try:
        nbins = operator.index(nbins)   # Python and numpy integers alike
    except TypeError:
        raise ValueError(f"radial_profile: nbins must be an integer, got {nbins!r}") from None
    if not 1 <= nbins <= 4096:
        raise ValueError(f"radial_profile: nbins must be in [1, 4096], got {nbins}")
    if not 0 <= int(frac_bits) <= 60:
        raise ValueError("radial_profile: frac_bits must be in [0, 60]")
    if not float(vmin) <= float(vmax):
        raise ValueError("radial_profile: empty value window")
    if F == 0:
        return
    dev = frames[0].device
    n = frames[0].numel()
    if not 1 <= n < 2 ** 31:
        raise ValueError("radial_profile: frames must have 1 .. 2^31 - 1 elements")
    _check_frames(frames, torch.float32, n, dev, "radial_profile in")
    if not radial_bound_ok(n, vmin, vmax, frac_bits):
        raise ValueError(f"radial_profile: max(|vmin|, |vmax|) * 2^frac_bits * n must stay below 2^53 "
                         f"(window [{vmin}, {vmax}], frac_bits {frac_bits}, {n} elements)")
    _validate_bin_map(bins, n, nbins, dev, "radial_profile")
    for t, dt, name in ((sums, torch.int64, "sums"), (counts, torch.int32, "counts"), (profile, torch.float32, "profile")):
        if t.shape != (F, nbins) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"radial_profile: {name} must be a contiguous {dt} [F, nbins] tensor on {dev}")
    if run is not None and (run.dtype != torch.int64 or run.shape != (2 * nbins + 1,) or run.device != dev
                            or not run.is_contiguous()):
        raise ValueError("radial_profile: run must be a contiguous int64 [2 * nbins + 1] tensor on the frames' device")
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.radial([_ptr(t) for t in frames[a:b]], n, _ptr(bins), nbins, float(vmin), float(vmax), int(frac_bits),
                 _ptr(sums[a]), _ptr(counts[a]), _ptr(profile[a]), 0 if run is None else _ptr(run), s)


def validate_dark_window(kind, adu_lo, adu_hi, what: str = "dark_accumulate"):
    """(kind, adu_lo, adu_hi) as Python ints, or ValueError."""
    try:
        kind, adu_lo, adu_hi = operator.index(kind), operator.index(adu_lo), operator.index(adu_hi)
    except TypeError:
        raise ValueError(f"{what}: kind and the ADU window must be integers") from None
    if kind not in (0, 1, 2):
        raise ValueError(f"{what}: unknown gain kind {kind}")
    if not 0 <= adu_lo <= adu_hi <= 65535:
        raise ValueError(f"{what}: the ADU window must satisfy 0 <= lo <= hi <= 65535, got [{adu_lo}, {adu_hi}]")
    return kind, adu_lo, adu_hi


def dark_accumulate(frames: Sequence[torch.Tensor], kind: int, adu_lo: int, adu_hi: int, cnt: torch.Tensor,
                    sum: torch.Tensor, sq: torch.Tensor, frames_so_far: int = 0, stream=None):
    """K-09 dark statistics (csrc/dark.hip; contract: ops.reference.dark_accumulate_reference).
    frames: F raw uint16 tensors of n elements (any layout) on one GPU; ``kind``: DetectorSpec.kernel_kind.
    ADDS every valid sample with adu_lo <= adu <= adu_hi to cnt int32 [NC, n], sum int64 [NC, n] and
    sq int64 [NC, n] on the frames' device -- the caller zeroes them once per run and passes in
    ``frames_so_far`` the frames they already hold (the int32 count bounds a run at 2^31 - 1 frames).
    One thread owns a pixel and there are no atomics: launches in flight on DIFFERENT streams must
    not share accumulators.  Everything is checked here, before any launch."""
    from .reference import DARK_MAX_FRAMES, DARK_NC

    kind, adu_lo, adu_hi = validate_dark_window(kind, adu_lo, adu_hi)
    F = len(frames)
    try:
        frames_so_far = operator.index(frames_so_far)
    except TypeError:
        raise ValueError("dark_accumulate: frames_so_far must be an integer") from None
    if frames_so_far < 0 or frames_so_far + F > DARK_MAX_FRAMES:
        raise ValueError(f"dark_accumulate: {frames_so_far} + {F} frames would take the run past 2^31 - 1 "
                         "(the int32 count)")
    if F == 0:
        return
    dev = frames[0].device
    n = frames[0].numel()
    if dev.type != "cuda":
        raise ValueError(f"dark_accumulate: frames on {dev}, expected a GPU")
    if not 1 <= n < 2 ** 31:
        raise ValueError("dark_accumulate: frames must have 1 .. 2^31 - 1 elements")
    _check_frames(frames, torch.uint16, n, dev, "dark_accumulate in")
    nc = DARK_NC[kind]
    for t, dt, name in ((cnt, torch.int32, "cnt"), (sum, torch.int64, "sum"), (sq, torch.int64, "sq")):
        if not isinstance(t, torch.Tensor) or t.shape != (nc, n) or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"dark_accumulate: {name} must be a contiguous, 16-B aligned {dt} [{nc}, {n}] tensor "
                             f"on {dev}")
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.dark([_ptr(t) for t in frames[a:b]], n, kind, adu_lo, adu_hi, _ptr(cnt), _ptr(sum), _ptr(sq), s)


def powder_accumulate(frames: Sequence[torch.Tensor], vmin: float, vmax: float, frac_bits: int, thr_above: float,
                      nfr: torch.Tensor, cnt: torch.Tensor, sum: torch.Tensor, sq: torch.Tensor, qmax: torch.Tensor,
                      above: torch.Tensor, keys: Optional[torch.Tensor] = None, key_min: int = 0,
                      frames_so_far: int = 0, stream=None):
    """K-11 powder statistics (csrc/powder.hip; contract: ops.reference.powder_accumulate_reference).
    frames: F float32 tensors of n elements (any layout) on one GPU.  ADDS every sample with vmin <= v <=
    vmax, quantised as q = round_half_even(v * 2^frac_bits), to the planar accumulators cnt int32 / sum
    int64 / sq int64 / qmax int32 / above int32 [NC, n] and the frames per class to nfr int64 [NC], on
    the frames' device.  NC = 2 iff ``keys`` (int32 [F] on the device) is given: frame f is class 1 iff
    keys[f] >= key_min.  The caller initialises the accumulators once per run (zeros, qmax INT32_MIN) and
    passes in ``frames_so_far`` the frames they already hold: a run holds at most
    ops.reference.powder_max_frames(vmin, vmax, frac_bits) frames.  One thread owns a pixel and there
    are no atomics: launches in flight on DIFFERENT streams must not share accumulators.  Everything is
    checked here, before any launch."""
    from .reference import validate_powder_params

    what = "powder_accumulate"
    lo, hi, S, thr, _Q, max_frames = validate_powder_params(vmin, vmax, frac_bits, thr_above, what)
    F = len(frames)
    try:
        frames_so_far, key_min = operator.index(frames_so_far), operator.index(key_min)
    except TypeError:
        raise ValueError(f"{what}: frames_so_far and key_min must be integers") from None
    if not -2 ** 31 <= key_min < 2 ** 31:
        raise ValueError(f"{what}: key_min must fit an int32")
    if frames_so_far < 0 or frames_so_far + F > max_frames:
        raise ValueError(f"{what}: {frames_so_far} + {F} frames would take the run past max_frames = {max_frames} "
                         "(the int32 count and the int64 sum of squares)")
    if not isinstance(nfr, torch.Tensor) or nfr.dtype != torch.int64 or nfr.dim() != 1 or nfr.numel() not in (1, 2) \
            or not nfr.is_contiguous() or nfr.data_ptr() % 8:
        raise ValueError(f"{what}: nfr must be a contiguous int64 [NC] tensor, NC 1 or 2")
    nc = nfr.numel()
    if (keys is not None) != (nc == 2):
        raise ValueError(f"{what}: keys are given iff there are 2 classes (NC = {nc})")
    if F == 0:
        return
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    n = frames[0].numel()
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{what}: frames must have 1 .. 2^31 - 1 elements")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    if nfr.device != dev:
        raise ValueError(f"{what}: nfr on {nfr.device}, expected {dev}")
    for t, dt, name in ((cnt, torch.int32, "cnt"), (sum, torch.int64, "sum"), (sq, torch.int64, "sq"),
                        (qmax, torch.int32, "qmax"), (above, torch.int32, "above")):
        if not isinstance(t, torch.Tensor) or t.shape != (nc, n) or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-B aligned {dt} [{nc}, {n}] tensor on {dev}")
    if keys is not None and (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or keys.shape != (F,)
                             or keys.device != dev or not keys.is_contiguous()):
        raise ValueError(f"{what}: keys must be a contiguous int32 [{F}] tensor on {dev}")
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.powder([_ptr(t) for t in frames[a:b]], n, lo, hi, S, thr, nc, 0 if keys is None else _ptr(keys[a:b]),
                 key_min, _ptr(nfr), _ptr(cnt), _ptr(sum), _ptr(sq), _ptr(qmax), _ptr(above), s)


def cube_accumulate(frames: Sequence[torch.Tensor], bins, nbins: int, vmin: float, vmax: float, frac_bits: int,
                    nfr: torch.Tensor, cnt: torch.Tensor, sum: torch.Tensor, sq: torch.Tensor,
                    frames_so_far: int = 0, stream=None):
    """K-15 cube (csrc/cube.hip; contract: ops.reference.cube_accumulate_reference).  frames: F float32
    tensors of n elements (any layout) on one GPU; bins: F integers on the HOST, frame f goes to bin
    bins[f] in 0 .. nbins - 1, or is dropped (not read) with bins[f] == -1.  ADDS every sample with vmin <=
    v <= vmax, quantised as q = round_half_even(v * 2^frac_bits), to the planar accumulators cnt int32 /
    sum int64 / sq int64 [nbins, n] and the frames per bin to nfr int64 [nbins], on the frames' device; a
    bin without a frame is neither read nor written.  The caller zeroes the accumulators once per run
    and passes in ``frames_so_far`` the frames they already hold (dropped ones included): a run holds
    at most ops.reference.powder_max_frames(vmin, vmax, frac_bits) frames.  One thread owns a pixel and
    there are no atomics: launches in flight on DIFFERENT streams must not share accumulators.
    Everything is checked here, before any launch."""
    from .reference import validate_cube_bins, validate_cube_nbins, validate_powder_params

    what = "cube_accumulate"
    lo, hi, S, _thr, _Q, max_frames = validate_powder_params(vmin, vmax, frac_bits, 0.0, what)
    nbins = validate_cube_nbins(nbins, what)
    F = len(frames)
    try:
        frames_so_far = operator.index(frames_so_far)
    except TypeError:
        raise ValueError(f"{what}: frames_so_far must be an integer") from None
    if frames_so_far < 0 or frames_so_far + F > max_frames:
        raise ValueError(f"{what}: {frames_so_far} + {F} frames would take the run past max_frames = {max_frames} "
                         "(the int32 count and the int64 sum of squares)")
    blist = validate_cube_bins(bins, F, nbins, what)
    if not isinstance(nfr, torch.Tensor) or nfr.dtype != torch.int64 or nfr.shape != (nbins,) \
            or not nfr.is_contiguous() or nfr.data_ptr() % 8:
        raise ValueError(f"{what}: nfr must be a contiguous int64 [{nbins}] tensor")
    if F == 0:
        return
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    n = frames[0].numel()
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    if not 1 <= n < 2 ** 31:
        raise ValueError(f"{what}: frames must have 1 .. 2^31 - 1 elements")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    if nfr.device != dev:
        raise ValueError(f"{what}: nfr on {nfr.device}, expected {dev}")
    for t, dt, name in ((cnt, torch.int32, "cnt"), (sum, torch.int64, "sum"), (sq, torch.int64, "sq")):
        if not isinstance(t, torch.Tensor) or t.shape != (nbins, n) or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-B aligned {dt} [{nbins}, {n}] tensor on {dev}")
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.cube([_ptr(t) for t in frames[a:b]], n, lo, hi, S, nbins, blist[a:b], _ptr(nfr), _ptr(cnt), _ptr(sum),
               _ptr(sq), s)


def pixel_hist_tile_pixels(nbins: int) -> int:
    """The consecutive pixels one workgroup of the K-12 kernel owns at ``nbins`` (a power of two, 64 .. 1024):
    the sizes around it are where the kernel changes path."""
    from .reference import validate_pixel_hist_params

    return int(_ext.load().pixel_hist_tile_pixels(validate_pixel_hist_params(0.0, 1.0, nbins, what="pixel_hist_tile_pixels")[2]))


def pixel_hist(frames: Sequence[torch.Tensor], lo: float, hi: float, nbins: int, hist: torch.Tensor,
               frames_so_far: int = 0, stream=None, _layout: int = 0):
    """K-12 per-pixel histograms (csrc/pixhist.hip; contract: ops.reference.pixel_hist_reference).
    frames: F float32 tensors of n elements (any layout) on one GPU.  Every sample with lo <= v <= hi ADDS 1
    to hist[p, min(nbins - 1, floor((v - lo) * inv_w))]; ``hist`` is a contiguous, 16-B aligned int32
    [n, nbins] tensor on the frames' device that the caller zeroes once per run and whose frames so far it
    passes in ``frames_so_far``: a run holds at most 2^31 - 1 frames.  One workgroup owns a pixel and there
    are no global atomics: launches in flight on DIFFERENT streams must not share an accumulator.
    Everything is checked here, before any launch.  ``_layout`` selects an LDS layout for measurements."""
    from .reference import validate_pixel_hist_params

    what = "pixel_hist"
    F = len(frames)
    flo, fhi, nbins, inv_w = validate_pixel_hist_params(lo, hi, nbins, frames_so_far=frames_so_far, frames=F, what=what)
    if _layout not in (0, 1, 2):
        raise ValueError(f"{what}: _layout must be 0, 1 or 2")
    if not isinstance(hist, torch.Tensor) or hist.dtype != torch.int32 or hist.dim() != 2 or hist.shape[1] != nbins \
            or not hist.is_contiguous() or hist.data_ptr() % 16:
        raise ValueError(f"{what}: hist must be a contiguous, 16-B aligned int32 [n, {nbins}] tensor")
    n = int(hist.shape[0])
    validate_pixel_hist_params(lo, hi, nbins, n=n, what=what)
    if F == 0:
        return
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    if frames[0].numel() != n:
        raise ValueError(f"{what}: frames of {frames[0].numel()} elements for hist [{n}, {nbins}]")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    if hist.device != dev:
        raise ValueError(f"{what}: hist on {hist.device}, expected {dev}")
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.pixel_hist([_ptr(t) for t in frames[a:b]], n, flo, fhi, inv_w, nbins, _ptr(hist), s, _layout)


def photons_lane_pixels(W: int) -> int:
    """The consecutive pixels one lane of the K-13 kernel owns at panel width ``W``: 4, or 1 when W % 4 != 0
    (the scalar path)."""
    return int(_ext.load().photons_lane_pixels(int(W)))


def photons_block_pixels(W: int) -> int:
    """The consecutive pixels one block of lanes of the K-13 kernel owns at panel width ``W``; frames of more
    than ``photons_max_grid()`` blocks give a workgroup several.  The sizes around both are where the kernel
    changes path."""
    return int(_ext.load().photons_block_pixels(int(W)))


def photons_max_grid() -> int:
    """Workgroups of the K-13 kernel at most."""
    return int(_ext.load().photons_max_grid())


def _photon_map(t, n: int, dev, name: str, what: str, R: Optional[int] = None):
    """A keep-mask / ROI label map on the device: uint8 [n], contiguous, 16-B aligned.  Labels are validated
    against ``R`` once per tensor (the check reads the map back; the result is cached on the tensor)."""
    if t is None:
        return 0
    if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.numel() != n or t.device != dev \
            or not t.is_contiguous() or t.data_ptr() % 16:
        raise ValueError(f"{what}: {name} must be a contiguous, 16-B aligned uint8 tensor of {n} elements on {dev}")
    if R is not None and getattr(t, "_pr_checked_roi", None) != (n, R):
        if bool(((t >= R) & (t != 255)).any()):
            raise ValueError(f"{what}: a label >= n_roi = {R} other than 255")
        t._pr_checked_roi = (n, R)
    return _ptr(t)


def photons(frames: Sequence[torch.Tensor], shape, adu_per_photon, cnt: torch.Tensor, psum: torch.Tensor,
            occ: torch.Tensor, pk: torch.Tensor, tot: torch.Tensor, vmax=None, thr_seed=None, thr_total=None,
            mask: Optional[torch.Tensor] = None, roi: Optional[torch.Tensor] = None, n_roi: Optional[int] = None,
            kmap: Optional[torch.Tensor] = None, frames_so_far: int = 0, stream=None, _variant: int = 0):
    """K-13 photon counting (csrc/photons.hip; contract: ops.reference.photon_count_reference).
    frames: F float32 tensors of ``shape`` = [P, H, W] (or [H, W]) on one GPU.  ADDS per pixel the samples
    (``cnt`` int32 [n]), the photons (``psum`` int64 [n]) and the frames with a photon (``occ`` int32 [n]) to
    accumulators the caller zeroes once per run and whose frames so far it passes in ``frames_so_far`` (a run
    holds 2^31 - 1 frames); fills ``pk`` int32 [F, R, 8] and ``tot`` int64 [F, R] (cleared by the call) and,
    when given, ``kmap`` uint8 [F, n].  ``mask`` / ``roi``: uint8 [n] on the device; ``n_roi`` = R (default 1;
    labels 0 .. R - 1, 255 = none).  One lane owns a pixel: launches in flight on DIFFERENT streams must not
    share an accumulator set.  Everything is checked here, before any launch.  ``_variant`` selects a launch
    shape for measurements (bit 0: 2 frames in flight instead of 4; bits 8 and up: another grid cap)."""
    from .reference import PHOTON_MAX_ROI, PHOTON_PK_BINS, photon_shape, validate_photon_params

    what = "photons"
    F = len(frames)
    pp = validate_photon_params(adu_per_photon, vmax, thr_seed, thr_total, frames_so_far=frames_so_far, frames=F,
                                what=what)
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    try:
        R = 1 if n_roi is None else operator.index(n_roi)
    except TypeError:
        raise ValueError(f"{what}: n_roi must be an integer, got {n_roi!r}") from None
    if not 1 <= R <= PHOTON_MAX_ROI:
        raise ValueError(f"{what}: {R} ROIs; 1 .. {PHOTON_MAX_ROI} are possible")
    if roi is None and R != 1:
        raise ValueError(f"{what}: {R} ROIs need labels")
    if F == 0:
        return
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    for t, dt, name in ((cnt, torch.int32, "cnt"), (psum, torch.int64, "psum"), (occ, torch.int32, "occ")):
        if not isinstance(t, torch.Tensor) or t.shape != (n,) or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % 16:
            raise ValueError(f"{what}: {name} must be a contiguous, 16-B aligned {dt} [{n}] tensor on {dev}")
    for t, dt, shp, name in ((pk, torch.int32, (F, R, PHOTON_PK_BINS), "pk"), (tot, torch.int64, (F, R), "tot")):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shp or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % 8:
            raise ValueError(f"{what}: {name} must be a contiguous {dt} {list(shp)} tensor on {dev}")
    if kmap is not None and (not isinstance(kmap, torch.Tensor) or tuple(kmap.shape) != (F, n)
                             or kmap.dtype != torch.uint8 or kmap.device != dev or not kmap.is_contiguous()
                             or (W % 4 == 0 and kmap.data_ptr() % 4)):   # the quad path stores words
        raise ValueError(f"{what}: kmap must be a contiguous, 4-B aligned uint8 [{F}, {n}] tensor on {dev}")
    pm = _photon_map(mask, n, dev, "mask", what)
    pr = _photon_map(roi, n, dev, "roi", what, R)
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        # chunks start at multiples of 64 frames: kmap[a] stays 4-B aligned when W % 4 == 0
        C.photons([_ptr(t) for t in frames[a:b]], P, H, W, pp.inv, pp.vmax, pp.thr_seed, pp.thr_total, pm, pr, R,
                  0 if kmap is None else _ptr(kmap[a:b]), _ptr(cnt), _ptr(psum), _ptr(occ), _ptr(pk[a:b]),
                  _ptr(tot[a:b]), s, int(_variant))


def roi_strip_rows(width: int) -> int:
    """The rows of one strip (one workgroup) of a K-16 rectangle ``width`` columns wide: a taller rectangle is
    cut into several strips.  The heights around it are where the kernel changes from one workgroup to several."""
    return int(_ext.load().roi_strip_rows(int(width)))


_ROI_PLANS: dict = {}    # (device index, (P, H, W), the rectangles' bytes) -> the device plan
_ROI_PLANS_MAX = 16


def roi_plan(shape, rects, device):
    """The device plan of K-16 (csrc/roi.hip RoiPlan) for validated int32 [R, 5] rectangles on frames of
    ``shape`` = (P, H, W): built once per (device, shape, rectangles), then reused by every launch."""
    import numpy as np

    dev = torch.device(device)
    idx = torch.cuda.current_device() if dev.index is None else dev.index
    rc = np.ascontiguousarray(rects, dtype=np.int32)
    key = (idx, tuple(int(s) for s in shape), rc.tobytes(), int(_ext.load().roi_strip_pixels()))
    plan = _ROI_PLANS.get(key)
    if plan is None:
        if len(_ROI_PLANS) >= _ROI_PLANS_MAX:
            _ROI_PLANS.pop(next(iter(_ROI_PLANS)))
        P, H, W = key[1]
        plan = _ROI_PLANS[key] = _ext.load().RoiPlan(rc.reshape(-1).tolist(), P, H, W, idx)
    return plan


def roi_stats(frames: Sequence[torch.Tensor], shape, rects, vmin, vmax, frac_bits, rows: torch.Tensor,
              proj_x: Optional[torch.Tensor] = None, proj_y: Optional[torch.Tensor] = None,
              mask: Optional[torch.Tensor] = None, stream=None):
    """K-16 ROI statistics (csrc/roi.hip; contract: ops.reference.roi_stats_reference).
    frames: F float32 tensors of ``shape`` = [P, H, W] (or [H, W]) on one GPU; ``rects``: int [R, 5] of (p, y0,
    y1, x0, x1), half-open.  Fills ``rows`` int64 [F, R, 8] (npix, sum, sy, sx, key, 0, 0, 0) and, when given,
    ``proj_x`` int64 [F, Lx] / ``proj_y`` int64 [F, Ly] (the rectangles' column / row sums one after the other);
    all three are cleared by the call for its F frames.  ``mask``: uint8 [n] on the device, non-zero = keep.
    One call is complete in itself and may run on any stream.  Everything is checked here, before any launch."""
    from .reference import ROI_ROW_WORDS, photon_shape, roi_offsets, validate_roi_params, validate_roi_rects

    what = "roi_stats"
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    rc = validate_roi_rects(rects, (P, H, W), what)
    lo, hi, S, _Q = validate_roi_params(vmin, vmax, frac_bits, rc, what)
    R = rc.shape[0]
    offx, offy = roi_offsets(rc)
    F = len(frames)
    if F == 0:
        return
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    if not isinstance(rows, torch.Tensor) or tuple(rows.shape) != (F, R, ROI_ROW_WORDS) or rows.dtype != torch.int64 \
            or rows.device != dev or not rows.is_contiguous() or rows.data_ptr() % 64:
        raise ValueError(f"{what}: rows must be a contiguous, 64-B aligned int64 [{F}, {R}, {ROI_ROW_WORDS}] tensor "
                         f"on {dev}")
    for t, L, name in ((proj_x, int(offx[-1]), "proj_x"), (proj_y, int(offy[-1]), "proj_y")):
        if t is not None and (not isinstance(t, torch.Tensor) or tuple(t.shape) != (F, L) or t.dtype != torch.int64
                              or t.device != dev or not t.is_contiguous() or t.data_ptr() % 8):
            raise ValueError(f"{what}: {name} must be a contiguous int64 [{F}, {L}] tensor on {dev}")
    pm = _photon_map(mask, n, dev, "mask", what)
    plan = roi_plan((P, H, W), rc, dev)
    C = _ext.load()
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.roi([_ptr(t) for t in frames[a:b]], plan, lo, hi, S, pm, _ptr(rows[a:b]),
              0 if proj_x is None else _ptr(proj_x[a:b]), 0 if proj_y is None else _ptr(proj_y[a:b]), s)


# elements per chunk of the K-10 scan (csrc/kernels.h kSparseChunk): one directory entry per chunk
SPARSE_CHUNK = 4096


def sparsify_scratch_bytes(n: int, cap: int, frames: int) -> int:
    """Bytes of the K-10 scratch block (cursors, chunk directory, staging rows) for batches of up to
    ``frames`` frames of ``n`` elements at ``cap`` entries per frame.  Pure arithmetic (the extension's
    sparsify_scratch_bytes computes the same figure; the launcher checks the block against its own)."""
    n, cap, frames = int(n), int(cap), int(frames)
    if not 1 <= n < 2 ** 31 or not 1 <= frames <= MAX_FRAMES or cap < 1 or frames * cap >= 2 ** 31:
        raise ValueError("sparsify_scratch_bytes: n, cap or frames out of range")
    chunks = max(1, (n // 4 + SPARSE_CHUNK // 4 - 1) // (SPARSE_CHUNK // 4))
    return 256 + (chunks * frames * 8 + 15) // 16 * 16 + frames * cap * 8


def sparsify(frames: Sequence[torch.Tensor], thr: float, vmax: float, cap: int, nnz: torch.Tensor,
             flags: torch.Tensor, offs: torch.Tensor, pix: torch.Tensor, val: torch.Tensor,
             mask: Optional[torch.Tensor] = None, keys: Optional[torch.Tensor] = None, key_min: int = 0,
             scratch: Optional[torch.Tensor] = None, stream=None):
    """K-10 zero suppression (csrc/sparse.hip; contract: ops.reference.sparsify_reference).
    frames: F (1 .. 64) float32 tensors of n elements (any layout) on one GPU.  Outputs (overwritten, no
    clearing needed): nnz int32 [F], flags uint8 [F] (bit 0 overflow, bit 1 skipped), offs int64
    [F + 1], pix int32 / val float32 of at least F * cap elements -- frame f's kept pixels at
    offs[f] .. offs[f + 1]; elements from offs[F] on are unspecified.  ``mask``: uint8 [n], non-zero =
    keep.  ``keys``: int32 [F] on the device; frame f is skipped unless keys[f] >= key_min.
    ``scratch``: a contiguous, 16-B aligned tensor of at least sparsify_scratch_bytes(n, cap, F) bytes
    that no other launch in flight uses (allocated here when None).  Everything is checked here,
    before any launch."""
    from .reference import validate_sparse_params

    F = len(frames)
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"sparsify: 1 .. {MAX_FRAMES} frames per launch, got {F}")
    thr, vmax, cap = validate_sparse_params(thr, vmax, cap, F)
    try:
        key_min = operator.index(key_min)
    except TypeError:
        raise ValueError("sparsify: key_min must be an integer") from None
    if not -2 ** 31 <= key_min < 2 ** 31:
        raise ValueError("sparsify: key_min must fit an int32")
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError("sparsify: frames must be tensors")
    dev = frames[0].device
    n = frames[0].numel()
    if dev.type != "cuda":
        raise ValueError(f"sparsify: frames on {dev}, expected a GPU")
    if not 1 <= n < 2 ** 31:
        raise ValueError("sparsify: frames must have 1 .. 2^31 - 1 elements")
    _check_frames(frames, torch.float32, n, dev, "sparsify in")
    for t, dt, k, name in ((nnz, torch.int32, F, "nnz"), (flags, torch.uint8, F, "flags"),
                           (offs, torch.int64, F + 1, "offs")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.shape != (k,) or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"sparsify: {name} must be a contiguous {dt} [{k}] tensor on {dev}")
    for t, dt, name in ((pix, torch.int32, "pix"), (val, torch.float32, "val")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() < F * cap or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"sparsify: {name} must be a contiguous {dt} tensor of at least F * cap = {F * cap} "
                             f"elements on {dev}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.numel() != n
                             or mask.device != dev or not mask.is_contiguous() or _ptr(mask) % 4):
        raise ValueError(f"sparsify: mask must be a contiguous, 4-B aligned uint8 [{n}] tensor on {dev}")
    if keys is not None and (not isinstance(keys, torch.Tensor) or keys.dtype != torch.int32 or keys.numel() != F
                             or keys.device != dev or not keys.is_contiguous()):
        raise ValueError(f"sparsify: keys must be a contiguous int32 [{F}] tensor on {dev}")
    need = sparsify_scratch_bytes(n, cap, F)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != dev or not scratch.is_contiguous() \
            or _ptr(scratch) % 16 or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"sparsify: scratch must be a contiguous, 16-B aligned tensor of at least {need} bytes "
                         f"on {dev} (sparsify_scratch_bytes)")
    C = _ext.load()
    if C.SPARSE_CHUNK != SPARSE_CHUNK or C.sparsify_scratch_bytes(n, cap, F) != need:
        raise RuntimeError("sparsify: SPARSE_CHUNK / sparsify_scratch_bytes disagree with the extension")
    s = _ext.stream_handle(stream)
    C.sparsify([_ptr(t) for t in frames], n, thr, vmax, cap, 0 if mask is None else _ptr(mask),
               0 if keys is None else _ptr(keys), key_min, _ptr(nnz), _ptr(flags), _ptr(offs), _ptr(pix), _ptr(val),
               _ptr(scratch), scratch.numel() * scratch.element_size(), s)


def droplets_scratch_bytes(n: int, cap_pix: int, cap: int, frames: int) -> int:
    """Bytes of the K-14 scratch block for batches of up to ``frames`` frames of ``n`` elements at ``cap_pix``
    active pixels and ``cap`` droplets per frame: K-10's flags / offsets (1 KiB), the (frame, block) droplet
    counts (8 KiB), K-10's own scratch and 52 B per row of F * cap_pix (index, value, parent, joined, qmax and the four
    int64 accumulators).  Pure arithmetic (the extension computes the same figure;
    the launcher checks the block against its own)."""
    n, cap_pix, cap, frames = int(n), int(cap_pix), int(cap), int(frames)
    if cap < 1 or frames * cap >= 2 ** 31:
        raise ValueError("droplets_scratch_bytes: cap out of range")
    rows = (cap_pix * frames + 3) // 4 * 4
    return 1024 + MAX_FRAMES * 32 * 4 + (sparsify_scratch_bytes(n, cap_pix, frames) + 15) // 16 * 16 + 52 * rows


def droplets(frames: Sequence[torch.Tensor], shape, params, cap_pix: int, cap: int, nact: torch.Tensor,
             ndrop: torch.Tensor, flags: torch.Tensor, offs: torch.Tensor, label: torch.Tensor, npix: torch.Tensor,
             adu: torch.Tensor, sy: torch.Tensor, sx: torch.Tensor, qmax: torch.Tensor,
             mask: Optional[torch.Tensor] = None, scratch: Optional[torch.Tensor] = None, stream=None, _phases: int = 15):
    """K-14 droplets (csrc/droplets.hip; contract: ops.reference.droplet_reference).
    frames: F (1 .. 64) float32 tensors of ``shape`` = [P, H, W] (or [H, W]) on one GPU.  ``params``: a
    ``DropletParams`` or the arguments of ``validate_droplet_params``.  Outputs (overwritten, no clearing
    needed): nact / ndrop int32 [F], flags uint8 [F] (bit 0 ndrop > cap, bit 2 nact > cap_pix), offs int64
    [F + 1], and the columns label / npix / qmax int32 and adu / sy / sx int64 of at least F * cap elements --
    frame f's droplets at offs[f] .. offs[f + 1], label ascending; elements from offs[F] on are unspecified.
    ``mask``: uint8 [n], non-zero = keep.  ``scratch``: a contiguous, 16-B aligned tensor of at least
    droplets_scratch_bytes(n, cap_pix, cap, F) bytes that no other launch in flight uses (allocated here when
    None; never needs clearing).  Everything is checked here, before any launch."""
    from .reference import _droplet_params, photon_shape, validate_droplet_caps

    what = "droplets"
    F = len(frames)
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"{what}: 1 .. {MAX_FRAMES} frames per launch, got {F}")
    P, H, W = photon_shape(shape, what)
    pp = _droplet_params(params, what)
    cap_pix, cap = validate_droplet_caps((P, H, W), pp, cap_pix, cap, F, what)
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    n = P * H * W
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    for t, dt, k, name in ((nact, torch.int32, F, "nact"), (ndrop, torch.int32, F, "ndrop"),
                           (flags, torch.uint8, F, "flags"), (offs, torch.int64, F + 1, "offs")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.shape != (k,) or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dt} [{k}] tensor on {dev}")
    for t, dt, name in ((label, torch.int32, "label"), (npix, torch.int32, "npix"), (adu, torch.int64, "adu"),
                        (sy, torch.int64, "sy"), (sx, torch.int64, "sx"), (qmax, torch.int32, "qmax")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.numel() < F * cap or t.device != dev \
                or not t.is_contiguous():
            raise ValueError(f"{what}: {name} must be a contiguous {dt} tensor of at least F * cap = {F * cap} "
                             f"elements on {dev}")
    if mask is not None and (not isinstance(mask, torch.Tensor) or mask.dtype != torch.uint8 or mask.numel() != n
                             or mask.device != dev or not mask.is_contiguous() or _ptr(mask) % 4):
        raise ValueError(f"{what}: mask must be a contiguous, 4-B aligned uint8 [{n}] tensor on {dev}")
    need = droplets_scratch_bytes(n, cap_pix, cap, F)
    if scratch is None:
        scratch = torch.empty(need, dtype=torch.uint8, device=dev)
    elif not isinstance(scratch, torch.Tensor) or scratch.device != dev or not scratch.is_contiguous() \
            or _ptr(scratch) % 16 or scratch.numel() * scratch.element_size() < need:
        raise ValueError(f"{what}: scratch must be a contiguous, 16-B aligned tensor of at least {need} bytes "
                         f"on {dev} (droplets_scratch_bytes)")
    C = _ext.load()
    if C.droplets_scratch_bytes(n, cap_pix, cap, F) != need:
        raise RuntimeError("droplets: droplets_scratch_bytes disagrees with the extension")
    s = _ext.stream_handle(stream)
    C.droplets([_ptr(t) for t in frames], P, H, W, pp.thr_low, pp.thr_seed, pp.vmax, pp.frac_bits, cap_pix, cap,
               0 if mask is None else _ptr(mask), _ptr(nact), _ptr(ndrop), _ptr(flags), _ptr(offs), _ptr(label),
               _ptr(npix), _ptr(adu), _ptr(sy), _ptr(sx), _ptr(qmax), _ptr(scratch),
               scratch.numel() * scratch.element_size(), s, int(_phases))


def roibin(frames: Sequence[torch.Tensor], shape, params, peaks: torch.Tensor, counts: torch.Tensor,
           codes: torch.Tensor, npk: torch.Tensor, nbox: torch.Tensor, nbad: torch.Tensor, nsat: torch.Tensor,
           flags: torch.Tensor, offs: torch.Tensor, ctr: torch.Tensor, rec: torch.Tensor, box: torch.Tensor,
           mask: Optional[torch.Tensor] = None, stream=None, _phases: int = 3):
    """K-17 roibin (csrc/roibin.hip; contract: ops.reference.roibin_reference).
    frames: F (1 .. 64) float32 tensors of ``shape`` = [P, H, W] (or [H, W]) on one GPU; ``params``: a
    reference.RoibinParams; ``peaks`` float32 [F, max_peaks, 8] and ``counts`` int32 [F]: the peak finder's outputs
    on the device.  Outputs (overwritten, no clearing needed): ``codes`` int16 [F, P, Hb, Wb] (the rows of frames
    with counts[f] < min_peaks are NOT written), ``npk`` / ``nbox`` / ``nbad`` / ``nsat`` int32 [F], ``flags``
    uint8 [F], ``offs`` int64 [F + 1], and the box columns ``ctr`` int32 [F * max_peaks], ``rec`` float32
    [F * max_peaks, 8], ``box`` float32 [F * max_peaks, 2R+1, 2R+1] -- frame f's boxes at offs[f] .. offs[f + 1];
    rows from offs[F] on are unspecified.  ``mask``: uint8 [n], non-zero = keep.  One call is complete in itself
    and may run on any stream.  Everything is checked here, before any launch.  ``_phases`` (measurements): 1 =
    headers and codes only, 2 = the boxes of a batch just binned."""
    from .reference import RoibinParams, photon_shape, validate_roibin_params

    what = "roibin"
    if not isinstance(params, RoibinParams):
        raise ValueError(f"{what}: params must be a RoibinParams (validate_roibin_params)")
    d = params._asdict()
    d.pop("inv")
    rp = validate_roibin_params(what=what, **d)
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    B, R, MP = rp.bin, rp.radius, rp.max_peaks
    Hb, Wb = -(-H // B), -(-W // B)
    F = len(frames)
    if not 1 <= F <= MAX_FRAMES:
        raise ValueError(f"{what}: 1 .. {MAX_FRAMES} frames per launch, got {F}")
    if _phases not in (1, 2, 3):
        raise ValueError(f"{what}: _phases must be 1, 2 or 3")
    if not isinstance(frames[0], torch.Tensor):
        raise ValueError(f"{what}: frames must be tensors")
    dev = frames[0].device
    if dev.type != "cuda":
        raise ValueError(f"{what}: frames on {dev}, expected a GPU")
    _check_frames(frames, torch.float32, n, dev, f"{what} in")
    Wn = 2 * R + 1
    for t, dt, shp, al, name in ((peaks, torch.float32, (F, MP, 8), 4, "peaks"), (counts, torch.int32, (F,), 4, "counts"),
                                 (codes, torch.int16, (F, P, Hb, Wb), 8, "codes"), (npk, torch.int32, (F,), 4, "npk"),
                                 (nbox, torch.int32, (F,), 4, "nbox"), (nbad, torch.int32, (F,), 4, "nbad"),
                                 (nsat, torch.int32, (F,), 4, "nsat"), (flags, torch.uint8, (F,), 1, "flags"),
                                 (offs, torch.int64, (F + 1,), 8, "offs"), (ctr, torch.int32, (F * MP,), 4, "ctr"),
                                 (rec, torch.float32, (F * MP, 8), 4, "rec"),
                                 (box, torch.float32, (F * MP, Wn, Wn), 4, "box")):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shp or t.dtype != dt or t.device != dev \
                or not t.is_contiguous() or t.data_ptr() % al:
            raise ValueError(f"{what}: {name} must be a contiguous, {al}-B aligned {dt} {list(shp)} tensor on {dev}")
    pm = _photon_map(mask, n, dev, "mask", what)
    C = _ext.load()
    if C.ROIBIN_MAX_PEAKS < MP or C.ROIBIN_MAX_RADIUS < R:
        raise RuntimeError(f"{what}: max_peaks / radius limits disagree with the extension")
    C.roibin([_ptr(t) for t in frames], P, H, W, B, rp.inv, rp.vmin, rp.vmax, R, rp.min_peaks, MP, pm, _ptr(peaks),
             _ptr(counts), _ptr(codes), _ptr(npk), _ptr(nbox), _ptr(nbad), _ptr(nsat), _ptr(flags), _ptr(offs),
             _ptr(ctr), _ptr(rec), _ptr(box), _ext.stream_handle(stream), int(_phases))


def mask_frames(frames: Sequence[torch.Tensor], zero: torch.Tensor, stream=None):
    """In place, ``np.where(mask, data, 0)`` (psana_ray/producer.py:92-95) over F float32 frames:
    pixel i of every frame becomes 0 where ``zero[i]`` (uint8, 1 = masked) is non-zero.  ONE launch
    per 64 frames (csrc/gather.hip mask_frames_kernel) -- the psana-calibrated upload path."""
    C = _ext.load()
    if not frames:
        return
    dev = frames[0].device
    n = frames[0].numel()
    _check_frames(frames, torch.float32, n, dev, "mask_frames")
    if zero.dtype != torch.uint8 or zero.numel() != n or zero.device != dev or not zero.is_contiguous() \
            or _ptr(zero) % 4:
        raise ValueError(f"mask_frames: zero must be a contiguous, 4-B aligned uint8 [{n}] tensor on {dev}")
    s = _ext.stream_handle(stream)
    for a, b in _chunks(len(frames)):
        C.mask_frames([_ptr(t) for t in frames[a:b]], _ptr(zero), n, s)


def gather_frames(frames: Sequence[torch.Tensor], out, stream=None):
    """Copy F leased f32 frames (scattered ring slots) into ``out``: a contiguous batch [F, ...]
    or a list of F contiguous destination tensors (e.g. the panel ranges of assembled frames);
    float32 or bfloat16 (converted on the fly, round-to-nearest-even).  ONE launch per 32 frames
    (csrc/gather.hip)."""
    C = _ext.load()
    F = len(frames)
    if F == 0:
        return out
    dev = frames[0].device
    n = frames[0].numel()
    _check_frames(frames, torch.float32, n, dev, "gather_frames in")
    outs = list(out) if isinstance(out, (list, tuple)) else None
    if outs is None:
        if out.device != dev or out.dtype not in (torch.float32, torch.bfloat16) or not out.is_contiguous():
            raise ValueError("gather_frames: out must be a contiguous float32/bfloat16 tensor on the frames' device")
        if out.shape[0] != F or out[0].numel() != n:
            raise ValueError(f"gather_frames: out shape {tuple(out.shape)} does not hold {F} frames of {n} elements")
        odt = out.dtype
        outs = [out[i] for i in range(F)]
    else:
        if len(outs) != F:
            raise ValueError(f"gather_frames: {len(outs)} destinations for {F} frames")
        odt = outs[0].dtype
        if odt not in (torch.float32, torch.bfloat16):
            raise ValueError("gather_frames: destinations must be float32/bfloat16")
        _check_frames(outs, odt, n, dev, "gather_frames out")
    if n % 4 or any(o.data_ptr() % 16 for o in outs):
        raise ValueError("gather_frames: frames must be multiples of 4 elements, destinations 16-B aligned")
    bf16 = odt == torch.bfloat16
    s = _ext.stream_handle(stream)
    for a, b in _chunks(F):
        C.gather_frames([_ptr(t) for t in frames[a:b]], [_ptr(o) for o in outs[a:b]], n, bf16, s)
    return out
