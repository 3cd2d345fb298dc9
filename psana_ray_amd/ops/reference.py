"""Pure-PyTorch fp32 golden models of every numeric op (K-01 .. K-07).

These are the oracles the HIP kernels are tested against and the
explicit compute path of ``device="cpu"`` pipelines (BASELINE config 1 runs without a GPU).  They
are written from the documented formulas and the *unpacked* constants (pedestals/gains per gain
range, gain configuration, status), not from the kernel's packed tables, so a packing bug is
caught too.
"""
from __future__ import annotations

import operator
from typing import List, NamedTuple, Optional

import numpy as np
import torch

from ..config import CommonModeParams, PeakFinderParams
from ..dark import MAX_FRAMES as DARK_MAX_FRAMES   # 2^31 - 1 frames per run (the int32 count)
from ..dark import NC_OF_KIND as DARK_NC           # candidates per kernel kind (epix10ka, jungfrau, plain)
from ..models.constants import CalibConstants
from ..models.detector import EPIX_CAND_A, EPIX_CAND_B


def decode_gain(raw: torch.Tensor, consts: CalibConstants):
    """K-01: per-pixel ADU, gain-range index and validity from raw u16 frames [F, P, H, W]."""
    s = consts.spec
    r = raw.to(torch.int32)
    if s.kind == "epix10ka":
        adu = r & 0x3FFF
        bit = (r >> 14) & 1
        cfg = torch.as_tensor(consts.gain_config.astype(np.int64), device=raw.device)
        a = torch.as_tensor(EPIX_CAND_A, device=raw.device)[cfg]
        b = torch.as_tensor(EPIX_CAND_B, device=raw.device)[cfg]
        g = torch.where(bit.bool(), b, a)
        valid = torch.ones_like(adu, dtype=torch.bool)
    elif s.kind == "jungfrau":
        adu = r & 0x3FFF
        gb = r >> 14
        g = torch.where(gb == 3, torch.full_like(gb, 2), gb & 1).to(torch.int64)
        valid = gb != 2
    else:
        adu = r
        g = torch.zeros_like(r, dtype=torch.int64)
        valid = torch.ones_like(r, dtype=torch.bool)
    return adu, g.to(torch.int64), valid


def _take(table: np.ndarray, g: torch.Tensor) -> torch.Tensor:
    t = torch.as_tensor(table, device=g.device)            # [G, P, H, W]
    F = g.shape[0]
    tt = t.unsqueeze(0).expand(F, *t.shape)                 # [F, G, P, H, W]
    return torch.gather(tt, 1, g.unsqueeze(1)).squeeze(1)


def masked_median(x: torch.Tensor, m: torch.Tensor, dim: int):
    """numpy-semantics median of x over ``dim`` restricted to m; returns (median, count)."""
    xs = torch.where(m, x, torch.full_like(x, float("inf"))).sort(dim=dim).values
    cnt = m.sum(dim=dim, keepdim=True)
    i0 = ((cnt - 1) // 2).clamp(min=0)
    i1 = (cnt // 2).clamp(min=0, max=x.shape[dim] - 1)
    a = torch.gather(xs, dim, i0)
    b = torch.gather(xs, dim, i1)
    return (a + b) * 0.5, cnt


def common_mode_reference(v: torch.Tensor, elig: torch.Tensor, consts: CalibConstants,
                          cm: CommonModeParams) -> torch.Tensor:
    """K-03 on pre-gain values v [F, P, H, W]: rows-by-bank then columns, per ASIC."""
    s = consts.spec
    F, P, H, W = v.shape
    R, C = s.asic_rows, s.asic_cols
    L = cm.bank_cols or s.bank_cols

    def to_tiles(x):
        return x.reshape(F, P, H // R, R, W // C, C).permute(0, 1, 2, 4, 3, 5).contiguous()

    def from_tiles(x):
        return x.permute(0, 1, 2, 4, 3, 5).reshape(F, P, H, W)

    t = to_tiles(v)
    e = to_tiles(elig)
    if cm.flags & 1:
        tb = t.reshape(*t.shape[:-1], C // L, L)
        eb = e.reshape(*e.shape[:-1], C // L, L)
        med, cnt = masked_median(tb, eb & (tb.abs() < cm.thr), dim=-1)
        ok = (cnt >= max(cm.npix_min, 1)) & (med.abs() <= cm.maxcorr)
        tb = torch.where(eb & ok, tb - med, tb)
        t = tb.reshape(t.shape)
    if cm.flags & 2:
        med, cnt = masked_median(t, e & (t.abs() < cm.thr), dim=-2)
        ok = (cnt >= max(cm.npix_min, 1)) & (med.abs() <= cm.maxcorr)
        t = torch.where(e & ok, t - med, t)
    return from_tiles(t)


def calibrate_reference(raw: torch.Tensor, consts: CalibConstants, mask: Optional[np.ndarray] = None,
                        cm: Optional[CommonModeParams] = None) -> torch.Tensor:
    """K-01..K-04: raw u16 [F, P, H, W] -> calibrated f32 [F, P, H, W] (keV), masked (truthy keeps)."""
    s = consts.spec
    if raw.dim() == 3:
        raw = raw.unsqueeze(0)
    adu, g, valid = decode_gain(raw, consts)
    ped = _take(consts.pedestals, g)
    gain = _take(consts.gains, g)
    v = adu.to(torch.float32) - ped
    keep = torch.ones(s.frame_shape, dtype=torch.bool, device=raw.device) if mask is None else \
        torch.as_tensor(np.asarray(mask).astype(bool), device=raw.device).expand(s.frame_shape)
    if cm is not None:
        cm_set = torch.zeros(max(s.n_gains, 1), dtype=torch.bool, device=raw.device)
        cm_set[list(consts.cm_gains)] = True
        status_good = torch.as_tensor(consts.status == 0, device=raw.device)
        # the output mask does NOT enter the estimate: the reference masks psana's calibrated frames
        # afterwards (np.where(mask, data, 0), psana_ray/producer.py:92-95), psana's common mode sees
        # only its own status constants
        elig = valid & status_good & cm_set[g]
        v = common_mode_reference(v, elig, consts, cm)
    gf = 1.0 / gain                      # float32, same rounding as the packed device table
    out = v * gf
    out = torch.where(valid, out, torch.zeros_like(out))
    out = torch.where(keep, out, torch.zeros_like(out))   # np.where(mask, data, 0) (producer.py:92-95)
    return out


def assemble_reference(frames: torch.Tensor, rows: np.ndarray, cols: np.ndarray, image_shape,
                       image_mask: Optional[np.ndarray] = None) -> torch.Tensor:
    """K-05 as a SCATTER from per-pixel image coordinates: [F, P, H, W] -> [F, 1, Himg, Wimg]."""
    F = frames.shape[0]
    himg, wimg = image_shape
    out = torch.zeros(F, himg * wimg, dtype=frames.dtype, device=frames.device)
    dst = torch.as_tensor((rows.astype(np.int64) * wimg + cols).ravel(), device=frames.device)
    out[:, dst] = frames.reshape(F, -1)
    if image_mask is not None:
        out = torch.where(torch.as_tensor(np.asarray(image_mask).astype(bool).ravel(), device=out.device),
                          out, torch.zeros_like(out))
    return out.reshape(F, 1, himg, wimg)


def peakfind_reference(frames: torch.Tensor, p: PeakFinderParams):
    """K-07 golden: per frame, an [n, 8] float tensor (panel,row,col,value,intensity,bkg,noise,snr)
    sorted by (panel,row,col), plus the [F, 2] summary (n pixels above thr, their sum)."""
    if frames.dim() == 3:
        frames = frames.unsqueeze(0)
    F, P, H, W = frames.shape
    R = p.radius
    h = R + 2
    x = frames.to(torch.float32)
    xp = torch.full((F, P, H + 2 * h, W + 2 * h), float("nan"), dtype=torch.float32, device=x.device)
    xp[:, :, h:h + H, h:h + W] = x

    def sh(dy, dx):
        return xp[:, :, h + dy:h + dy + H, h + dx:h + dx + W]

    above = x > p.thr_peak
    summary = torch.stack([above.sum(dim=(1, 2, 3)).to(torch.float32),
                           torch.where(above, x, torch.zeros_like(x)).sum(dim=(1, 2, 3))], dim=1)
    is_max = above.clone()
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            n = sh(dy, dx)
            before = dy < 0 or (dy == 0 and dx < 0)
            okn = (x > n) if before else (x >= n)
            is_max &= okn | torch.isnan(n)
    ring = [(dy, dx) for dy in range(-h, h + 1) for dx in range(-h, h + 1) if max(abs(dy), abs(dx)) > R]
    s = torch.zeros_like(x)
    nr = torch.zeros_like(x)
    for dy, dx in ring:
        n = sh(dy, dx)
        ok = ~torch.isnan(n)
        s += torch.where(ok, n, torch.zeros_like(n))
        nr += ok.to(torch.float32)
    bkg = torch.where(nr > 0, s / nr.clamp(min=1), torch.zeros_like(s))
    # two-pass variance (the one-pass s2/nr - bkg^2 cancels in fp32 on an offset background), and no
    # clamp at 0: an Inf in the ring gives Inf - Inf = NaN, which reaches snr and rejects the pixel
    ss = torch.zeros_like(x)
    for dy, dx in ring:
        n = sh(dy, dx)
        c = n - bkg
        ss += torch.where(torch.isnan(n), torch.zeros_like(n), c * c)
    noise = torch.where(nr > 0, (ss / nr.clamp(min=1)).sqrt(), torch.zeros_like(s))
    # NaN-propagating max(noise, 1e-6), written as the kernel writes it
    snr = (x - bkg) / torch.where(noise < 1e-6, torch.full_like(noise, 1e-6), noise)
    inten = torch.zeros_like(x)
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            n = sh(dy, dx)
            inten += torch.where(torch.isnan(n), torch.zeros_like(n), n - bkg)
    keep = is_max & (snr >= p.son_min)
    peaks: List[torch.Tensor] = []
    for f in range(F):
        idx = keep[f].nonzero()
        pk, r, c = idx[:, 0], idx[:, 1], idx[:, 2]
        rec = torch.stack([pk.float(), r.float(), c.float(), x[f, pk, r, c], inten[f, pk, r, c],
                           bkg[f, pk, r, c], noise[f, pk, r, c], snr[f, pk, r, c]], dim=1)
        peaks.append(rec)
    return peaks, summary


RADIAL_EXCLUDED = 0xFFFF   # bin-map entry of a pixel that never contributes (gap, masked, out of range)


def radial_bound_ok(n: int, vmin: float, vmax: float, frac_bits: int) -> bool:
    """max(|vmin|, |vmax|) * 2^S * n < 2^53: every int64 sum converts to double exactly."""
    m = max(abs(float(np.float32(vmin))), abs(float(np.float32(vmax))))   # the window as the kernel sees it
    return bool(np.isfinite(m)) and m * (2.0 ** int(frac_bits)) * int(n) < 2.0 ** 53


def radial_profile_reference(frames: torch.Tensor, bins, nbins: int, vmin: float, vmax: float, frac_bits: int):
    """K-08 golden: radial profiles by exact INTEGER accumulation.  ``frames``: [F, ...] float32 (any
    frame layout of n elements), ``bins``: uint16 [n] (0xFFFF = excluded, else < nbins).  A pixel
    contributes iff its bin is not 0xFFFF and vmin <= v <= vmax (NaN fails, +-inf is outside); it adds
    q = int64(round_half_even(v * 2^S)) to sum[f, bin] and 1 to count[f, bin].  Returns (sum int64
    [F, nbins], count int32 [F, nbins], profile float32 [F, nbins] = float32(double(sum) * 2^-S /
    double(count)), +0 where count == 0)."""
    F = frames.shape[0]
    x = frames.reshape(F, -1).to(torch.float32).cpu()
    n = x.shape[1]
    b = torch.as_tensor(np.asarray(bins.cpu() if isinstance(bins, torch.Tensor) else bins).reshape(-1).astype(np.int64))
    if b.numel() != n:
        raise ValueError(f"radial: bin map of {b.numel()} entries for frames of {n} elements")
    if not 1 <= int(nbins) <= 4096:
        raise ValueError("radial: nbins must be in [1, 4096]")
    if not radial_bound_ok(n, vmin, vmax, frac_bits):
        raise ValueError("radial: max(|vmin|, |vmax|) * 2^frac_bits * n must stay below 2^53")
    inb = b != RADIAL_EXCLUDED
    if bool((b[inb] >= nbins).any()) or bool((b < 0).any()):
        raise ValueError("radial: bin map entry >= nbins")
    lo, hi = np.float32(vmin), np.float32(vmax)
    ok = inb.unsqueeze(0) & (x >= float(lo)) & (x <= float(hi))
    q = torch.where(ok, torch.round(x * float(2 ** int(frac_bits))), torch.zeros_like(x)).to(torch.int64)
    idx = torch.where(inb, b, torch.zeros_like(b))
    sums = torch.zeros((F, nbins), dtype=torch.int64)
    counts = torch.zeros((F, nbins), dtype=torch.int64)
    sums.index_add_(1, idx, q)
    counts.index_add_(1, idx, ok.to(torch.int64))
    return sums, counts.to(torch.int32), radial_profile_from_sums(sums, counts, frac_bits)


def radial_profile_from_sums(sums: torch.Tensor, counts: torch.Tensor, frac_bits: int) -> torch.Tensor:
    """float32(double(sum) * 2^-S / double(count)), +0 where count == 0."""
    c = counts.to(torch.float64)
    mean = sums.to(torch.float64) * (2.0 ** -int(frac_bits)) / torch.where(c > 0, c, torch.ones_like(c))
    return torch.where(c > 0, mean, torch.zeros_like(mean)).to(torch.float32)


def dark_accumulate_reference(frames: torch.Tensor, kind: int, adu_lo: int, adu_hi: int):
    """K-09 golden: dark-run statistics by exact INTEGER accumulation.  ``frames``: [F, ...] raw uint16
    (any frame layout of n elements); ``kind``: DetectorSpec.kernel_kind.  Decode of a raw word r:
    epix10ka (0) adu = r & 0x3FFF, candidate (r >> 14) & 1, always valid (bit 15 ignored); jungfrau (1)
    adu = r & 0x3FFF, candidate 0, 1, 2 for gb = r >> 14 = 0, 1, 3, gb == 2 invalid; plain (2) adu = r,
    candidate 0.  A sample contributes iff it is valid and adu_lo <= adu <= adu_hi (inclusive); it adds
    1 to cnt[c, p], adu to sum[c, p], adu * adu to sq[c, p].  Returns (cnt int32 [NC, n], sum int64
    [NC, n], sq int64 [NC, n]) of these frames alone."""
    kind, adu_lo, adu_hi = int(kind), int(adu_lo), int(adu_hi)
    if kind not in (0, 1, 2):
        raise ValueError(f"dark: unknown gain kind {kind}")
    if not 0 <= adu_lo <= adu_hi <= 65535:
        raise ValueError(f"dark: the ADU window must satisfy 0 <= lo <= hi <= 65535, got [{adu_lo}, {adu_hi}]")
    if frames.dtype != torch.uint16:
        raise ValueError(f"dark: frames must be uint16, got {frames.dtype}")
    F = frames.shape[0]
    if F > DARK_MAX_FRAMES:
        raise ValueError("dark: more than 2^31 - 1 frames")
    r = frames.cpu().reshape(F, -1).view(torch.int16).to(torch.int64) & 0xFFFF
    if kind == 0:
        adu, cand, valid = r & 0x3FFF, (r >> 14) & 1, torch.ones_like(r, dtype=torch.bool)
    elif kind == 1:
        gb = r >> 14
        adu, cand, valid = r & 0x3FFF, torch.where(gb == 3, torch.full_like(gb, 2), gb), gb != 2
    else:
        adu, cand, valid = r, torch.zeros_like(r), torch.ones_like(r, dtype=torch.bool)
    ok = valid & (adu >= adu_lo) & (adu <= adu_hi)
    cnt, s, q = [], [], []
    for c in range(DARK_NC[kind]):
        m = (ok & (cand == c)).to(torch.int64)
        cnt.append(m.sum(dim=0))
        s.append((m * adu).sum(dim=0))
        q.append((m * adu * adu).sum(dim=0))
    return torch.stack(cnt).to(torch.int32), torch.stack(s), torch.stack(q)


SPARSE_MAX_FRAMES = 64
SPARSE_FLAG_OVERFLOW = 1   # nnz[f] > cap: the frame stores nothing
SPARSE_FLAG_SKIPPED = 2    # keys[f] < key_min: the frame was not looked at


def validate_sparse_params(thr, vmax, cap, frames: int, what: str = "sparsify"):
    """(thr, vmax) as the float32 values the kernel sees and cap as a Python int, or ValueError."""
    try:
        cap = operator.index(cap)
    except TypeError:
        raise ValueError(f"{what}: cap must be an integer, got {cap!r}") from None
    with np.errstate(over="ignore"):   # a double beyond the float32 range becomes inf and is refused
        lo, hi = float(np.float32(thr)), float(np.float32(vmax))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{what}: the value window must be finite, got [{thr}, {vmax}]")
    if not lo <= hi:
        raise ValueError(f"{what}: empty value window [{thr}, {vmax}]")
    if cap < 1 or int(frames) * cap >= 2 ** 31:
        raise ValueError(f"{what}: cap must be >= 1 with F * cap < 2^31, got cap {cap} for {frames} frames")
    return lo, hi, cap


def sparsify_reference(frames: torch.Tensor, thr: float, vmax: float, cap: int, mask=None, keys=None,
                       key_min: int = 0):
    """K-10 golden: zero suppression.  ``frames``: [F, ...] float32 (any frame layout of n elements),
    1 <= F <= 64.  A pixel is kept iff its ``mask`` entry (uint8 [n], when given) is non-zero and
    thr <= v <= vmax (NaN fails, +-inf is outside the finite window, -0.0 is kept iff thr <= 0 with its
    sign bit).  Frame f is processed iff ``keys`` (int32 [F]) is absent or keys[f] >= key_min;
    otherwise it is skipped (nnz 0, flag bit 1).  Returns (nnz int32 [F] -- exact, also past cap --,
    flags uint8 [F] -- bit 0 = nnz > cap --, offs int64 [F + 1], pix int32 [offs[F]], val float32
    [offs[F]]): frame f's kept pixels in ascending index order at offs[f] .. offs[f + 1], none when it
    overflows."""
    F = int(frames.shape[0])
    if not 1 <= F <= SPARSE_MAX_FRAMES:
        raise ValueError(f"sparsify: 1 .. {SPARSE_MAX_FRAMES} frames per batch, got {F}")
    if frames.dtype != torch.float32:
        raise ValueError(f"sparsify: frames must be float32, got {frames.dtype}")
    lo, hi, cap = validate_sparse_params(thr, vmax, cap, F)
    x = frames.detach().cpu().reshape(F, -1)
    n = x.shape[1]
    if not 1 <= n < 2 ** 31:
        raise ValueError("sparsify: frames must have 1 .. 2^31 - 1 elements")
    keep = (x >= lo) & (x <= hi)
    if mask is not None:
        m = torch.as_tensor(np.asarray(mask.cpu() if isinstance(mask, torch.Tensor) else mask)).reshape(-1)
        if m.dtype != torch.uint8 or m.numel() != n:
            raise ValueError(f"sparsify: mask must be uint8 [{n}]")
        keep &= (m != 0).unsqueeze(0)
    live = torch.ones(F, dtype=torch.bool)
    if keys is not None:
        k = torch.as_tensor(np.asarray(keys.cpu() if isinstance(keys, torch.Tensor) else keys)).reshape(-1)
        if k.dtype != torch.int32 or k.numel() != F:
            raise ValueError(f"sparsify: keys must be int32 [{F}]")
        live = k >= int(key_min)
    nnz = torch.zeros(F, dtype=torch.int32)
    flags = torch.zeros(F, dtype=torch.uint8)
    offs = torch.zeros(F + 1, dtype=torch.int64)
    pix, val = [], []
    for f in range(F):
        stored = 0
        if not bool(live[f]):
            flags[f] = SPARSE_FLAG_SKIPPED
        else:
            idx = torch.nonzero(keep[f]).reshape(-1)   # ascending
            nnz[f] = idx.numel()
            if idx.numel() > cap:
                flags[f] = SPARSE_FLAG_OVERFLOW
            else:
                stored = idx.numel()
                pix.append(idx.to(torch.int32))
                val.append(x[f][idx])
        offs[f + 1] = offs[f] + stored
    pix = torch.cat(pix) if pix else torch.zeros(0, dtype=torch.int32)
    val = torch.cat(val) if val else torch.zeros(0, dtype=torch.float32)
    return nnz, flags, offs, pix, val


# K-11 powder statistics: the defaults of the contract (docs/ARCHITECTURE.md, "Powder statistics")
POWDER_VMIN = -float(2 ** 20)    # the K-08 window
POWDER_VMAX = float(2 ** 20)
POWDER_FRAC_BITS = 2
POWDER_THR_ABOVE = 20.0          # the peak finder's and K-10's default threshold
POWDER_QMAX_NONE = -2 ** 31      # qmax of a pixel without a sample (INT32_MIN)


def _powder_q(lo: float, hi: float, frac_bits: int) -> int:
    """Q = ceil(max(|vmin|, |vmax|) * 2^S) in Python integers (no |q| of a contributing sample exceeds it)."""
    from fractions import Fraction

    m = max(abs(Fraction(lo)), abs(Fraction(hi))) * (1 << frac_bits)
    return -((-m.numerator) // m.denominator)


def validate_powder_params(vmin, vmax, frac_bits, thr_above, what: str = "powder_accumulate"):
    """(vmin, vmax, thr_above) as the float32 values the kernel sees, frac_bits as a Python int, Q and
    the run bound max_frames = min(2^31 - 1, (2^63 - 1) // max(1, Q * Q)) -- or ValueError."""
    try:
        frac_bits = operator.index(frac_bits)
    except TypeError:
        raise ValueError(f"{what}: frac_bits must be an integer, got {frac_bits!r}") from None
    try:
        with np.errstate(over="ignore"):   # a double beyond the float32 range becomes inf and is refused
            lo, hi, thr = float(np.float32(vmin)), float(np.float32(vmax)), float(np.float32(thr_above))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the value window and thr_above must be numbers") from None
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{what}: the value window must be finite, got [{vmin}, {vmax}]")
    if not lo <= hi:
        raise ValueError(f"{what}: empty value window [{vmin}, {vmax}]")
    if not 0 <= frac_bits <= 16:
        raise ValueError(f"{what}: frac_bits must be in [0, 16], got {frac_bits}")
    if thr != thr:
        raise ValueError(f"{what}: thr_above is NaN")
    Q = _powder_q(lo, hi, frac_bits)
    if Q >= 2 ** 31:
        raise ValueError(f"{what}: max(|vmin|, |vmax|) * 2^frac_bits must stay below 2^31 (q and qmax are int32), "
                         f"got {Q}")
    return lo, hi, frac_bits, thr, Q, min(2 ** 31 - 1, (2 ** 63 - 1) // max(1, Q * Q))


def powder_max_frames(vmin=POWDER_VMIN, vmax=POWDER_VMAX, frac_bits=POWDER_FRAC_BITS) -> int:
    """Frames a powder run holds at most: the int32 count and the int64 sum of squares both fit."""
    return validate_powder_params(vmin, vmax, frac_bits, 0.0, "powder_max_frames")[5]


def powder_accumulate_reference(frames: torch.Tensor, vmin: float, vmax: float, frac_bits: int, thr_above: float,
                                keys=None, key_min: int = 0):
    """K-11 golden: per-pixel powder statistics by exact INTEGER accumulation.  ``frames``: [F, ...]
    float32 (any frame layout of n elements).  Frame f is class 1 ("hit") iff ``keys`` (int32 [F]) is
    given and keys[f] >= key_min, else class 0; NC = 2 with keys, 1 without.  A sample v contributes iff
    vmin <= v <= vmax as float32 (NaN fails, +-inf is outside); it gives q = int64(round_half_even(v *
    2^S)) and adds 1 to cnt[c, p], q to sum[c, p], q * q to sq[c, p], (v >= thr_above) to above[c, p] and
    raises qmax[c, p] to q.  Returns (nfr int64 [NC], cnt int32 [NC, n], sum int64 [NC, n], sq int64
    [NC, n], qmax int32 [NC, n] -- INT32_MIN where no sample --, above int32 [NC, n]) of these frames
    alone."""
    lo, hi, S, thr, _Q, max_frames = validate_powder_params(vmin, vmax, frac_bits, thr_above, "powder")
    if frames.dtype != torch.float32:
        raise ValueError(f"powder: frames must be float32, got {frames.dtype}")
    F = int(frames.shape[0])
    if F < 1:
        raise ValueError("powder: no frames")
    if F > max_frames:
        raise ValueError(f"powder: {F} frames are more than the {max_frames} a run holds at these parameters")
    x = frames.detach().cpu().reshape(F, -1)
    n = x.shape[1]
    if not 1 <= n < 2 ** 31:
        raise ValueError("powder: frames must have 1 .. 2^31 - 1 elements")
    cls = torch.zeros(F, dtype=torch.int64)
    nc = 1
    if keys is not None:
        k = torch.as_tensor(np.asarray(keys.cpu() if isinstance(keys, torch.Tensor) else keys)).reshape(-1)
        if k.dtype != torch.int32 or k.numel() != F:
            raise ValueError(f"powder: keys must be int32 [{F}]")
        cls = (k >= int(key_min)).to(torch.int64)
        nc = 2
    ok = (x >= lo) & (x <= hi)
    q = torch.where(ok, torch.round(x * float(2 ** S)), torch.zeros_like(x)).to(torch.int64)
    hot = ok & (x >= thr)
    none = torch.full_like(q, POWDER_QMAX_NONE)
    nfr, cnt, s, sq, qmax, above = [], [], [], [], [], []
    for c in range(nc):
        m = ok & (cls == c).unsqueeze(1)
        mi = m.to(torch.int64)
        nfr.append((cls == c).sum())
        cnt.append(mi.sum(dim=0))
        s.append((mi * q).sum(dim=0))
        sq.append((mi * q * q).sum(dim=0))
        qmax.append(torch.where(m, q, none).amax(dim=0))
        above.append((hot & m).to(torch.int64).sum(dim=0))
    return (torch.stack(nfr).to(torch.int64), torch.stack(cnt).to(torch.int32), torch.stack(s), torch.stack(sq),
            torch.stack(qmax).to(torch.int32), torch.stack(above).to(torch.int32))


# K-15 cube: K-11's window, quantisation and run bound (validate_powder_params), per bin of a scan variable
# (docs/ARCHITECTURE.md, "Cube: the integer contract")
CUBE_MAX_BINS = 4096
CUBE_DROPPED = -1                # the bin of a frame that is not accumulated
CUBE_BYTES_PER_PIXEL = 20        # cnt int32 + sum int64 + sq int64 of one bin


def validate_cube_nbins(nbins, what: str = "cube_accumulate") -> int:
    try:
        nbins = operator.index(nbins)
    except TypeError:
        raise ValueError(f"{what}: nbins must be an integer, got {nbins!r}") from None
    if not 1 <= nbins <= CUBE_MAX_BINS:
        raise ValueError(f"{what}: nbins must be in [1, {CUBE_MAX_BINS}], got {nbins}")
    return nbins


def validate_cube_bins(bins, frames: int, nbins: int, what: str = "cube_accumulate") -> List[int]:
    """``bins`` (a sequence, numpy array or CPU tensor of ``frames`` integers in -1 .. nbins - 1) as a list
    of Python ints -- or ValueError."""
    if isinstance(bins, torch.Tensor):
        if bins.device.type != "cpu":
            raise ValueError(f"{what}: bins live on the host, got a tensor on {bins.device}")
        bins = bins.numpy()
    try:
        b = np.asarray(bins)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: bins must be integers") from None
    if b.ndim != 1 or b.shape[0] != frames:
        raise ValueError(f"{what}: {b.size if b.ndim == 1 else b.shape} bins for {frames} frames")
    if frames and b.dtype.kind not in "iu":
        raise ValueError(f"{what}: bins must be integers, got {b.dtype}")
    out = [int(v) for v in b]
    if any(not CUBE_DROPPED <= v < nbins for v in out):
        raise ValueError(f"{what}: bins must be in -1 .. {nbins - 1}")
    return out


def cube_accumulate_reference(frames: torch.Tensor, bins, nbins: int, vmin: float, vmax: float, frac_bits: int):
    """K-15 golden: per-pixel, per-bin statistics by exact INTEGER accumulation.  ``frames``: [F, ...]
    float32 (any frame layout of n elements); ``bins``: F integers, frame f belongs to bin bins[f] in 0 ..
    nbins - 1 or is dropped with -1.  A sample v of a kept frame contributes iff vmin <= v <= vmax as
    float32 (NaN fails, +-inf is outside); it gives q = int64(round_half_even(v * 2^S)) and adds 1 to
    cnt[b, p], q to sum[b, p] and q * q to sq[b, p].  Returns the increments (nfr int64 [B], cnt int32
    [B, n], sum int64 [B, n], sq int64 [B, n]) of these frames alone."""
    lo, hi, S, _thr, _Q, max_frames = validate_powder_params(vmin, vmax, frac_bits, 0.0, "cube")
    B = validate_cube_nbins(nbins, "cube")
    if frames.dtype != torch.float32:
        raise ValueError(f"cube: frames must be float32, got {frames.dtype}")
    F = int(frames.shape[0])
    if F < 1:
        raise ValueError("cube: no frames")
    if F > max_frames:
        raise ValueError(f"cube: {F} frames are more than the {max_frames} a run holds at these parameters")
    x = frames.detach().cpu().reshape(F, -1)
    n = x.shape[1]
    if not 1 <= n < 2 ** 31:
        raise ValueError("cube: frames must have 1 .. 2^31 - 1 elements")
    b = torch.tensor(validate_cube_bins(bins, F, B, "cube"), dtype=torch.int64)
    kept = b >= 0
    row = b.clamp(min=0)   # a dropped frame adds zeros to bin 0
    ok = (x >= lo) & (x <= hi) & kept.unsqueeze(1)
    q = torch.where(ok, torch.round(x * float(2 ** S)), torch.zeros_like(x)).to(torch.int64)
    nfr = torch.zeros(B, dtype=torch.int64).index_add_(0, row, kept.to(torch.int64))
    cnt = torch.zeros((B, n), dtype=torch.int64).index_add_(0, row, ok.to(torch.int64))
    s = torch.zeros((B, n), dtype=torch.int64).index_add_(0, row, q)
    sq = torch.zeros((B, n), dtype=torch.int64).index_add_(0, row, q * q)
    return nfr, cnt.to(torch.int32), s, sq


# K-12 per-pixel histograms: the defaults of the contract (docs/ARCHITECTURE.md, "Pixel histograms: the
# integer contract").  The default window is 128 wide with 64 bins: bins of exactly 2.0, inv_w exactly 0.5.
HIST_LO = -32.0
HIST_HI = 96.0
HIST_BINS = 64
HIST_MAX_BINS = 1024
HIST_MAX_FRAMES = 2 ** 31 - 1    # a bin gains at most 1 per frame: the int32 count is the only bound


def validate_pixel_hist_params(lo, hi, nbins, n=None, frames_so_far=0, frames=0, what: str = "pixel_hist"):
    """(lo, hi) as the float32 values the kernel sees, nbins as a Python int and the scale inv_w =
    float32(float64(nbins) / (float64(hi) - float64(lo))) as a Python float -- or ValueError.  With ``n``
    (elements per frame) also checks n * nbins < 2^31; with ``frames_so_far`` / ``frames`` that the run stays
    at or below HIST_MAX_FRAMES = 2^31 - 1 frames."""
    try:
        nbins = operator.index(nbins)
    except TypeError:
        raise ValueError(f"{what}: nbins must be an integer, got {nbins!r}") from None
    try:
        with np.errstate(over="ignore"):   # a double beyond the float32 range becomes inf and is refused
            flo, fhi = float(np.float32(lo)), float(np.float32(hi))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the window must be two numbers") from None
    if not (np.isfinite(flo) and np.isfinite(fhi)):
        raise ValueError(f"{what}: the window must be finite, got [{lo}, {hi}]")
    if not flo < fhi:
        raise ValueError(f"{what}: the window needs lo < hi as float32, got [{lo}, {hi}]")
    if not 1 <= nbins <= HIST_MAX_BINS:
        raise ValueError(f"{what}: nbins must be in [1, {HIST_MAX_BINS}], got {nbins}")
    with np.errstate(over="ignore", under="ignore"):
        inv_w = float(np.float32(np.float64(nbins) / (np.float64(fhi) - np.float64(flo))))
    if not np.isfinite(inv_w) or not inv_w > 0.0:
        raise ValueError(f"{what}: the scale nbins / (hi - lo) = {inv_w} is not a finite positive float32")
    if n is not None:
        try:
            n = operator.index(n)
        except TypeError:
            raise ValueError(f"{what}: the frame size must be an integer") from None
        if n < 1 or n * nbins >= 2 ** 31:
            raise ValueError(f"{what}: {n} elements x {nbins} bins: n >= 1 and n * nbins < 2^31 (int32 word indices)")
    try:
        frames_so_far, frames = operator.index(frames_so_far), operator.index(frames)
    except TypeError:
        raise ValueError(f"{what}: frame counts must be integers") from None
    if frames_so_far < 0 or frames < 0 or frames_so_far + frames > HIST_MAX_FRAMES:
        raise ValueError(f"{what}: {frames_so_far} + {frames} frames would take the run past {HIST_MAX_FRAMES} "
                         "(the int32 count of a bin)")
    return flo, fhi, nbins, inv_w


def pixel_hist_reference(frames: torch.Tensor, lo: float, hi: float, nbins: int) -> torch.Tensor:
    """K-12 golden: per-pixel histograms by exact INTEGER accumulation.  ``frames``: [F, ...] float32 (any
    frame layout of n elements).  A sample v of pixel p contributes iff lo <= v <= hi as float32 (NaN fails,
    +-inf is outside); it adds 1 to hist[p, b], b = min(nbins - 1, int(floor((v - lo) * inv_w))), where the
    subtraction and the multiply are two float32 operations, each rounded to nearest, and inv_w =
    float32(float64(nbins) / (float64(hi) - float64(lo))).  Returns hist int32 [n, nbins] of these frames
    alone."""
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
        raise ValueError(f"pixel_hist: frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    F = int(frames.shape[0]) if frames.dim() >= 1 else 0
    if F < 1:
        raise ValueError("pixel_hist: no frames")
    x = frames.detach().cpu().reshape(F, -1)
    n = int(x.shape[1])
    flo, fhi, nbins, inv_w = validate_pixel_hist_params(lo, hi, nbins, n=n, frames=F)
    hist = torch.zeros((n, nbins), dtype=torch.int64)
    tlo, tinv = torch.tensor(flo, dtype=torch.float32), torch.tensor(inv_w, dtype=torch.float32)
    for a in range(0, F, 64):   # bounded temporaries; integers add in any order
        xb = x[a:a + 64]
        ok = (xb >= flo) & (xb <= fhi)
        d = xb - tlo                 # float32
        y = d * tinv                 # float32, a second rounding
        b = torch.floor(torch.where(ok, y, torch.zeros_like(y))).to(torch.int64).clamp_(0, nbins - 1)
        hist.scatter_add_(1, b.t().contiguous(), ok.t().contiguous().to(torch.int64))
    return hist.to(torch.int32)


# K-13 photon counting: the defaults and bounds of the contract (docs/ARCHITECTURE.md, "Photon counting: the
# integer contract").
PHOTON_THR_SEED = 0.5
PHOTON_THR_TOTAL = 0.9
PHOTON_MAX_WHOLE = 254           # floor(vmax * inv) at most: a merge on top still fits the byte of kmap
PHOTON_VMAX_PHOTONS = 250        # the default vmax is this many adu_per_photon
PHOTON_MAX_ROI = 8
PHOTON_ROI_NONE = 255            # the label of a pixel in no ROI
PHOTON_PK_BINS = 8               # pk[..., j] counts k == j + 1, the last bin k >= 8
PHOTON_MAX_FRAMES = 2 ** 31 - 1  # cnt and occ gain at most 1 per frame (psum at most 255: far inside an int64)


class PhotonParams(NamedTuple):
    """The validated parameters of K-13 as the kernel sees them (every float a float32 value)."""
    adu_per_photon: float
    inv: float          # float32(1 / float64(adu_per_photon))
    vmax: float
    thr_seed: float
    thr_total: float


class PhotonCounts(NamedTuple):
    """What :func:`photon_count_reference` returns (the accumulators are the increments of these frames)."""
    kmap: torch.Tensor   # uint8 [F, n]
    cnt: torch.Tensor    # int32 [n]
    psum: torch.Tensor   # int64 [n]
    occ: torch.Tensor    # int32 [n]
    pk: torch.Tensor     # int32 [F, R, 8]
    tot: torch.Tensor    # int64 [F, R]


def validate_photon_params(adu_per_photon, vmax=None, thr_seed=None, thr_total=None, frames_so_far=0, frames=0,
                           what: str = "photons") -> PhotonParams:
    """The parameters as float32 values and the scale ``inv = float32(1.0 / float64(adu_per_photon))`` -- or
    ValueError.  ``vmax`` None: ``PHOTON_VMAX_PHOTONS * adu_per_photon``.  Requires adu_per_photon > 0 with a
    finite positive inv, ``floor(float32(vmax) * inv) <= 254`` and ``0 < thr_seed <= thr_total < 2``; with
    ``frames_so_far`` / ``frames`` that the run stays at or below PHOTON_MAX_FRAMES = 2^31 - 1 frames."""
    if isinstance(adu_per_photon, PhotonParams):
        adu_per_photon, _inv, vmax, thr_seed, thr_total = adu_per_photon
    try:
        with np.errstate(over="ignore", under="ignore"):
            adu = float(np.float32(adu_per_photon))
            fmax = float(np.float32(PHOTON_VMAX_PHOTONS * adu if vmax is None else vmax))
            ts = float(np.float32(PHOTON_THR_SEED if thr_seed is None else thr_seed))
            tt = float(np.float32(PHOTON_THR_TOTAL if thr_total is None else thr_total))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: adu_per_photon, vmax and the thresholds must be numbers") from None
    if not (np.isfinite(adu) and adu > 0.0):
        raise ValueError(f"{what}: adu_per_photon must be finite and positive, got {adu_per_photon}")
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        inv = float(np.float32(1.0 / np.float64(adu)))
    if not (np.isfinite(inv) and inv > 0.0):
        raise ValueError(f"{what}: the scale 1 / adu_per_photon = {inv} is not a finite positive float32")
    if fmax != fmax:
        raise ValueError(f"{what}: vmax is NaN")
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        whole = np.floor(np.float32(fmax) * np.float32(inv))
    if not whole <= PHOTON_MAX_WHOLE:
        raise ValueError(f"{what}: floor(vmax / adu_per_photon) = {whole} must be at most {PHOTON_MAX_WHOLE} "
                         "(photons per pixel fit a byte)")
    if not 0.0 < ts <= tt < 2.0:
        raise ValueError(f"{what}: the thresholds need 0 < thr_seed <= thr_total < 2, got {thr_seed}, {thr_total}")
    try:
        frames_so_far, frames = operator.index(frames_so_far), operator.index(frames)
    except TypeError:
        raise ValueError(f"{what}: frame counts must be integers") from None
    if frames_so_far < 0 or frames < 0 or frames_so_far + frames > PHOTON_MAX_FRAMES:
        raise ValueError(f"{what}: {frames_so_far} + {frames} frames would take the run past {PHOTON_MAX_FRAMES} "
                         "(the int32 counts of a pixel)")
    return PhotonParams(adu, inv, fmax, ts, tt)


def photon_shape(shape, what: str = "photons"):
    """``(P, H, W)`` of a frame shape: 3-D as it is (the calib layout), 2-D as one panel (an image) -- or
    ValueError.  1 <= P * H * W < 2^31."""
    try:
        shape = tuple(operator.index(s) for s in shape)
    except TypeError:
        raise ValueError(f"{what}: the shape must be a sequence of integers, got {shape!r}") from None
    if len(shape) == 2:
        shape = (1, *shape)
    if len(shape) != 3 or min(shape) < 1 or shape[0] * shape[1] * shape[2] >= 2 ** 31:
        raise ValueError(f"{what}: the shape must be [P, H, W] or [H, W] with 1 <= P * H * W < 2^31, got {shape}")
    return shape


def validate_photon_maps(shape, mask=None, roi=None, n_roi=None, what: str = "photons"):
    """Host check of the keep-mask and the ROI labels (numpy arrays or CPU tensors) for frames of ``shape``.
    Returns ``(mask uint8 [n] or None, roi uint8 [n] or None, R)``: R = ``n_roi``, or without it 1 + the
    largest label other than 255 (1 without labels).  ValueError for a wrong size or dtype, R outside 1 .. 8,
    several ROIs without labels, or a label >= R other than 255."""
    P, H, W = photon_shape(shape, what)
    n = P * H * W

    def flat(a, name):
        if a is None:
            return None
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
        if a.dtype == np.bool_:
            a = a.astype(np.uint8)
        if a.dtype != np.uint8:
            raise ValueError(f"{what}: {name} is {a.dtype}, expected uint8")
        if a.size != n:
            raise ValueError(f"{what}: {name} of {a.size} elements for frames of {n}")
        return np.ascontiguousarray(a.reshape(-1))

    mask, roi = flat(mask, "mask"), flat(roi, "roi")
    if n_roi is None:
        R = 1
        if roi is not None:
            lab = roi[roi != PHOTON_ROI_NONE]
            R = 1 + (int(lab.max()) if lab.size else 0)
    else:
        try:
            R = operator.index(n_roi)
        except TypeError:
            raise ValueError(f"{what}: n_roi must be an integer, got {n_roi!r}") from None
    if not 1 <= R <= PHOTON_MAX_ROI:
        raise ValueError(f"{what}: {R} ROIs; 1 .. {PHOTON_MAX_ROI} are possible (labels 0 .. 7, 255 = none)")
    if roi is None and R != 1:
        raise ValueError(f"{what}: {R} ROIs need labels")
    if roi is not None and bool(((roi >= R) & (roi != PHOTON_ROI_NONE)).any()):
        raise ValueError(f"{what}: a label >= n_roi = {R} other than {PHOTON_ROI_NONE}")
    return mask, roi, R


def photon_count_reference(frames: torch.Tensor, shape, params, mask=None, roi=None, n_roi=None) -> PhotonCounts:
    """K-13 golden: photons per pixel by the float32 operations of the contract, then integers.  ``frames``:
    [F, ...] float32 of ``shape`` = [P, H, W] (or [H, W]); ``params``: a :class:`PhotonParams`, or the
    arguments of :func:`validate_photon_params` as a tuple / dict / bare adu_per_photon.

    ok = kept by the mask && v > 0 && v <= vmax; x = ok ? v * inv : 0 (one float32 multiply); w = floor(x),
    r = x - w.  Pixel p is a seed iff r_p >= thr_seed and it beats every 4-connected neighbour of its panel
    (r_p > r_q, or equal with p < q: padded shifts make a missing neighbour r = 0); k = w + (seed && r_p +
    max neighbour r >= thr_total).  Returns kmap, the increments of cnt / psum / occ, and per frame pk
    [R, 8] (pixels of ROI r with k == j + 1, the last bin k >= 8) and tot [R] (their sum of k)."""
    what = "photons"
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
        raise ValueError(f"{what}: frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    F = int(frames.shape[0]) if frames.dim() >= 1 else 0
    if F < 1:
        raise ValueError(f"{what}: no frames")
    if isinstance(params, PhotonParams):
        pp = validate_photon_params(params, frames=F, what=what)
    elif isinstance(params, dict):
        pp = validate_photon_params(**params, frames=F, what=what)
    elif isinstance(params, (tuple, list)):
        pp = validate_photon_params(*params, frames=F, what=what)
    else:
        pp = validate_photon_params(params, frames=F, what=what)
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    x = frames.detach().cpu().reshape(F, -1)
    if x.shape[1] != n:
        raise ValueError(f"{what}: frames of {x.shape[1]} elements for the shape {(P, H, W)}")
    mask, roi, R = validate_photon_maps((P, H, W), mask, roi, n_roi, what)
    inv = torch.tensor(pp.inv, dtype=torch.float32)
    ok = (x > 0.0) & (x <= torch.tensor(pp.vmax, dtype=torch.float32))
    if mask is not None:
        ok &= torch.from_numpy(mask != 0)
    scaled = torch.where(ok, x * inv, torch.zeros_like(x))     # float32
    whole = torch.floor(scaled)
    r = (scaled - whole).reshape(F, P, H, W)                   # exact
    rp = torch.nn.functional.pad(r, (1, 1, 1, 1))              # zeros around every panel
    up, down = rp[..., :-2, 1:-1], rp[..., 2:, 1:-1]
    left, right = rp[..., 1:-1, :-2], rp[..., 1:-1, 2:]
    seed = (r >= torch.tensor(pp.thr_seed, dtype=torch.float32)) & (r > up) & (r > left) & (r >= right) & (r >= down)
    rmax = torch.maximum(torch.maximum(up, down), torch.maximum(left, right))
    merge = seed & ((r + rmax) >= torch.tensor(pp.thr_total, dtype=torch.float32))
    k = (whole.to(torch.int64) + merge.reshape(F, n).to(torch.int64))
    pk = torch.zeros((F, R * PHOTON_PK_BINS), dtype=torch.int64)
    tot = torch.zeros((F, R), dtype=torch.int64)
    lab = torch.zeros(n, dtype=torch.int64) if roi is None else torch.from_numpy(roi.astype(np.int64))
    counted = (k >= 1) & (lab < R)
    labc = torch.where(lab < R, lab, torch.zeros_like(lab)).expand(F, n)
    pk.scatter_add_(1, labc * PHOTON_PK_BINS + (k.clamp(1, PHOTON_PK_BINS) - 1), counted.to(torch.int64))
    tot.scatter_add_(1, labc, torch.where(counted, k, torch.zeros_like(k)))
    return PhotonCounts(k.to(torch.uint8), ok.sum(dim=0).to(torch.int32), k.sum(dim=0),
                        (k >= 1).sum(dim=0).to(torch.int32), pk.reshape(F, R, PHOTON_PK_BINS).to(torch.int32), tot)


# ---- K-14 droplets ---------------------------------------------------------------------------------------------
DROPLET_MAX_FRAMES = 64
DROPLET_VMAX = float(2 ** 20)        # the K-08 window's upper end
DROPLET_FRAC_BITS = 2
DROPLET_MAX_FRAC_BITS = 16
DROPLET_PIX_CAP_DIV = 16             # default cap_pix = n // 16 active pixels per frame
DROPLET_CAP_DIV = 64                 # default cap = n // 64 droplets per frame
DROPLET_FLAG_OVERFLOW = 1            # ndrop[f] > cap: the frame stores nothing
DROPLET_FLAG_PIX_OVERFLOW = 4        # nact[f] > cap_pix: the frame is not labelled, ndrop[f] = 0


class DropletParams(NamedTuple):
    """The validated parameters of K-14 as the kernel sees them (every float a float32 value)."""
    thr_low: float
    thr_seed: float
    vmax: float
    frac_bits: int
    qlim: int           # Q = ceil(vmax * 2^frac_bits) < 2^31: no q is larger


class DropletList(NamedTuple):
    """What :func:`droplet_reference` returns: every output of one launch (columns cut at offs[F])."""
    nact: torch.Tensor    # int32 [F]
    ndrop: torch.Tensor   # int32 [F]
    flags: torch.Tensor   # uint8 [F]
    offs: torch.Tensor    # int64 [F + 1]
    label: torch.Tensor   # int32 [offs[F]]
    npix: torch.Tensor    # int32
    adu: torch.Tensor     # int64
    sy: torch.Tensor      # int64
    sx: torch.Tensor      # int64
    qmax: torch.Tensor    # int32


def validate_droplet_params(thr_low, thr_seed=None, vmax=None, frac_bits=None, what: str = "droplets") -> DropletParams:
    """The parameters as float32 values with Q = ceil(vmax * 2^frac_bits) -- or ValueError.  ``thr_seed`` None:
    thr_low; ``vmax`` None: 2^20; ``frac_bits`` None: 2.  Requires finite 0 < thr_low <= thr_seed <= vmax,
    frac_bits in 0 .. 16 and Q < 2^31."""
    if isinstance(thr_low, DropletParams):
        thr_low, thr_seed, vmax, frac_bits, _q = thr_low
    try:
        with np.errstate(over="ignore", under="ignore"):
            lo = float(np.float32(thr_low))
            seed = lo if thr_seed is None else float(np.float32(thr_seed))
            hi = float(np.float32(DROPLET_VMAX if vmax is None else vmax))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: thr_low, thr_seed and vmax must be numbers") from None
    try:
        S = operator.index(DROPLET_FRAC_BITS if frac_bits is None else frac_bits)
    except TypeError:
        raise ValueError(f"{what}: frac_bits must be an integer, got {frac_bits!r}") from None
    if not (np.isfinite(lo) and np.isfinite(seed) and np.isfinite(hi)):
        raise ValueError(f"{what}: thr_low, thr_seed and vmax must be finite float32 values, got {thr_low}, {thr_seed}, "
                         f"{vmax}")
    if not 0.0 < lo <= seed <= hi:
        raise ValueError(f"{what}: need 0 < thr_low <= thr_seed <= vmax, got {lo}, {seed}, {hi}")
    if not 0 <= S <= DROPLET_MAX_FRAC_BITS:
        raise ValueError(f"{what}: frac_bits must be 0 .. {DROPLET_MAX_FRAC_BITS}, got {S}")
    q = int(np.ceil(hi * float(2 ** S)))    # exact in float64: a float32 value times a power of two
    if q >= 2 ** 31:
        raise ValueError(f"{what}: ceil(vmax * 2^frac_bits) = {q} must be below 2^31 (q and qmax are int32)")
    return DropletParams(lo, seed, hi, S, q)


def _droplet_params(params, what: str = "droplets") -> DropletParams:
    if isinstance(params, DropletParams):
        return validate_droplet_params(params, what=what)
    if isinstance(params, dict):
        return validate_droplet_params(**params, what=what)
    if isinstance(params, (tuple, list)):
        return validate_droplet_params(*params, what=what)
    return validate_droplet_params(params, what=what)


def validate_droplet_caps(shape, params, cap_pix=None, cap=None, frames: int = 1, what: str = "droplets"):
    """``(cap_pix, cap)`` as Python ints -- defaults max(1, n // 16) and max(1, n // 64) -- or ValueError: both
    >= 1 with F * cap_pix < 2^31 and F * cap < 2^31, 1 <= F <= 64, and
    Q * (max(H, W) - 1) * min(H * W, cap_pix) <= 2^63 - 1, so that no sum of a stored droplet can wrap."""
    P, H, W = photon_shape(shape, what)
    pp = _droplet_params(params, what)
    n = P * H * W
    try:
        F = operator.index(frames)
        cap_pix = max(1, n // DROPLET_PIX_CAP_DIV) if cap_pix is None else operator.index(cap_pix)
        cap = max(1, n // DROPLET_CAP_DIV) if cap is None else operator.index(cap)
    except TypeError:
        raise ValueError(f"{what}: cap_pix, cap and the frame count must be integers") from None
    if not 1 <= F <= DROPLET_MAX_FRAMES:
        raise ValueError(f"{what}: 1 .. {DROPLET_MAX_FRAMES} frames per launch, got {F}")
    if cap_pix < 1 or F * cap_pix >= 2 ** 31:
        raise ValueError(f"{what}: cap_pix must be >= 1 with F * cap_pix < 2^31, got {cap_pix} for {F} frames")
    if cap < 1 or F * cap >= 2 ** 31:
        raise ValueError(f"{what}: cap must be >= 1 with F * cap < 2^31, got {cap} for {F} frames")
    if pp.qlim * (max(H, W) - 1) * min(H * W, cap_pix) > 2 ** 63 - 1:
        raise ValueError(f"{what}: Q * (max(H, W) - 1) * min(H * W, cap_pix) = {pp.qlim} * {max(H, W) - 1} * "
                         f"{min(H * W, cap_pix)} passes 2^63 - 1: lower vmax, frac_bits or cap_pix")
    return cap_pix, cap


def droplet_mask(shape, mask, what: str = "droplets"):
    """The keep-mask as a contiguous numpy uint8 [n] (bool accepted), or None -- or ValueError."""
    P, H, W = photon_shape(shape, what)
    if mask is None:
        return None
    m = mask.detach().cpu().numpy() if isinstance(mask, torch.Tensor) else np.asarray(mask)
    if m.dtype == np.bool_:
        m = m.astype(np.uint8)
    if m.dtype != np.uint8 or m.size != P * H * W:
        raise ValueError(f"{what}: mask must be uint8 of {P * H * W} elements, got {m.dtype} of {m.size}")
    return np.ascontiguousarray(m.reshape(-1))


def droplet_reference(frames: torch.Tensor, shape, params, mask=None, cap_pix=None, cap=None) -> DropletList:
    """K-14 golden: droplets of every frame.  ``frames``: [F, ...] float32 of ``shape`` = [P, H, W] (or [H, W]),
    1 <= F <= 64; ``params``: a :class:`DropletParams`, or the arguments of :func:`validate_droplet_params` as a
    tuple / dict / bare thr_low.

    A pixel is active iff the mask keeps it and thr_low <= v <= vmax (float32 compares).  Labels come from
    iterated minimum propagation over the four in-panel neighbours with pointer jumping: every active pixel ends
    with the lowest linear index of its 4-connected set.  A set is kept iff one of its pixels has v >= thr_seed.
    q = int64(rint(v * 2^S)) (float32 multiply, ties to even); npix, adu = sum q, sy / sx = sum q * row / column,
    qmax per kept set, in ascending label order.  A frame with nact > cap_pix has ndrop 0 and flag bit 2; one
    with ndrop > cap has flag bit 0; either stores nothing."""
    what = "droplets"
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
        raise ValueError(f"{what}: frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    F = int(frames.shape[0]) if frames.dim() >= 1 else 0
    if F < 1:
        raise ValueError(f"{what}: no frames")
    pp = _droplet_params(params, what)
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    cap_pix, cap = validate_droplet_caps((P, H, W), pp, cap_pix, cap, F, what)
    x = frames.detach().cpu().reshape(F, -1).numpy()
    if x.shape[1] != n:
        raise ValueError(f"{what}: frames of {x.shape[1]} elements for the shape {(P, H, W)}")
    m = droplet_mask((P, H, W), mask, what)
    with np.errstate(invalid="ignore"):
        act = (x >= np.float32(pp.thr_low)) & (x <= np.float32(pp.vmax))
    if m is not None:
        act &= (m != 0)[None, :]
    # minimum propagation: lab = lowest index seen so far, n where inactive
    idx = np.arange(n, dtype=np.int64)
    lab = np.where(act, idx[None, :], n)
    a4 = act.reshape(F, P, H, W)
    while True:
        l4 = lab.reshape(F, P, H, W)
        pad = np.full((F, P, H + 2, W + 2), n, dtype=np.int64)
        pad[:, :, 1:-1, 1:-1] = l4
        nb = np.minimum(np.minimum(pad[:, :, :-2, 1:-1], pad[:, :, 2:, 1:-1]),
                        np.minimum(pad[:, :, 1:-1, :-2], pad[:, :, 1:-1, 2:]))
        new = np.where(a4, np.minimum(l4, nb), n).reshape(F, n)
        # pointer jumping: the label is a pixel of the same set, whose label is no larger
        ext = np.concatenate([new, np.full((F, 1), n, dtype=np.int64)], axis=1)
        for _ in range(4):
            ext[:, :n] = np.take_along_axis(ext, ext[:, :n], axis=1)
        new = ext[:, :n]
        if np.array_equal(new, lab):
            break
        lab = new
    scale = np.float32(2 ** pp.frac_bits)
    nact = act.sum(axis=1).astype(np.int64)
    ndrop = np.zeros(F, dtype=np.int64)
    flags = np.zeros(F, dtype=np.uint8)
    offs = np.zeros(F + 1, dtype=np.int64)
    cols = {k: [] for k in ("label", "npix", "adu", "sy", "sx", "qmax")}
    for f in range(F):
        stored = 0
        if nact[f] > cap_pix:
            flags[f] |= DROPLET_FLAG_PIX_OVERFLOW
        else:
            ai = np.nonzero(act[f])[0]
            v = x[f, ai]
            roots, inv = np.unique(lab[f, ai], return_inverse=True)   # ascending
            seeded = np.zeros(roots.size, dtype=bool)
            np.logical_or.at(seeded, inv, v >= np.float32(pp.thr_seed))
            ndrop[f] = int(seeded.sum())
            if ndrop[f] > cap:
                flags[f] |= DROPLET_FLAG_OVERFLOW
            else:
                stored = int(ndrop[f])
                q = np.rint(v * scale).astype(np.int64)
                r = ai % (H * W)
                yy, xx = r // W, r % W
                k = roots.size

                def red(w):
                    out = np.zeros(k, dtype=np.int64)
                    np.add.at(out, inv, w)
                    return out[seeded]

                qm = np.zeros(k, dtype=np.int64)
                np.maximum.at(qm, inv, q)
                cols["label"].append(roots[seeded].astype(np.int32))
                cols["npix"].append(red(np.ones_like(q)).astype(np.int32))
                cols["adu"].append(red(q))
                cols["sy"].append(red(q * yy))
                cols["sx"].append(red(q * xx))
                cols["qmax"].append(qm[seeded].astype(np.int32))
        offs[f + 1] = offs[f] + stored
    dt = {"label": np.int32, "npix": np.int32, "adu": np.int64, "sy": np.int64, "sx": np.int64, "qmax": np.int32}
    out = {k: torch.from_numpy(np.concatenate(v) if v else np.zeros(0, dtype=dt[k])) for k, v in cols.items()}
    return DropletList(torch.from_numpy(nact.astype(np.int32)), torch.from_numpy(ndrop.astype(np.int32)),
                       torch.from_numpy(flags), torch.from_numpy(offs), out["label"], out["npix"], out["adu"], out["sy"],
                       out["sx"], out["qmax"])


# ---- K-16 ROI statistics -----------------------------------------------------------------------------------------
# (docs/ARCHITECTURE.md, "ROI: the integer contract")
ROI_MAX_RECTS = 16
ROI_VMIN = POWDER_VMIN               # the K-08 window
ROI_VMAX = POWDER_VMAX
ROI_FRAC_BITS = 2
ROI_ROW_WORDS = 8                    # npix, sum, sy, sx, key, 0, 0, 0: one 64-byte line per (frame, rectangle)
ROI_PROJ = ("none", "x", "y", "both")
ROI_QMAX_NONE = -2 ** 31             # qmax of a rectangle without a sample (INT32_MIN); its imax is -1


def validate_roi_proj(proj, what: str = "roi_stats"):
    """(wants proj_x, wants proj_y) of a projection selector -- or ValueError."""
    if proj is None:
        proj = "none"
    if proj not in ROI_PROJ:
        raise ValueError(f"{what}: proj must be one of {', '.join(ROI_PROJ)}, got {proj!r}")
    return proj in ("x", "both"), proj in ("y", "both")


def validate_roi_rects(rects, shape, what: str = "roi_stats") -> np.ndarray:
    """The rectangles as int32 [R, 5] rows (p, y0, y1, x0, x1), half-open, for frames of ``shape`` = [P, H, W]
    (or [H, W]: one panel) -- or ValueError.  1 <= R <= 16, 0 <= p < P, 0 <= y0 < y1 <= H, 0 <= x0 < x1 <= W;
    rectangles are independent (they may overlap or be equal)."""
    P, H, W = photon_shape(shape, what)
    try:
        a = np.asarray(rects.cpu() if isinstance(rects, torch.Tensor) else rects)
    except (TypeError, ValueError):
        raise ValueError(f"{what}: the rectangles must be an integer [R, 5] array") from None
    if a.dtype == object or a.ndim != 2 or a.shape[1] != 5 or not (np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{what}: the rectangles must be an integer [R, 5] array of (p, y0, y1, x0, x1), got "
                         f"{a.dtype} {list(a.shape)}")
    if not 1 <= a.shape[0] <= ROI_MAX_RECTS:
        raise ValueError(f"{what}: {a.shape[0]} rectangles; 1 .. {ROI_MAX_RECTS} are possible")
    a = a.astype(np.int64)
    for r, (p, y0, y1, x0, x1) in enumerate(a.tolist()):
        if not (0 <= p < P and 0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
            raise ValueError(f"{what}: rectangle {r} = (p={p}, y={y0}:{y1}, x={x0}:{x1}) is empty or lies outside "
                             f"frames of shape {(P, H, W)}")
    return np.ascontiguousarray(a.astype(np.int32))


def roi_offsets(rects: np.ndarray):
    """(offx, offy): int64 [R + 1] running sums of the rectangles' widths and heights."""
    r = np.asarray(rects, dtype=np.int64)
    return (np.concatenate([[0], np.cumsum(r[:, 4] - r[:, 3])]).astype(np.int64),
            np.concatenate([[0], np.cumsum(r[:, 2] - r[:, 1])]).astype(np.int64))


def validate_roi_params(vmin, vmax, frac_bits, rects=None, what: str = "roi_stats"):
    """(vmin, vmax) as the float32 values the kernel sees, frac_bits as a Python int and Q = ceil(max(|vmin|,
    |vmax|) * 2^S) -- or ValueError: the window must be finite with vmin <= vmax, 0 <= S <= 16, Q < 2^31 (q is an
    int32) and, for every rectangle of ``rects`` (validated int [R, 5]), Q * area * max(y1 - 1, x1 - 1, 1) <=
    2^63 - 1 (the int64 moments)."""
    lo, hi, S, _thr, Q, _mf = validate_powder_params(vmin, vmax, frac_bits, 0.0, what)
    if rects is not None:
        for r, (_p, y0, y1, x0, x1) in enumerate(np.asarray(rects).tolist()):
            worst = Q * (y1 - y0) * (x1 - x0) * max(y1 - 1, x1 - 1, 1)
            if worst > 2 ** 63 - 1:
                raise ValueError(f"{what}: rectangle {r}: Q * area * max(y1 - 1, x1 - 1, 1) = {worst} must stay at or "
                                 f"below 2^63 - 1 (the int64 moments sy / sx); narrow the window or lower frac_bits")
    return lo, hi, S, Q


def roi_key_decode(key):
    """(qmax int32, imax int32) of key words (any shape; int64 bit patterns or uint64): the largest q and the
    LOWEST frame index that attains it; INT32_MIN and -1 where key == 0 (no sample)."""
    k = np.asarray(key.cpu() if isinstance(key, torch.Tensor) else key)
    k = np.ascontiguousarray(k).view(np.uint64) if k.dtype == np.int64 else k.astype(np.uint64)
    none = k == 0
    q = ((k >> np.uint64(32)).astype(np.int64) - 2 ** 31)
    i = 0xFFFFFFFF - (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (np.where(none, ROI_QMAX_NONE, q).astype(np.int32), np.where(none, -1, i).astype(np.int32))


def roi_stats_reference(frames: torch.Tensor, shape, rects, vmin: float, vmax: float, frac_bits: int, mask=None,
                        proj="none"):
    """K-16 golden: per frame and rectangle the integer statistics of the contract.  ``frames``: [F, ...] float32
    of ``shape`` = [P, H, W] (or [H, W]); ``rects``: int [R, 5] of (p, y0, y1, x0, x1); ``mask``: uint8 [n] or
    None, non-zero = keep.  A pixel counts iff the mask keeps it and vmin <= v <= vmax as float32 (NaN fails, +-inf
    is outside); q = int64(round_half_even(v * 2^S)).  Returns ``(rows, proj_x, proj_y)``: rows int64 [F, R, 8] =
    npix, sum q, sum q * y, sum q * x, key, 0, 0, 0 (y, x inside the panel; key the uint64 bit pattern of the
    maximum of ((uint32) q ^ 0x80000000) << 32 | (0xFFFFFFFF - idx), 0 without a sample); proj_x int64 [F, Lx] and
    proj_y int64 [F, Ly], the rectangles' column and row sums one after the other (zero columns when ``proj``
    does not select the axis)."""
    what = "roi_stats"
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
        raise ValueError(f"{what}: frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    F = int(frames.shape[0]) if frames.dim() >= 1 else 0
    if F < 1:
        raise ValueError(f"{what}: no frames")
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    rc = validate_roi_rects(rects, (P, H, W), what)
    lo, hi, S, _Q = validate_roi_params(vmin, vmax, frac_bits, rc, what)
    want_x, want_y = validate_roi_proj(proj, what)
    x = frames.detach().cpu().reshape(F, -1)
    if x.shape[1] != n:
        raise ValueError(f"{what}: frames of {x.shape[1]} elements for the shape {(P, H, W)}")
    x = x.reshape(F, P, H, W)
    mask, _roi, _R = validate_photon_maps((P, H, W), mask, None, None, what)
    keep = None if mask is None else torch.from_numpy(mask != 0).reshape(P, H, W)
    R = rc.shape[0]
    rows = np.zeros((F, R, ROI_ROW_WORDS), dtype=np.int64)
    px, py = [], []
    for r, (p, y0, y1, x0, x1) in enumerate(rc.tolist()):
        sub = x[:, p, y0:y1, x0:x1]
        ok = (sub >= lo) & (sub <= hi)
        if keep is not None:
            ok &= keep[p, y0:y1, x0:x1]
        q = torch.where(ok, torch.round(torch.where(ok, sub, torch.zeros_like(sub)) * float(2 ** S)),
                        torch.zeros_like(sub)).to(torch.int64)
        ys = torch.arange(y0, y1, dtype=torch.int64).reshape(1, -1, 1)
        xs = torch.arange(x0, x1, dtype=torch.int64).reshape(1, 1, -1)
        rows[:, r, 0] = ok.sum(dim=(1, 2)).numpy()
        rows[:, r, 1] = q.sum(dim=(1, 2)).numpy()
        rows[:, r, 2] = (q * ys).sum(dim=(1, 2)).numpy()
        rows[:, r, 3] = (q * xs).sum(dim=(1, 2)).numpy()
        idx = ((p * H + ys) * W + xs).numpy().astype(np.uint64)
        key = ((q.numpy() + 2 ** 31).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - idx)
        key = np.where(ok.numpy(), key, np.uint64(0)).reshape(F, -1).max(axis=1)
        rows[:, r, 4] = key.view(np.int64)
        if want_x:
            px.append(q.sum(dim=1))
        if want_y:
            py.append(q.sum(dim=2))
    empty = torch.zeros((F, 0), dtype=torch.int64)
    return (torch.from_numpy(rows), torch.cat(px, dim=1) if px else empty, torch.cat(py, dim=1) if py else empty)


# K-17 roibin: the contract's constants (docs/ARCHITECTURE.md, "Roibin: the contract")
ROIBIN_BINS = (1, 2, 4)
ROIBIN_BIN = 2
ROIBIN_STEP = 1.0
ROIBIN_RADIUS = 4
ROIBIN_MAX_RADIUS = 7
ROIBIN_MAX_PEAKS = 4096              # the sort keys of a frame fit LDS
ROIBIN_MAX_FRAMES = 64
ROIBIN_VMIN = POWDER_VMIN            # the K-08 window
ROIBIN_VMAX = POWDER_VMAX
ROIBIN_CODE_NONE = -32768            # the code of a block without a counting pixel
ROIBIN_CODE_MAX = 32767              # codes are clamped to -32767 .. 32767
ROIBIN_Q_BOUND = 2 ** 25             # max(|vmin|, |vmax|) * inv stays below it: 2 S + c fits an int32 at B = 4
ROIBIN_FLAG_OVERFLOW = 1             # npk[f] > max_peaks: which records survived is arbitrary, so no boxes
ROIBIN_FLAG_SKIPPED = 2              # counts[f] < min_peaks: the frame was neither read nor written
ROIBIN_FLAG_BAD = 4                  # a record was not a pixel of the frame (counted in nbad)
ROIBIN_NAN_BITS = 0x7FC00000         # a box cell outside the panel


class RoibinParams(NamedTuple):
    bin: int
    step: float        # as float32
    inv: float         # float32(1.0 / float64(step))
    vmin: float
    vmax: float
    radius: int
    max_peaks: int
    min_peaks: int


class RoibinBatch(NamedTuple):
    npk: torch.Tensor      # int32 [F]
    nbox: torch.Tensor     # int32 [F]
    nbad: torch.Tensor     # int32 [F]
    nsat: torch.Tensor     # int32 [F]
    flags: torch.Tensor    # uint8 [F]
    offs: torch.Tensor     # int64 [F + 1]
    ctr: torch.Tensor      # int32 [K]
    rec: torch.Tensor      # float32 [K, 8]
    box: torch.Tensor      # float32 [K, 2R+1, 2R+1]
    codes: torch.Tensor    # int16 [kept, P, Hb, Wb]: the kept frames only, in frame order


def validate_roibin_params(bin=ROIBIN_BIN, step=ROIBIN_STEP, vmin=ROIBIN_VMIN, vmax=ROIBIN_VMAX, radius=ROIBIN_RADIUS,
                           max_peaks=ROIBIN_MAX_PEAKS, min_peaks=0, what: str = "roibin") -> RoibinParams:
    """The parameters as the values the kernel sees, with ``inv = float32(1.0 / float64(step))`` -- or ValueError.
    Requires bin in {1, 2, 4}, a finite float32 step > 0 with a finite positive inv, a finite window vmin <= vmax
    with ``max(|vmin|, |vmax|) * inv < 2^25`` (float32), radius in 0 .. 7, max_peaks in 1 .. 4096, min_peaks in
    0 .. 2^31 - 1."""
    if isinstance(bin, RoibinParams):
        bin, step, _inv, vmin, vmax, radius, max_peaks, min_peaks = bin
    try:
        B, R = operator.index(bin), operator.index(radius)
        mp, mn = operator.index(max_peaks), operator.index(min_peaks)
    except TypeError:
        raise ValueError(f"{what}: bin, radius, max_peaks and min_peaks must be integers") from None
    if B not in ROIBIN_BINS:
        raise ValueError(f"{what}: bin must be one of {ROIBIN_BINS}, got {B}")
    if not 0 <= R <= ROIBIN_MAX_RADIUS:
        raise ValueError(f"{what}: the box radius must be in 0 .. {ROIBIN_MAX_RADIUS}, got {R}")
    if not 1 <= mp <= ROIBIN_MAX_PEAKS:
        raise ValueError(f"{what}: max_peaks must be in 1 .. {ROIBIN_MAX_PEAKS}, got {mp}")
    if not 0 <= mn < 2 ** 31:
        raise ValueError(f"{what}: min_peaks must be in 0 .. 2^31 - 1, got {mn}")
    try:
        with np.errstate(over="ignore", under="ignore"):
            st, lo, hi = float(np.float32(step)), float(np.float32(vmin)), float(np.float32(vmax))
    except (TypeError, ValueError):
        raise ValueError(f"{what}: step, vmin and vmax must be numbers") from None
    if not (np.isfinite(st) and st > 0.0):
        raise ValueError(f"{what}: step must be finite and positive, got {step}")
    with np.errstate(over="ignore", under="ignore", divide="ignore"):
        inv = float(np.float32(1.0 / np.float64(st)))
    if not (np.isfinite(inv) and inv > 0.0):
        raise ValueError(f"{what}: the scale 1 / step = {inv} is not a finite positive float32")
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError(f"{what}: the value window must be finite, got [{vmin}, {vmax}]")
    if not lo <= hi:
        raise ValueError(f"{what}: empty value window [{vmin}, {vmax}]")
    with np.errstate(over="ignore"):
        top = np.float32(max(abs(lo), abs(hi))) * np.float32(inv)
    if not top < ROIBIN_Q_BOUND:
        raise ValueError(f"{what}: max(|vmin|, |vmax|) / step = {float(top):g} must stay below 2^25 "
                         "(the block sums are int32)")
    return RoibinParams(B, st, inv, lo, hi, R, mp, mn)


def roibin_code_shape(shape, bin, what: str = "roibin"):
    """``(P, Hb, Wb)`` of the codes of frames of ``shape``: Hb = ceil(H / bin), Wb = ceil(W / bin)."""
    P, H, W = photon_shape(shape, what)
    B = int(bin)
    return P, -(-H // B), -(-W // B)


def roibin_frame_bytes(shape, params) -> int:
    """Bytes of a kept frame's codes (what crosses to the host per kept frame, boxes aside)."""
    P, Hb, Wb = roibin_code_shape(shape, params.bin)
    return 2 * P * Hb * Wb


def roibin_valid_records(rec: np.ndarray, shape) -> "tuple[np.ndarray, np.ndarray]":
    """(valid bool [k], ctr int64 [k]) of float32 records [k, 8]: (p, y, x) finite, integral and inside the frame."""
    P, H, W = shape
    valid = np.ones(rec.shape[0], dtype=bool)
    idx = []
    with np.errstate(invalid="ignore"):
        for col, dim in ((0, P), (1, H), (2, W)):
            v = rec[:, col].astype(np.float64)
            ok = np.isfinite(v) & (v >= 0) & (v < dim) & (np.floor(v) == v)
            valid &= ok
            idx.append(np.where(ok, v, 0).astype(np.int64))
    ctr = (idx[0] * H + idx[1]) * W + idx[2]
    return valid, np.where(valid, ctr, 0)


def roibin_reference(frames: torch.Tensor, shape, peaks, counts, params=None, mask=None, **kw) -> RoibinBatch:
    """K-17 golden: lossless peak boxes and binned codes.  ``frames``: [F, ...] float32 of ``shape`` = [P, H, W] (or
    [H, W]), 1 <= F <= 64; ``peaks``: float32 [F, max_peaks, 8] and ``counts``: int32 [F], the peak finder's
    outputs (or hand-made ones); ``params``: a RoibinParams, or the keywords of validate_roibin_params (max_peaks
    must equal peaks.shape[1]); ``mask``: uint8 [n] or None, non-zero = keep.

    Frame f is kept iff counts[f] >= min_peaks; a skipped frame has flags 2 and no codes.  Codes of a kept frame:
    per B x B block (clipped to the panel) the sum S and the count c of q = int(round_half_even(v * inv)) over the
    pixels the mask keeps with vmin <= v <= vmax (float32; NaN and +-inf never count); -32768 when c == 0, else
    clamp(floor_div(2 S + c, 2 c), -32767, 32767), a clamped block adding 1 to nsat[f].  Boxes: npk = max(counts,
    0); npk > max_peaks sets flag bit 0 and gives no boxes; otherwise the records whose (p, y, x) are finite,
    integral and inside the frame (the others add 1 to nbad[f], flag bit 2), ordered by ctr = (p * H + y) * W + x
    with ties by slot: ctr, a bit copy of the record, and the (2R+1)^2 window as bit copies, 0x7FC00000 outside
    the panel.  offs = exclusive scan of nbox."""
    what = "roibin"
    if params is not None and (kw or not isinstance(params, RoibinParams)):
        raise ValueError(f"{what}: give a RoibinParams or the keywords of validate_roibin_params, not both")
    if params is not None:
        kw = params._asdict()
        kw.pop("inv")
    rp = validate_roibin_params(what=what, **kw)
    if not isinstance(frames, torch.Tensor) or frames.dtype != torch.float32:
        raise ValueError(f"{what}: frames must be a float32 tensor, got {getattr(frames, 'dtype', type(frames))}")
    F = int(frames.shape[0]) if frames.dim() >= 1 else 0
    if not 1 <= F <= ROIBIN_MAX_FRAMES:
        raise ValueError(f"{what}: 1 .. {ROIBIN_MAX_FRAMES} frames per batch, got {F}")
    P, H, W = photon_shape(shape, what)
    n = P * H * W
    x = frames.detach().cpu().reshape(F, -1)
    if x.shape[1] != n:
        raise ValueError(f"{what}: frames of {x.shape[1]} elements for the shape {(P, H, W)}")
    x = x.reshape(F, P, H, W)
    pk = peaks.detach().cpu() if isinstance(peaks, torch.Tensor) else torch.as_tensor(np.asarray(peaks))
    ct = counts.detach().cpu() if isinstance(counts, torch.Tensor) else torch.as_tensor(np.asarray(counts))
    if pk.dtype != torch.float32 or tuple(pk.shape) != (F, rp.max_peaks, 8):
        raise ValueError(f"{what}: peaks must be float32 [{F}, {rp.max_peaks}, 8], got {pk.dtype} {list(pk.shape)}")
    if ct.dtype != torch.int32 or tuple(ct.shape) != (F,):
        raise ValueError(f"{what}: counts must be int32 [{F}], got {ct.dtype} {list(ct.shape)}")
    mask, _roi, _R = validate_photon_maps((P, H, W), mask, None, None, what)
    B, R = rp.bin, rp.radius
    Hb, Wb = -(-H // B), -(-W // B)
    cnt = ct.numpy().astype(np.int64)
    kept = cnt >= rp.min_peaks
    npk = np.maximum(cnt, 0)
    over = kept & (npk > rp.max_peaks)

    # codes of the kept frames
    kf = np.nonzero(kept)[0]
    xk = x[torch.from_numpy(kf)]
    ok = (xk >= rp.vmin) & (xk <= rp.vmax)
    if mask is not None:
        ok &= torch.from_numpy(mask != 0).reshape(1, P, H, W)
    q = torch.round(torch.where(ok, xk, torch.zeros_like(xk)) * rp.inv).to(torch.int32)   # one float32 multiply
    qp = torch.zeros((len(kf), P, Hb * B, Wb * B), dtype=torch.int32)
    cp = torch.zeros((len(kf), P, Hb * B, Wb * B), dtype=torch.int32)
    qp[:, :, :H, :W] = q
    cp[:, :, :H, :W] = ok.to(torch.int32)
    S = qp.reshape(-1, P, Hb, B, Wb, B).sum(dim=(3, 5), dtype=torch.int32)
    c = cp.reshape(-1, P, Hb, B, Wb, B).sum(dim=(3, 5), dtype=torch.int32)
    m = torch.div(2 * S + c, 2 * c.clamp(min=1), rounding_mode="floor")
    sat = (c > 0) & ((m > ROIBIN_CODE_MAX) | (m < -ROIBIN_CODE_MAX))
    codes = torch.where(c > 0, m.clamp(-ROIBIN_CODE_MAX, ROIBIN_CODE_MAX),
                        torch.full_like(m, ROIBIN_CODE_NONE)).to(torch.int16)
    nsat = np.zeros(F, dtype=np.int32)
    nsat[kf] = sat.sum(dim=(1, 2, 3)).numpy()

    # boxes
    nbox = np.zeros(F, dtype=np.int32)
    nbad = np.zeros(F, dtype=np.int32)
    flags = np.where(kept, 0, ROIBIN_FLAG_SKIPPED).astype(np.uint8)
    flags[over] |= ROIBIN_FLAG_OVERFLOW
    Wn = 2 * R + 1
    xbits = x.numpy().view(np.uint32)
    ctrs, recs, boxes = [], [], []
    for f in range(F):
        if not kept[f] or over[f]:
            continue
        rec = pk[f, :int(npk[f])].numpy()
        valid, ctr = roibin_valid_records(rec, (P, H, W))
        nbad[f] = int((~valid).sum())
        if nbad[f]:
            flags[f] |= ROIBIN_FLAG_BAD
        slots = np.nonzero(valid)[0]
        slots = slots[np.argsort(ctr[slots], kind="stable")]   # ties by slot
        nbox[f] = len(slots)
        for s in slots.tolist():
            cc = int(ctr[s])
            p, y, xx = cc // (H * W), (cc // W) % H, cc % W
            b = np.full((Wn, Wn), ROIBIN_NAN_BITS, dtype=np.uint32)
            y0, y1, x0, x1 = max(y - R, 0), min(y + R + 1, H), max(xx - R, 0), min(xx + R + 1, W)
            b[y0 - (y - R):y1 - (y - R), x0 - (xx - R):x1 - (xx - R)] = xbits[f, p, y0:y1, x0:x1]
            ctrs.append(cc)
            recs.append(rec[s].view(np.uint32).copy())
            boxes.append(b)
    offs = np.zeros(F + 1, dtype=np.int64)
    offs[1:] = np.cumsum(nbox)
    K = len(ctrs)
    rec_a = (np.stack(recs) if K else np.zeros((0, 8), np.uint32)).view(np.float32)
    box_a = (np.stack(boxes) if K else np.zeros((0, Wn, Wn), np.uint32)).view(np.float32)
    return RoibinBatch(torch.from_numpy(npk.astype(np.int32)), torch.from_numpy(nbox), torch.from_numpy(nbad),
                       torch.from_numpy(nsat), torch.from_numpy(flags), torch.from_numpy(offs),
                       torch.from_numpy(np.asarray(ctrs, dtype=np.int32)), torch.from_numpy(rec_a),
                       torch.from_numpy(box_a), codes)
