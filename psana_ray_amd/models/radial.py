"""Radial binning of a detector for the on-GPU azimuthal integration (K-08, csrc/radial.hip).

``RadialBinning.from_geometry`` turns the pixel placement of :mod:`.geometry` into the static
uint16 bin map the kernel reads: one entry per frame element, ``0xFFFF`` for an element that never
contributes (panel gap, masked pixel, radius outside ``r_range``), else the index of its bin.  Bins
are uniform in the chosen unit -- radius in pixels (``"r_px"``) or momentum transfer
``q = 4 pi sin(theta) / lambda`` in 1/Angstrom (``"q"``, from the sample-detector distance, the
pixel size and ONE photon energy for the run; a per-event energy is out of scope).
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Optional

import numpy as np

from .detector import Mode
from .geometry import Geometry

EXCLUDED = 0xFFFF
MAX_BINS = 4096
HC_KEV_A = 12.398419843320026   # h c in keV * Angstrom
# defaults of the value window and the fixed-point fraction: +-2^20 at S = 8 keeps
# max|v| * 2^S * n below 2^53 up to 2^24-pixel frames (Jungfrau-16M)
DEFAULT_FRAC_BITS = 8
DEFAULT_VMIN = -float(2 ** 20)
DEFAULT_VMAX = float(2 ** 20)


@dataclass
class RadialBinning:
    layout: str                 # "calib" ([P, H, W] frames) or "image" ([1, Himg, Wimg] frames)
    frame_shape: tuple
    nbins: int
    unit: str                   # "r_px" | "q"
    lo: float                   # range covered by the bins, in ``unit``
    hi: float
    center_px: tuple            # (row, col) of the beam centre in image pixels
    bins: np.ndarray            # uint16 [n], n = prod(frame_shape)
    centers: np.ndarray         # float64 [nbins] bin centres in ``unit``
    pixels_per_bin: np.ndarray  # int64 [nbins] pixels mapped to each bin (static, before the value window)
    distance_mm: Optional[float] = None
    photon_energy_kev: Optional[float] = None

    @classmethod
    def from_geometry(cls, geometry: Geometry, layout, nbins: int, center_px=None, r_range=None, unit: str = "r_px",
                      distance_mm: Optional[float] = None, photon_energy_kev: Optional[float] = None,
                      mask=None) -> "RadialBinning":
        """layout: "calib" / "image" (or the Mode).  center_px: (row, col) in image pixels, default the
        image centre.  r_range: (lo, hi) in ``unit``, default 0 .. the largest pixel value.  mask:
        frame-shaped uint8 / bool, 1 = keep."""
        layout = layout.value if isinstance(layout, Mode) else str(layout)
        if layout not in ("calib", "image"):
            raise ValueError(f"radial binning: layout must be 'calib' or 'image', got {layout!r}")
        nbins = int(nbins)
        if not 1 <= nbins <= MAX_BINS:
            raise ValueError(f"radial binning: nbins must be in [1, {MAX_BINS}]")
        if unit not in ("r_px", "q"):
            raise ValueError(f"radial binning: unit must be 'r_px' or 'q', got {unit!r}")
        himg, wimg = geometry.image_shape
        cy, cx = ((himg - 1) / 2.0, (wimg - 1) / 2.0) if center_px is None else (float(center_px[0]), float(center_px[1]))
        r = np.hypot(geometry.rows.astype(np.float64) - cy, geometry.cols.astype(np.float64) - cx)   # [P, H, W]
        if unit == "q":
            if not distance_mm or not photon_energy_kev or distance_mm <= 0 or photon_energy_kev <= 0:
                raise ValueError("radial binning: unit 'q' needs distance_mm and photon_energy_kev (> 0)")
            two_theta = np.arctan(r * geometry.spec.pixel_size_um * 1e-3 / float(distance_mm))
            val = 4.0 * math.pi * np.sin(0.5 * two_theta) * float(photon_energy_kev) / HC_KEV_A
        else:
            val = r
        if r_range is None:
            lo, hi = 0.0, float(np.nextafter(val.max(), np.inf))
        else:
            lo, hi = float(r_range[0]), float(r_range[1])
        if not hi > lo:
            raise ValueError("radial binning: r_range must have hi > lo")
        k = np.floor((val - lo) * (nbins / (hi - lo))).astype(np.int64)
        inside = (val >= lo) & (val < hi)
        k = np.clip(k, 0, nbins - 1)   # guards the rounding of the last bin's upper edge
        pix = np.where(inside, k, EXCLUDED).astype(np.uint16)   # calib layout [P, H, W]
        if layout == "calib":
            shape = tuple(geometry.rows.shape)
            bins = pix.reshape(-1)
        else:
            shape = (1, himg, wimg)
            idx = geometry.index_map()   # image element -> flat source pixel, -1 = gap
            bins = np.where(idx >= 0, pix.reshape(-1)[np.maximum(idx, 0)], EXCLUDED).astype(np.uint16)
        if mask is not None:
            m = np.asarray(mask)
            if m.size != bins.size:
                raise ValueError(f"radial binning: mask of shape {m.shape} does not match the {layout} frames {shape}")
            bins = np.where(m.reshape(-1) != 0, bins, EXCLUDED).astype(np.uint16)
        bins = np.ascontiguousarray(bins)
        edges = lo + (hi - lo) * np.arange(nbins + 1, dtype=np.float64) / nbins
        ppb = np.bincount(bins[bins != EXCLUDED].astype(np.int64), minlength=nbins).astype(np.int64)
        return cls(layout, shape, nbins, unit, lo, hi, (cy, cx), bins, 0.5 * (edges[:-1] + edges[1:]), ppb,
                   None if distance_mm is None else float(distance_mm),
                   None if photon_energy_kev is None else float(photon_energy_kev))

    def bins_tensor(self, device):
        """The bin map as a uint16 tensor on ``device`` (what ops.kernels.radial_profile takes)."""
        import torch

        return torch.from_numpy(self.bins.view(np.int16)).view(torch.uint16).to(device).contiguous()

    def params(self) -> dict:
        """What must agree for two accumulators to be mergeable (psana_ray_amd.radial.merge)."""
        import zlib

        return {"layout": self.layout, "frame_shape": [int(s) for s in self.frame_shape], "nbins": int(self.nbins),
                "unit": self.unit, "lo": float(self.lo), "hi": float(self.hi),
                "center_px": [float(self.center_px[0]), float(self.center_px[1])],
                "distance_mm": self.distance_mm, "photon_energy_kev": self.photon_energy_kev,
                "bins_crc32": int(zlib.crc32(self.bins.tobytes()))}
