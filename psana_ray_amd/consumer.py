"""``psana-ray-consumer``: installed consumer entry point (the reference only ships
examples/psana_consumer.py and never installs it, SURVEY R-14 / Q-9).

    psana-ray-consumer [consumer_id] [--queue_name my] [--ray_namespace default] [--task peakfind]

Joins the queue session through :class:`~psana_ray_amd.data_reader.DataReader` (same defaults as
the producer, fixing Q-3), reads ``[rank, idx, data, photon_energy]`` items (4 fields, fixing the
example's 3-field unpack, Q-1) until the explicit end of stream (fixing Q-2), and runs a task:
``print`` (the reference example's behaviour), ``peakfind`` (on-GPU K-07 peak finder over
zero-copy leased batches), ``radial`` (on-GPU K-08 azimuthal integration: per-frame radial profiles
and an exact integer run accumulator), ``dark`` (on-GPU K-09 dark-run statistics of a RAW queue:
per-pixel integer count / sum / sum of squares per gain candidate), ``sparse`` (on-GPU K-10 zero
suppression: the pixels inside a value window as (index, value) pairs, optionally only of frames with
at least ``--min_peaks`` peaks), ``powder`` (on-GPU K-11 powder statistics: exact per-pixel run sum,
spread, maximum and count above a threshold of the calibrated frames, misses and hits apart with
``--min_peaks``), ``hist`` (on-GPU K-12 per-pixel histograms: the exact spectrum of every pixel of the
calibrated frames, for gain maps), ``photons`` (on-GPU K-13 photon counting: photons per pixel with psana's
neighbour merge, run maps and the per-frame P(k) of up to 8 ROIs), ``droplets`` (on-GPU K-14 connected-pixel
clusters of every frame: label, pixel count, summed charge and centre of mass as integers), ``cube`` (on-GPU
K-15 cube: exact per-pixel run sums of the calibrated frames per bin of the photon energy or of a per-event
table), ``roi`` (on-GPU K-16 ROI statistics: per frame the sum, centre of mass, maximum and projections of up to
16 rectangles, read from the rectangles alone) or ``none``.  ``--out`` writes the peak lists / the radial accumulator / the dark
statistics / the sparse frames / the powder statistics to an ``.npz`` (several consumers' radial files add
with ``psana_ray_amd.radial.merge``, dark files with ``psana_ray_amd.dark.merge``, sparse files join with
``psana_ray_amd.sparse.merge``, powder files merge with ``psana_ray_amd.powder.merge``, histogram files with
``psana_ray_amd.hist.merge``, photon files with ``psana_ray_amd.photons.merge``, droplet files with
``psana_ray_amd.droplets.merge``, cube files with ``psana_ray_amd.cube.merge``, ROI files with
``psana_ray_amd.roi.merge``).
"""
from __future__ import annotations

import argparse
import logging
import os
import signal
import sys
import time

from .config import (DEFAULT_LOG_LEVEL, DEFAULT_PREFETCH, DEFAULT_QUEUE_NAME, DEFAULT_RAY_ADDRESS,
                     DEFAULT_RAY_NAMESPACE, LOG_LEVELS)

log = logging.getLogger("psana_ray_amd.consumer")


def build_parser():
    ap = argparse.ArgumentParser(description="psana-ray consumer")
    ap.add_argument("consumer_id", nargs="?", type=int, default=None,
                    help="consumer id (examples/psana_consumer.py:51); default: claim the next free id")
    ap.add_argument("--ray_address", type=str, default=DEFAULT_RAY_ADDRESS)
    ap.add_argument("--ray_namespace", type=str, default=DEFAULT_RAY_NAMESPACE)
    ap.add_argument("--queue_name", type=str, default=DEFAULT_QUEUE_NAME)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--task", type=str, default="print", choices=["print", "peakfind", "radial", "dark", "sparse", "powder", "hist", "photons", "droplets", "cube", "roi", "roibin", "train", "none"],
                    help="train: online PeakNetLite training from peak-finder labels (trainer.py); radial: radial "
                         "profile I(r) / I(q) of every frame + run accumulator (--nbins ... --radial_mask); dark: "
                         "per-pixel dark-run statistics of a RAW queue (--adu_min / --adu_max); sparse: zero-suppressed "
                         "frames to disk (--sparse_thr ... --min_peaks); powder: per-pixel run sums / spread / max of the "
                         "calibrated frames, misses and hits apart (--powder_vmin ... --min_peaks); hist: per-pixel "
                         "histograms of the calibrated frames (--hist_lo --hist_hi --hist_bins); photons: photons per pixel "
                         "of the calibrated frames (--adu_per_photon ... --photon_roi); droplets: connected clusters of "
                         "pixels above a threshold per frame (--drop_thr_low ... --drop_mask); cube: per-pixel run sums "
                         "per bin of the photon energy or of a per-event table (--cube_by ... --cube_frac_bits); roi: per frame "
                         "the sum, centre of mass, maximum and projections of up to 16 rectangles (--roi ... --roi_mask); roibin: per "
                         "hit a lossless box around every peak plus the frame binned to int16 codes (--rb_bin ... --rb_mask, "
                         "--min_peaks)")
    ap.add_argument("--lr", type=float, default=1e-3, help="--task train: AdamW learning rate")
    ap.add_argument("--save", type=str, default=None, help="--task train: write the model state_dict here")
    ap.add_argument("--ddp", action="store_true",
                    help="--task train: data-parallel training over the consumer processes of a torchrun launch "
                         "(gradients all-reduced by RCCL on GPUs, gloo on the CPU)")
    ap.add_argument("--batch", type=int, default=None,
                    help="frames per peak-finder / training batch (default: config.pipeline_shape -- 64, or 32 when "
                         "the launch puts more ranks than GPUs on this node)")
    ap.add_argument("--prefetch", type=int, default=None,
                    help=f"read-ahead bound: frames delivered but not read yet + grants outstanding (default "
                         f"max({DEFAULT_PREFETCH}, 2 x --batch)); what a crashed consumer can lose")
    ap.add_argument("--max_frames", type=int, default=None)
    ap.add_argument("--thr_peak", type=float, default=20.0)
    ap.add_argument("--son_min", type=float, default=5.0)
    ap.add_argument("--out", type=str, default=None,
                    help="write peaks (npz) when --task peakfind; the radial accumulator + per-frame profiles (npz) "
                         "when --task radial; the dark statistics (psana_ray_amd.dark.DarkStats npz) when --task dark; "
                         "the sparse frames (psana_ray_amd.sparse.SparseFrames npz) when --task sparse; the powder "
                         "statistics (psana_ray_amd.powder.PowderStats npz) when --task powder; the per-pixel histograms "
                         "(psana_ray_amd.hist.PixelHist npz) when --task hist; the photon statistics "
                         "(psana_ray_amd.photons.PhotonStats npz) when --task photons; the droplet lists "
                         "(psana_ray_amd.droplets.DropletFrames npz) when --task droplets; the cube "
                         "(psana_ray_amd.cube.CubeStats npz) when --task cube; the per-frame ROI records "
                         "(psana_ray_amd.roi.RoiFrames npz) when --task roi; the peak boxes and binned codes "
                         "(psana_ray_amd.roibin.RoibinFrames npz) when --task roibin")
    g = ap.add_argument_group("--task radial")
    g.add_argument("--nbins", type=int, default=512, help="radial bins (1 .. 4096)")
    g.add_argument("--center", type=str, default=None, help="beam centre Y,X in image pixels (default: image centre)")
    g.add_argument("--r_range", type=str, default=None, help="LO,HI of the bins in --unit (default: 0 .. the largest)")
    g.add_argument("--unit", type=str, default="r_px", choices=["r_px", "q"],
                   help="bin in pixel radius, or in q = 4 pi sin(theta) / lambda [1/A] (needs --distance_mm and "
                        "--photon_energy_kev)")
    g.add_argument("--distance_mm", type=float, default=None, help="sample-detector distance")
    g.add_argument("--photon_energy_kev", type=float, default=None, help="photon energy of the run (fixed)")
    g.add_argument("--vmin", type=float, default=None, help="value window: pixels below are ignored (default -2^20)")
    g.add_argument("--vmax", type=float, default=None, help="value window: pixels above are ignored (default 2^20)")
    g.add_argument("--radial_mask", type=str, default=None, help="frame-shaped uint8 .npy, 1 = keep")
    g.add_argument("--detector_name", type=str, default=None,
                   help="detector of the queue's frames when the session does not name it (older producers)")
    g = ap.add_argument_group("--task dark")
    g.add_argument("--adu_min", type=int, default=0, help="ADU window: samples below are ignored (default 0)")
    g.add_argument("--adu_max", type=int, default=65535, help="ADU window: samples above are ignored (default 65535)")
    add_sparse_arguments(ap)
    add_powder_arguments(ap)
    add_hist_arguments(ap)
    add_photon_arguments(ap)
    add_droplet_arguments(ap)
    add_cube_arguments(ap)
    add_roi_arguments(ap)
    add_roibin_arguments(ap)
    ap.add_argument("--timeout", type=float, default=300.0)
    ap.add_argument("--metrics_interval", type=float, default=10.0, help="seconds between rate lines; 0 disables")
    ap.add_argument("--metrics_json", type=str, default=None, help="append per-interval metrics as JSON lines")
    ap.add_argument("--log_level", type=str, default=DEFAULT_LOG_LEVEL, choices=LOG_LEVELS)
    return ap


def add_sparse_arguments(ap):
    """The flags of ``--task sparse`` (the producer CLI's ``--consumer_task sparse`` takes the same)."""
    g = ap.add_argument_group("--task sparse")
    g.add_argument("--sparse_thr", type=float, default=20.0,
                   help="keep pixels with thr <= value (default 20.0, the peak finder's threshold)")
    g.add_argument("--sparse_vmax", type=float, default=float(2 ** 20), help="... and value <= vmax (default 2^20)")
    g.add_argument("--sparse_cap", type=int, default=None,
                   help="pixels kept per frame at most (default n // 16); a frame with more stores nothing and is "
                        "flagged")
    g.add_argument("--sparse_mask", type=str, default=None, help="frame-shaped uint8 .npy, 1 = keep")
    g.add_argument("--min_peaks", type=int, default=0,
                   help="hit filter: keep a frame only if the peak finder (--thr_peak / --son_min) finds at least N "
                        "peaks, decided on the device (default 0: no peak finder)")
    g.add_argument("--part_frames", type=int, default=0,
                   help="K > 0: write parts STEM.00000.npz, ... of at most K frames while running, instead of one "
                        "file at the end")


def add_roibin_arguments(ap):
    """The flags of ``--task roibin`` (the producer CLI's ``--consumer_task roibin`` takes the same); the hit filter
    is --min_peaks / --thr_peak / --son_min and the parts are --part_frames, as for ``--task sparse``."""
    g = ap.add_argument_group("--task roibin")
    g.add_argument("--rb_bin", type=int, default=2, choices=[1, 2, 4],
                   help="the frame is binned B x B outside the peak boxes (default 2)")
    g.add_argument("--rb_step", type=float, default=1.0,
                   help="a code is the block mean in units of step, to within step / 2 (default 1.0); "
                        "max(|vmin|, |vmax|) / step must stay below 2^25")
    g.add_argument("--rb_box", type=int, default=4,
                   help="R in 0 .. 7: the lossless box around a peak is (2R+1) x (2R+1) pixels (default 4)")
    g.add_argument("--rb_vmin", type=float, default=-float(2 ** 20),
                   help="value window: pixels below do not count in a block (default -2^20)")
    g.add_argument("--rb_vmax", type=float, default=float(2 ** 20),
                   help="value window: pixels above do not count in a block (default 2^20)")
    g.add_argument("--rb_mask", type=str, default=None,
                   help=".npy keep-mask of the frames' shape: non-zero = keep (default: every pixel)")


def load_keep_mask(flag, path, shape):
    """``flag`` (``--rb_mask``): a uint8 keep-mask [n] of the frames' shape (an image may come without its leading
    axis of 1), or None; ValueError for another shape."""
    import numpy as np

    if not path:
        return None
    mask = np.load(path)   # allow_pickle stays False
    shape = tuple(shape)
    if tuple(mask.shape) != shape and not (shape[0] == 1 and tuple(mask.shape) == shape[1:]):
        raise ValueError(f"{flag} is {tuple(mask.shape)}, the frames are {shape}")
    return (mask != 0).astype(np.uint8).reshape(-1)


def roibin_consumer(args, endpoint, shape, name, layout, check_ring=True):
    """The RoibinConsumer of ``--task roibin`` / ``--consumer_task roibin`` from the ``--rb_*`` flags."""
    from .config import PeakFinderParams
    from .pipeline import RoibinConsumer

    return RoibinConsumer(endpoint, shape, bin=args.rb_bin, step=args.rb_step, vmin=args.rb_vmin, vmax=args.rb_vmax,
                          radius=args.rb_box, mask=load_keep_mask("--rb_mask", args.rb_mask, shape),
                          min_peaks=args.min_peaks,
                          peak_params=PeakFinderParams(thr_peak=getattr(args, "thr_peak", 20.0),
                                                       son_min=getattr(args, "son_min", 5.0)),
                          detector=name, layout=layout, batch=args.batch, check_ring=check_ring)


def roibin_start_line(cid, cons) -> str:
    p = cons.params
    _P, Hb, Wb = cons.code_shape
    return (f"Consumer {cid} roibin: bin={p.bin} step={p.step:g} window=[{p.vmin:g},{p.vmax:g}] box={2 * p.radius + 1}x"
            f"{2 * p.radius + 1} max_peaks={p.max_peaks} min_peaks={p.min_peaks} codes={Hb}x{Wb} "
            f"frame_bytes={cons.frame_bytes} batch={cons.batch}")


def roibin_final_line(cid, cons) -> str:
    m = cons.metrics()
    return (f"Consumer {cid} roibin: frames={cons.frames} kept={m['frames_kept']} skipped={m['frames_skipped']} "
            f"boxes={m['boxes']} overflowed={m['frames_overflowed']} saturated={m['saturated']}")


def add_powder_arguments(ap):
    """The flags of ``--task powder`` (the producer CLI's ``--consumer_task powder`` takes the same); the hit
    filter is --min_peaks / --thr_peak / --son_min, as for ``--task sparse``."""
    g = ap.add_argument_group("--task powder")
    g.add_argument("--powder_vmin", type=float, default=-float(2 ** 20),
                   help="value window: samples below are ignored (default -2^20)")
    g.add_argument("--powder_vmax", type=float, default=float(2 ** 20),
                   help="value window: samples above are ignored (default 2^20)")
    g.add_argument("--powder_frac_bits", type=int, default=2,
                   help="values are accumulated as round(v * 2^S), S in 0 .. 16 (default 2); max(|vmin|, |vmax|) * 2^S "
                        "must stay below 2^31 and bounds the frames of a run (printed at start)")
    g.add_argument("--powder_thr", type=float, default=20.0,
                   help="count per pixel the samples with value >= thr (default 20.0, the peak finder's threshold)")


def add_hist_arguments(ap):
    """The flags of ``--task hist`` (the producer CLI's ``--consumer_task hist`` takes the same)."""
    g = ap.add_argument_group("--task hist")
    g.add_argument("--hist_lo", type=float, default=-32.0, help="window: samples below are ignored (default -32)")
    g.add_argument("--hist_hi", type=float, default=96.0, help="window: samples above are ignored (default 96)")
    g.add_argument("--hist_bins", type=int, default=64,
                   help="equal bins of [hist_lo, hist_hi], 1 .. 1024 (default 64: bins of 2.0); pixels x bins must "
                        "stay below 2^31, and every consumer stream holds pixels x bins x 4 bytes on the device")


def add_photon_arguments(ap):
    """The flags of ``--task photons`` (the producer CLI's ``--consumer_task photons`` takes the same)."""
    g = ap.add_argument_group("--task photons")
    g.add_argument("--adu_per_photon", type=float, default=None,
                   help="calibrated value of one photon (required for the task)")
    g.add_argument("--photon_vmax", type=float, default=None,
                   help="samples above are ignored (default 250 x adu_per_photon; floor(vmax / adu_per_photon) "
                        "must stay at or below 254)")
    g.add_argument("--photon_seed", type=float, default=0.5,
                   help="a pixel's fractional remainder must reach this to seed a merge (default 0.5)")
    g.add_argument("--photon_total", type=float, default=0.9,
                   help="a seed's remainder plus its largest neighbour's must reach this to count one more photon "
                        "(default 0.9)")
    g.add_argument("--photon_mask", type=str, default=None,
                   help=".npy keep-mask of the frames' shape: non-zero = keep (default: every pixel)")
    g.add_argument("--photon_roi", type=str, default=None,
                   help=".npy uint8 ROI labels of the frames' shape: 0 .. 7, 255 = in no ROI (default: one ROI of "
                        "every pixel); P(k) and the photon total are kept per frame and ROI")


def add_droplet_arguments(ap):
    """The flags of ``--task droplets`` (the producer CLI's ``--consumer_task droplets`` takes the same)."""
    g = ap.add_argument_group("--task droplets")
    g.add_argument("--drop_thr_low", type=float, default=None,
                   help="a pixel is active with thr_low <= value <= vmax (required for the task)")
    g.add_argument("--drop_thr_seed", type=float, default=None,
                   help="a cluster is kept when one of its pixels reaches this (default: thr_low)")
    g.add_argument("--drop_vmax", type=float, default=float(2 ** 20),
                   help="pixels above are inactive and split a cluster (default 2^20)")
    g.add_argument("--drop_frac_bits", type=int, default=2,
                   help="charge is summed as round(v * 2^S), S in 0 .. 16 (default 2); vmax * 2^S must stay below 2^31")
    g.add_argument("--drop_pix_cap", type=int, default=None,
                   help="active pixels per frame at most (default n // 16); a frame with more is not labelled and is "
                        "flagged")
    g.add_argument("--drop_cap", type=int, default=None,
                   help="droplets per frame at most (default n // 64); a frame with more stores nothing and is flagged")
    g.add_argument("--drop_mask", type=str, default=None,
                   help=".npy keep-mask of the frames' shape: non-zero = keep (default: every pixel)")


def add_cube_arguments(ap):
    """The flags of ``--task cube`` (the producer CLI's ``--consumer_task cube`` takes the same)."""
    g = ap.add_argument_group("--task cube")
    g.add_argument("--cube_by", type=str, default="photon_energy", choices=["photon_energy", "gevt"],
                   help="what bins a frame: its photon energy (--cube_edges / --cube_edges_file) or its global event "
                        "number through a table (--cube_table)")
    g.add_argument("--cube_edges", type=str, default=None,
                   help="LO,HI,N: N equal energy bins, edges np.linspace(LO, HI, N + 1); frames outside are dropped")
    g.add_argument("--cube_edges_file", type=str, default=None,
                   help="float .npy of B + 1 strictly increasing bin edges")
    g.add_argument("--cube_table", type=str, default=None,
                   help="--cube_by gevt: integer 1-D .npy, table[gevt] = bin in 0 .. B - 1 or -1 (dropped); a gevt "
                        "outside the table is dropped")
    g.add_argument("--cube_bins", type=int, default=None,
                   help="--cube_by gevt: the number of bins B (default: the table's largest value + 1)")
    g.add_argument("--cube_vmin", type=float, default=-float(2 ** 20),
                   help="value window: samples below are ignored (default -2^20)")
    g.add_argument("--cube_vmax", type=float, default=float(2 ** 20),
                   help="value window: samples above are ignored (default 2^20)")
    g.add_argument("--cube_frac_bits", type=int, default=2,
                   help="values are accumulated as round(v * 2^S), S in 0 .. 16 (default 2); max(|vmin|, |vmax|) * 2^S "
                        "must stay below 2^31 and bounds the frames of a run (printed at start)")


def add_roi_arguments(ap):
    """The flags of ``--task roi`` (the producer CLI's ``--consumer_task roi`` takes the same)."""
    g = ap.add_argument_group("--task roi")
    g.add_argument("--roi", action="append", default=None, metavar="SPEC",
                   help="a rectangle P,Y0:Y1,X0:X1 (panel, rows, columns; half-open) -- Y0:Y1,X0:X1 for 2-D (image) "
                        "frames; repeat for up to 16 rectangles, which may overlap")
    g.add_argument("--roi_file", type=str, default=None,
                   help="integer .npy of [R, 5] rows (p, y0, y1, x0, x1) -- [R, 4] for 2-D frames -- instead of --roi")
    g.add_argument("--roi_proj", type=str, default="none", choices=["none", "x", "y", "both"],
                   help="also keep per frame every rectangle's sum over its rows per column (x), over its columns per "
                        "row (y), or both (default none)")
    g.add_argument("--roi_vmin", type=float, default=-float(2 ** 20),
                   help="value window: pixels below are ignored (default -2^20)")
    g.add_argument("--roi_vmax", type=float, default=float(2 ** 20),
                   help="value window: pixels above are ignored (default 2^20)")
    g.add_argument("--roi_frac_bits", type=int, default=2,
                   help="values are summed as round(v * 2^S), S in 0 .. 16 (default 2); Q = max(|vmin|, |vmax|) * 2^S "
                        "must stay below 2^31, and Q x area x the largest row / column index of a rectangle within "
                        "2^63 - 1")
    g.add_argument("--roi_mask", type=str, default=None,
                   help=".npy keep-mask of the frames' shape: non-zero = keep (default: every pixel)")


def roi_check_flags(args):
    """What can be said about the ``--roi*`` flags before the frames' shape is known, or a ValueError: a source of
    rectangles (one, not both), well-formed specs, a possible window."""
    from .ops.reference import validate_roi_params
    from .roi import RoiSet

    if not args.roi and args.roi_file is None:
        raise ValueError("no rectangle: --roi P,Y0:Y1,X0:X1 (repeatable) or --roi_file PATH.npy")
    if args.roi and args.roi_file is not None:
        raise ValueError("give --roi or --roi_file, not both")
    for spec in args.roi or ():
        try:
            RoiSet.parse_spec(spec, 3)
        except ValueError:
            RoiSet.parse_spec(spec, 2)   # malformed for both: this one's message
    validate_roi_params(args.roi_vmin, args.roi_vmax, args.roi_frac_bits, None, "roi")


def roi_consumer(args, endpoint, shape, name, layout, check_ring=True, batch=None):
    """The RoiConsumer of ``--task roi`` / ``--consumer_task roi`` from the ``--roi*`` flags (ValueError / OSError)."""
    from .pipeline import RoiConsumer
    from .roi import RoiSet

    roi_check_flags(args)
    shape = tuple(shape)
    fshape = shape[1:] if layout == "image" and len(shape) == 3 and shape[0] == 1 else shape   # an image is 2-D
    rs = RoiSet.from_file(args.roi_file, fshape) if args.roi_file is not None else RoiSet.from_specs(args.roi, fshape)
    mask = None
    if args.roi_mask:
        import numpy as np

        m = np.load(args.roi_mask)   # allow_pickle stays False
        if tuple(m.shape) not in (shape, fshape):
            raise ValueError(f"--roi_mask is {tuple(m.shape)}, the frames are {shape}")
        mask = (m != 0).astype(np.uint8).reshape(-1)
    return RoiConsumer(endpoint, fshape, rs, vmin=args.roi_vmin, vmax=args.roi_vmax, frac_bits=args.roi_frac_bits,
                       proj=args.roi_proj, mask=mask, detector=name, layout=layout, batch=batch,
                       check_ring=check_ring)


def roi_start_line(cid, cons) -> str:
    return (f"Consumer {cid} roi: rois={cons.n_roi} proj={cons.proj} window=[{cons.vmin:g},{cons.vmax:g}] "
            f"frac_bits={cons.frac_bits} batch={cons.batch} row_bytes={cons.row_bytes}")


def roi_final_line(cid, cons, name, layout) -> str:
    return (f"Consumer {cid} roi: frames={cons.frames} rois={cons.n_roi} row_bytes={cons.row_bytes} detector={name} "
            f"layout={layout}")


def cube_binning(args):
    """The :class:`psana_ray_amd.cube.CubeBinning` of the ``--cube_*`` flags, or a ValueError / OSError."""
    import numpy as np

    from .cube import CubeBinning

    if args.cube_by == "photon_energy":
        if args.cube_table is not None or args.cube_bins is not None:
            raise ValueError("--cube_table / --cube_bins belong to --cube_by gevt")
        if args.cube_edges is not None and args.cube_edges_file is not None:
            raise ValueError("give --cube_edges or --cube_edges_file, not both")
        if args.cube_edges is not None:
            parts = args.cube_edges.split(",")
            try:
                lo, hi, n = float(parts[0]), float(parts[1]), int(parts[2])
                if len(parts) != 3:
                    raise ValueError
            except (ValueError, IndexError):
                raise ValueError(f"--cube_edges needs LO,HI,N, got {args.cube_edges!r}") from None
            return CubeBinning.linspace(lo, hi, n)
        if args.cube_edges_file is not None:
            return CubeBinning("photon_energy", edges=np.load(args.cube_edges_file, allow_pickle=False))
        raise ValueError("no bin source: --cube_edges LO,HI,N or --cube_edges_file PATH.npy (or --cube_by gevt "
                         "--cube_table PATH.npy)")
    if args.cube_edges is not None or args.cube_edges_file is not None:
        raise ValueError("--cube_edges / --cube_edges_file belong to --cube_by photon_energy")
    if args.cube_table is None:
        raise ValueError("no bin source: --cube_by gevt needs --cube_table PATH.npy")
    return CubeBinning("gevt", table=np.load(args.cube_table, allow_pickle=False), nbins=args.cube_bins)


def cube_start_line(cid, cons) -> str:
    return (f"Consumer {cid} cube: by={cons.binning.by} bins={cons.nbins} max_frames={cons.max_frames} "
            f"window=[{cons.vmin:g},{cons.vmax:g}] frac_bits={cons.frac_bits} set_bytes={cons.set_bytes}")


def cube_final_line(cid, st, consumed: int) -> str:
    if st is None:
        return f"Consumer {cid} cube: frames={consumed} binned=0 dropped=0 bins_filled=0/0"
    binned = int(st.frames.sum())
    return (f"Consumer {cid} cube: frames={binned + st.dropped} binned={binned} dropped={st.dropped} "
            f"bins_filled={int((st.frames > 0).sum())}/{st.nbins}")


def load_droplet_mask(path, shape):
    """``--drop_mask``: a uint8 keep-mask [n] of the frames' shape (an image may come without its leading axis of
    1), or None; ValueError for another shape."""
    import numpy as np

    if not path:
        return None
    mask = np.load(path)   # allow_pickle stays False
    shape = tuple(shape)
    if tuple(mask.shape) != shape and not (shape[0] == 1 and tuple(mask.shape) == shape[1:]):
        raise ValueError(f"--drop_mask is {tuple(mask.shape)}, the frames are {shape}")
    return (mask != 0).astype(np.uint8).reshape(-1)


def droplet_consumer(args, endpoint, shape, name, layout, check_ring=True):
    """The DropletConsumer of ``--task droplets`` / ``--consumer_task droplets`` from the ``--drop_*`` flags."""
    from .pipeline import DropletConsumer

    return DropletConsumer(endpoint, shape, args.drop_thr_low, thr_seed=args.drop_thr_seed, vmax=args.drop_vmax,
                           frac_bits=args.drop_frac_bits, pix_cap=args.drop_pix_cap, cap=args.drop_cap,
                           mask=load_droplet_mask(args.drop_mask, shape), detector=name, layout=layout,
                           batch=args.batch, check_ring=check_ring)


def droplet_start_line(cid, cons) -> str:
    pp = cons.params
    return (f"Consumer {cid} droplets: thr_low={pp.thr_low:g} thr_seed={pp.thr_seed:g} vmax={pp.vmax:g} "
            f"frac_bits={pp.frac_bits} pix_cap={cons.pix_cap} cap={cons.cap} batch={cons.batch} "
            f"scratch_bytes={cons.scratch_bytes} x {max(1, len(cons.streams))}")


def droplet_final_line(cid, cons, name, layout) -> str:
    m = cons.metrics()
    return (f"Consumer {cid} droplets: frames={cons.frames} detector={name} layout={layout} "
            f"stored={m['frames_stored']} droplets={m['droplets_stored']} overflowed={m['frames_overflowed']}")


def load_photon_maps(args, shape):
    """(mask, roi) of ``--photon_mask`` / ``--photon_roi`` as uint8 [n] arrays or None; ValueError for another
    shape or non-integer labels (an image may come without its leading axis of 1)."""
    import numpy as np

    shape = tuple(shape)
    out = []
    for flag, path in (("--photon_mask", args.photon_mask), ("--photon_roi", args.photon_roi)):
        if not path:
            out.append(None)
            continue
        a = np.load(path)   # allow_pickle stays False
        if tuple(a.shape) != shape and not (shape[0] == 1 and tuple(a.shape) == shape[1:]):
            raise ValueError(f"{flag} is {tuple(a.shape)}, the frames are {shape}")
        if flag == "--photon_mask":
            a = (a != 0).astype(np.uint8)
        elif a.dtype != np.uint8:
            if a.dtype.kind not in "iu" or a.size and (int(a.min()) < 0 or int(a.max()) > 255):
                raise ValueError(f"{flag} must hold integer labels 0 .. 7 or 255, got {a.dtype}")
            a = a.astype(np.uint8)
        out.append(np.ascontiguousarray(a).reshape(-1))
    return tuple(out)


def _init_data_parallel(device) -> int:
    """Join the torchrun group of the training consumers: RCCL ("nccl") on GPUs, gloo on the CPU."""
    import torch
    import torch.distributed as dist

    if "WORLD_SIZE" not in os.environ or "RANK" not in os.environ:
        raise SystemExit("--ddp needs a torchrun launch (RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT)")
    dev = torch.device(device)
    if not dist.is_initialized():
        kw = {"device_id": dev} if dev.type == "cuda" else {}
        dist.init_process_group("nccl" if dev.type == "cuda" else "gloo", **kw)
    log.info("data-parallel training: rank %d of %d (%s)", dist.get_rank(), dist.get_world_size(),
             dist.get_backend())
    return dist.get_rank()


def resolve_batch(batch=None) -> int:
    """--batch, else the library's pipeline shape for the ranks sharing this GPU (the producer CLI's
    co-consumer and bench.py resolve the same way)."""
    from .pipeline import resolve_consumer_batch

    return resolve_consumer_batch(batch)


def _pair(text, what):
    try:
        a, b = (float(x) for x in text.split(","))
    except ValueError:
        raise SystemExit(f"{what}: expected two comma-separated numbers, got {text!r}")
    return a, b


def radial_binning(args, detector_name: str, layout: str, frame_shape):
    """The RadialBinning of ``--task radial`` for a queue of ``layout`` frames of ``detector_name``."""
    import numpy as np

    from .models import RadialBinning, get_detector, make_geometry

    geo = make_geometry(get_detector(detector_name))
    mask = np.load(args.radial_mask) if args.radial_mask else None   # allow_pickle stays False
    rb = RadialBinning.from_geometry(geo, layout, args.nbins,
                                     center_px=_pair(args.center, "--center") if args.center else None,
                                     r_range=_pair(args.r_range, "--r_range") if args.r_range else None,
                                     unit=args.unit, distance_mm=args.distance_mm,
                                     photon_energy_kev=args.photon_energy_kev, mask=mask)
    if frame_shape is not None and int(np.prod(frame_shape)) != rb.bins.size:
        raise ValueError(f"the queue's frames {tuple(frame_shape)} are not {layout} frames of {detector_name} "
                         f"{rb.frame_shape}")
    return rb


def _has_whole_frames(reader, task: str, what: str) -> bool:
    """The guards of the tasks that run a pipeline consumer on whole frames: False, after logging why,
    without the distributed queue or on a queue of panel shards (the caller returns 2)."""
    if reader.endpoint is None:
        log.error("--task %s needs the distributed queue (a producer session)", task)
        return False
    if reader.panel_shards > 1:
        log.error("--task %s: the producers queue panel shards (--panel_shards %d); %s need whole frames (out of "
                  "scope)", task, reader.panel_shards, what)
        return False
    return True


def _drive(args, reader, stop, progress, cons, raw_meta=None, each=None) -> int:
    """Feed ``cons`` until the end of the stream, ``stop`` or --max_frames; ``progress["n"]`` counts
    frames.  raw_meta: None to poll the queue; on a raw ring (--calibrate_on_read) the function that
    gives an item's meta tuple -- the items are calibrated here, then processed.  each: called after
    every iteration.  Returns 0, or 1 when the queue died."""
    from .data_reader import DataReaderError, EndOfStream
    from .queue.endpoint import EndOfStream as QueueEOS
    from .queue.endpoint import QueuePeerError

    rc = 0
    try:
        while not stop["flag"] and (args.max_frames is None or progress["n"] < args.max_frames):
            left = None if args.max_frames is None else args.max_frames - progress["n"]
            if raw_meta is None:
                cons.poll(timeout=1.0, max_items=left)
            else:
                items = reader.read_batch(cons.batch if left is None else min(cons.batch, left), timeout=1.0)
                if items:
                    meta = [raw_meta(it) for it in items]
                    frames = reader.calibrate(items)
                    st = cons.process_frames([frames[i] for i in range(len(items))], meta)
                    if st is not None:
                        frames.record_stream(st)
            progress["n"] = cons.frames
            if each is not None:
                each()
    except (EndOfStream, QueueEOS):
        log.info("Consumer %s: end of stream", reader.consumer_id)
    except (DataReaderError, QueuePeerError) as e:
        print(f"DataReader error: {e}")
        print("Queue actor is dead. Exiting...")
        rc = 1
    progress["n"] = cons.frames
    return rc


def run_radial(args, reader, stop, progress) -> int:
    """--task radial: integrate until the end of the stream; ``progress["n"]`` counts frames."""
    import torch

    from . import radial
    from .pipeline import RadialProfileConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "radial", "radial profiles"):
        return 2
    det = (reader.session_meta or {}).get("detector") or {}
    name = det.get("name") or args.detector_name
    if not name:
        log.error("--task radial: the session does not name its detector; pass --detector_name")
        return 2
    ring = reader.endpoint.ring
    cal = reader.calibrator
    if cal is not None:
        layout, shape = cal.mode.value, cal.out_shape
    else:
        layout, shape = det.get("mode"), tuple(ring.frame_shape)
        if layout is None:   # --detector_name fallback: tell the layouts apart by the frame shape
            from .models import get_detector

            layout = "calib" if shape == tuple(get_detector(name).frame_shape) else "image"
    if layout not in ("calib", "image"):
        log.error("--task radial: the queue carries %s frames; radial profiles need calibrated ones", layout)
        return 2
    try:
        binning = radial_binning(args, name, layout, shape)
        cons = RadialProfileConsumer(reader.endpoint, binning, vmin=args.vmin, vmax=args.vmax, batch=args.batch,
                                     keep_results=bool(args.out), check_ring=cal is None)
    except (ValueError, KeyError) as e:
        log.error("--task radial: %s", e)
        return 2
    rc = _drive(args, reader, stop, progress, cons,
                raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt))
    run_sum, run_count, frames = cons.synchronize()
    print(f"Consumer {cid} radial: frames={frames} nbins={binning.nbins} unit={binning.unit} layout={layout} "
          f"detector={name} pixels={int(run_count.sum())}", flush=True)
    if args.out:
        recs = [(p.cpu().numpy() if isinstance(p, torch.Tensor) else p, m) for p, m in cons.results]
        radial.save(args.out, binning, cons.vmin, cons.vmax, cons.frac_bits, run_sum, run_count, frames, recs)
    return rc


def run_dark(args, reader, stop, progress) -> int:
    """--task dark: accumulate the raw frames' statistics until the end of the stream (they are read
    as they are: a --calibrate_on_read queue's raw items are NOT calibrated)."""
    import torch

    from .models import get_detector
    from .pipeline import DarkStatsConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "dark", "dark statistics"):
        return 2
    name = ((reader.session_meta or {}).get("detector") or {}).get("name") or args.detector_name
    if not name:
        log.error("--task dark: the session does not name its detector; pass --detector_name")
        return 2
    if reader.endpoint.ring.dtype != torch.uint16:
        log.error("--task dark: the queue carries %s frames; dark statistics need raw uint16 ones (a producer with "
                  "--mode raw or --calibrate_on_read)", str(reader.endpoint.ring.dtype).replace("torch.", ""))
        return 2
    try:
        cons = DarkStatsConsumer(reader.endpoint, get_detector(name), adu_lo=args.adu_min, adu_hi=args.adu_max,
                                 batch=args.batch)
    except (ValueError, KeyError) as e:
        log.error("--task dark: %s", e)
        return 2
    rc = _drive(args, reader, stop, progress, cons)   # always polls: raw items are what it wants
    st = cons.stats()
    print(f"Consumer {cid} dark: frames={st.frames} detector={name} window=[{st.adu_lo},{st.adu_hi}] "
          f"samples={int(st.cnt.sum())} per_candidate={[int(c) for c in st.cnt.sum(axis=1)]}", flush=True)
    if args.out:
        st.save(args.out)
    return rc


class SparseWriter:
    """Where the finished batches of --task sparse (and, with ``concat`` = roibin.concat, of --task roibin) go:
    frame objects with ``__len__``, ``select`` and ``save`` that ``concat`` joins.  ``part_frames == 0``:
    everything is kept and
    written to ``out`` by :meth:`close`.  ``part_frames = K > 0``: parts ``stem.00000.npz, ...`` of at
    most K frames, written by ONE background thread through a queue of depth 1 -- the run holds at
    most two parts in host memory (the one being filled and the one being written)."""

    def __init__(self, out, part_frames: int = 0, concat=None):
        import queue
        import threading

        if concat is None:
            from .sparse import concat
        self.concat = concat
        self.out = out
        self.part_frames = max(0, int(part_frames or 0))
        self.paths = []
        self._held, self._held_frames, self._part = [], 0, 0
        self._error = None
        self._q = self._thread = None
        if out and self.part_frames:
            self._q = queue.Queue(maxsize=1)
            self._thread = threading.Thread(target=self._work, name="sparse-writer", daemon=True)
            self._thread.start()

    def part_path(self, k: int) -> str:
        stem = self.out[:-4] if self.out.endswith(".npz") else self.out
        return f"{stem}.{k:05d}.npz"

    def _work(self):
        while True:
            job = self._q.get()
            if job is None:
                return
            path, parts = job
            try:
                self.concat(parts).save(path)
            except Exception as e:  # noqa: BLE001 - reported by close()
                self._error = e

    def _emit(self, parts):
        path = self.part_path(self._part)
        self._part += 1
        self.paths.append(path)
        self._q.put((path, parts))   # blocks while the previous part is still being written

    def add(self, batches):
        """Finished batches (frame objects), oldest first."""
        if not self.out:
            return
        for sf in batches:
            if not self.part_frames:
                self._held.append(sf)
                continue
            a = 0
            while a < len(sf):   # cut the batch at part boundaries
                take = min(len(sf) - a, self.part_frames - self._held_frames)
                self._held.append(sf if take == len(sf) else sf.select(range(a, a + take)))
                self._held_frames += take
                a += take
                if self._held_frames == self.part_frames:
                    self._emit(self._held)
                    self._held, self._held_frames = [], 0

    def close(self, empty):
        """Write what is left.  ``empty``: a frame object of no frames with the run's parameters (a run
        without frames still writes its file)."""
        if not self.out:
            return
        if self.part_frames:
            if self._held or not self.paths:
                self._emit(self._held or [empty])
            self._q.put(None)
            self._thread.join()
            if self._error is not None:
                raise self._error
        else:
            self.concat(self._held or [empty]).save(self.out)
            self.paths.append(self.out)


def load_sparse_mask(path, shape):
    """``--sparse_mask``: a uint8 keep-mask [n] of the frames' shape (an image may come without its
    leading axis of 1), or None; ValueError for another shape."""
    import numpy as np

    if not path:
        return None
    mask = np.load(path)   # allow_pickle stays False
    shape = tuple(shape)
    if tuple(mask.shape) != shape and not (shape[0] == 1 and tuple(mask.shape) == shape[1:]):
        raise ValueError(f"--sparse_mask is {tuple(mask.shape)}, the frames are {shape}")
    return (mask != 0).astype(np.uint8).reshape(-1)


def sparse_layout(reader, args, needs="zero suppression needs"):
    """(detector name, layout, frame shape) of the frames --task sparse (or powder) will see, or a ValueError."""
    import torch

    det = (reader.session_meta or {}).get("detector") or {}
    name = det.get("name") or getattr(args, "detector_name", None) or ""
    ring = reader.endpoint.ring
    cal = reader.calibrator
    if cal is not None:
        return name, cal.mode.value, tuple(cal.out_shape)
    shape = tuple(ring.frame_shape)
    layout = det.get("mode")
    if ring.dtype != torch.float32 or layout == "raw":
        raise ValueError(f"the queue carries raw uint16 frames without a calibration recipe; {needs} "
                         "calibrated ones (a producer with --mode calib / image, or --calibrate_on_read)")
    if layout is None:
        layout = "calib" if len(shape) == 3 else "image"
    return name, layout, shape


def run_sparse(args, reader, stop, progress) -> int:
    """--task sparse: zero-suppress until the end of the stream; ``progress["n"]`` counts frames."""
    from .config import PeakFinderParams
    from .pipeline import SparseFrameConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "sparse", "sparse frames"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args)
        mask = load_sparse_mask(args.sparse_mask, shape)
        cons = SparseFrameConsumer(reader.endpoint, shape, thr=args.sparse_thr, vmax=args.sparse_vmax,
                                   cap=args.sparse_cap, mask=mask, min_peaks=args.min_peaks,
                                   peak_params=PeakFinderParams(thr_peak=args.thr_peak, son_min=args.son_min),
                                   detector=name, layout=layout, batch=args.batch, check_ring=cal is None)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task sparse: %s", e)
        return 2
    writer = SparseWriter(args.out, args.part_frames)
    rc = _drive(args, reader, stop, progress, cons,
                raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy),
                each=lambda: writer.add(cons.take_results()))
    cons.synchronize()
    writer.add(cons.take_results())
    writer.close(cons.empty())
    m = cons.metrics()
    print(f"Consumer {cid} sparse: frames={cons.frames} stored={m['frames_stored']} skipped={m['frames_skipped']} "
          f"overflowed={m['frames_overflowed']} pixels={m['pixels_stored']}", flush=True)
    return rc


def run_roibin(args, reader, stop, progress) -> int:
    """--task roibin: peak boxes and binned codes until the end of the stream; ``progress["n"]`` counts frames."""
    from . import roibin

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "roibin", "peak boxes and binned frames"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="roibin needs")
    except ValueError as e:
        log.error("--task roibin: %s", e)
        return 2
    if not name:
        log.error("--task roibin: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = roibin_consumer(args, reader.endpoint, shape, name, layout, check_ring=cal is None)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task roibin: %s", e)
        return 2
    print(roibin_start_line(cid, cons), flush=True)
    writer = SparseWriter(args.out, args.part_frames, concat=roibin.concat)
    rc = _drive(args, reader, stop, progress, cons,
                raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy),
                each=lambda: writer.add(cons.take_results()))
    cons.synchronize()
    writer.add(cons.take_results())
    writer.close(cons.empty())
    print(roibin_final_line(cid, cons), flush=True)
    return rc


def run_powder(args, reader, stop, progress) -> int:
    """--task powder: accumulate until the end of the stream; ``progress["n"]`` counts frames."""
    from .config import PeakFinderParams
    from .pipeline import PowderConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "powder", "powder statistics"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="powder statistics need")
    except ValueError as e:
        log.error("--task powder: %s", e)
        return 2
    if not name:
        log.error("--task powder: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = PowderConsumer(reader.endpoint, shape, vmin=args.powder_vmin, vmax=args.powder_vmax,
                              frac_bits=args.powder_frac_bits, thr_above=args.powder_thr, min_peaks=args.min_peaks,
                              peak_params=PeakFinderParams(thr_peak=args.thr_peak, son_min=args.son_min),
                              detector=name, layout=layout, batch=args.batch, check_ring=cal is None)
    except (ValueError, KeyError) as e:
        log.error("--task powder: %s", e)
        return 2
    print(f"Consumer {cid} powder: max_frames={cons.max_frames} window=[{cons.vmin:g},{cons.vmax:g}] "
          f"frac_bits={cons.frac_bits} thr={cons.thr_above:g} min_peaks={cons.min_peaks}", flush=True)
    try:
        rc = _drive(args, reader, stop, progress, cons,
                    raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt))
    except ValueError as e:   # the run reached max_frames
        log.error("--task powder: %s", e)
        rc = 2
    st = cons.stats()
    fr = [int(f) for f in st.frames]
    print(f"Consumer {cid} powder: frames={fr[0]}+{fr[1] if len(fr) > 1 else 0} detector={name} layout={layout} "
          f"samples={int(st.cnt.sum())} above={int(st.above.sum())}", flush=True)
    if args.out:
        st.save(args.out)
    return rc


def run_hist(args, reader, stop, progress) -> int:
    """--task hist: accumulate until the end of the stream; ``progress["n"]`` counts frames."""
    from .pipeline import PixelHistConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "hist", "pixel histograms"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="pixel histograms need")
    except ValueError as e:
        log.error("--task hist: %s", e)
        return 2
    if not name:
        log.error("--task hist: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = PixelHistConsumer(reader.endpoint, shape, lo=args.hist_lo, hi=args.hist_hi, nbins=args.hist_bins,
                                 detector=name, layout=layout, batch=args.batch, check_ring=cal is None)
    except (ValueError, KeyError) as e:
        log.error("--task hist: %s", e)
        return 2
    print(f"Consumer {cid} hist: window=[{cons.lo:g},{cons.hi:g}] bins={cons.nbins} "
          f"accumulator_bytes={cons.acc_bytes}", flush=True)
    try:
        rc = _drive(args, reader, stop, progress, cons,
                    raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt))
    except ValueError as e:   # the run reached 2^31 - 1 frames
        log.error("--task hist: %s", e)
        rc = 2
    ph = cons.stats()
    print(f"Consumer {cid} hist: frames={ph.frames} detector={name} layout={layout} "
          f"samples={int(ph.hist.sum(dtype='int64'))}", flush=True)
    if args.out:
        ph.save(args.out)
    return rc


def run_photons(args, reader, stop, progress) -> int:
    """--task photons: count until the end of the stream; ``progress["n"]`` counts frames."""
    from .pipeline import PhotonConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "photons", "photon counting"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="photon counting needs")
    except ValueError as e:
        log.error("--task photons: %s", e)
        return 2
    if not name:
        log.error("--task photons: the session does not name its detector; pass --detector_name")
        return 2
    try:
        mask, roi = load_photon_maps(args, shape)
        cons = PhotonConsumer(reader.endpoint, shape, args.adu_per_photon, vmax=args.photon_vmax,
                              thr_seed=args.photon_seed, thr_total=args.photon_total, mask=mask, roi=roi,
                              detector=name, layout=layout, batch=args.batch, check_ring=cal is None)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task photons: %s", e)
        return 2
    pp = cons.params
    print(f"Consumer {cid} photons: adu_per_photon={pp.adu_per_photon:g} vmax={pp.vmax:g} seed={pp.thr_seed:g} "
          f"total={pp.thr_total:g} rois={cons.n_roi}", flush=True)
    try:
        rc = _drive(args, reader, stop, progress, cons,
                    raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy))
    except ValueError as e:   # the run reached 2^31 - 1 frames
        log.error("--task photons: %s", e)
        rc = 2
    st = cons.stats()
    print(f"Consumer {cid} photons: frames={st.frames} detector={name} layout={layout} "
          f"samples={int(st.cnt.sum(dtype='int64'))} photons={int(st.psum.sum())}", flush=True)
    if args.out:
        st.save(args.out)
    return rc


def run_cube(args, reader, stop, progress) -> int:
    """--task cube: accumulate until the end of the stream; ``progress["n"]`` counts frames."""
    from .pipeline import CubeConsumer

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "cube", "the cube"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="the cube needs")
    except ValueError as e:
        log.error("--task cube: %s", e)
        return 2
    if not name:
        log.error("--task cube: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = CubeConsumer(reader.endpoint, shape, cube_binning(args), vmin=args.cube_vmin, vmax=args.cube_vmax,
                            frac_bits=args.cube_frac_bits, detector=name, layout=layout, batch=args.batch,
                            check_ring=cal is None)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task cube: %s", e)
        return 2
    print(cube_start_line(cid, cons), flush=True)
    try:
        rc = _drive(args, reader, stop, progress, cons,
                    raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy))
    except ValueError as e:   # the run reached max_frames
        log.error("--task cube: %s", e)
        rc = 2
    st = cons.stats()
    print(cube_final_line(cid, st, cons.frames), flush=True)
    if args.out:
        st.save(args.out)
    return rc


def run_roi(args, reader, stop, progress) -> int:
    """--task roi: per-frame ROI records until the end of the stream; ``progress["n"]`` counts frames."""
    cid = reader.consumer_id
    if not _has_whole_frames(reader, "roi", "ROI statistics"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="ROI statistics need")
    except ValueError as e:
        log.error("--task roi: %s", e)
        return 2
    if not name:
        log.error("--task roi: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = roi_consumer(args, reader.endpoint, shape, name, layout, check_ring=cal is None, batch=args.batch)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task roi: %s", e)
        return 2
    print(roi_start_line(cid, cons), flush=True)
    rc = _drive(args, reader, stop, progress, cons,
                raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy))
    st = cons.stats()
    print(roi_final_line(cid, cons, name, layout), flush=True)
    if args.out:
        st.save(args.out)
    return rc


def run_droplets(args, reader, stop, progress) -> int:
    """--task droplets: find droplets until the end of the stream; ``progress["n"]`` counts frames."""
    from . import droplets

    cid = reader.consumer_id
    if not _has_whole_frames(reader, "droplets", "droplets"):
        return 2
    cal = reader.calibrator
    try:
        name, layout, shape = sparse_layout(reader, args, needs="droplets need")
    except ValueError as e:
        log.error("--task droplets: %s", e)
        return 2
    if not name:
        log.error("--task droplets: the session does not name its detector; pass --detector_name")
        return 2
    try:
        cons = droplet_consumer(args, reader.endpoint, shape, name, layout, check_ring=cal is None)
    except (ValueError, KeyError, OSError) as e:
        log.error("--task droplets: %s", e)
        return 2
    print(droplet_start_line(cid, cons), flush=True)
    held = []
    rc = _drive(args, reader, stop, progress, cons,
                raw_meta=None if cal is None else lambda it: (it.rank, it.idx, it.gevt, it.photon_energy),
                each=lambda: held.extend(cons.take_results()))
    cons.synchronize()
    held.extend(cons.take_results())
    print(droplet_final_line(cid, cons, name, layout), flush=True)
    if args.out:
        droplets.concat(held or [cons.empty()]).save(args.out)
    return rc


def main(argv=None) -> int:
    args = build_parser().parse_args(argv)
    if args.task == "droplets" and args.drop_thr_low is None:
        print("psana-ray-consumer: --task droplets needs --drop_thr_low", file=sys.stderr)
        return 2
    if args.task == "photons" and args.adu_per_photon is None:
        print("psana-ray-consumer: --task photons needs --adu_per_photon", file=sys.stderr)
        return 2
    if args.task == "cube":   # the bin source is checked before the queue is joined
        try:
            cube_binning(args)
        except (ValueError, OSError) as e:
            print(f"psana-ray-consumer: --task cube: {e}", file=sys.stderr)
            return 2
    if args.task == "roi":   # the rectangles are checked before the queue is joined
        try:
            roi_check_flags(args)
        except (ValueError, OSError) as e:
            print(f"psana-ray-consumer: --task roi: {e}", file=sys.stderr)
            return 2
    logging.basicConfig(level=getattr(logging, args.log_level), format="%(asctime)s - %(levelname)s - %(message)s")
    import numpy as np
    import torch

    from .config import PeakFinderParams
    from .data_reader import DataReader, DataReaderError, EndOfStream

    args.batch = resolve_batch(args.batch)

    stop = {"flag": False}

    def handler(sig, frame):
        print("Ctrl+C pressed. Shutting down...")
        stop["flag"] = True

    signal.signal(signal.SIGINT, handler)
    t0 = time.time()
    n = 0
    peaks_total = 0
    records = []
    from .utils.metrics import Registry, Reporter

    registry = Registry()
    registry.register("consumer", lambda: {"frames_consumed": n, "peaks": peaks_total})
    reporter = None
    with DataReader(args.ray_address, args.queue_name, args.ray_namespace, consumer_id=args.consumer_id,
                    device=args.device, timeout_s=args.timeout,
                    prefetch=args.prefetch or max(DEFAULT_PREFETCH, 2 * args.batch)) as reader:
        cid = reader.consumer_id
        if reader.endpoint is not None:
            registry.register("queue", reader.endpoint.metrics)
        reporter = Reporter(registry, rank=cid if cid is not None else 0, interval=args.metrics_interval,
                            json_path=args.metrics_json).start()
        pf = None
        run_task = {"radial": run_radial, "dark": run_dark, "sparse": run_sparse, "powder": run_powder,
                    "hist": run_hist, "photons": run_photons, "droplets": run_droplets, "cube": run_cube,
                    "roi": run_roi, "roibin": run_roibin}.get(args.task)
        if run_task is not None:   # the tasks that run a pipeline consumer to the end of the stream
            progress = {"n": 0}
            registry.register(args.task, lambda: {"frames_consumed": progress["n"]})
            rc = run_task(args, reader, stop, progress)
            n = progress["n"]
            if rc:
                reporter.stop(final_sample=False)
                return rc
        if args.task == "peakfind":
            from .ops import kernels

            params = PeakFinderParams(thr_peak=args.thr_peak, son_min=args.son_min)
        if args.task == "train":
            if reader.endpoint is None:
                log.error("--task train needs the distributed queue (a producer session)")
                return 2
            from .trainer import OnlinePeakNetTrainer

            ring = reader.endpoint.ring
            shape = reader.calibrator.out_shape if reader.calibrator is not None else ring.frame_shape
            dp_rank = 0
            if args.ddp:
                dp_rank = _init_data_parallel(ring.device)
            trainer = OnlinePeakNetTrainer(shape, ring.device, lr=args.lr,
                                           params=PeakFinderParams(thr_peak=args.thr_peak, son_min=args.son_min),
                                           ddp=args.ddp)
            registry.register("trainer", lambda: {"steps": trainer.steps, "loss": trainer.last_loss})
            try:
                with trainer.join():
                    for batch in reader.batches(args.batch, torch.float32, timeout=1.0):
                        trainer.step(batch.data)
                        n += len(batch)
                        peaks_total = trainer.positives
                        if stop["flag"] or (args.max_frames is not None and n >= args.max_frames):
                            break
            except DataReaderError as e:
                print(f"DataReader error: {e}")
                return 1
            log.info("Consumer %s: %d training steps, last loss %.4f", cid, trainer.steps, trainer.last_loss)
            print(f"Consumer {cid} trained: steps={trainer.steps} frames={n} loss={trainer.last_loss:.4f} "
                  f"params={trainer.param_checksum():.9e}", flush=True)
            if args.save and dp_rank == 0:
                torch.save(trainer.model.state_dict(), args.save)
            if args.ddp:
                import torch.distributed as dist

                dist.destroy_process_group()
        reads_here = args.task in ("print", "peakfind", "none")   # the tasks above ran to their end already
        while reads_here and not stop["flag"] and (args.max_frames is None or n < args.max_frames):
            try:
                if args.task == "peakfind" and reader.endpoint is not None:
                    items = reader.read_batch(args.batch, timeout=1.0)
                    if not items:
                        continue
                    meta_items = [(it.rank, it.idx, it.gevt) for it in items]
                    if reader.calibrator is not None:    # raw ring (--calibrate_on_read): calibrate here
                        frames = reader.calibrate(items)
                    else:
                        frames = [it.data for it in items]
                    shape = tuple(frames[0].shape)
                    dev = frames[0].device
                    F = len(items)
                    if dev.type == "cuda":
                        pk = torch.empty((F, params.max_peaks, 8), dtype=torch.float32, device=dev)
                        cnt = torch.zeros(F, dtype=torch.int32, device=dev)
                        sm = torch.zeros((F, 2), dtype=torch.float32, device=dev)
                        kernels.peakfind([frames[i] for i in range(F)], shape, params, pk, cnt, sm)
                        cnt_h = cnt.cpu()
                        for i, it in enumerate(items):
                            k = min(int(cnt_h[i]), params.max_peaks)
                            peaks_total += k
                            if args.out:
                                records.append((*meta_items[i], pk[i, :k].cpu().numpy()))
                    else:
                        from .ops import reference

                        pl, _ = reference.peakfind_reference(torch.stack([frames[i] for i in range(F)]), params)
                        for m, p in zip(meta_items, pl):
                            peaks_total += p.shape[0]
                            if args.out:
                                records.append((*m, p.numpy()))
                    if reader.calibrator is None:
                        for it in items:
                            it.release()
                    n += F
                else:
                    result = reader.read(timeout=1.0)
                    if result is None:
                        print(f"Consumer {cid} waiting for data...")
                        continue
                    rank, idx, data, photon_energy = result
                    if args.task == "print":
                        print(f"Consumer {cid} processed: rank={rank} | idx={idx} | shape={tuple(data.shape)} "
                              f"| photon_energy={photon_energy}")
                    n += 1
            except EndOfStream:
                log.info("Consumer %s: end of stream", cid)
                break
            except DataReaderError as e:
                print(f"DataReader error: {e}")
                print("Queue actor is dead. Exiting...")
                return 1
    if reporter is not None:
        reporter.stop(final_sample=args.metrics_interval > 0 or args.metrics_json is not None)
    dt = time.time() - t0
    log.info("Consumer %s: %d frames in %.2f s (%.1f frames/s), %d peaks", cid, n, dt, n / max(dt, 1e-9), peaks_total)
    if args.out and records:
        counts = np.array([r[3].shape[0] for r in records], dtype=np.int64)
        np.savez(args.out, rank=np.array([r[0] for r in records]), idx=np.array([r[1] for r in records]),
                 gevt=np.array([r[2] for r in records]), counts=counts,
                 peaks=np.concatenate([r[3].reshape(-1, 8) for r in records]).astype(np.float32))
    return 0


def cli(argv=None) -> int:
    """Console entry: startup failures (no store, no queue session, a queue of another frame
    shape) end with one clear line and rc 1 instead of a traceback."""
    try:
        return main(argv)
    except (TimeoutError, ConnectionError, RuntimeError) as e:
        log.error("consumer could not join the queue: %s", e)
        return 1


if __name__ == "__main__":
    sys.exit(cli())
