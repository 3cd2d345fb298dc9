#!/usr/bin/env python3
"""Per-kernel micro-benchmarks on one MI355X (epix10k2M unless --detector), with rooflines.

Times each HIP kernel over a batch of frames with HIP events (median of --iters) and reports
frames/s, effective HBM GB/s (algorithmic bytes: raw u16 in + f32 out, + f32 in for the peak
finder / assembly) and the fraction of the measured 6.29 TB/s HBM roof
(/opt/skills/guides/MI355X_MICROARCH.md:36).  Also times the pinned host -> HBM copy.
Writes one JSON line per kernel (and to --json-out).
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

import numpy as np
import torch

from psana_ray_amd.config import CommonModeParams, PeakFinderParams
from psana_ray_amd.models import Calibrator, Mode
from psana_ray_amd.ops import _ext, kernels
from psana_ray_amd.source import SyntheticRun

HBM_ROOF = 6.29e12


def timeit(fn, iters=20, warmup=5, reps=8):
    """Median/min GPU seconds of one ``fn()``.

    ``fn`` is captured ``reps`` times into a HIP graph and the graph is replayed between events, so
    the number is device time only (the Python wrappers' argument validation costs more host time
    than some of these kernels take on the GPU; eager event timing would measure the host).
    Falls back to eager timing when capture is impossible."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    g = None
    try:
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(reps):
                fn()
        g.replay()
        torch.cuda.synchronize()
    except Exception as e:  # noqa: BLE001 - report and time eagerly
        print(json.dumps({"warning": f"graph capture failed ({e}); eager timing"}), flush=True)
        g, reps = None, 1
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        if g is not None:
            g.replay()
        else:
            fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e-3 / reps)
    return statistics.median(ts), min(ts)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--detector", default="epix10k2M")
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--json-out", default=None)
    ap.add_argument("--only", default=None, help="comma list of kernels to run")
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    F = a.frames
    src = SyntheticRun("synthetic", 0, a.detector, pool_frames=min(F, 16), pinned=True, gen_device="cuda")
    spec = src.spec
    pool = torch.from_numpy(src.pool.view(np.int16)).view(torch.uint16)
    raw = pool.to(dev).repeat((F + pool.shape[0] - 1) // pool.shape[0], 1, 1, 1)[:F].contiguous()
    rl = [raw[i] for i in range(F)]
    out = torch.empty((F, *spec.frame_shape), dtype=torch.float32, device=dev)
    ol = [out[i] for i in range(F)]
    npix = spec.npix
    results = []
    only = set(a.only.split(",")) if a.only else None

    def report(name, t, nbytes, extra=None, frames=None):
        """frames: the batch that was timed (default: --frames)."""
        F = a.frames if frames is None else frames
        med, best = t
        r = {"kernel": name, "detector": spec.name, "frames": F, "ms_median": round(med * 1e3, 4),
             "us_per_frame": round(med * 1e6 / F, 3), "frames_per_s": round(F / med, 1),
             "GB_per_s": round(nbytes / med / 1e9, 1), "hbm_roof_frac": round(nbytes / med / HBM_ROOF, 3)}
        if extra:
            r.update(extra)
        results.append(r)
        print(json.dumps(r), flush=True)

    def want(k):
        return only is None or k in only

    cal = Calibrator(src.consts, dev, Mode.calib)
    if want("calib_basic"):
        report("calib_basic", timeit(lambda: cal.run(rl, ol), a.iters), F * npix * 6)
    if want("calib_basic"):
        C = _ext.load()
        rp = [int(t.data_ptr()) for t in rl]
        op = [int(t.data_ptr()) for t in ol]
        report("convert_u16_f32 (bandwidth reference)",
               timeit(lambda: C.convert_u16_f32(rp, op, npix, _ext.stream_handle()), a.iters), F * npix * 6)
    if want("calib_cm") and spec.kind != "plain":
        for name, flags in (("rows+cols", 3), ("rows", 1), ("cols", 2), ("memory phases only", 0)):
            c = Calibrator(src.consts, dev, Mode.calib, common_mode=CommonModeParams(flags=flags))
            report(f"calib_cm({name})", timeit(lambda: c.run(rl, ol), a.iters), F * npix * 6)
    if want("calib_cm_image") and spec.kind != "plain":
        # image mode with common mode: the CM kernel writes the assembled image from LDS + gap fill
        c = Calibrator(src.consts, dev, Mode.image, common_mode=CommonModeParams())
        img = torch.empty((F, *c.out_shape), dtype=torch.float32, device=dev)
        il = [img[i] for i in range(F)]
        report("calib_cm_image(fused)", timeit(lambda: c.run(rl, il), a.iters), F * npix * 2 + img.numel() * 4)
    if want("calib_image") and spec.kind != "plain":
        C = _ext.load()
        cali = Calibrator(src.consts, dev, Mode.image)
        tm = cali.tile_map
        img = torch.empty((F, *cali.out_shape), dtype=torch.float32, device=dev)
        il = [img[i] for i in range(F)]
        nout = int(np.prod(cali.out_shape))
        op = [int(t.data_ptr()) for t in ol]
        ip = [int(t.data_ptr()) for t in il]
        extra = {"image_shape": list(cali.out_shape),
                 "tile_direct_frac": round(tm.direct_px / max(1, tm.staged_px + tm.direct_px), 4)}
        report("calib_image(fused, tiles)", timeit(lambda: cali.run(rl, il), a.iters), F * (npix * 2 + nout * 4), extra)
        report("assemble(index map)", timeit(lambda: kernels.assemble(ol, il, cali.idx, npix), a.iters),
               F * (npix * 4 + nout * 4))
        report("assemble(tiles)",
               timeit(lambda: C.image_tiles(op, ip, False, spec.kernel_kind, 0, 0, npix, spec.panel_rows,
                                            spec.panel_cols, int(cali._tiles.data_ptr()), tm.n_tiles, tm.tiles_x,
                                            int(cali._codes.data_ptr()), tm.image_shape[0], tm.image_shape[1],
                                            _ext.stream_handle()), a.iters),
               F * (npix * 4 + nout * 4))
    if want("peakfind"):
        cal.run(rl, ol)
        p = PeakFinderParams()
        peaks = torch.empty((F, p.max_peaks, 8), dtype=torch.float32, device=dev)
        counts = torch.zeros(F, dtype=torch.int32, device=dev)
        summ = torch.zeros((F, 2), dtype=torch.float32, device=dev)
        C = _ext.load()
        sums = torch.zeros(F, dtype=torch.float32, device=dev)
        op = [int(t.data_ptr()) for t in ol]
        report("read_f32 reference (K=16)",
               timeit(lambda: C.read_f32(op, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()), a.iters),
               F * npix * 4)
        report("peakfind", timeit(lambda: kernels.peakfind(ol, spec.frame_shape, p, peaks, counts, summ), a.iters),
               F * npix * 4, {"peaks_per_frame": float(counts.float().mean())})
    if want("radial"):
        # K-08 radial profile on a 64-frame batch (the consumer's batch) with the geometry bin map,
        # 1024 bins; the read floor and the peak finder on the SAME frames in the same run
        from psana_ray_amd.models import RadialBinning, make_geometry

        FR, nb = 64, 1024
        raw64 = pool.to(dev).repeat((FR + pool.shape[0] - 1) // pool.shape[0], 1, 1, 1)[:FR].contiguous()
        out64 = torch.empty((FR, *spec.frame_shape), dtype=torch.float32, device=dev)
        fl = [out64[i] for i in range(FR)]
        cal.run([raw64[i] for i in range(FR)], fl)
        rb = RadialBinning.from_geometry(make_geometry(spec), "calib", nb)
        bins = rb.bins_tensor(dev)
        rsum = torch.zeros((FR, nb), dtype=torch.int64, device=dev)
        rcnt = torch.zeros((FR, nb), dtype=torch.int32, device=dev)
        rprof = torch.zeros((FR, nb), dtype=torch.float32, device=dev)
        run = torch.zeros(2 * nb + 1, dtype=torch.int64, device=dev)
        C = _ext.load()
        fp64 = [int(t.data_ptr()) for t in fl]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        p = PeakFinderParams()
        peaks = torch.empty((FR, p.max_peaks, 8), dtype=torch.float32, device=dev)
        counts = torch.zeros(FR, dtype=torch.int32, device=dev)
        summ = torch.zeros((FR, 2), dtype=torch.float32, device=dev)
        t_read = timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()), a.iters)
        report("read_f32 reference (K=16)", t_read, FR * npix * 4, frames=FR)
        report("peakfind", timeit(lambda: kernels.peakfind(fl, spec.frame_shape, p, peaks, counts, summ), a.iters),
               FR * npix * 4, frames=FR)
        t_rad = timeit(lambda: kernels.radial_profile(fl, bins, nb, rsum, rcnt, rprof, -2.0 ** 20, 2.0 ** 20, 8, run=run),
                       a.iters)
        report("radial", t_rad, FR * npix * 4 + npix * 2,
               {"nbins": nb, "pixels_binned_per_frame": float(rcnt.sum(dim=1).float().mean()),
                "vs_read_floor": round(t_rad[0] / t_read[0], 3)}, frames=FR)
    if want("dark"):
        # K-09 dark statistics: 64 SEPARATELY allocated raw frames (ring slots are not contiguous) into
        # zeroed accumulators, and calib_basic on the SAME 64 frames in the same process -- alternating
        # rounds, the median round of each.  Bytes: the raw frames plus one read-modify-write of the
        # accumulator planes of every candidate the batch hit (20 B per pixel and candidate, each way).
        FR, rounds = 64, 5
        dl = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        dout = torch.empty((FR, *spec.frame_shape), dtype=torch.float32, device=dev)
        dol = [dout[i] for i in range(FR)]
        nc, kind = spec.n_candidates, spec.kernel_kind
        dcnt = torch.zeros((nc, npix), dtype=torch.int32, device=dev)
        dsum = torch.zeros((nc, npix), dtype=torch.int64, device=dev)
        dsq = torch.zeros((nc, npix), dtype=torch.int64, device=dev)
        kernels.dark_accumulate(dl, kind, 0, 65535, dcnt, dsum, dsq)
        torch.cuda.synchronize()
        hit = (dcnt.view(nc, -1, 4) != 0).any(dim=2).float().mean(dim=1).tolist()   # per candidate: lanes that RMW
        for t in (dcnt, dsum, dsq):
            t.zero_()
        t_cal, t_dark = [], []
        for _ in range(rounds):
            t_cal.append(timeit(lambda: cal.run(dl, dol), a.iters))
            t_dark.append(timeit(lambda: kernels.dark_accumulate(dl, kind, 0, 65535, dcnt, dsum, dsq), a.iters))
        mc = sorted(t_cal)[rounds // 2]
        md = sorted(t_dark)[rounds // 2]
        report("calib_basic", mc, FR * npix * 6, {"rounds_us_per_frame": [round(t[0] * 1e6 / FR, 3) for t in t_cal]},
               frames=FR)
        report("dark", md, FR * npix * 2 + int(sum(hit) * npix * 40),
               {"rounds_us_per_frame": [round(t[0] * 1e6 / FR, 3) for t in t_dark],
                "candidate_rmw_fraction": [round(h, 4) for h in hit],
                "vs_calib_basic": round(md[0] / mc[0], 3)}, frames=FR)
    if want("sparsify"):
        # K-10 zero suppression: 64 SEPARATELY allocated calib frames; the read floor and the radial
        # profile on the SAME frames in the same process -- alternating rounds, the median round of
        # each.  Three thresholds (quantiles of the batch: about 0.02 %, 1 % and 5 % kept), the
        # measured densities reported.  The pack kernel's share is measured directly: the pack phase
        # alone, replayed on the scratch block the full launch just filled.
        from psana_ray_amd.models import RadialBinning, make_geometry

        FR, rounds, nb = 64, 5, 1024
        C = _ext.load()
        sraw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        sfl = [torch.empty(spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(FR)]
        cal.run(sraw, sfl)
        torch.cuda.synchronize()
        sample = torch.cat([t.reshape(-1)[::16] for t in sfl]).float()
        sample = sample[torch.isfinite(sample)].sort().values
        thrs = [float(sample[min(sample.numel() - 1, int(sample.numel() * (1.0 - q)))]) for q in (0.0002, 0.01, 0.05)]
        cap = npix // 16
        nnz = torch.zeros(FR, dtype=torch.int32, device=dev)
        flg = torch.zeros(FR, dtype=torch.uint8, device=dev)
        offs = torch.zeros(FR + 1, dtype=torch.int64, device=dev)
        spix = torch.empty(FR * cap, dtype=torch.int32, device=dev)
        sval = torch.empty(FR * cap, dtype=torch.float32, device=dev)
        scr = torch.empty(kernels.sparsify_scratch_bytes(npix, cap, FR), dtype=torch.uint8, device=dev)
        rb = RadialBinning.from_geometry(make_geometry(spec), "calib", nb)
        bins = rb.bins_tensor(dev)
        rsum = torch.zeros((FR, nb), dtype=torch.int64, device=dev)
        rcnt = torch.zeros((FR, nb), dtype=torch.int32, device=dev)
        rprof = torch.zeros((FR, nb), dtype=torch.float32, device=dev)
        run = torch.zeros(2 * nb + 1, dtype=torch.int64, device=dev)
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        fp64 = [int(t.data_ptr()) for t in sfl]

        def sp(thr):
            return lambda: kernels.sparsify(sfl, thr, 2.0 ** 20, cap, nnz, flg, offs, spix, sval, scratch=scr)

        # every frame skipped (keys below key_min): the clear, an empty scan and the pack's header
        # work -- what the two launches cost apart from reading and compacting frames
        skip_keys = torch.zeros(FR, dtype=torch.int32, device=dev)
        t_read, t_rad, t_sp, t_idle = [], [], [[] for _ in thrs], []
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            t_rad.append(timeit(lambda: kernels.radial_profile(sfl, bins, nb, rsum, rcnt, rprof, -2.0 ** 20, 2.0 ** 20, 8,
                                                               run=run), a.iters))
            for k, thr in enumerate(thrs):
                t_sp[k].append(timeit(sp(thr), a.iters))
            t_idle.append(timeit(lambda: kernels.sparsify(sfl, thrs[0], 2.0 ** 20, cap, nnz, flg, offs, spix, sval,
                                                          keys=skip_keys, key_min=1, scratch=scr), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mrad = med(t_read), med(t_rad)
        report("read_f32 reference (K=16)", mr, FR * npix * 4, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("radial", mrad, FR * npix * 4 + npix * 2,
               {"nbins": nb, "rounds_us_per_frame": us(t_rad), "vs_read_floor": round(mrad[0] / mr[0], 3)}, frames=FR)
        report("sparsify(all frames skipped)", med(t_idle), 0, {"rounds_us_per_frame": us(t_idle)}, frames=FR)
        for k, thr in enumerate(thrs):
            sp(thr)()
            torch.cuda.synchronize()
            kept = int(nnz.sum())
            stored = int(offs[FR])
            ms = med(t_sp[k])
            t_pack = timeit(lambda: C.sparsify(fp64, npix, thr, 2.0 ** 20, cap, 0, 0, 0, int(nnz.data_ptr()),
                                               int(flg.data_ptr()), int(offs.data_ptr()), int(spix.data_ptr()),
                                               int(sval.data_ptr()), int(scr.data_ptr()), scr.numel(),
                                               _ext.stream_handle(), 2), a.iters)
            report("sparsify", ms, FR * npix * 4 + stored * 16,
                   {"thr": round(thr, 3), "cap": cap, "density": round(kept / (FR * npix), 6),
                    "frames_overflowed": int((flg & 1).sum()), "pixels_stored": stored,
                    "bytes_written": stored * 16 + FR * 13 + 8,   # staging + packed pairs, and the header
                    "pack_us_per_frame": round(t_pack[0] * 1e6 / FR, 3), "pack_share": round(t_pack[0] / ms[0], 3),
                    "rounds_us_per_frame": us(t_sp[k]), "vs_read_floor": round(ms[0] / mr[0], 3),
                    "vs_radial": round(ms[0] / mrad[0], 3)}, frames=FR)
    if want("powder"):
        # K-11 powder statistics: 64 SEPARATELY allocated calib frames (ring slots are not contiguous),
        # and the read floor on the SAME frames in the same process -- alternating rounds, the median
        # round of each.  Three cases: one class; two classes with 1 frame in 16 a hit; two classes
        # with every frame a hit (class 0 untouched).  Bytes: 4 B per pixel and frame plus one
        # read-modify-write of the accumulator words of every class with a frame in the batch (28 B
        # per pixel and class, each way): 1.22x the floor's bytes with one class touched, 1.44x with two.
        from psana_ray_amd.ops.reference import (POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE, POWDER_VMAX,
                                                 POWDER_VMIN)

        FR, rounds = 64, 5
        C = _ext.load()
        praw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        pfl = [torch.empty(spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(FR)]
        cal.run(praw, pfl)
        torch.cuda.synchronize()
        pflat = [t.reshape(-1) for t in pfl]
        fp64 = [int(t.data_ptr()) for t in pfl]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)

        def acc_set(nc):
            return (torch.zeros(nc, dtype=torch.int64, device=dev), torch.zeros((nc, npix), dtype=torch.int32, device=dev),
                    torch.zeros((nc, npix), dtype=torch.int64, device=dev),
                    torch.zeros((nc, npix), dtype=torch.int64, device=dev),
                    torch.full((nc, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                    torch.zeros((nc, npix), dtype=torch.int32, device=dev))

        def reset(acc):   # every timed window starts a run (it stays far below max_frames)
            for t, v in zip(acc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0)):
                t.fill_(v)

        cases = [("NC=1", None, 1),
                 ("NC=2, 1 hit in 16", torch.tensor([int(f % 16 == 0) for f in range(FR)], dtype=torch.int32, device=dev), 2),
                 ("NC=2, all hits", torch.ones(FR, dtype=torch.int32, device=dev), 1)]
        accs = [acc_set(1 if keys is None else 2) for _, keys, _ in cases]

        def pw(k):
            keys = cases[k][1]
            return lambda: kernels.powder_accumulate(pflat, POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS, POWDER_THR_ABOVE,
                                                     *accs[k], keys=keys, key_min=1)

        t_read, t_pw = [], [[] for _ in cases]
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for k in range(len(cases)):
                reset(accs[k])
                t_pw[k].append(timeit(pw(k), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr = med(t_read)
        report("read_f32 reference (K=16)", mr, FR * npix * 4, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        for k, (name, keys, touched) in enumerate(cases):
            mp = med(t_pw[k])
            nbytes = FR * npix * 4 + touched * npix * 56
            report(f"powder({name})", mp, nbytes,
                   {"classes_touched": touched, "rounds_us_per_frame": us(t_pw[k]),
                    "bytes_vs_read_floor": round(nbytes / (FR * npix * 4), 3),
                    "vs_read_floor": round(mp[0] / mr[0], 3), "TB_per_s": round(nbytes / mp[0] / 1e12, 3)}, frames=FR)
    if want("hist"):
        # K-12 per-pixel histograms: 64 SEPARATELY allocated float32 frames per launch, with the read floor
        # and the powder kernel (one class) on the SAME frames in the same process -- alternating rounds, the
        # median round of each.  Inputs are synthetic so that the accumulator traffic is known: "dark" is
        # Gaussian around 0 with sigma = 2.0 (one bin of the default 64-bin window), "uniform" covers the
        # window evenly (every line of the accumulator is touched: the worst flush).  Bytes: 4 B per pixel and
        # frame plus a read and a write of every 128-B line of the accumulator that one launch touches
        # (counted on the device after one launch into a cleared accumulator).  Every case runs in the three
        # LDS layouts of the kernel: 0 = odd row pitch (the default), 1 = word-major, 2 = unpadded pitch.
        from psana_ray_amd.ops.reference import (HIST_HI, HIST_LO, POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE,
                                                 POWDER_VMAX, POWDER_VMIN)

        FR, rounds = 64, 5
        C = _ext.load()
        gen = torch.Generator(device=dev).manual_seed(12)
        inputs = {"dark": [torch.randn(npix, generator=gen, device=dev) * 2.0 for _ in range(FR)],
                  "uniform": [HIST_LO + torch.rand(npix, generator=gen, device=dev) * (HIST_HI - HIST_LO)
                              for _ in range(FR)]}
        cases = [("64 bins, dark", "dark", 64), ("64 bins, uniform", "uniform", 64), ("256 bins, dark", "dark", 256)]
        hists = {nb: torch.zeros((npix, nb), dtype=torch.int32, device=dev) for nb in (64, 256)}
        touched = []
        for _, inp, nb in cases:
            h = hists[nb]
            h.zero_()
            kernels.pixel_hist(inputs[inp], HIST_LO, HIST_HI, nb, h)
            torch.cuda.synchronize()
            touched.append((int((h.view(-1, 32) != 0).any(dim=1).sum()) * 128, int((h.view(-1, 4) != 0).any(dim=1).sum()) * 16))
        fp64 = [int(t.data_ptr()) for t in inputs["dark"]]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        pacc = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int64, device=dev),
                torch.full((1, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int32, device=dev))

        def hist_fn(k, layout):
            _, inp, nb = cases[k]
            return lambda: kernels.pixel_hist(inputs[inp], HIST_LO, HIST_HI, nb, hists[nb], _layout=layout)

        layouts = (0, 1, 2)
        t_read, t_pw, t_h = [], [], {(k, lay): [] for k in range(len(cases)) for lay in layouts}
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for t, v in zip(pacc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0)):   # every timed window starts a run
                t.fill_(v)
            t_pw.append(timeit(lambda: kernels.powder_accumulate(inputs["dark"], POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS,
                                                                 POWDER_THR_ABOVE, *pacc), a.iters))
            for key in t_h:
                hists[cases[key[0]][2]].zero_()
                t_h[key].append(timeit(hist_fn(*key), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mp = med(t_read), med(t_pw)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("powder(NC=1)", mp, fbytes + npix * 56, {"rounds_us_per_frame": us(t_pw),
                                                        "vs_read_floor": round(mp[0] / mr[0], 3)}, frames=FR)
        for (k, lay), ts in t_h.items():
            name, _, nb = cases[k]
            mh = med(ts)
            nbytes = fbytes + 2 * touched[k][0]
            report(f"pixel_hist({name}, layout {lay})", mh, nbytes,
                   {"nbins": nb, "lds_layout": lay, "rounds_us_per_frame": us(ts),
                    "accumulator_bytes": npix * nb * 4, "lines_touched_bytes": touched[k][0],
                    "chunks16_touched_bytes": touched[k][1], "bytes_vs_read_floor": round(nbytes / fbytes, 3),
                    "vs_read_floor": round(mh[0] / mr[0], 3), "vs_powder": round(mh[0] / mp[0], 3),
                    "TB_per_s": round(nbytes / mh[0] / 1e12, 3)}, frames=FR)
    if want("photons"):
        # K-13 photon counting: 64 SEPARATELY allocated float32 frames per launch, with the read floor and the
        # powder kernel (one class) on the SAME frames in the same process -- alternating rounds, the median
        # round of each.  Inputs are synthetic: "background" is Poisson(0.02) photons per pixel of 10.0 each plus
        # Gaussian noise of 0.1 photon (pixels with k >= 1 are rare: the LDS counters and the merge atomics are
        # nearly idle), "dense" gives EVERY pixel 1 .. 3 photons (every lane of every wave counts into the same
        # few LDS words: the worst case of the counters).  Bytes: 4 B per pixel and frame, a read and a write of
        # the 16 B of accumulators per pixel and launch, and 1 B per pixel and frame where kmap is written.
        from psana_ray_amd.ops.reference import (POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE, POWDER_VMAX,
                                                 POWDER_VMIN)

        FR, rounds, adu = 64, 5, 10.0
        C = _ext.load()
        gen = torch.Generator(device=dev).manual_seed(13)
        shape3 = spec.frame_shape if len(spec.frame_shape) == 3 else (1, *spec.frame_shape)
        rate = torch.full((npix,), 0.02, device=dev)
        inputs = {"background": [(torch.poisson(rate, generator=gen) + 0.1 * torch.randn(npix, generator=gen, device=dev))
                                 * adu for _ in range(FR)],
                  "dense": [(1.0 + torch.randint(0, 3, (npix,), generator=gen, device=dev).float()
                             + 0.3 * torch.rand(npix, generator=gen, device=dev)) * adu for _ in range(FR)]}
        # (name, input, kmap, launch variant): the shape in use first, then the background case in the other launch
        # shapes that were tried: 2 frames in flight instead of 4, and one block per workgroup (no grid cap)
        cases = [("background", "background", False, 0), ("dense", "dense", False, 0),
                 ("background + kmap", "background", True, 0), ("background, 2 frames in flight", "background", False, 1),
                 ("background, grid cap 4096", "background", False, 4096 << 8),
                 ("background, grid cap 512", "background", False, 512 << 8)]
        acc = (torch.zeros(npix, dtype=torch.int32, device=dev), torch.zeros(npix, dtype=torch.int64, device=dev),
               torch.zeros(npix, dtype=torch.int32, device=dev))
        pk = torch.zeros((FR, 1, 8), dtype=torch.int32, device=dev)
        tot = torch.zeros((FR, 1), dtype=torch.int64, device=dev)
        kmap = torch.zeros((FR, npix), dtype=torch.uint8, device=dev)
        kbar = {}
        for name, frames in inputs.items():
            kernels.photons(frames, shape3, adu, *acc, pk, tot)
            torch.cuda.synchronize()
            kbar[name] = float(tot.sum()) / (FR * npix)
        fp64 = [int(t.data_ptr()) for t in inputs["background"]]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        pacc = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int64, device=dev),
                torch.full((1, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int32, device=dev))

        def phot_fn(k):
            _, inp, with_map, variant = cases[k]
            return lambda: kernels.photons(inputs[inp], shape3, adu, *acc, pk, tot, kmap=kmap if with_map else None,
                                           _variant=variant)

        t_read, t_pw, t_ph = [], [], {k: [] for k in range(len(cases))}
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for t, v in zip(pacc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0)):   # every timed window starts a run
                t.fill_(v)
            t_pw.append(timeit(lambda: kernels.powder_accumulate(inputs["background"], POWDER_VMIN, POWDER_VMAX,
                                                                 POWDER_FRAC_BITS, POWDER_THR_ABOVE, *pacc), a.iters))
            for k in t_ph:
                for t in acc:
                    t.zero_()
                t_ph[k].append(timeit(phot_fn(k), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mp = med(t_read), med(t_pw)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("powder(NC=1)", mp, fbytes + npix * 56, {"rounds_us_per_frame": us(t_pw),
                                                        "vs_read_floor": round(mp[0] / mr[0], 3)}, frames=FR)
        for k, ts in t_ph.items():
            name, inp, with_map, variant = cases[k]
            mh = med(ts)
            nbytes = fbytes + npix * 32 + (FR * npix if with_map else 0)
            report(f"photons({name})", mh, nbytes,
                   {"photons_per_pixel": round(kbar[inp], 4), "kmap": with_map, "variant": variant,
                    "rounds_us_per_frame": us(ts),
                    "bytes_vs_read_floor": round(nbytes / fbytes, 3), "vs_read_floor": round(mh[0] / mr[0], 3),
                    "vs_powder": round(mh[0] / mp[0], 3), "TB_per_s": round(nbytes / mh[0] / 1e12, 3)}, frames=FR)
    if want("droplets"):
        # K-14 droplets: 64 SEPARATELY allocated float32 frames per launch, with the read floor and sparsify (same
        # window, cap = pix_cap) on the SAME frames in the same process -- alternating rounds, the median round of
        # each.  Input: the synthetic photon background of the photons row (Poisson(0.02) photons of 10.0 per pixel
        # plus Gaussian noise of 1.0).  Three thresholds: 3.0 (photons and their rare noise neighbours), and the
        # quantiles of the batch that make about 1 % and 5 % of the pixels active (the last deep in the noise:
        # ragged random clusters).  pix_cap = cap = n // 16, so that no case overflows.  The phases are timed one by
        # one on the scratch block a full launch just filled.
        FR, rounds, adu = 64, 5, 10.0
        C = _ext.load()
        gen = torch.Generator(device=dev).manual_seed(13)
        shape3 = spec.frame_shape if len(spec.frame_shape) == 3 else (1, *spec.frame_shape)
        rate = torch.full((npix,), 0.02, device=dev)
        dfl = [(torch.poisson(rate, generator=gen) + 0.1 * torch.randn(npix, generator=gen, device=dev)) * adu
               for _ in range(FR)]
        sample = torch.cat([t[::16] for t in dfl]).sort().values
        cases = [("photon background", 3.0, 5.0)]
        for q in (0.01, 0.05):
            thr = float(sample[int(sample.numel() * (1.0 - q))])
            cases.append((f"{q:.0%} active", thr, thr))
        capp = capd = npix // 16
        nact = torch.zeros(FR, dtype=torch.int32, device=dev)
        ndrop = torch.zeros(FR, dtype=torch.int32, device=dev)
        flg = torch.zeros(FR, dtype=torch.uint8, device=dev)
        offs = torch.zeros(FR + 1, dtype=torch.int64, device=dev)
        i32 = lambda: torch.empty(FR * capd, dtype=torch.int32, device=dev)   # noqa: E731
        i64 = lambda: torch.empty(FR * capd, dtype=torch.int64, device=dev)   # noqa: E731
        cols = (i32(), i32(), i64(), i64(), i64(), i32())
        scr = torch.empty(kernels.droplets_scratch_bytes(npix, capp, capd, FR), dtype=torch.uint8, device=dev)
        spix = torch.empty(FR * capp, dtype=torch.int32, device=dev)
        sval = torch.empty(FR * capp, dtype=torch.float32, device=dev)
        sscr = torch.empty(kernels.sparsify_scratch_bytes(npix, capp, FR), dtype=torch.uint8, device=dev)
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        fp64 = [int(t.data_ptr()) for t in dfl]

        def dr_fn(k, phases=15):
            _, lo, seed = cases[k]
            return lambda: kernels.droplets(dfl, shape3, dict(thr_low=lo, thr_seed=seed), capp, capd, nact, ndrop, flg,
                                            offs, *cols, scratch=scr, _phases=phases)

        def sp_fn(k):
            return lambda: kernels.sparsify(dfl, cases[k][1], 2.0 ** 20, capp, nact, flg, offs, spix, sval, scratch=sscr)

        t_read, t_sp, t_dr = [], {k: [] for k in range(len(cases))}, {k: [] for k in range(len(cases))}
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for k in t_dr:
                t_sp[k].append(timeit(sp_fn(k), a.iters))
                t_dr[k].append(timeit(dr_fn(k), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr = med(t_read)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        for k, (name, lo, seed) in enumerate(cases):
            dr_fn(k)()
            torch.cuda.synchronize()
            active, drops, stored = int(nact.sum()), int(ndrop.sum()), int(offs[FR])
            over = int((flg != 0).sum())
            phase = {}
            for pname, bit in (("scan", 1), ("index_link", 2), ("reduce", 4), ("count_pack", 8)):
                dr_fn(k)()   # a full launch leaves the state every phase starts from
                phase[pname + "_us_per_frame"] = round(timeit(dr_fn(k, bit), a.iters)[0] * 1e6 / FR, 3)
            ms, md = med(t_sp[k]), med(t_dr[k])
            report(f"sparsify({name})", ms, fbytes + active * 16,
                   {"thr": round(lo, 3), "cap": capp, "density": round(active / (FR * npix), 6),
                    "rounds_us_per_frame": us(t_sp[k]), "vs_read_floor": round(ms[0] / mr[0], 3)}, frames=FR)
            report(f"droplets({name})", md, fbytes + active * 16,
                   {"thr_low": round(lo, 3), "thr_seed": round(seed, 3), "pix_cap": capp, "cap": capd,
                    "density": round(active / (FR * npix), 6), "droplets_per_frame": round(drops / FR, 1),
                    "droplets_stored": stored, "frames_overflowed": over, "scratch_bytes": scr.numel(), **phase,
                    "rounds_us_per_frame": us(t_dr[k]), "vs_read_floor": round(md[0] / mr[0], 3),
                    "vs_sparsify": round(md[0] / ms[0], 3)}, frames=FR)
    if want("cube"):
        # K-15 cube: 64 SEPARATELY allocated calib frames into nbins = 64 accumulator planes, the batch's frames
        # spread over G = 1, 2, 8, 64 bins (G = 64: every frame in a bin of its own, a delay scan with jitter),
        # alternating in the same process with the read floor and powder(NC=1) on the SAME frames -- the median
        # round of each.  Bytes: 4 B per pixel and frame plus one read-modify-write of the 20 B per pixel of
        # every bin with a frame in the batch: 4 n F + 2 * 20 n G (1.16x the floor's bytes at G = 1, 11x at 64).
        from psana_ray_amd.ops.reference import (POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE, POWDER_VMAX,
                                                 POWDER_VMIN)

        FR, rounds, NB = 64, 5, 64
        C = _ext.load()
        craw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        cfl = [torch.empty(spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(FR)]
        cal.run(craw, cfl)
        torch.cuda.synchronize()
        del craw
        cflat = [t.reshape(-1) for t in cfl]
        fp64 = [int(t.data_ptr()) for t in cfl]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        pacc = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int64, device=dev),
                torch.full((1, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int32, device=dev))
        cacc = (torch.zeros(NB, dtype=torch.int64, device=dev), torch.zeros((NB, npix), dtype=torch.int32, device=dev),
                torch.zeros((NB, npix), dtype=torch.int64, device=dev),
                torch.zeros((NB, npix), dtype=torch.int64, device=dev))
        groups = (1, 2, 8, 64)
        cbins = [[(f % G) * (NB // G) for f in range(FR)] for G in groups]

        def reset(acc, fills):   # every timed window starts a run (it stays far below max_frames)
            for t, v in zip(acc, fills):
                t.fill_(v)

        def cb(k):
            return lambda: kernels.cube_accumulate(cflat, cbins[k], NB, POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS,
                                                   *cacc)

        t_read, t_pow, t_cube = [], [], [[] for _ in groups]
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            reset(pacc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0))
            t_pow.append(timeit(lambda: kernels.powder_accumulate(cflat, POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS,
                                                                  POWDER_THR_ABOVE, *pacc), a.iters))
            for k in range(len(groups)):
                reset(cacc, (0, 0, 0, 0))
                t_cube[k].append(timeit(cb(k), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mp = med(t_read), med(t_pow)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("powder(NC=1)", mp, fbytes + npix * 56,
               {"rounds_us_per_frame": us(t_pow), "bytes_vs_read_floor": round((fbytes + npix * 56) / fbytes, 3),
                "vs_read_floor": round(mp[0] / mr[0], 3)}, frames=FR)
        m1 = med(t_cube[0])
        for k, G in enumerate(groups):
            mc = med(t_cube[k])
            nbytes = fbytes + 2 * 20 * npix * G
            report(f"cube(G={G})", mc, nbytes,
                   {"nbins": NB, "groups": G, "rounds_us_per_frame": us(t_cube[k]),
                    "bytes_vs_read_floor": round(nbytes / fbytes, 3), "vs_read_floor": round(mc[0] / mr[0], 3),
                    "vs_powder": round(mc[0] / mp[0], 3), "time_vs_G1": round(mc[0] / m1[0], 3),
                    "bytes_vs_G1": round(nbytes / (fbytes + 40 * npix), 3),
                    "TB_per_s": round(nbytes / mc[0] / 1e12, 3)}, frames=FR)
    if want("roi"):
        # K-16 ROI statistics: 64 SEPARATELY allocated calib frames, four sets of rectangles, alternating in the
        # same process with the read floor, powder(NC=1) on the SAME frames and the smallest launch there is (one
        # pixel: the clear and a grid of 64 workgroups) -- the median round of each.  Bytes: 4 B per pixel of the
        # rectangles and frame, plus the rows (64 B per rectangle and frame) and the projection words.
        from psana_ray_amd.ops.reference import (POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE, POWDER_VMAX,
                                                 POWDER_VMIN, ROI_FRAC_BITS, ROI_VMAX, ROI_VMIN)

        FR, rounds = 64, 5
        C = _ext.load()
        P, H, W = spec.frame_shape
        rraw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        rfl = [torch.empty(spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(FR)]
        cal.run(rraw, rfl)
        torch.cuda.synchronize()
        del rraw
        rflat = [t.reshape(-1) for t in rfl]
        fp64 = [int(t.data_ptr()) for t in rfl]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        pacc = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int64, device=dev),
                torch.full((1, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int32, device=dev))
        panels = [(p, 0, H, 0, W) for p in range(min(P, 16))]
        sh, sw, th = min(64, H), min(384, W), min(352, H)
        cases = (("a: whole panels", panels, "none"), ("b: whole panels, both projections", panels, "both"),
                 (f"c: one {sh}x{sw} stripe, proj x", [(P // 2, (H - sh) // 2, (H - sh) // 2 + sh, 0, sw)], "x"),
                 (f"d: one {th}x16 stripe, proj y", [(P // 2, 0, th, 16, 32)], "y"),
                 ("empty: one pixel", [(0, 0, 1, 0, 1)], "none"))

        def bufs(rects, proj):
            Lx = sum(r[4] - r[3] for r in rects) if proj in ("x", "both") else 0
            Ly = sum(r[2] - r[1] for r in rects) if proj in ("y", "both") else 0
            return (torch.zeros((FR, len(rects), 8), dtype=torch.int64, device=dev),
                    torch.zeros((FR, Lx), dtype=torch.int64, device=dev) if Lx else None,
                    torch.zeros((FR, Ly), dtype=torch.int64, device=dev) if Ly else None)

        rb = [bufs(r, p) for _, r, p in cases]
        strip0, ahead0 = C.roi_strip_pixels(), C.roi_rows_ahead()
        # the shipped launch shape, then (measurements only) two larger strip sizes, and 1 and 2 row iterations'
        # loads in flight forced (shipped: 2 for grids of up to 2048 workgroups, 1 beyond)
        strips = (strip0, 2 * strip0, 4 * strip0, -1, -2)

        def rf(k, sp):
            _, rects, _proj = cases[k]
            rows, px, py = rb[k]

            def fn():
                kernels.roi_stats(rflat, spec.frame_shape, rects, ROI_VMIN, ROI_VMAX, ROI_FRAC_BITS, rows, px, py)
            C.roi_strip_pixels(sp if sp > 0 else strip0)   # the plan is built (and cached per strip size) here
            C.roi_rows_ahead(-sp if sp < 0 else ahead0)        # read at launch (and so at graph capture)
            fn()
            return fn

        t_read, t_pow, t_roi = [], [], {(k, sp): [] for k in range(len(cases)) for sp in strips}
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for t, v in zip(pacc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0)):
                t.fill_(v)
            t_pow.append(timeit(lambda: kernels.powder_accumulate(rflat, POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS,
                                                                  POWDER_THR_ABOVE, *pacc), a.iters))
            for k in range(len(cases)):
                for sp in strips:
                    t_roi[k, sp].append(timeit(rf(k, sp), a.iters))
        C.roi_strip_pixels(strip0)
        C.roi_rows_ahead(ahead0)
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mp = med(t_read), med(t_pow)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("powder(NC=1)", mp, fbytes + npix * 56,
               {"rounds_us_per_frame": us(t_pow), "vs_read_floor": round(mp[0] / mr[0], 3)}, frames=FR)
        me = med(t_roi[len(cases) - 1, strip0])
        for sp in strips:
            for k, (name, rects, proj) in enumerate(cases):
                mc = med(t_roi[k, sp])
                area = sum((r[2] - r[1]) * (r[4] - r[3]) for r in rects)
                out_b = sum(0 if t is None else t.numel() * 8 for t in rb[k])
                nbytes = FR * area * 4 + out_b
                report(f"roi({name})" + ("" if sp == strip0 else f" [strips of {sp} px]" if sp > 0 else
                                        f" [{-sp} row iteration(s) of loads in flight]"), mc, nbytes,
                       {"rois": len(rects), "proj": proj, "strip_pixels": sp if sp > 0 else strip0,
                        "rows_ahead": -sp if sp < 0 else ahead0, "area_frac": round(area / npix, 5),
                        "us_per_batch": round(mc[0] * 1e6, 2),
                        "rounds_us_per_batch": [round(t[0] * 1e6, 2) for t in t_roi[k, sp]],
                        "vs_read_floor": round(mc[0] / mr[0], 3), "vs_powder": round(mc[0] / mp[0], 3),
                        "vs_empty_launch": round(mc[0] / me[0], 3)}, frames=FR)
    if want("roibin"):
        # K-17 roibin: 64 SEPARATELY allocated calib frames, alternating in the same process with the read floor and
        # powder(NC=1) on the SAME frames -- the median round of each.  The binning kernel (headers + codes, phase 1)
        # at B = 1, 2, 4 with about 100 hand-made records per frame; the box kernel (phase 2) at about 100 and at 2048
        # records per frame, R = 4; the whole call at B = 2.  Bytes: the frame plus 2 B per code (binning); per box
        # the record read twice, 36 B of ctr + rec and (2R+1)^2 words read and written (boxes).
        from psana_ray_amd.ops.reference import (POWDER_FRAC_BITS, POWDER_QMAX_NONE, POWDER_THR_ABOVE, POWDER_VMAX,
                                                 POWDER_VMIN, validate_roibin_params)

        FR, rounds, MP, R = 64, 5, 2048, 4
        C = _ext.load()
        P, H, W = spec.frame_shape
        rraw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(FR)]
        rfl = [torch.empty(spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(FR)]
        cal.run(rraw, rfl)
        torch.cuda.synchronize()
        del rraw
        rflat = [t.reshape(-1) for t in rfl]
        fp64 = [int(t.data_ptr()) for t in rfl]
        sums = torch.zeros(FR, dtype=torch.float32, device=dev)
        pacc = (torch.zeros(1, dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int64, device=dev), torch.zeros((1, npix), dtype=torch.int64, device=dev),
                torch.full((1, npix), POWDER_QMAX_NONE, dtype=torch.int32, device=dev),
                torch.zeros((1, npix), dtype=torch.int32, device=dev))
        rng = np.random.default_rng(0)
        rec = rng.random((FR, MP, 8)).astype(np.float32)
        rec[:, :, 0] = rng.integers(0, P, (FR, MP))
        rec[:, :, 1] = rng.integers(0, H, (FR, MP))
        rec[:, :, 2] = rng.integers(0, W, (FR, MP))
        peaks = torch.from_numpy(rec).to(dev)
        cnt = {"100": torch.from_numpy(rng.integers(80, 121, FR).astype(np.int32)).to(dev),
               "2048": torch.full((FR,), MP, dtype=torch.int32, device=dev)}
        Wn = 2 * R + 1
        hd = {k: torch.zeros(FR, dtype=torch.int32, device=dev) for k in ("npk", "nbox", "nbad", "nsat")}
        hd["flags"] = torch.zeros(FR, dtype=torch.uint8, device=dev)
        hd["offs"] = torch.zeros(FR + 1, dtype=torch.int64, device=dev)
        cols = {"ctr": torch.zeros(FR * MP, dtype=torch.int32, device=dev),
                "rec": torch.zeros((FR * MP, 8), dtype=torch.float32, device=dev),
                "box": torch.zeros((FR * MP, Wn, Wn), dtype=torch.float32, device=dev)}
        pr = {B: validate_roibin_params(bin=B, radius=R, max_peaks=MP) for B in (1, 2, 4)}
        codes = {B: torch.zeros((FR, P, -(-H // B), -(-W // B)), dtype=torch.int16, device=dev) for B in (1, 2, 4)}

        def rb(B, which, phases):
            def fn():
                kernels.roibin(rflat, spec.frame_shape, pr[B], peaks, cnt[which], codes[B], **hd, **cols, _phases=phases)
            return fn

        cases = [(f"roibin bin(B={B})", B, "100", 1) for B in (1, 2, 4)] + \
                [(f"roibin boxes(~{w} peaks, R={R})", 2, w, 2) for w in ("100", "2048")] + \
                [("roibin(B=2, ~100 peaks)", 2, "100", 3)]
        t_read, t_pow, t_rb = [], [], [[] for _ in cases]
        for _ in range(rounds):
            t_read.append(timeit(lambda: C.read_f32(fp64, npix, 16, False, int(sums.data_ptr()), _ext.stream_handle()),
                                 a.iters))
            for t, v in zip(pacc, (0, 0, 0, 0, POWDER_QMAX_NONE, 0)):
                t.fill_(v)
            t_pow.append(timeit(lambda: kernels.powder_accumulate(rflat, POWDER_VMIN, POWDER_VMAX, POWDER_FRAC_BITS,
                                                                  POWDER_THR_ABOVE, *pacc), a.iters))
            for k, (_name, B, which, phases) in enumerate(cases):
                if phases == 2:
                    rb(B, which, 1)()   # the headers of this record set
                t_rb[k].append(timeit(rb(B, which, phases), a.iters))
        med = lambda ts: sorted(ts)[rounds // 2]   # noqa: E731
        us = lambda ts: [round(t[0] * 1e6 / FR, 3) for t in ts]   # noqa: E731
        mr, mp = med(t_read), med(t_pow)
        fbytes = FR * npix * 4
        report("read_f32 reference (K=16)", mr, fbytes, {"rounds_us_per_frame": us(t_read)}, frames=FR)
        report("powder(NC=1)", mp, fbytes + npix * 56,
               {"rounds_us_per_frame": us(t_pow), "vs_read_floor": round(mp[0] / mr[0], 3)}, frames=FR)
        for k, (name, B, which, phases) in enumerate(cases):
            mc = med(t_rb[k])
            nb = int(cnt[which].sum())
            nbytes = (fbytes + codes[B].numel() * 2 if phases & 1 else 0) + \
                     (nb * (32 + 36 + 8 * Wn * Wn) if phases & 2 else 0)
            report(name, mc, nbytes,
                   {"bin": B, "boxes": nb, "rounds_us_per_frame": us(t_rb[k]), "us_per_batch": round(mc[0] * 1e6, 2),
                    "bytes_vs_read_floor": round(nbytes / fbytes, 3), "vs_read_floor": round(mc[0] / mr[0], 3),
                    "vs_powder": round(mc[0] / mp[0], 3)}, frames=FR)
    if want("h2d"):
        C = _ext.load()
        hp = src.pool
        n = hp.shape[0]

        def h2d():
            C.memcpy_h2d_batch([int(raw[i].data_ptr()) for i in range(F)],
                               [int(hp[i % n].ctypes.data) for i in range(F)], spec.raw_frame_bytes, _ext.stream_handle())
        med, best = timeit(h2d, a.iters)
        r = {"kernel": "h2d_pinned", "detector": spec.name, "frames": F, "ms_median": round(med * 1e3, 4),
             "frames_per_s": round(F / med, 1), "GB_per_s": round(F * spec.raw_frame_bytes / med / 1e9, 1)}
        results.append(r)
        print(json.dumps(r), flush=True)
    if a.json_out:
        with open(a.json_out, "w") as f:
            for r in results:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
