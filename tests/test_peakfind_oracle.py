"""The fp32 golden model of the K-07 peak finder (ops.reference.peakfind_reference, the kernel's
twin and the CPU fallback) against the independent float64 per-candidate model of
tests/_peakfind_oracle.py, with per-peak summation bounds.  Runs anywhere (no GPU)."""
import math

import numpy as np
import pytest
import torch

from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.ops import reference
from tests import _peakfind_oracle as orc

RADII = (1, 2)


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", orc.FIXTURES)
def test_float64_model_fixture_preconditions(name, R):
    """What each fixture is built to exercise holds in the float64 model itself: no candidate is
    borderline at son_min, and the planted winners / losers come out by coordinates."""
    fx = orc.fixture(name)
    fx.assert_precondition(R)
    o = fx.oracle(R)
    son = fx.son_min(R)
    orc.assert_coordinates(fx, R, lambda f: {orc._key(c) for c in orc.accepted(o[f], son)})
    if name in ("ties", "many_frames"):
        for f in range(len(o)):   # exactly one winner per plateau: the planted winners and nothing else
            assert sorted(orc._key(c) for c in orc.accepted(o[f], son)) == sorted(fx.winners[f])
    if name == "empty_ring":
        nrs = {orc._key(c): c["nr"] for c in o[0]["cands"]}
        assert all(n == 0 for n in nrs.values()) if R == 2 else all(n > 0 for n in nrs.values()), nrs
        if R == 2:
            assert all(c["bkg"] == 0 and c["noise"] == 0 and c["snr"] == float(c["value"]) / 1e-6
                       for c in o[0]["cands"])
    if name == "threshold":
        assert o[0]["count"] == 4   # three checkerboard candidates + nextafter(thr); the pixel AT thr is none
        by = {orc._key(c): c for c in o[0]["cands"]}
        for k in ((0, 5, 6), (0, 5, 18), (0, 5, 30)):
            assert by[k]["bkg"] == 0 and by[k]["noise"] == 1 and by[k]["snr"] == float(by[k]["value"])
        assert float(by[(0, 5, 6)]["value"]) == son and float(by[(0, 5, 18)]["value"]) < son
    if name == "nonfinite":
        by = {orc._key(c): c for c in o[0]["cands"]}
        full = 40 if R == 1 else 56
        assert by[(0, 6, 6)]["nr"] == full - 2          # two NaNs in its ring
        assert math.isnan(by[(0, 20, 10)]["snr"]) and math.isnan(by[(0, 20, 30)]["snr"])   # +Inf / -Inf in the ring
        assert by[(1, 10, 10)]["snr"] == math.inf and o[0]["sum"] == math.inf
    if name.startswith("paths_"):
        assert all(f["count"] > 512 for f in o), [f["count"] for f in o]
        assert all(len(orc.accepted(f, son)) > 16 for f in o)
    if name.startswith("offset_"):
        assert all(len(orc.accepted(f, son)) >= 30 for f in o)


def golden(fx, R):
    params = PeakFinderParams(thr_peak=fx.thr_peak, son_min=fx.son_min(R), radius=R, max_peaks=fx.max_peaks)
    return reference.peakfind_reference(torch.from_numpy(fx.frames.copy()), params)


@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", orc.FIXTURES)
def test_golden_vs_float64(name, R):
    fx = orc.fixture(name)
    fx.assert_precondition(R)
    peaks, summary = golden(fx, R)
    o = fx.oracle(R)
    for f in range(len(o)):
        rec = peaks[f].numpy()
        orc.check_frame(rec, rec.shape[0], summary[f].numpy(), o[f], fx.son_min(R), R, f"{name} R={R} frame {f}")
    orc.assert_coordinates(fx, R, lambda f: {tuple(int(v) for v in r[:3]) for r in peaks[f].numpy()})


def test_golden_threshold_equality():
    """snr == son_min exactly is kept, one ulp below is dropped; a pixel at thr_peak is no candidate."""
    fx = orc.fixture("threshold")
    for R in RADII:
        peaks, summary = golden(fx, R)
        rec = {tuple(int(v) for v in r[:3]): r for r in peaks[0].numpy()}
        assert rec[(0, 5, 6)][7] == np.float32(orc.THR_EQ_SON) and rec[(0, 5, 6)][5] == 0 and rec[(0, 5, 6)][6] == 1
        assert (0, 5, 18) not in rec and (0, 15, 10) not in rec
        assert summary[0, 0] == 4


def test_f32_two_pass_within_bounds():
    """The calibration of the bounds: a numpy float32 two-pass evaluation (sequential sums, written
    in the test helper, independent of the kernel) stays inside them on every fixture; the worst
    error / bound ratios are printed (and quoted in the helper's docstring)."""
    worst = dict(bkg=0.0, noise=0.0, intensity=0.0)
    for name in orc.FIXTURES:
        fx = orc.fixture(name)
        for R in RADII:
            for f, o in enumerate(fx.oracle(R)):
                for c in o["cands"]:
                    bkg, noise, snr, inten = orc.f32_two_pass(fx.frames[f], c, R)
                    E_b, E_n, E_i = orc.bounds(c, R)
                    for k, got, want, tol in (("bkg", bkg, c["bkg"], E_b), ("noise", noise, c["noise"], E_n),
                                              ("intensity", inten, c["intensity"], E_i)):
                        assert orc._within(got, want, tol), (name, R, f, orc._key(c), k, got, want, tol)
                        if all(map(math.isfinite, (got, want, tol))) and tol > 0:
                            worst[k] = max(worst[k], abs(got - want) / tol)
                    iv = orc.snr_interval(c, R)
                    if iv is None:
                        assert orc._same_nonfinite(snr, c["snr"]), (name, R, f, orc._key(c), snr, c["snr"])
                    else:
                        assert iv[0] <= snr <= iv[1], (name, R, f, orc._key(c), snr, iv)
    print(f"fp32 two-pass vs float64, worst error / bound: {worst}")   # shown with pytest -s
    assert max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", ["offset_1000", "offset_5000"])
def test_old_one_pass_formula_violates_noise_bound(name):
    """The retired one-pass variance s2/nr - bkg^2 in float32 must FAIL the noise bound on the offset
    fixtures: the bounds are tight enough to catch the fault the two-pass variance removed."""
    fx = orc.fixture(name)
    R = 1
    bad, n, worst = 0, 0, 0.0
    for f, o in enumerate(fx.oracle(R)):
        for c in orc.accepted(o, fx.son_min(R)):
            _, E_n, _ = orc.bounds(c, R)
            err = abs(orc.f32_one_pass_noise(fx.frames[f], c, R) - c["noise"])
            n += 1
            bad += err > E_n
            worst = max(worst, err / E_n)
    print(f"{name}: one-pass noise outside the bound on {bad} of {n} peaks, worst error / bound {worst:.1f}")
    assert n >= 60 and bad > n // 2 and worst > 10.0
