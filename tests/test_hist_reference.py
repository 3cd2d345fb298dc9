"""K-12 golden model (ops.reference.pixel_hist_reference), its parameter checks, and the host side of a
pixel-histogram run: PixelHist views, file format, merge and the gain derivation."""
import numpy as np
import pytest
import torch

from psana_ray_amd import hist as H
from psana_ray_amd.ops.reference import HIST_MAX_FRAMES, pixel_hist_reference, validate_pixel_hist_params

F32 = np.float32


def _np_model(x, lo, hi, nbins):
    """Independent float64 model: np.histogram per pixel (its last bin is closed on the right too)."""
    x = np.asarray(x, np.float64)
    out = np.zeros((x.shape[1], nbins), np.int32)
    for p in range(x.shape[1]):
        v = x[:, p]
        out[p] = np.histogram(v[np.isfinite(v)], bins=nbins, range=(lo, hi))[0]
    return out


@pytest.mark.parametrize("lo,hi,nbins", [(-32.0, 96.0, 64), (0.0, 1.0, 3), (-7.5, 11.25, 255), (100.0, 1124.0, 1024),
                                         (-3.0, 4.0, 1)])
def test_bin_centres_match_a_float64_histogram(lo, hi, nbins):
    """Values at bin centres: no rounding question arises, so float32 bins equal float64 bins."""
    rng = np.random.default_rng(nbins)
    F, n = 37, 29
    centres = lo + (np.arange(nbins) + 0.5) * (hi - lo) / nbins
    x = centres[rng.integers(0, nbins, size=(F, n))].astype(F32)
    got = pixel_hist_reference(torch.from_numpy(x), lo, hi, nbins)
    assert got.dtype == torch.int32 and tuple(got.shape) == (n, nbins)
    assert np.array_equal(got.numpy(), _np_model(x, lo, hi, nbins))
    assert int(got.sum()) == F * n


def test_edges_specials_and_minus_zero():
    lo, hi, nbins = -32.0, 96.0, 64
    na = np.nextafter
    x = np.array([[lo, hi, na(F32(lo), F32(-np.inf)), na(F32(hi), F32(np.inf)), np.nan, np.inf, -np.inf, 0.0, -0.0,
                   na(F32(hi), F32(0))]], F32)
    h = pixel_hist_reference(torch.from_numpy(x), lo, hi, nbins).numpy()
    assert h[0].nonzero()[0].tolist() == [0] and h[1].nonzero()[0].tolist() == [63]      # the window's edges
    assert h[2:7].sum() == 0                                                             # one ulp outside, NaN, +-inf
    assert h[7, 16] == 1 and h[8, 16] == 1 and h[9, 63] == 1
    # -0.0 with lo = 0 goes to bin 0
    z = pixel_hist_reference(torch.tensor([[-0.0, 0.0]]), 0.0, 8.0, 4).numpy()
    assert z[:, 0].tolist() == [1, 1] and z.sum() == 2
    # nbins = 1: everything inside the window, the closed right edge included
    one = pixel_hist_reference(torch.tensor([[-1.0, 0.0, 1.0, 1.0000001, np.nan]]), -1.0, 1.0, 1).numpy()
    assert one.reshape(-1).tolist() == [1, 1, 1, 0, 0]


def test_the_two_float32_roundings_are_the_contract():
    """(v - lo) * inv_w with two float32 roundings, not the float64 value: a case where they differ."""
    lo, hi, nbins = F32(0.1), F32(0.7), 3
    flo, fhi, nb, inv_w = validate_pixel_hist_params(lo, hi, nbins)
    assert inv_w == float(F32(np.float64(3) / (np.float64(fhi) - np.float64(flo))))
    rng = np.random.default_rng(3)
    v = rng.uniform(float(lo), float(hi), size=4096).astype(F32)
    want = np.minimum(nbins - 1, np.floor((v - F32(flo)) * F32(inv_w)).astype(np.int64))
    h = pixel_hist_reference(torch.from_numpy(v.reshape(1, -1)), lo, hi, nbins).numpy()
    assert np.array_equal(h.argmax(axis=1), want) and h.sum() == v.size


def test_frames_add_and_batches_beyond_64():
    rng = np.random.default_rng(9)
    x = torch.from_numpy(rng.normal(10, 30, size=(150, 11)).astype(F32))
    whole = pixel_hist_reference(x, -32.0, 96.0, 64)
    parts = pixel_hist_reference(x[:70], -32.0, 96.0, 64) + pixel_hist_reference(x[70:], -32.0, 96.0, 64)
    assert torch.equal(whole, parts)
    assert torch.equal(pixel_hist_reference(x.reshape(150, 1, 11), -32.0, 96.0, 64), whole)


def test_parameter_refusals():
    v = validate_pixel_hist_params
    assert v(-32, 96, 64) == (-32.0, 96.0, 64, 0.5)
    for lo, hi in ((1.0, 1.0), (2.0, 1.0), (1.0, 1.0 + 1e-9)):   # the last pair is equal as float32
        with pytest.raises(ValueError, match="lo < hi"):
            v(lo, hi, 8)
    for lo, hi in ((float("nan"), 1.0), (0.0, float("inf")), (float("-inf"), 0.0), (0.0, 1e39)):
        with pytest.raises(ValueError, match="finite"):
            v(lo, hi, 8)
    for nb in (0, -1, 1025):
        with pytest.raises(ValueError, match="nbins must be in"):
            v(0.0, 1.0, nb)
    with pytest.raises(ValueError, match="integer"):
        v(0.0, 1.0, 8.5)
    with pytest.raises(ValueError, match="numbers"):
        v("a", 1.0, 8)
    # n * nbins < 2^31
    assert v(0.0, 1.0, 1024, n=2 ** 21 - 1)[2] == 1024
    for n, nb in ((2 ** 21, 1024), (2 ** 31, 1), (0, 4)):
        with pytest.raises(ValueError, match=r"2\^31"):
            v(0.0, 1.0, nb, n=n)
    # a scale that is infinite as float32 (a denormal window).  A zero scale cannot come from a finite
    # float32 window -- the smallest is 1 / (2 * FLT_MAX), a positive subnormal, accepted here -- so the
    # native launcher, which takes the scale itself, refuses zero (tests/test_hist_gpu.py)
    with pytest.raises(ValueError, match="scale"):
        v(0.0, 1e-45, 1024)
    with pytest.raises(ValueError, match="scale"):
        v(0.0, 1e-42, 1024)
    assert 0.0 < v(-3.4e38, 3.4e38, 1)[3] < 2e-39
    # the frame bound
    assert v(0.0, 1.0, 8, frames_so_far=HIST_MAX_FRAMES - 64, frames=64)[2] == 8
    with pytest.raises(ValueError, match="past 2147483647"):
        v(0.0, 1.0, 8, frames_so_far=HIST_MAX_FRAMES - 63, frames=64)
    with pytest.raises(ValueError):
        v(0.0, 1.0, 8, frames_so_far=-1)
    with pytest.raises(ValueError, match="float32"):
        pixel_hist_reference(torch.zeros((2, 3), dtype=torch.float64), 0.0, 1.0, 4)
    with pytest.raises(ValueError, match="no frames"):
        pixel_hist_reference(torch.zeros((0, 3)), 0.0, 1.0, 4)


def _ph(hist, lo=0.0, hi=8.0, frames=None, shape=None, **kw):
    hist = np.asarray(hist, np.int32)
    args = dict(detector="tiny", layout="calib", shape=shape or (hist.shape[0],), lo=lo, hi=hi, nbins=hist.shape[1],
                frames=int(hist.sum(axis=1).max()) if frames is None else frames, hist=hist)
    args.update(kw)
    return H.PixelHist(**args)


def test_views_on_hand_made_histograms():
    h = _ph([[0, 0, 0, 0], [2, 0, 2, 0], [0, 4, 0, 0], [1, 3, 3, 1], [0, 0, 0, 5]])
    assert h.edges().tolist() == [0.0, 2.0, 4.0, 6.0, 8.0] and h.centers().tolist() == [1.0, 3.0, 5.0, 7.0]
    assert h.edges().dtype == np.float64 and h.centers().dtype == np.float64
    assert h.total().tolist() == [3, 7, 5, 6] and h.total().dtype == np.int64
    m = h.mode()
    assert np.isnan(m[0]) and m[1:].tolist() == [1.0, 3.0, 3.0, 7.0]       # ties go to the lowest bin
    # quantile: t = q * N, first non-empty bin with C >= t, linear inside it
    q50 = h.quantile(0.5)
    assert np.isnan(q50[0])
    assert q50[1:].tolist() == [2.0, 3.0, 4.0, 7.0]      # [2,0,2,0]: t = 2 = C[0] -> right edge of bin 0
    assert h.quantile(0.0)[1:].tolist() == [0.0, 2.0, 0.0, 6.0]
    assert h.quantile(1.0)[1:].tolist() == [6.0, 4.0, 8.0, 8.0]
    assert h.quantile(0.75)[1:].tolist() == [5.0, 3.5, 4.0 + (6 - 4) / 3 * 2, 7.5]
    with pytest.raises(ValueError):
        h.quantile(1.5)
    # centroid over the bins whose centre lies in [2, 6]: centres 3 and 5
    c = h.centroid(2.0, 6.0)
    assert np.isnan(c[0]) and np.isnan(c[4]) and c[1:4].tolist() == [5.0, 3.0, 4.0]
    assert np.isnan(h.centroid(2.0, 6.0, min_count=5)[[1, 2]]).all() and h.centroid(2.0, 6.0, min_count=5)[3] == 4.0
    assert h.centroid(3.0, 3.0)[2] == 3.0                                    # the window is closed
    with pytest.raises(ValueError, match="no bin centre"):
        h.centroid(3.5, 4.5)


def test_centroid_is_within_half_a_bin_of_the_float64_mean():
    """Every sample differs from the centre of its bin by at most w / 2, so the centroid differs from the
    float64 mean of the same samples by at most w / 2 (+ 2^-40 |mean| for the float64 arithmetic).  The
    samples stay 5 % of a bin -- far more than a float32 ulp -- away from every edge, so float32 and
    float64 binning agree."""
    lo, hi, nbins = -32.0, 96.0, 64
    w = (hi - lo) / nbins
    rng = np.random.default_rng(12)
    F, n = 200, 40
    k = rng.integers(0, nbins, size=(F, n))
    x = (lo + (k + rng.uniform(0.05, 0.95, size=(F, n))) * w).astype(F32)
    x[rng.random((F, n)) < 0.1] = np.nan
    h = _ph(pixel_hist_reference(torch.from_numpy(x), lo, hi, nbins).numpy(), lo, hi, frames=F)
    c = h.centers()
    for a, b in ((lo, hi), (0.0, 30.0), (-10.0, -2.0)):
        sel = (c >= a) & (c <= b)
        e = h.edges()
        left, right = e[:-1][sel].min(), e[1:][sel].max()      # the samples of exactly those bins
        x64 = x.astype(np.float64)
        inside = (x64 > left) & (x64 < right)
        cnt = inside.sum(axis=0)
        mean = np.where(inside, x64, 0.0).sum(axis=0) / np.maximum(cnt, 1)
        got = h.centroid(a, b)
        assert np.array_equal(np.isnan(got), cnt == 0)
        ok = cnt > 0
        assert np.all(np.abs(got[ok] - mean[ok]) <= w / 2 + 2.0 ** -40 * np.abs(mean[ok]))


def test_save_load_round_trips_bitwise_and_merge_is_exact(tmp_path):
    rng = np.random.default_rng(1)
    a = _ph(rng.integers(0, 9, size=(24, 16)), lo=-1.5, hi=0.1, frames=200, shape=(2, 3, 4))
    b = _ph(rng.integers(0, 9, size=(24, 16)), lo=-1.5, hi=0.1, frames=300, shape=(2, 3, 4))
    pa, pb = a.save(tmp_path / "a.npz"), b.save(tmp_path / "b.npz")
    la = H.PixelHist.load(pa)
    assert la.key() == a.key() and la.frames == 200 and la.hist.dtype == np.int32 and np.array_equal(la.hist, a.hist)
    assert (la.lo, la.hi) == (float(F32(-1.5)), float(F32(0.1)))               # the float32 window, bitwise
    with np.load(pa, allow_pickle=False) as z:                                 # plain arrays only, compressed
        assert sorted(z.files) == sorted(("format", "detector", "layout", "shape", "lo", "hi", "nbins", "frames", "hist"))
        assert str(z["format"]) == H.HIST_FORMAT and z["frames"].dtype == np.int64 and z["hist"].dtype == np.int32
        assert z["hist"].shape == (24, 16) and z["lo"].dtype == np.float32
    m = H.merge([pa, pb])
    assert m.frames == 500 and np.array_equal(m.hist, a.hist + b.hist) and m.hist.dtype == np.int32
    assert H.main(["merge", pa, pb, "--out", str(tmp_path / "m.npz")]) == 0
    assert np.array_equal(H.PixelHist.load(tmp_path / "m.npz").hist, m.hist)
    for k, kw in enumerate((dict(lo=-1.25), dict(hi=0.2), dict(detector="other"), dict(layout="image"),
                            dict(shape=(2, 4, 3)))):
        pc = _ph(a.hist, **{**dict(lo=-1.5, hi=0.1, frames=200, shape=(2, 3, 4)), **kw}).save(tmp_path / f"c{k}.npz")
        with pytest.raises(ValueError, match="differ in"):
            H.merge([pa, pc])
        assert H.main(["merge", pa, pc, "--out", str(tmp_path / "no.npz")]) == 2
    pn = _ph(a.hist[:, :8], lo=-1.5, hi=0.1, frames=200, shape=(2, 3, 4)).save(tmp_path / "n.npz")
    with pytest.raises(ValueError, match="differ in nbins"):
        H.merge([pa, pn])
    # a merged run past 2^31 - 1 frames
    big = _ph(a.hist, lo=-1.5, hi=0.1, frames=2 ** 30, shape=(2, 3, 4)).save(tmp_path / "big.npz")
    almost = _ph(a.hist, lo=-1.5, hi=0.1, frames=2 ** 30 - 1, shape=(2, 3, 4)).save(tmp_path / "almost.npz")
    assert H.merge([big, almost]).frames == 2 ** 31 - 1
    with pytest.raises(ValueError, match="longer than 2147483647"):
        H.merge([big, big])
    with pytest.raises(ValueError):
        H.merge([])
    np.savez(tmp_path / "x.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="not a pixel-histogram file"):
        H.PixelHist.load(tmp_path / "x.npz")
    with pytest.raises(ValueError, match="int32"):
        H.PixelHist("tiny", "calib", (24,), 0.0, 1.0, 16, 9, a.hist.astype(np.int64))
    with pytest.raises(ValueError):
        _ph(a.hist, shape=(23,))
    with pytest.raises(ValueError, match="frames"):                            # a bin above the run's frames
        _ph(a.hist, frames=3)


def test_gain_correction_recovers_known_gain_factors(tmp_path):
    """A synthetic flat-field run: every pixel sees photons of energy E; its true gain is base * f with a
    known per-pixel f, so calibrating with the BASE gains puts the peak at E * f.  The bound: the centroid
    is within w / 2 of the mean of the samples it covers, which here is E * f up to the sampling error of
    the mean, itself kept below w / 100 by construction (symmetric pairs around E * f).  So
    |centroid - E f| <= w / 2 + w / 100 =: d, corr = E / centroid, recovered = base / corr = base *
    centroid / E, and |recovered / (base f) - 1| = |centroid - E f| / (E f) <= d / (E f_min), plus 2^-22
    for the float32 roundings of corr and of the division."""
    from psana_ray_amd.models import get_detector
    from psana_ray_amd.models.constants import CalibConstants

    spec = get_detector("tiny_epix")
    base = CalibConstants.random(spec, seed=4)
    n = int(np.prod(spec.frame_shape))
    rng = np.random.default_rng(8)
    f = rng.uniform(0.9, 1.1, size=n)
    E, lo, hi, nbins = 40.0, -32.0, 96.0, 64
    w = (hi - lo) / nbins
    F = 60
    half = rng.normal(0.0, 1.5, size=(F // 2, n))
    noise = np.concatenate([half, -half])                       # symmetric: the sample mean is E f exactly
    x = (E * f[None, :] + noise).astype(F32)
    x[:, 5] = np.nan                                            # a pixel without samples keeps its base gain
    hist = pixel_hist_reference(torch.from_numpy(x), lo, hi, nbins).numpy()
    h = H.PixelHist("tiny_epix", "calib", spec.frame_shape, lo, hi, nbins, F, hist)
    assert np.all(np.abs(x[:, np.arange(n) != 5] - E) < 24.0)  # every sample inside the peak window below
    corr = H.derive_gain_correction(h, E - 24.0, E + 24.0, expected=E, min_count=10)
    assert corr.dtype == np.float32 and corr.shape == (n,) and np.isnan(corr[5]) and np.isfinite(np.delete(corr, 5)).all()
    out = H.apply_gain_correction(base, corr, gain_range=0)
    got = out.gains[0].reshape(-1).astype(np.float64)
    want = base.gains[0].reshape(-1).astype(np.float64) * f
    bound = (w / 2 + w / 100) / (E * f.min()) + 2.0 ** -22
    keep = np.arange(n) != 5
    assert np.all(np.abs(got[keep] / want[keep] - 1.0) <= bound)
    assert np.abs(got[keep] / want[keep] - 1.0).max() < bound and bound < 0.03     # a 10 % spread is resolved
    assert got[5] == base.gains[0].reshape(-1)[5]
    # everything else is copied, the input is untouched
    assert np.array_equal(out.gains[1:], base.gains[1:]) and np.array_equal(out.pedestals, base.pedestals)
    assert np.array_equal(out.status, base.status) and np.array_equal(out.gain_config, base.gain_config)
    assert out.gains is not base.gains and tuple(out.cm_gains) == tuple(base.cm_gains)
    assert np.isnan(H.derive_gain_correction(h, E - 24.0, E + 24.0, E, min_count=F + 1)).all()
    with pytest.raises(ValueError, match="gain_range"):
        H.apply_gain_correction(base, corr, gain_range=9)
    with pytest.raises(ValueError, match="pixels"):
        H.apply_gain_correction(base, corr[:-1], gain_range=0)
    with pytest.raises(ValueError, match="positive"):
        H.derive_gain_correction(h, 0.0, 50.0, expected=0.0)
    # the CLI: gain writes constants that load, and the correction
    ph, pb = h.save(tmp_path / "h.npz"), base.save(tmp_path / "base.npz")
    po, pc = str(tmp_path / "consts.npz"), str(tmp_path / "corr.npy")
    assert H.main(["gain", ph, "--peak", f"{E - 24},{E + 24}", "--expected", str(E), "--base", pb, "--gain_range", "0",
                   "--min_count", "10", "--out", po, "--corr_out", pc]) == 0
    assert np.array_equal(CalibConstants.load(po).gains, out.gains)
    assert np.array_equal(np.load(pc).reshape(-1), corr, equal_nan=True) and np.load(pc).shape == spec.frame_shape
    assert H.main(["gain", ph, "--peak", "40", "--expected", str(E), "--base", pb, "--gain_range", "0", "--out", po]) == 2
    assert H.main(["info", ph]) == 0
    assert H.main(["spectrum", ph, "--out", str(tmp_path / "s.npy")]) == 0
    assert np.array_equal(np.load(tmp_path / "s.npy"), h.total())
