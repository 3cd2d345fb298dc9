"""K-13 photon counting: the golden model (ops.reference.photon_count_reference) against the independent
per-pixel oracle of tests/_photons_oracle.py, the physics it is for, the exact views of PhotonStats and the
parameter refusals.  Runs anywhere (no GPU)."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from psana_ray_amd import photons as PH
from psana_ray_amd.ops import reference as R
from tests._photons_oracle import photons_oracle

ADU = 9.5


def _same(got: R.PhotonCounts, want: dict):
    for k in ("kmap", "cnt", "psum", "occ", "pk", "tot"):
        g = getattr(got, k).numpy()
        assert g.dtype == want[k].dtype and np.array_equal(g, want[k]), k


def _values(rng, shape, nf):
    """Values around every threshold of the contract: whole photons, remainders near 0.5 / 0.9, pairs that sum
    near 0.9, zeros, negatives and specials."""
    n = int(np.prod(shape))
    base = rng.integers(0, 4, size=(nf, n)).astype(np.float32)
    frac = rng.choice(np.array([0.0, 0.1, 0.25, 0.4, 0.45, 0.5, 0.55, 0.6, 0.9, 0.95], np.float32), size=(nf, n))
    x = ((base + frac) * np.float32(ADU)).astype(np.float32)
    x[rng.random((nf, n)) < 0.25] = 0.0
    spec = rng.random((nf, n))
    x[spec < 0.02] = np.nan
    x[(spec >= 0.02) & (spec < 0.04)] = np.inf
    x[(spec >= 0.04) & (spec < 0.06)] = -3.0
    x[(spec >= 0.06) & (spec < 0.07)] = -0.0
    return x


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (1, 5, 1), (2, 3, 4), (3, 5, 7)])
def test_golden_model_equals_the_per_pixel_oracle(shape):
    rng = np.random.default_rng(sum(shape))
    x = _values(rng, shape, 5)
    _same(R.photon_count_reference(torch.from_numpy(x), shape, ADU), photons_oracle(x, shape, ADU))
    n = x.shape[1]
    mask = (rng.random(n) < 0.8).astype(np.uint8)
    roi = rng.choice(np.array([0, 1, 2, 255], np.uint8), size=n)
    got = R.photon_count_reference(torch.from_numpy(x), shape, dict(adu_per_photon=ADU, vmax=3.2 * ADU, thr_seed=0.45,
                                                                    thr_total=1.0), mask, roi, 3)
    _same(got, photons_oracle(x, shape, ADU, vmax=3.2 * ADU, thr_seed=0.45, thr_total=1.0, mask=mask, roi=roi, n_roi=3))


def test_seeded_values_around_the_thresholds():
    shape = (2, 9, 12)
    rng = np.random.default_rng(13)
    n = int(np.prod(shape))
    inv = np.float32(1.0 / np.float64(np.float32(ADU)))
    # remainders within a few ulps of thr_seed, and pairs whose float32 sum is within a few ulps of thr_total
    r = rng.choice(np.array([0.5, 0.4, 0.9, 0.45, 0.3], np.float32), size=(6, n))
    r = np.nextafter(r, np.float32(2.0) * (rng.integers(0, 2, size=r.shape) > 0).astype(np.float32))
    for _ in range(2):
        r = np.where(rng.random(r.shape) < 0.5, np.nextafter(r, np.float32(0)), r).astype(np.float32)
    x = (r / inv).astype(np.float32)
    x[rng.random(x.shape) < 0.3] = 0.0
    got = R.photon_count_reference(torch.from_numpy(x), shape, ADU)
    _same(got, photons_oracle(x, shape, ADU))
    assert 0 < int(got.psum.sum()) < x.size


def _split_photons(shape, rng, n_photons, n_half=0):
    """One frame with isolated photons, each split a / (1 - a), a in (0.5, 1), over a horizontal or vertical
    pair inside one panel, events at least 3 pixels apart; some lie along panel edges.  The first ``n_half``
    have a = 0.5 + 1e-9: in float32 both shares are exactly one half (the larger share is put at the lower
    index, where the tie-break looks for the seed).  Returns (frame [n], the pixel of each larger share)."""
    P, H, W = shape
    frame = np.zeros(shape, np.float32)
    taken = np.zeros(shape, bool)
    big = []
    cand = [(p, y, x) for p in range(P) for y in (0, H - 1) for x in range(0, W, 5)]   # panel edges first
    cand += [(int(rng.integers(P)), int(rng.integers(H)), int(rng.integers(W))) for _ in range(50 * n_photons)]
    for p, y, x in cand:
        if len(big) == n_photons:
            break
        half = len(big) < n_half
        dy, dx = ((0, 1), (1, 0), (0, -1), (-1, 0))[int(rng.integers(2 if half else 4))]
        y2, x2 = y + dy, x + dx
        if not (0 <= y2 < H and 0 <= x2 < W):
            continue   # never a pair across a panel edge
        lo_y, hi_y, lo_x, hi_x = max(0, min(y, y2) - 3), max(y, y2) + 4, max(0, min(x, x2) - 3), max(x, x2) + 4
        if taken[p, lo_y:hi_y, lo_x:hi_x].any():
            continue
        a = 0.5 + 1e-9 if half else float(rng.uniform(0.55, 0.95))
        frame[p, y, x] = np.float32(a * ADU)
        frame[p, y2, x2] = np.float32((1.0 - a) * ADU)
        taken[p, y, x] = taken[p, y2, x2] = True
        big.append((p * H + y) * W + x)
    assert len(big) == n_photons
    return frame.reshape(-1), np.array(big)


def test_split_photons_are_recovered_where_rounding_loses_them():
    shape = (3, 24, 30)
    frame, big = _split_photons(shape, np.random.default_rng(5), 40, n_half=6)
    got = R.photon_count_reference(torch.from_numpy(frame)[None], shape, ADU)
    k = got.kmap[0].numpy()
    assert int(k.sum()) == 40 and np.array_equal(np.flatnonzero(k), np.sort(big)) and set(k[big]) == {1}
    assert got.pk[0, 0].tolist() == [40, 0, 0, 0, 0, 0, 0, 0] and int(got.tot[0, 0]) == 40
    # the same input through round(v * inv) loses the photons whose shares are both one half in float32 (half
    # to even drops both); for a clearly above one half it finds the pair's photon too
    inv = np.float32(1.0 / np.float64(np.float32(ADU)))
    assert int(np.rint(frame * inv).sum()) == 40 - 6
    # and a lone pixel of 0.6 photon (no partner: noise, not a split photon) is one photon to round() but none
    # to the merge, which wants 0.9 of a photon in the pair
    noisy = frame.reshape(shape).copy()
    free = np.argwhere(noisy[2] == 0)
    for y, x in free[(free[:, 0] > 3) & (free[:, 1] > 3)][::97][:5]:
        if not noisy[2, y - 2:y + 3, x - 2:x + 3].any():
            noisy[2, y, x] = np.float32(0.6 * ADU)
    assert int((noisy != frame.reshape(shape)).sum()) >= 2
    assert int(R.photon_count_reference(torch.from_numpy(noisy.reshape(1, -1)), shape, ADU).psum.sum()) == 40
    assert int(np.rint(noisy * inv).sum()) > 40 - 6


def test_a_photon_over_four_pixels_is_not_recovered():
    """The documented limit (psana's too): 0.3 / 0.3 / 0.2 / 0.2 has no seed."""
    x = np.zeros((1, 4, 4), np.float32)
    x[0, 1:3, 1:3] = np.array([[0.3, 0.3], [0.2, 0.2]], np.float32) * np.float32(ADU)
    assert int(R.photon_count_reference(torch.from_numpy(x)[None], (1, 4, 4), ADU).psum.sum()) == 0


def test_mean_photons_and_kbar_are_exact_rationals():
    shape = (2, 3, 4)
    rng = np.random.default_rng(3)
    x = _values(rng, shape, 7)
    n = x.shape[1]
    mask = np.ones(n, np.uint8)
    mask[[1, 5]] = 0
    roi = np.array([0, 1] * (n // 2), np.uint8)
    roi[3] = 255
    out = R.photon_count_reference(torch.from_numpy(x), shape, ADU, mask, roi, 2)
    pp = R.validate_photon_params(ADU)
    st = PH.PhotonStats.from_maps("t", "calib", shape, pp, mask, roi, 2, 7, out.cnt.numpy(), out.psum.numpy(),
                                  out.occ.numpy(), rank=[0] * 7, idx=list(range(7)), gevt=list(range(7)),
                                  photon_energy=[float("nan")] * 7, pk=out.pk.numpy(), tot=out.tot.numpy())
    assert st.roi_npix.tolist() == [int(((roi == r) & (mask != 0)).sum()) for r in range(2)]
    mp, oc = st.mean_photons(), st.occupancy()
    assert mp.dtype == np.float64
    for p in range(n):
        c = int(out.cnt[p])
        if c == 0:
            assert np.isnan(mp[p]) and np.isnan(oc[p])
        else:
            assert mp[p] == float(Fraction(int(out.psum[p]), c)) and oc[p] == float(Fraction(int(out.occ[p]), c))
    assert np.isnan(mp[1]) and np.isnan(mp[5])
    for r in range(2):
        kb, tab = st.kbar(r), st.pk_table(r)
        assert tab.shape == (7, 9) and (tab.sum(axis=1) == st.roi_npix[r]).all() and (tab >= 0).all()
        for f in range(7):
            assert kb[f] == float(Fraction(int(out.tot[f, r]), int(st.roi_npix[r])))
            assert tab[f, 1:].tolist() == out.pk[f, r].tolist()
    with pytest.raises(ValueError, match="ROI 2 of 2"):
        st.kbar(2)


def test_parameter_refusals():
    v = R.validate_photon_params
    pp = v(ADU)
    assert pp.inv == float(np.float32(1.0 / np.float64(np.float32(ADU)))) and pp.thr_seed == 0.5
    assert pp.thr_total == float(np.float32(0.9)) and pp.vmax == float(np.float32(250 * np.float32(ADU)))
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-46, 1e39, "x", None):
        with pytest.raises(ValueError):
            v(bad)
    assert np.floor(np.float32(254.5) * np.float32(1.0)) == 254 and v(1.0, vmax=254.5)
    with pytest.raises(ValueError, match="at most 254"):
        v(1.0, vmax=255.0)
    for bad in (float("nan"), float("inf")):
        with pytest.raises(ValueError):
            v(1.0, vmax=bad)
    for ts, tt in ((0.0, 0.9), (-0.1, 0.9), (0.95, 0.9), (0.5, 2.0), (float("nan"), 0.9), (0.5, float("nan"))):
        with pytest.raises(ValueError, match="thr_seed <= thr_total"):
            v(1.0, thr_seed=ts, thr_total=tt)
    assert v(1.0, thr_seed=0.9, thr_total=0.9) and v(1.0, frames_so_far=2 ** 31 - 2, frames=1)
    with pytest.raises(ValueError, match="past 2147483647"):
        v(1.0, frames_so_far=2 ** 31 - 2, frames=2)
    x = torch.zeros((1, 24))
    for kw in (dict(mask=np.ones(23, np.uint8)), dict(roi=np.zeros(25, np.uint8)), dict(roi=np.full(24, 1, np.uint8), n_roi=1),
               dict(n_roi=2), dict(roi=np.zeros(24, np.uint8), n_roi=9), dict(roi=np.zeros(24, np.uint8), n_roi=0),
               dict(roi=np.zeros(24, np.int32)), dict(roi=np.full(24, 8, np.uint8))):
        with pytest.raises(ValueError):
            R.photon_count_reference(x, (2, 3, 4), ADU, **kw)
    for shape in ((2, 3, 5), (24,), (1, 2, 3, 4), (0, 3, 8)):
        with pytest.raises(ValueError):
            R.photon_count_reference(x, shape, ADU)
    with pytest.raises(ValueError):
        R.photon_count_reference(x.double(), (2, 3, 4), ADU)
    # labels of 255 alone make one (empty) ROI; R follows the largest label
    out = R.photon_count_reference(x + 10.0, (2, 3, 4), ADU, roi=np.full(24, 255, np.uint8))
    assert out.pk.shape == (1, 1, 8) and int(out.pk.sum()) == 0 and int(out.psum.sum()) == 24
    assert R.photon_count_reference(x, (2, 3, 4), ADU, roi=np.array([0, 3] * 12, np.uint8)).pk.shape == (1, 4, 8)
