"""K-14 golden model (ops.reference.droplet_reference) against the flood-fill oracle of
tests/_droplets_oracle.py, its invariants, the physics it is for, and every ValueError of the contract."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import reference as R
from tests._droplets_oracle import droplets_oracle, patterns, random_frames, same_as_oracle

f32 = np.float32
SHAPES = [(1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 5, 7), (3, 8, 12)]


def _gold(x, shape, **kw):
    par = {k: kw.pop(k) for k in ("thr_low", "thr_seed", "vmax", "frac_bits") if k in kw}
    return R.droplet_reference(torch.as_tensor(np.asarray(x, f32)).reshape(-1, int(np.prod(shape))), shape, par, **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_golden_equals_oracle_on_patterns(shape):
    pats = patterns(shape)
    x = np.stack([p.reshape(-1) for p in pats.values()])
    n = x.shape[1]
    kw = dict(thr_low=5.0, thr_seed=10.5, vmax=100.0, frac_bits=2, cap_pix=n, cap=n)
    same_as_oracle(_gold(x, shape, **kw), droplets_oracle(x, shape, **kw))
    kw["thr_seed"] = 5.0
    got = _gold(x, shape, **kw)
    same_as_oracle(got, droplets_oracle(x, shape, **kw))
    names = list(pats)
    nd = dict(zip(names, got.ndrop.tolist()))
    if "diagonal" in nd:
        assert nd["diagonal"] == 2 and nd["row_end"] == 2
    if "panel_edge" in nd:
        assert nd["panel_edge"] == 2
    for k in ("L", "U", "comb", "spiral", "serpentine"):
        if k in nd:
            assert nd[k] == 1, k
    assert nd["checkerboard"] == shape[0] * ((shape[1] * shape[2] + 1) // 2)


@pytest.mark.parametrize("frac", [0.001, 0.05, 0.3, 0.59])
def test_golden_equals_oracle_on_random_frames(frac):
    shape = (2, 9, 13)
    n = 2 * 9 * 13
    x = random_frames(shape, 3, frac, seed=int(frac * 1000))
    mask = (np.random.default_rng(5).random(n) > 0.1).astype(np.uint8)
    for m in (None, mask):
        for S in (0, 2):
            kw = dict(thr_low=2.0, thr_seed=30.0, vmax=55.0, frac_bits=S, mask=m, cap_pix=n, cap=n)
            same_as_oracle(_gold(x, shape, **kw), droplets_oracle(x, shape, **kw))


def test_mask_and_vmax_cut_a_droplet():
    shape = (1, 3, 7)
    x = np.zeros(shape, f32)
    x[0, 1, :] = 10.0
    kw = dict(thr_low=5.0, vmax=100.0, cap_pix=21, cap=21)
    assert _gold(x, shape, **kw).ndrop.tolist() == [1]
    m = np.ones(21, np.uint8)
    m[7 + 3] = 0
    g = _gold(x, shape, mask=m, **kw)
    assert g.ndrop.tolist() == [2] and g.npix.tolist() == [3, 3] and g.label.tolist() == [7, 11]
    x[0, 1, 3] = np.nextafter(f32(100.0), f32(np.inf))
    g = _gold(x, shape, **kw)
    assert g.ndrop.tolist() == [2] and g.nact.tolist() == [6]
    same_as_oracle(g, droplets_oracle(x.reshape(1, -1), shape, **kw))


def test_window_edges_and_seed():
    shape = (1, 1, 9)
    lo, hi, seed = f32(5.0), f32(100.0), f32(20.0)
    dn, up = lambda v: np.nextafter(f32(v), f32(-np.inf)), lambda v: np.nextafter(f32(v), f32(np.inf))
    x = np.array([[lo, 0, dn(lo), 0, hi, 0, up(hi), 0, np.nan],
                  [dn(seed), lo, 0, seed, lo, 0, np.inf, -np.inf, -0.0],
                  [2.125, 0, 2.375, 0, 2.5, 0, 3.5, 0, -7.0]], f32)
    kw = dict(thr_low=5.0, thr_seed=5.0, vmax=100.0, frac_bits=2, cap_pix=9, cap=9)
    g = _gold(x[:1], shape, **kw)
    assert g.nact.tolist() == [2] and g.label.tolist() == [0, 4]
    kw["thr_seed"] = 20.0
    g = _gold(x[1:2], shape, **kw)
    assert g.nact.tolist() == [4] and g.ndrop.tolist() == [1] and g.label.tolist() == [3]   # the candidate at 0 is dropped
    g = _gold(x[2:], shape, thr_low=2.0, frac_bits=0, cap_pix=9, cap=9)
    assert g.adu.tolist() == [2, 2, 2, 4]   # rint: 2.125 -> 2, 2.375 -> 2, 2.5 -> 2 (tie to even), 3.5 -> 4
    g = _gold(x[2:], shape, thr_low=2.0, frac_bits=2, cap_pix=9, cap=9)
    assert g.adu.tolist() == [8, 10, 10, 14]   # 8.5 -> 8 and 9.5 -> 10: ties to even
    same_as_oracle(g, droplets_oracle(x[2:], shape, thr_low=2.0, frac_bits=2, cap_pix=9, cap=9))


def test_invariants():
    shape = (3, 8, 12)
    n = 3 * 8 * 12
    x = random_frames(shape, 5, 0.3, seed=11)
    kw = dict(thr_low=2.0, vmax=55.0, frac_bits=2, cap_pix=n, cap=n)
    g = _gold(x, shape, **kw)
    act = (x >= 2.0) & (x <= 55.0)
    q = np.where(act, np.rint(np.where(act, x, 0) * f32(4)), 0).astype(np.int64)
    for f in range(5):
        a, b = int(g.offs[f]), int(g.offs[f + 1])
        assert int(g.npix[a:b].sum()) == int(g.nact[f]) == int(act[f].sum())
        assert int(g.adu[a:b].sum()) == int(q[f].sum())
        lab = g.label[a:b].numpy()
        assert (np.diff(lab) > 0).all()
        assert (g.qmax[a:b] <= g.adu[a:b]).all()
    perm = [3, 0, 4, 2, 1]
    h = _gold(x[perm], shape, **kw)
    for i, f in enumerate(perm):
        assert h.nact[i] == g.nact[f] and h.ndrop[i] == g.ndrop[f]
        for k in ("label", "npix", "adu", "sy", "sx", "qmax"):
            assert torch.equal(getattr(h, k)[int(h.offs[i]):int(h.offs[i + 1])],
                               getattr(g, k)[int(g.offs[f]):int(g.offs[f + 1])])


def test_capacity_edges():
    shape = (1, 4, 8)
    x = np.zeros((3, 32), f32)
    x[:, [0, 2, 4, 9]] = 10.0
    x[1, 20] = 10.0
    kw = dict(thr_low=5.0)
    g = _gold(x, shape, cap_pix=32, cap=4, **kw)
    assert g.ndrop.tolist() == [4, 5, 4] and g.flags.tolist() == [0, 1, 0] and g.offs.tolist() == [0, 4, 4, 8]
    g = _gold(x, shape, cap_pix=4, cap=8, **kw)
    assert g.nact.tolist() == [4, 5, 4] and g.ndrop.tolist() == [4, 0, 4] and g.flags.tolist() == [0, 4, 0]
    assert g.label.tolist() == [0, 2, 4, 9] * 2
    same_as_oracle(g, droplets_oracle(x, shape, cap_pix=4, cap=8, **kw))


def test_scipy_label_agrees():
    ndi = pytest.importorskip("scipy.ndimage")
    shape = (3, 8, 12)
    x = random_frames(shape, 2, 0.4, seed=3)
    n = x.shape[1]
    g = _gold(x, shape, thr_low=2.0, vmax=55.0, cap_pix=n, cap=n)
    act = ((x >= 2.0) & (x <= 55.0)).reshape(2, *shape)
    for f in range(2):
        labels = []
        for p in range(3):
            lab, k = ndi.label(act[f, p], structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])
            labels += [p * 96 + int(np.flatnonzero(lab.reshape(-1) == j + 1)[0]) for j in range(k)]
        assert sorted(labels) == g.label[int(g.offs[f]):int(g.offs[f + 1])].tolist()


def test_shared_photon_is_one_droplet_where_photon_counting_sees_none():
    """One 10-ADU photon shared 0.3 / 0.3 / 0.2 / 0.2 over a 2 x 2 block."""
    from psana_ray_amd.droplets import DropletFrames

    shape = (1, 4, 4)
    x = np.zeros(shape, f32)
    x[0, 1:3, 1:3] = [[3.0, 3.0], [2.0, 2.0]]
    xt = torch.as_tensor(x).reshape(1, -1)
    assert int(R.photon_count_reference(xt, shape, 10.0).kmap.sum()) == 0
    g = R.droplet_reference(xt, shape, dict(thr_low=1.5), cap_pix=16, cap=16)
    assert g.ndrop.tolist() == [1] and g.npix.tolist() == [4] and g.adu.tolist() == [40]
    d = DropletFrames.from_lists("t", "calib", shape, R.validate_droplet_params(1.5), None, [0], [0], [0], [0.0],
                                 g.nact.numpy(), g.ndrop.numpy(), g.flags.numpy(), g.offs.numpy(),
                                 {k: getattr(g, k).numpy() for k in ("label", "npix", "adu", "sy", "sx", "qmax")})
    assert d.photons(10.0).tolist() == [1]
    assert d.energy().tolist() == [10.0]
    panel, cy, cx = d.com(0)
    assert panel.tolist() == [0] and cy.tolist() == [1.4] and cx.tolist() == [1.5]


@pytest.mark.parametrize("kw", [
    dict(thr_low=0.0), dict(thr_low=-1.0), dict(thr_low=float("nan")), dict(thr_low=float("inf")),
    dict(thr_low=5.0, thr_seed=4.0), dict(thr_low=5.0, thr_seed=20.0, vmax=10.0), dict(thr_low=5.0, vmax=float("inf")),
    dict(thr_low=5.0, vmax=1e39), dict(thr_low=5.0, frac_bits=-1), dict(thr_low=5.0, frac_bits=17),
    dict(thr_low=5.0, frac_bits=2.5), dict(thr_low="x"), dict(thr_low=5.0, vmax=2.0 ** 20, frac_bits=11),
])
def test_bad_params(kw):
    with pytest.raises(ValueError):
        R.validate_droplet_params(**kw)


def test_params_are_float32_and_bounds():
    p = R.validate_droplet_params(0.1, vmax=100.3, frac_bits=3)
    assert p.thr_low == float(f32(0.1)) and p.thr_seed == p.thr_low and p.vmax == float(f32(100.3))
    assert p.qlim == int(np.ceil(float(f32(100.3)) * 8))
    assert R.validate_droplet_params(5.0).qlim == 2 ** 22
    assert R.validate_droplet_params(5.0, vmax=2.0 ** 20, frac_bits=10).qlim == 2 ** 30
    assert R.validate_droplet_caps((16, 352, 384), p) == (16 * 352 * 384 // 16, 16 * 352 * 384 // 64)
    assert R.validate_droplet_caps((1, 1, 1), p) == (1, 1)
    for bad in (dict(cap_pix=0), dict(cap=0), dict(cap_pix=2 ** 31), dict(cap=2 ** 25, frames=64), dict(frames=0),
                dict(frames=65), dict(cap=1.5)):
        with pytest.raises(ValueError):
            R.validate_droplet_caps((2, 5, 7), p, **bad)
    # Q * (max(H, W) - 1) * min(H * W, cap_pix) <= 2^63 - 1
    big = R.validate_droplet_params(5.0, vmax=2.0 ** 14, frac_bits=16)   # Q = 2^30
    R.validate_droplet_caps((1, 2 ** 15, 2 ** 15), big, cap_pix=2 ** 17)
    with pytest.raises(ValueError):
        R.validate_droplet_caps((1, 2 ** 15, 2 ** 15), big, cap_pix=2 ** 19)
    with pytest.raises(ValueError):
        R.droplet_reference(torch.zeros(1, 4, dtype=torch.float64), (2, 2), 5.0)
    with pytest.raises(ValueError):
        R.droplet_reference(torch.zeros(1, 5), (2, 2), 5.0)
    with pytest.raises(ValueError):
        R.droplet_reference(torch.zeros(1, 4), (2, 2), 5.0, mask=np.ones(5, np.uint8))
    with pytest.raises(ValueError):
        R.droplet_reference(torch.zeros(65, 4), (2, 2), 5.0)
