"""K-13 photon-counting kernel (csrc/photons.hip) against the golden model, word for word for every output,
on the smallest shapes where each hazard exists."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

GUARD = 64            # guard words (bytes for kmap) behind every buffer
GUARD_WORD = 0x5EED
GUARD_BYTE = 0xA5
ADU = 2.0             # inv = 0.5 exactly: v / 2 has the remainder one expects
NAMES = ("kmap", "cnt", "psum", "occ", "pk", "tot")
f32 = np.float32


def _guarded(shape, dtype, dev, fill=0):
    words = int(np.prod(shape))
    al = (words + 15) // 16 * 16
    raw = torch.full((al + GUARD,), GUARD_BYTE if dtype == torch.uint8 else GUARD_WORD, dtype=dtype, device=dev)
    v = raw[:words].view(*shape)
    v.fill_(fill)
    return raw, v, words


class Bufs:
    """Fresh outputs on the device, every tensor followed by guard words."""

    def __init__(self, F, n, R, dev, kmap=True, pre=None):
        self.raw = {}
        self.t = {}
        self.words = {}
        spec = {"cnt": ((n,), torch.int32), "psum": ((n,), torch.int64), "occ": ((n,), torch.int32),
                "pk": ((F, R, 8), torch.int32), "tot": ((F, R), torch.int64)}
        if kmap:
            spec["kmap"] = ((F, n), torch.uint8)
        for name, (shape, dt) in spec.items():
            # pk / tot / kmap start as garbage: the call clears or overwrites them
            fill = 0 if name in ("cnt", "psum", "occ") else 0x77
            self.raw[name], self.t[name], self.words[name] = _guarded(shape, dt, dev, fill)
            if pre is not None and name in pre:
                self.t[name].copy_(torch.as_tensor(pre[name]).to(dt))

    def host(self):
        torch.cuda.synchronize()
        for name, r in self.raw.items():
            tail = r[self.words[name]:].cpu()
            assert bool((tail == (GUARD_BYTE if r.dtype == torch.uint8 else GUARD_WORD)).all()), \
                f"guard words behind {name} were written"
        return {k: v.cpu() for k, v in self.t.items()}


def _run(x, shape, dev, adu=ADU, mask=None, roi=None, n_roi=None, kmap=True, bufs=None, split=None, separate=False,
         stream=None, **par):
    """x: float32 [F, n] on the host.  Returns the outputs on the host (guards checked)."""
    x = torch.as_tensor(x, dtype=torch.float32)
    F, n = x.shape
    if separate or (4 * n) % 16:
        frames = [x[f].clone().to(dev) for f in range(F)]
    else:
        xd = x.to(dev)
        frames = [xd[f] for f in range(F)]
    R = n_roi or 1
    b = Bufs(F, n, R, dev, kmap) if bufs is None else bufs
    md = None if mask is None else torch.as_tensor(mask, dtype=torch.uint8).to(dev)
    rd = None if roi is None else torch.as_tensor(roi, dtype=torch.uint8).to(dev)
    a = 0
    for k in (split or [F]):
        kernels.photons(frames[a:a + k], shape, adu, b.t["cnt"], b.t["psum"], b.t["occ"], b.t["pk"][a:a + k],
                        b.t["tot"][a:a + k], mask=md, roi=rd, n_roi=n_roi,
                        kmap=b.t["kmap"][a:a + k] if "kmap" in b.t else None, frames_so_far=a, stream=stream, **par)
        a += k
    assert a == F
    return b.host()


def _ref(x, shape, adu=ADU, mask=None, roi=None, n_roi=None, **par):
    out = reference.photon_count_reference(torch.as_tensor(x, dtype=torch.float32), shape,
                                           dict(adu_per_photon=adu, **par), mask, roi, n_roi)
    return out._asdict()


def _same(got, want, names=NAMES):
    for name in names:
        if name not in got:
            continue
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), f"{name} differs at {(g != w).nonzero()[:4].tolist()}"


def _values(shape, F, seed, adu=ADU):
    """Whole photons plus remainders around 0.5 / 0.9, a quarter empty, a few specials."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    base = rng.integers(0, 3, size=(F, n)).astype(f32) * (rng.random((F, n)) < 0.3)
    frac = rng.choice(np.array([0.0, 0.125, 0.25, 0.375, 0.4375, 0.5, 0.5625, 0.625, 0.875, 0.9375], f32), size=(F, n))
    x = ((base + frac) * f32(adu)).astype(f32)
    x[rng.random((F, n)) < 0.25] = 0.0
    s = rng.random((F, n))
    x[s < 0.01] = np.nan
    x[(s >= 0.01) & (s < 0.02)] = np.inf
    x[(s >= 0.02) & (s < 0.03)] = -5.0
    x[(s >= 0.03) & (s < 0.04)] = -0.0
    return x


def _maps(n, seed, R=3):
    rng = np.random.default_rng(seed)
    return (rng.random(n) < 0.85).astype(np.uint8), rng.choice(np.array([*range(R), 255], np.uint8), size=n)


@pytest.mark.parametrize("shape", [(2, 5, 12), (2, 5, 7), (3, 1, 8), (3, 1, 5), (2, 6, 1), (1, 1, 1), (1, 1, 3), (1, 3, 1),
                                   (1, 1, 4), (1, 2, 4)])
def test_small_shapes_both_paths(native, cuda_device, shape):
    """W % 4 == 0 (a lane owns a quad) and W % 4 != 0 (a lane owns a pixel), H = 1, W = 1, n < 4."""
    n = int(np.prod(shape))
    x = _values(shape, 6, 1 + n)
    _same(_run(x, shape, cuda_device), _ref(x, shape))
    mask, roi = _maps(n, n)
    _same(_run(x, shape, cuda_device, mask=mask, roi=roi, n_roi=3), _ref(x, shape, mask=mask, roi=roi, n_roi=3))


def test_block_and_lane_boundaries(native, cuda_device):
    """One row below, at and above a block of lanes (the wrapper exports its pixels), for both paths."""
    b4, b1 = kernels.photons_block_pixels(16), kernels.photons_block_pixels(7)
    assert kernels.photons_lane_pixels(16) == 4 and kernels.photons_lane_pixels(7) == 1 and b4 == 4 * b1
    shapes = [(1, b4 // 16 + d, 16) for d in (-1, 0, 1)] + [(2, b4 // 32, 16), (1, b4 // 12, 12), (1, b4 // 12 + 1, 12)]
    shapes += [(1, b1 + d, 1) for d in (-1, 0, 1)] + [(1, b1 // 7, 7), (1, b1 // 7 + 1, 7), (1, 2, b1 + 1)]
    for shape in shapes:
        n = int(np.prod(shape))
        x = _values(shape, 3, n)
        mask, roi = _maps(n, n, 2)
        _same(_run(x, shape, cuda_device, mask=mask, roi=roi, n_roi=2), _ref(x, shape, mask=mask, roi=roi, n_roi=2))


@pytest.mark.parametrize("W", [512, 257])
def test_a_workgroup_owns_several_blocks(native, cuda_device, W):
    """More blocks than the largest grid: every workgroup walks two blocks and merges its counters once."""
    bp, grid = kernels.photons_block_pixels(W), kernels.photons_max_grid()
    H = (bp * (grid + 2)) // (2 * W) + 1
    shape = (2, H, W)
    n = 2 * H * W
    assert grid * bp < n <= 2 * grid * bp
    x = _values(shape, 2, W)
    mask, roi = _maps(n, W, 8)
    _same(_run(x, shape, cuda_device, mask=mask, roi=roi, n_roi=8), _ref(x, shape, mask=mask, roi=roi, n_roi=8))


@pytest.mark.parametrize("F", [1, 2, 3, 4, 5, 6, 7, 8, 9, 63, 64])
def test_every_remainder_of_the_frame_groups(native, cuda_device, F):
    shape = (2, 5, 12)
    x = _values(shape, F, 100 + F)
    _same(_run(x, shape, cuda_device), _ref(x, shape))


def test_more_frames_than_one_launch(native, cuda_device):
    """67 frames: two launches inside one call, the per-frame rows of the second follow the first's."""
    for shape in ((2, 5, 12), (2, 5, 7)):
        x = _values(shape, 67, 7)
        _same(_run(x, shape, cuda_device, separate=True), _ref(x, shape))
        _same(_run(x, shape, cuda_device, split=[3, 64]), _ref(x, shape))


@pytest.mark.parametrize("W", [4, 8, 5])
def test_nothing_pairs_across_a_panel_or_row_edge(native, cuda_device, W):
    shape = (2, 3, W)
    x = np.zeros((2, *shape), f32)
    x[0, 0, 2, 1] = 0.625 * ADU     # last row of panel 0 ...
    x[0, 1, 0, 1] = 0.375 * ADU     # ... above the first row of panel 1
    x[1, 0, 0, W - 1] = 0.625 * ADU   # last column of a row ...
    x[1, 0, 1, 0] = 0.375 * ADU       # ... before the first column of the next
    got = _run(x.reshape(2, -1), shape, cuda_device)
    assert int(got["kmap"].sum()) == 0 and int(got["psum"].sum()) == 0
    _same(got, _ref(x.reshape(2, -1), shape))
    # the same pairs inside a panel do merge
    x2 = np.zeros((2, *shape), f32)
    x2[0, 0, 1, 1], x2[0, 0, 2, 1] = 0.625 * ADU, 0.375 * ADU
    x2[1, 1, 1, W - 2], x2[1, 1, 1, W - 1] = 0.375 * ADU, 0.625 * ADU
    got = _run(x2.reshape(2, -1), shape, cuda_device)
    assert got["kmap"].reshape(2, *shape)[0, 0, 1, 1] == 1 and got["kmap"].reshape(2, *shape)[1, 1, 1, W - 1] == 1
    assert int(got["kmap"].sum()) == 2
    _same(got, _ref(x2.reshape(2, -1), shape))


@pytest.mark.parametrize("W", [8, 6])
def test_equal_remainders_have_exactly_one_seed(native, cuda_device, W):
    """Two equal neighbours and a plateau of three, along a row (inside a quad and across two) and down a
    column: the lowest index is the seed."""
    shape = (1, 5, W)
    x = np.zeros((4, *shape), f32)
    x[0, 0, 1, 1:3] = 0.625 * ADU
    x[1, 0, 1, 3:6] = 0.625 * ADU
    x[2, 0, 1:4, 2] = 0.625 * ADU
    x[3, 0, 2, 3:5] = 0.5 * ADU
    x[3, 0, 3, 3] = 0.5 * ADU
    got = _run(x.reshape(4, -1), shape, cuda_device)
    k = got["kmap"].reshape(4, 5, W)
    assert k[0].nonzero().tolist() == [[1, 1]] and k[1].nonzero().tolist() == [[1, 3]]
    assert k[2].nonzero().tolist() == [[1, 2]] and k[3].nonzero().tolist() == [[2, 3]]
    _same(got, _ref(x.reshape(4, -1), shape))


def test_threshold_edges(native, cuda_device):
    """r == thr_seed, r + rmax == thr_total and each one ulp below; x an exact integer; v == vmax and one ulp
    above.  adu = 2, so every remainder below is exact."""
    shape = (1, 3, 16)
    below = lambda v: np.nextafter(f32(v), f32(0))   # noqa: E731
    above = lambda v: np.nextafter(f32(v), f32(np.inf))   # noqa: E731
    x = np.zeros(shape, f32)
    x[0, 1, 1], x[0, 1, 2] = 0.5 * ADU, 0.375 * ADU           # seed at the threshold, total at the threshold: 1
    x[0, 1, 5], x[0, 1, 6] = below(0.5 * ADU), 0.4375 * ADU   # seed one ulp below: 0
    x[0, 1, 13] = 3.0 * ADU                                   # an exact integer: 3, no remainder
    x[0, 0, 0], x[0, 0, 2] = 5.5 * ADU, above(5.5 * ADU)      # v == vmax counts, one ulp above does not
    par = dict(thr_seed=0.5, thr_total=0.875, vmax=5.5 * ADU)
    got = _run(x.reshape(1, -1), shape, cuda_device, **par)
    k = got["kmap"].reshape(shape)[0]
    assert k[1].tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 3, 0, 0]
    assert k[0, 0] == 5 and k[0, 2] == 0 and got["cnt"].reshape(shape)[0, 0, :3].tolist() == [1, 0, 0]
    _same(got, _ref(x.reshape(1, -1), shape, **par))
    # the pair's total one ulp below thr_total (the threshold moved up by one ulp: the sum stays exact)
    par["thr_total"] = float(above(0.875))
    got = _run(x.reshape(1, -1), shape, cuda_device, **par)
    assert got["kmap"].reshape(shape)[0, 1].tolist() == [0] * 13 + [3, 0, 0]
    _same(got, _ref(x.reshape(1, -1), shape, **par))


@pytest.mark.parametrize("W", [8, 7])
def test_specials_in_every_position(native, cuda_device, W):
    """NaN, +-inf, negatives and -0.0 at every column of a row whose other pixels carry remainders."""
    shape = (1, 3, W)
    specials = [float("nan"), float("inf"), float("-inf"), -3.0, -0.0]
    x = np.empty((len(specials) * W, *shape), f32)
    x[:] = (np.array([0.625, 0.375, 1.5, 0.25, 0.9375, 0.5, 2.625, 0.4375], f32)[:W] * f32(ADU))[None, None, None, :]
    for i, s in enumerate(specials):
        for c in range(W):
            x[i * W + c, 0, 1, c] = s
    F = x.shape[0]
    got = _run(x.reshape(F, -1), shape, cuda_device)
    _same(got, _ref(x.reshape(F, -1), shape))
    assert got["cnt"].reshape(shape)[0, 1].tolist() == [F - len(specials)] * W and got["cnt"][0] == F


def test_a_masked_neighbour_reads_as_no_remainder(native, cuda_device):
    shape = (1, 3, 8)
    x = np.zeros(shape, f32)
    x[0, 1, 3], x[0, 1, 4] = 0.625 * ADU, 0.375 * ADU
    x[0, 2, 3] = 0.75 * ADU     # a larger neighbour below: masked, it neither takes the seed nor adds
    mask = np.ones(shape, np.uint8)
    mask[0, 2, 3] = 0
    got = _run(x.reshape(1, -1), shape, cuda_device, mask=mask.reshape(-1))
    assert got["kmap"].reshape(shape)[0].nonzero().tolist() == [[1, 3]]
    _same(got, _ref(x.reshape(1, -1), shape, mask=mask.reshape(-1)))
    mask[0, 1, 4] = 0           # now the partner is masked too: 0.625 alone is below thr_total
    got = _run(x.reshape(1, -1), shape, cuda_device, mask=mask.reshape(-1))
    assert int(got["kmap"].sum()) == 0 and int(got["cnt"].sum()) == 1
    _same(got, _ref(x.reshape(1, -1), shape, mask=mask.reshape(-1)))


def test_254_whole_photons_and_a_merge_make_255_and_the_last_bin(native, cuda_device):
    shape = (1, 2, 8)
    x = np.zeros((2, *shape), f32)
    x[0, 0, 0, 1], x[0, 0, 0, 2] = 254.75 * ADU, 0.5 * ADU
    x[0, 0, 1, 5] = 8.0 * ADU
    x[1, 0, 1, 0], x[1, 0, 1, 7], x[1, 0, 0, 4] = 7.0 * ADU, 9.0 * ADU, 100.0 * ADU
    roi = np.zeros(shape, np.uint8)
    roi[0, 0, 4] = 255          # in no ROI: counted into psum, not into pk / tot
    par = dict(vmax=254.9 * ADU)
    got = _run(x.reshape(2, -1), shape, cuda_device, roi=roi.reshape(-1), n_roi=1, **par)
    k = got["kmap"].reshape(2, 2, 8)
    assert k[0, 0, 1] == 255 and k[0, 0, 2] == 0 and k[0, 1, 5] == 8
    assert got["pk"][0, 0].tolist() == [0] * 7 + [2] and int(got["tot"][0, 0]) == 263
    assert got["pk"][1, 0].tolist() == [0, 0, 0, 0, 0, 0, 1, 1] and int(got["tot"][1, 0]) == 16
    assert int(got["psum"].reshape(shape)[0, 0, 4]) == 100
    _same(got, _ref(x.reshape(2, -1), shape, roi=roi.reshape(-1), n_roi=1, **par))


def test_preloaded_accumulators_and_a_carry_across_2_32(native, cuda_device):
    shape = (2, 5, 12)
    n = 120
    x = _values(shape, 9, 77)
    x[:, 17] = 3.0 * ADU
    rng = np.random.default_rng(9)
    pre = {"cnt": rng.integers(0, 2 ** 30, n), "occ": rng.integers(0, 2 ** 30, n),
           "psum": rng.integers(0, 2 ** 62, n, dtype=np.int64)}
    pre["psum"][17] = 2 ** 32 - 5
    pre["psum"][18] = 0x0123456789ABCDEF
    want = _ref(x, shape)
    assert int(want["psum"][17]) == 27
    for names in (True, False):   # with and without kmap: the accumulators are the same
        got = _run(x, shape, cuda_device, kmap=names, bufs=Bufs(9, n, 1, cuda_device, names, pre))
        for k in ("cnt", "occ", "psum"):
            assert torch.equal(got[k], torch.as_tensor(pre[k]).to(want[k].dtype) + want[k]), k
        assert int(got["psum"][17]) == 2 ** 32 + 22
        _same(got, want, ("kmap", "pk", "tot"))


def test_two_streams_with_their_own_sets_add_to_one_streams_result(native, cuda_device):
    shape = (2, 5, 12)
    x = _values(shape, 12, 5)
    one = _run(x, shape, cuda_device)
    s1, s2 = torch.cuda.Stream(cuda_device), torch.cuda.Stream(cuda_device)
    torch.cuda.synchronize()
    a = _run(x[:7], shape, cuda_device, stream=s1)
    b = _run(x[7:], shape, cuda_device, stream=s2)
    for k in ("cnt", "psum", "occ"):
        assert torch.equal(a[k] + b[k], one[k]), k
    for k in ("kmap", "pk", "tot"):
        assert torch.equal(torch.cat([a[k], b[k]]), one[k]), k
    _same(one, _ref(x, shape))


def test_everything_is_checked_before_any_launch(native, cuda_device):
    dev = cuda_device
    shape, n = (2, 3, 4), 24
    fr = [torch.ones(n, device=dev)]
    ok = dict(cnt=torch.zeros(n, dtype=torch.int32, device=dev), psum=torch.zeros(n, dtype=torch.int64, device=dev),
              occ=torch.zeros(n, dtype=torch.int32, device=dev), pk=torch.zeros((1, 1, 8), dtype=torch.int32, device=dev),
              tot=torch.zeros((1, 1), dtype=torch.int64, device=dev))
    lab = lambda v: torch.full((n,), v, dtype=torch.uint8, device=dev)   # noqa: E731
    bad = [dict(adu_per_photon=0.0), dict(adu_per_photon=float("nan")), dict(vmax=255.0 * ADU), dict(thr_seed=0.0),
           dict(thr_seed=0.95), dict(thr_total=2.0), dict(shape=(2, 3, 5)), dict(shape=(24,)),
           dict(cnt=ok["cnt"][:-1]), dict(psum=ok["psum"].int()), dict(occ=ok["occ"].cpu()),
           dict(pk=torch.zeros((1, 2, 8), dtype=torch.int32, device=dev)), dict(tot=ok["tot"].int()),
           dict(mask=torch.ones(n - 1, dtype=torch.uint8, device=dev)), dict(mask=torch.ones(n, dtype=torch.int32, device=dev)),
           dict(roi=lab(0)[:-1]), dict(roi=lab(1), n_roi=1), dict(roi=lab(8), n_roi=8), dict(n_roi=2),
           dict(roi=lab(0), n_roi=9), dict(roi=lab(0), n_roi=0), dict(kmap=torch.zeros((1, n + 1), dtype=torch.uint8, device=dev)),
           dict(kmap=torch.zeros((1, n), dtype=torch.int32, device=dev)), dict(frames_so_far=2 ** 31 - 1),
           dict(frames=[torch.ones(n + 1, device=dev)]), dict(frames=[torch.ones(n, device=dev).double()]),
           dict(frames=[torch.ones(n)])]
    for kw in bad:
        args = dict(frames=fr, shape=shape, adu_per_photon=ADU, **ok)
        args.update(kw)
        with pytest.raises(ValueError):
            kernels.photons(**args)
    torch.cuda.synchronize()
    assert all(int(t.abs().sum()) == 0 for t in ok.values())
    kernels.photons(fr, shape, ADU, **ok, roi=lab(255), n_roi=1)   # 255 alone is fine: nothing in pk
    torch.cuda.synchronize()
    # a plateau of 0.5 per panel: its first pixel is the one seed
    assert int(ok["psum"].sum()) == 2 and int(ok["cnt"].sum()) == n and int(ok["pk"].sum()) == 0
