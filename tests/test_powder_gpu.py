"""K-11 powder-statistics kernel (csrc/powder.hip) against the integer golden model, word for word for
all six outputs, on the smallest shapes where each hazard exists."""
import numpy as np
import pytest
import torch

from psana_ray_amd.models import get_detector
from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

NAMES = ("nfr", "cnt", "sum", "sq", "qmax", "above")
DTYPES = (torch.int64, torch.int32, torch.int64, torch.int64, torch.int32, torch.int32)
NONE = -2 ** 31
VMIN, VMAX, S, THR = -float(2 ** 20), float(2 ** 20), 2, 20.0
GUARD = 64          # guard words behind every accumulator
GUARD_WORD = 0x5EED


class Acc:
    """A fresh accumulator set on the device, every tensor followed by GUARD guard words."""

    def __init__(self, nc, n, dev, pre=None):
        self.nc, self.n = nc, n
        self.raw, self.t = [], []
        for name, dt in zip(NAMES, DTYPES):
            words = nc if name == "nfr" else nc * n
            words_al = (words + 3) // 4 * 4
            r = torch.full((words_al + GUARD,), GUARD_WORD, dtype=dt, device=dev)
            v = r[:words].view(nc) if name == "nfr" else r[:words].view(nc, n)
            v.fill_(NONE if name == "qmax" else 0)
            if pre is not None and name in pre:
                v.copy_(torch.as_tensor(pre[name]).to(dt).reshape(v.shape))
            self.raw.append(r)
            self.t.append(v)

    def host(self):
        torch.cuda.synchronize()
        for r, name in zip(self.raw, NAMES):
            words = self.nc if name == "nfr" else self.nc * self.n
            assert bool((r[words:].cpu() == GUARD_WORD).all()), f"guard words behind {name} were written"
        return tuple(v.cpu() for v in self.t)


def _run(x, dev, keys=None, key_min=0, acc=None, separate=False, params=(VMIN, VMAX, S, THR), split=None):
    """x: float32 [F, n] on the host.  Frames are rows of one device tensor or, with ``separate``, F
    allocations of their own; ``split``: launch sizes (default: one call)."""
    F, n = x.shape
    if separate:
        frames = [x[f].clone().to(dev) for f in range(F)]
    else:
        assert (4 * n) % 16 == 0 or F == 1
        xd = x.to(dev)
        frames = [xd[f] for f in range(F)]
    acc = Acc(1 if keys is None else 2, n, dev) if acc is None else acc
    kd = None if keys is None else torch.as_tensor(keys, dtype=torch.int32).to(dev)
    a = 0
    for k in (split or [F]):
        kernels.powder_accumulate(frames[a:a + k], *params, *acc.t, keys=None if kd is None else kd[a:a + k].clone(),
                                  key_min=key_min, frames_so_far=a)
        a += k
    assert a == F
    return acc.host()


def _ref(x, keys=None, key_min=0, params=(VMIN, VMAX, S, THR)):
    k = None if keys is None else torch.as_tensor(keys, dtype=torch.int32)
    return reference.powder_accumulate_reference(x, *params, keys=k, key_min=key_min)


def _same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype, name
        assert g.shape == w.shape, name
        assert torch.equal(g, w), f"{name} differs at {(g != w).nonzero()[:4].tolist()}"


def _plus(pre, want):
    """Golden words after adding ``want`` to the preloaded set ``pre`` (tuples in NAMES order)."""
    return tuple(torch.maximum(p, w) if name == "qmax" else p + w for p, w, name in zip(pre, want, NAMES))


def _frames(shape, seed, scale=30.0):
    """Calibrated-looking values: noise around 0 with both signs, some bright pixels, a few specials."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    flat = x.reshape(-1)
    flat[::17] = flat[::17].abs() * 40.0 + 20.0
    flat[5::29] = float("nan")
    flat[7::31] = float("inf")
    flat[11::37] = -0.0
    return x.contiguous()


def test_1027_tail_and_partial_workgroup(native, cuda_device):
    """n = 1027: two 1024-pixel workgroups, the second partial, and the n % 4 = 3 scalar tail.  Frames of
    4108 B are separate allocations."""
    x = _frames((9, 1027), 1)
    x[:, 1024:] = VMAX
    x[4, 1026] = -17.25
    _same(_run(x, cuda_device, separate=True), _ref(x))


@pytest.mark.parametrize("n", [3, 5, 1026, 1027])
def test_unaligned_class1_planes(native, cuda_device, n):
    """n % 4 != 0 with NC = 2: the planes of class 1 start at n elements, not 16-B aligned."""
    x = _frames((7, n), 2 + n)
    keys = [0, 5, 1, 7, 2, 0, 9]
    _same(_run(x, cuda_device, keys=keys, key_min=2, separate=True), _ref(x, keys, 2))


@pytest.mark.parametrize("F", [1, 3, 4, 7, 8, 9, 13, 64])
@pytest.mark.parametrize("nc", [1, 2])
def test_tiny_epix_unroll_remainders(native, cuda_device, F, nc):
    """Every remainder of the 8 / 4 / 1 frame groups, for both passes: with NC = 2 the classes split the
    frames unevenly (class 1 gets every third frame)."""
    n = get_detector("tiny_epix").npix
    x = _frames((F, n), 10 + F)
    keys = None if nc == 1 else [3 * (f % 3 == 0) for f in range(F)]
    _same(_run(x, cuda_device, keys=keys, key_min=3), _ref(x, keys, 3))


def test_tiny_epix_67_frames_two_launches(native, cuda_device):
    n = get_detector("tiny_epix").npix
    x = _frames((67, n), 3)
    keys = [(f * 7) % 5 for f in range(67)]
    _same(_run(x, cuda_device, keys=keys, key_min=3, separate=True), _ref(x, keys, 3))
    _same(_run(x, cuda_device, separate=True), _ref(x))


def _special_values():
    na = np.nextafter
    f32 = np.float32
    vals = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, VMIN, VMAX,
            float(na(f32(VMIN), f32(-np.inf))), float(na(f32(VMAX), f32(np.inf))),
            float(na(f32(VMIN), f32(0))), float(na(f32(VMAX), f32(0))),
            THR, float(na(f32(THR), f32(0))), float(na(f32(THR), f32(np.inf)))]
    for k in (0, 1, 2, 3, 80, 81, 4001, 4002):          # ties (k + 0.5) / 2^S, both signs and parities
        vals += [(k + 0.5) / 2 ** S, -(k + 0.5) / 2 ** S]
    return vals


def test_window_rounding_and_threshold_in_every_lane_position(native, cuda_device):
    """Every special value in every position of a lane's four pixels (frame f rotates the list by f), a
    pixel whose samples are all negative (qmax < 0) and one that never contributes (qmax INT32_MIN)."""
    vals = _special_values()
    L = len(vals)
    n = 64 * 4 * 2
    F = L
    x = torch.empty((F, n), dtype=torch.float32)
    for f in range(F):
        for p in range(n):
            x[f, p] = vals[(p + f) % L]
    x[:, 40] = torch.linspace(-900.5, -0.25, F)       # all negative
    x[:, 41] = float("nan")                           # never contributes
    x[:, 42] = float(np.nextafter(np.float32(VMAX), np.float32(np.inf)))
    want = _ref(x)
    assert int(want[4][0, 40]) < 0 and int(want[4][0, 41]) == NONE and int(want[1][0, 41]) == 0
    assert int(want[4][0, 42]) == NONE
    _same(_run(x, cuda_device), want)
    keys = [f % 2 for f in range(F)]
    _same(_run(x, cuda_device, keys=keys, key_min=1), _ref(x, keys, 1))


@pytest.mark.parametrize("keys, key_min", [([0] * 9, 1), ([5] * 9, 1), ([0, 1] * 4 + [0], 1),
                                           ([4, 3, 4, 3, 4, 3, 4, 3, 4], 4), ([-1, 0, -1, 0, 1, -5, 0, 0, -1], 0)])
def test_classes(native, cuda_device, keys, key_min):
    """All miss, all hit, alternating, keys == key_min and key_min - 1, negative keys."""
    n = get_detector("tiny_epix").npix
    x = _frames((9, n), 21)
    want = _ref(x, keys, key_min)
    assert want[0].tolist() == [sum(k < key_min for k in keys), sum(k >= key_min for k in keys)]
    _same(_run(x, cuda_device, keys=keys, key_min=key_min), want)


@pytest.mark.parametrize("empty", [0, 1])
@pytest.mark.parametrize("n", [2112, 1027])
def test_class_without_frames_is_left_exactly_as_it_was(native, cuda_device, empty, n):
    """A class with no frame in the launch, preloaded with an arbitrary bit pattern, is bit-identical
    afterwards (its words are neither read nor written), nfr included."""
    x = _frames((9, n), 22)
    keys = [1 - empty] * 9
    pat = torch.arange(2 * n, dtype=torch.int64).reshape(2, n)
    pre = {"nfr": torch.tensor([0x123456789A, -77]), "cnt": pat % 1000 - 500, "sum": pat * 0x0123456789 - 2 ** 45,
           "sq": -(pat * 0x1F3D5B79) - 1, "qmax": pat % 4001 - 2000, "above": -(pat % 77)}
    acc = Acc(2, n, cuda_device, pre=pre)
    before = tuple(t.cpu().clone() for t in acc.t)
    got = _run(x, cuda_device, keys=keys, key_min=1, acc=acc, separate=True)
    want = _plus(before, _ref(x, keys, 1))
    for g, w, b, name in zip(got, want, before, NAMES):
        assert torch.equal(g[empty], b[empty]), name
        assert torch.equal(g[1 - empty], w[1 - empty]), name


def test_preloaded_accumulators_carry_and_order(native, cuda_device):
    """sum = 2^32 - 5 and -(2^32) + 5, sq = 2^40 - 3, cnt = 2^20 preloaded: the adds carry across the
    32-bit boundary in both directions.  The same call twice accumulates; a permuted frame order and a
    different batch split give the same words."""
    dev = cuda_device
    n = get_detector("tiny_epix").npix
    F = 11
    x = _frames((F, n), 5)
    keys = [0, 2, 0, 0, 2, 2, 0, 2, 0, 0, 2]
    want = _ref(x, keys, 1)
    pre = {"cnt": torch.full((2, n), 2 ** 20), "sq": torch.full((2, n), 2 ** 40 - 3),
           "sum": torch.stack([torch.full((n,), 2 ** 32 - 5), torch.full((n,), -(2 ** 32) + 5)]),
           "qmax": torch.full((2, n), -3), "above": torch.full((2, n), 9), "nfr": torch.tensor([2 ** 33, 5])}

    def fresh():
        a = Acc(2, n, dev, pre=pre)
        return a, tuple(t.cpu().clone() for t in a.t)

    acc, p0 = fresh()
    once = _plus(p0, want)
    _same(_run(x, dev, keys=keys, key_min=1, acc=acc), once)
    s = want[2]
    assert bool((s[0] > 5).any()) and bool((s[0] < -5).any()) and bool((s[1] > 5).any()) and bool((s[1] < -5).any())
    _same(_run(x, dev, keys=keys, key_min=1, acc=acc), _plus(once, want))
    perm = torch.randperm(F, generator=torch.Generator().manual_seed(6)).tolist()
    acc, _ = fresh()
    _same(_run(x[perm].contiguous(), dev, keys=[keys[i] for i in perm], key_min=1, acc=acc), once)
    acc, _ = fresh()
    _same(_run(x, dev, keys=keys, key_min=1, acc=acc, split=[3, 1, 7]), once)


def test_largest_adds_64_frames_of_vmax(native, cuda_device):
    """A frame of vmax at the default parameters (q = 2^22, q * q = 2^44) over 64 frames: the largest
    in-batch partials, sq = 2^50 and sum = 2^28; and of vmin (sum = -2^28)."""
    n = 1024 + 8
    x = torch.full((64, n), VMAX)
    x[:, 1::2] = VMIN
    want = _ref(x)
    assert int(want[3].min()) == 2 ** 50 and int(want[2].max()) == 2 ** 28 and int(want[2].min()) == -2 ** 28
    _same(_run(x, cuda_device), want)


def test_small_window_many_frac_bits(native, cuda_device):
    """--powder_vmax 1024 --powder_frac_bits 12 (a detector calibrated in photons), and the extreme
    Q = 2^31 - 2^7 (a run of two frames at most) with q * q near 2^62."""
    n = get_detector("tiny_epix").npix
    x = _frames((5, n), 23, scale=3.0)
    p = (-1024.0, 1024.0, 12, 0.5)
    _same(_run(x, cuda_device, params=p), _ref(x, params=p))
    top = float(np.float32(2 ** 15 - 2 ** -9))
    p = (-top, top, 16, 1.0)
    assert reference.powder_max_frames(-top, top, 16) == 2
    y = torch.full((2, 1024), top)
    y[:, ::3] = -top
    want = _ref(y, params=p)
    assert int(want[3].max()) == 2 * (2 ** 31 - 2 ** 7) ** 2
    _same(_run(y, cuda_device, params=p), want)


def test_epix10k2m_production_shape(native, cuda_device):
    """3 frames of epix10k2M, NC = 2: 2112 workgroups."""
    spec = get_detector("epix10k2M")
    assert spec.npix // 1024 == 2112
    x = _frames((3, spec.npix), 8)
    keys = [4, 0, 9]
    _same(_run(x, cuda_device, keys=keys, key_min=2), _ref(x, keys, 2))


def test_validation_raises_before_any_launch(native, cuda_device):
    dev = cuda_device
    n = 64
    MARK = 0x5A5A
    frames = [torch.ones(n, dtype=torch.float32, device=dev)]
    keys1 = torch.zeros(1, dtype=torch.int32, device=dev)

    def acc(nc=1, nn=n, **dts):
        return tuple(torch.full((nc,) if name == "nfr" else (nc, nn), MARK, dtype=dts.get(name, dt), device=dev)
                     for name, dt in zip(NAMES, DTYPES))

    def off(a, i):     # accumulator i replaced by a misaligned view of the same shape
        t = torch.full((a[i].numel() + 4,), MARK, dtype=a[i].dtype, device=dev)[1:a[i].numel() + 1].view(a[i].shape)
        return a[:i] + (t,) + a[i + 1:]

    good = acc()
    big = torch.zeros(n + 8, dtype=torch.float32, device=dev)
    max_frames = reference.powder_max_frames(VMIN, VMAX, S)
    assert max_frames == 524287
    cases = [
        dict(frames=[torch.zeros(n, dtype=torch.uint16, device=dev)]),           # raw frames
        dict(frames=[big[1:n + 1]]),                                              # misaligned frame
        dict(frames=[frames[0], torch.zeros(n + 4, dtype=torch.float32, device=dev)]),   # unequal numel
        dict(frames=[torch.ones(n, dtype=torch.float32)]),                        # frames on the host
        dict(acc=acc(cnt=torch.int64)), dict(acc=acc(sum=torch.int32)), dict(acc=acc(sq=torch.int32)),
        dict(acc=acc(qmax=torch.int64)), dict(acc=acc(above=torch.int64)), dict(acc=acc(nfr=torch.int32)),
        dict(acc=acc(nn=n + 4)),                                                  # wrong shape
        dict(acc=acc(nc=2)),                                                      # NC = 2 without keys
        dict(keys=keys1),                                                         # keys with NC = 1
        dict(acc=acc(nc=2), keys=torch.zeros(2, dtype=torch.int32, device=dev)),  # keys length
        dict(acc=acc(nc=2), keys=torch.zeros(1, dtype=torch.int64, device=dev)),  # keys dtype
        dict(acc=acc(nc=2), keys=torch.zeros(1, dtype=torch.int32)),              # keys on the host
        dict(acc=tuple(t.cpu() for t in acc())),                                  # accumulators on the host
        dict(vmin=1.0, vmax=0.0),                                                 # window not ordered
        dict(vmax=float("inf")), dict(vmin=float("nan")), dict(vmax=1e39),        # window not finite
        dict(frac_bits=-1), dict(frac_bits=17), dict(frac_bits=1.5),
        dict(vmax=float(2 ** 20), frac_bits=11),                                  # Q = 2^31
        dict(thr=float("nan")),
        dict(frames_so_far=max_frames),                                           # the run is full
        dict(frames_so_far=-1),
    ] + [dict(acc=off(acc(), i)) for i in range(1, 6)]                            # misaligned accumulators
    for case in cases:
        a = case.get("acc", good)
        with pytest.raises(ValueError):
            kernels.powder_accumulate(case.get("frames", frames), case.get("vmin", VMIN), case.get("vmax", VMAX),
                                      case.get("frac_bits", S), case.get("thr", THR), *a, keys=case.get("keys"),
                                      frames_so_far=case.get("frames_so_far", 0))
        torch.cuda.synchronize()
        for t in (*a, *good):
            assert bool((t == MARK).all()), case
    # one below the bound still runs
    kernels.powder_accumulate(frames, VMIN, VMAX, S, THR, *good, frames_so_far=max_frames - 1)
    torch.cuda.synchronize()
    assert bool((good[1] == MARK + 1).all()) and bool((good[2] == MARK + 4).all()) and int(good[0][0]) == MARK + 1
    assert bool((good[3] == MARK + 16).all()) and bool((good[4] == MARK).all()) and bool((good[5] == MARK).all())
