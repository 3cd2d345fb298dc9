"""K-15 cube kernel (csrc/cube.hip) against the integer golden model, word for word for all four outputs,
on the smallest shapes where each hazard exists."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

NAMES = ("nfr", "cnt", "sum", "sq")
DTYPES = (torch.int64, torch.int32, torch.int64, torch.int64)
VMIN, VMAX, S = -float(2 ** 20), float(2 ** 20), 2
GUARD = 64          # guard words behind every accumulator
GUARD_WORD = 0x5EED


class Acc:
    """A fresh accumulator set on the device, every tensor followed by GUARD guard words."""

    def __init__(self, B, n, dev, pre=None):
        self.B, self.n = B, n
        self.raw, self.t = [], []
        for name, dt in zip(NAMES, DTYPES):
            words = B if name == "nfr" else B * n
            words_al = (words + 3) // 4 * 4
            r = torch.full((words_al + GUARD,), GUARD_WORD, dtype=dt, device=dev)
            v = r[:words].view(B) if name == "nfr" else r[:words].view(B, n)
            v.fill_(0)
            if pre is not None and name in pre:
                v.copy_(torch.as_tensor(pre[name]).to(dt).reshape(v.shape))
            self.raw.append(r)
            self.t.append(v)

    def host(self):
        torch.cuda.synchronize()
        for r, name in zip(self.raw, NAMES):
            words = self.B if name == "nfr" else self.B * self.n
            assert bool((r[words:].cpu() == GUARD_WORD).all()), f"guard words behind {name} were written"
        return tuple(v.cpu() for v in self.t)


def _device_frames(x, dev):
    """Rows of one device tensor where a row is 16-B aligned, else F allocations of their own."""
    F, n = x.shape
    if (4 * n) % 16 == 0:
        xd = x.to(dev)
        return [xd[f] for f in range(F)]
    return [x[f].clone().to(dev) for f in range(F)]


def _run(x, bins, B, dev, acc=None, params=(VMIN, VMAX, S), split=None, frames_so_far=0):
    """x: float32 [F, n] on the host; ``split``: launch sizes (default: one call)."""
    F, n = x.shape
    frames = _device_frames(x, dev)
    acc = Acc(B, n, dev) if acc is None else acc
    a = 0
    for k in (split or [F]):
        kernels.cube_accumulate(frames[a:a + k], list(bins[a:a + k]), B, *params, *acc.t,
                                frames_so_far=frames_so_far + a)
        a += k
    assert a == F
    return acc.host()


def _ref(x, bins, B, params=(VMIN, VMAX, S)):
    return reference.cube_accumulate_reference(x, bins, B, *params)


def _same(got, want):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype, name
        assert g.shape == w.shape, name
        assert torch.equal(g, w), f"{name} differs at {(g != w).nonzero()[:4].tolist()}"


def _plus(pre, want):
    return tuple(p + w for p, w in zip(pre, want))


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


@pytest.mark.parametrize("n", [1, 3, 4, 5, 1020, 1023, 1024, 1025, 1028, 2049])
def test_sizes_around_a_block_with_interleaved_bins(native, cuda_device, n):
    """Around one 256-lane block of quads (1024 pixels), both n % 4 paths, planes b >= 1 unaligned when
    n % 4 != 0.  13 frames in 3 bins, not pre-sorted, two of them dropped."""
    bins = [2, 0, -1, 2, 1, 0, 0, 2, -1, 1, 2, 0, 2]
    x = _frames((13, n), 100 + n)
    x[2] = float("nan")   # a dropped frame is not read: whatever it holds adds nothing
    want = _ref(x, bins, 3)
    assert want[0].tolist() == [4, 2, 5]
    _same(_run(x, bins, 3, cuda_device), want)


@pytest.mark.parametrize("F", [1, 2, 7, 8, 9, 12, 13, 64])
@pytest.mark.parametrize("n", [1024, 1025])
def test_every_remainder_of_the_frame_groups_in_one_bin(native, cuda_device, F, n):
    """All frames in one bin (G = 1), the last of two: every remainder of the 8 / 4 / 1 loads in flight."""
    x = _frames((F, n), 10 + F)
    bins = [1] * F
    _same(_run(x, bins, 2, cuda_device), _ref(x, bins, 2))


@pytest.mark.parametrize("F", [1, 2, 7, 8, 9, 12, 13, 64])
@pytest.mark.parametrize("n", [1028, 1023])
def test_every_frame_in_a_bin_of_its_own(native, cuda_device, F, n):
    """G = F: every frame is a group of its own, with 16-B aligned planes (n % 4 == 0) and without."""
    x = _frames((F, n), 30 + F)
    bins = [(f * 37 + 5) % 64 for f in range(F)]   # distinct, unsorted
    assert len(set(bins)) == F
    _same(_run(x, bins, 64, cuda_device), _ref(x, bins, 64))


@pytest.mark.parametrize("n", [1024, 1025])
def test_group_sizes_8_4_1_1_and_a_jittered_scan(native, cuda_device, n):
    bins = [7, 7, 3, 7, 63, 7, 3, 7, 0, 7, 3, 7, 3, 7]
    assert sorted(bins.count(b) for b in set(bins)) == [1, 1, 4, 8]
    x = _frames((14, n), 50)
    _same(_run(x, bins, 64, cuda_device), _ref(x, bins, 64))
    # a delay scan with jitter: 64 frames over about 40 bins -- single frames, pairs and triples, some dropped
    g = torch.Generator().manual_seed(51)
    bins = (torch.rand(64, generator=g) * 41).to(torch.int64).sub(1).tolist()
    sizes = [bins.count(b) for b in set(bins) if b >= 0]
    assert sizes.count(1) >= 5 and max(sizes) >= 3 and -1 in bins
    x = _frames((64, n), 52)
    _same(_run(x, bins, 40, cuda_device), _ref(x, bins, 40))


@pytest.mark.parametrize("B, n", [(1, 1025), (2, 5), (3, 4), (64, 5), (4096, 4), (4096, 5), (4096, 1024)])
def test_first_and_last_bin_only_and_the_others_keep_their_pattern(native, cuda_device, B, n):
    """Frames in bin 0 and bin B - 1 only; every other bin, preloaded with a bit pattern, is bit-identical
    afterwards (neither read nor written), nfr included."""
    F = 9
    bins = [0 if f % 2 else B - 1 for f in range(F)]
    x = _frames((F, n), 60 + B)
    pat = torch.arange(B * n, dtype=torch.int64).reshape(B, n)
    pre = {"nfr": torch.arange(B, dtype=torch.int64) * 0x12345678 - 77, "cnt": pat % 1000 - 500,
           "sum": pat * 0x0123456789 - 2 ** 45, "sq": -(pat * 0x1F3D5B79) - 1}
    acc = Acc(B, n, cuda_device, pre=pre)
    before = tuple(t.cpu().clone() for t in acc.t)
    got = _run(x, bins, B, cuda_device, acc=acc)
    _same(got, _plus(before, _ref(x, bins, B)))
    for g, b, name in zip(got, before, NAMES):
        assert torch.equal(g[1:B - 1], b[1:B - 1]), name


def test_all_dropped_writes_nothing(native, cuda_device):
    n, B = 1028, 3
    x = _frames((9, n), 70)
    pat = torch.arange(B * n, dtype=torch.int64).reshape(B, n)
    pre = {"nfr": torch.tensor([0x123456789A, -77, 5]), "cnt": pat % 1000 - 500, "sum": pat * 0x0123456789 - 2 ** 45,
           "sq": -(pat * 0x1F3D5B79) - 1}
    acc = Acc(B, n, cuda_device, pre=pre)
    before = tuple(t.cpu().clone() for t in acc.t)
    _same(_run(x, [-1] * 9, B, cuda_device, acc=acc), before)
    assert _ref(x, [-1] * 9, B)[0].tolist() == [0, 0, 0]


def _special_values():
    na = np.nextafter
    f32 = np.float32
    vals = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, VMIN, VMAX,
            float(na(f32(VMIN), f32(-np.inf))), float(na(f32(VMAX), f32(np.inf))),
            float(na(f32(VMIN), f32(0))), float(na(f32(VMAX), f32(0)))]
    for k in (0, 1, 2, 3, 80, 81, 4001, 4002):          # ties (k + 0.5) / 2^S, both signs and parities
        vals += [(k + 0.5) / 2 ** S, -(k + 0.5) / 2 ** S]
    return vals


def test_window_and_rounding_in_every_lane_position(native, cuda_device):
    """Every special value in every position of a lane's four pixels (frame f rotates the list by f), in
    groups of several frames and in single-frame groups."""
    vals = _special_values()
    L = len(vals)
    n = 64 * 4 * 2
    x = torch.empty((L, n), dtype=torch.float32)
    for f in range(L):
        for p in range(n):
            x[f, p] = vals[(p + f) % L]
    x[:, 41] = float("nan")                           # never contributes
    bins = [f % 3 for f in range(L)]
    want = _ref(x, bins, 3)
    assert int(want[1][:, 41].sum()) == 0 and 0 < int(want[1][0, 0]) < bins.count(0)
    _same(_run(x, bins, 3, cuda_device), want)
    bins = list(range(L))
    _same(_run(x, bins, L, cuda_device), _ref(x, bins, L))


def test_preloaded_accumulators_carry_order_and_split(native, cuda_device):
    """sum = 2^32 - 5 and -(2^32) + 5, sq = 2^40 - 3, cnt = 2^20 preloaded: the adds carry across the
    32-bit boundary in both directions.  The same call twice accumulates; a permuted frame order and a
    different batch split give the same words."""
    dev = cuda_device
    n, F, B = 3072, 11, 2
    x = _frames((F, n), 5)
    bins = [0, 1, 0, 0, 1, 1, 0, 1, 0, 0, 1]
    want = _ref(x, bins, B)
    pre = {"cnt": torch.full((B, n), 2 ** 20), "sq": torch.full((B, n), 2 ** 40 - 3),
           "sum": torch.stack([torch.full((n,), 2 ** 32 - 5), torch.full((n,), -(2 ** 32) + 5)]),
           "nfr": torch.tensor([2 ** 33, 5])}

    def fresh():
        a = Acc(B, n, dev, pre=pre)
        return a, tuple(t.cpu().clone() for t in a.t)

    acc, p0 = fresh()
    once = _plus(p0, want)
    _same(_run(x, bins, B, dev, acc=acc), once)
    s = want[2]
    assert bool((s[0] > 5).any()) and bool((s[0] < -5).any()) and bool((s[1] > 5).any()) and bool((s[1] < -5).any())
    _same(_run(x, bins, B, dev, acc=acc, frames_so_far=F), _plus(once, want))
    perm = torch.randperm(F, generator=torch.Generator().manual_seed(6)).tolist()
    acc, _ = fresh()
    _same(_run(x[perm].contiguous(), [bins[i] for i in perm], B, dev, acc=acc), once)
    acc, _ = fresh()
    _same(_run(x, bins, B, dev, acc=acc, split=[3, 1, 7]), once)


def test_count_reaches_int32_max_with_a_consistent_frames_so_far(native, cuda_device):
    """Q = 1: a run holds 2^31 - 1 frames.  cnt preloaded with 2^31 - 1 - F and as many frames_so_far: the F
    frames take it to exactly 2^31 - 1."""
    p = (-1.0, 1.0, 0)
    top = 2 ** 31 - 1
    assert reference.powder_max_frames(*p) == top
    F, n = 9, 1028
    x = torch.ones((F, n))
    x[:, ::3] = -1.0
    pre = {"cnt": torch.full((2, n), top - F), "nfr": torch.tensor([0, top - F])}
    acc = Acc(2, n, cuda_device, pre=pre)
    got = _run(x, [1] * F, 2, cuda_device, acc=acc, params=p, frames_so_far=top - F)
    assert bool((got[1][1] == top).all()) and bool((got[1][0] == top - F).all()) and got[0].tolist() == [0, top]
    assert bool((got[3][1] == F).all()) and bool((got[2][1, 1] == F).all()) and bool((got[2][1, 0] == -F).all())


def test_largest_adds(native, cuda_device):
    """64 frames of vmax / vmin in one bin at the default parameters (q = +-2^22: sq = 2^50, sum = +-2^28),
    and the extreme Q = 2^31 - 2^7 (a run of two frames at most) with q * q near 2^62."""
    n = 1024 + 8
    x = torch.full((64, n), VMAX)
    x[:, 1::2] = VMIN
    want = _ref(x, [2] * 64, 3)
    assert int(want[3][2].min()) == 2 ** 50 and int(want[2].max()) == 2 ** 28 and int(want[2].min()) == -2 ** 28
    _same(_run(x, [2] * 64, 3, cuda_device), want)
    top = float(np.float32(2 ** 15 - 2 ** -9))
    p = (-top, top, 16)
    assert reference.powder_max_frames(*p) == 2
    y = torch.full((2, 1024), top)
    y[:, ::3] = -top
    for bins in ([1, 1], [1, 0]):
        want = _ref(y, bins, 2, params=p)
        assert int(want[3].max()) == bins.count(1) * (2 ** 31 - 2 ** 7) ** 2
        _same(_run(y, bins, 2, cuda_device, params=p), want)


def test_two_streams_with_their_own_sets_add_up_to_one_set(native, cuda_device):
    dev = cuda_device
    n, F, B = 3072, 24, 5
    x = _frames((F, n), 80)
    bins = [(f * 3) % 6 - 1 for f in range(F)]
    frames = _device_frames(x, dev)
    sets = [Acc(B, n, dev), Acc(B, n, dev)]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    torch.cuda.synchronize()
    for a in range(0, F, 4):
        k = (a // 4) % 2
        kernels.cube_accumulate(frames[a:a + 4], bins[a:a + 4], B, VMIN, VMAX, S, *sets[k].t, frames_so_far=a,
                                stream=streams[k])
    h0, h1 = sets[0].host(), sets[1].host()
    assert int(h0[0].sum()) > 0 and int(h1[0].sum()) > 0
    _same(_plus(h0, h1), _ref(x, bins, B))
    _same(_run(x, bins, B, dev), _ref(x, bins, B))


def test_validation_raises_before_any_launch(native, cuda_device):
    dev = cuda_device
    n, B = 64, 3
    MARK = 0x5A5A
    frames = [torch.ones(n, dtype=torch.float32, device=dev)]

    def acc(nb=B, nn=n, **dts):
        return tuple(torch.full((nb,) if name == "nfr" else (nb, nn), MARK, dtype=dts.get(name, dt), device=dev)
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
        dict(frames=[frames[0], torch.zeros(n + 4, dtype=torch.float32, device=dev)], bins=[0, 0]),   # unequal numel
        dict(frames=[torch.ones(n, dtype=torch.float32)]),                        # frames on the host
        dict(acc=acc(cnt=torch.int64)), dict(acc=acc(sum=torch.int32)), dict(acc=acc(sq=torch.int32)),
        dict(acc=acc(nfr=torch.int32)),
        dict(acc=acc(nn=n + 4)),                                                  # wrong shape
        dict(acc=acc(nb=B + 1)),                                                  # planes for another nbins
        dict(acc=tuple(t.cpu() for t in acc())),                                  # accumulators on the host
        dict(bins=[B]), dict(bins=[-2]), dict(bins=[0, 0]), dict(bins=[]), dict(bins=[0.5]), dict(bins=None),
        dict(bins=torch.zeros(1, dtype=torch.int32, device=dev)),                 # bins on the device
        dict(nbins=0), dict(nbins=4097), dict(nbins=2.5),
        dict(vmin=1.0, vmax=0.0),                                                 # window not ordered
        dict(vmax=float("inf")), dict(vmin=float("nan")), dict(vmax=1e39),        # window not finite
        dict(frac_bits=-1), dict(frac_bits=17), dict(frac_bits=1.5),
        dict(vmax=float(2 ** 20), frac_bits=11),                                  # Q = 2^31
        dict(frames_so_far=max_frames),                                           # the run is full
        dict(frames_so_far=-1),
    ] + [dict(acc=off(acc(), i)) for i in range(1, 4)]                            # misaligned accumulators
    for case in cases:
        a = case.get("acc", good)
        with pytest.raises(ValueError):
            kernels.cube_accumulate(case.get("frames", frames), case.get("bins", [1]), case.get("nbins", B),
                                    case.get("vmin", VMIN), case.get("vmax", VMAX), case.get("frac_bits", S), *a,
                                    frames_so_far=case.get("frames_so_far", 0))
        torch.cuda.synchronize()
        for t in (*a, *good):
            assert bool((t == MARK).all()), case
    # one below the bound still runs; numpy and CPU-tensor bins are taken
    kernels.cube_accumulate(frames, np.array([1], np.int64), B, VMIN, VMAX, S, *good, frames_so_far=max_frames - 1)
    torch.cuda.synchronize()
    assert good[0].tolist() == [MARK, MARK + 1, MARK]
    assert bool((good[1][1] == MARK + 1).all()) and bool((good[2][1] == MARK + 4).all())
    assert bool((good[3][1] == MARK + 16).all())
    for t in good[1:]:
        assert bool((t[0] == MARK).all()) and bool((t[2] == MARK).all())
