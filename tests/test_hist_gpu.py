"""K-12 per-pixel histogram kernel (csrc/pixhist.hip) against the integer golden model, word for word, on
the smallest shapes where each hazard exists.  Every accumulator is followed by guard words."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import _ext
from psana_ray_amd.ops import kernels, reference
from psana_ray_amd.ops.kernels import pixel_hist, pixel_hist_tile_pixels

pytestmark = pytest.mark.gpu

F32 = np.float32
GUARD = 64
GUARD_WORD = 0x5EED5EED
LO, HI = -32.0, 96.0
ALL_BINS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 1024]


class Acc:
    """hist int32 [n, nbins] on the device, followed by GUARD guard words; ``pre``: its content before."""

    def __init__(self, n, nbins, dev, pre=None):
        self.words = n * nbins
        self.raw = torch.full(((self.words + 3) // 4 * 4 + GUARD,), GUARD_WORD, dtype=torch.int32, device=dev)
        self.hist = self.raw[:self.words].view(n, nbins)
        self.hist.zero_()
        if pre is not None:
            self.hist.copy_(torch.as_tensor(pre, dtype=torch.int32).reshape(n, nbins))

    def host(self):
        torch.cuda.synchronize()
        assert bool((self.raw[self.words:].cpu() == GUARD_WORD).all()), "guard words behind hist were written"
        return self.hist.cpu()


def _dev_frames(x, dev):
    """Every frame an allocation of its own (ring slots are not contiguous, and n need not be a multiple of 4)."""
    return [x[f].clone().to(dev) for f in range(x.shape[0])]


def _run(x, lo, hi, nbins, dev, pre=None, split=None, layout=0):
    x = torch.as_tensor(x)
    F, n = x.shape
    frames = _dev_frames(x, dev)
    acc = Acc(n, nbins, dev, pre)
    a = 0
    for k in (split or [F]):
        pixel_hist(frames[a:a + k], lo, hi, nbins, acc.hist, frames_so_far=a, _layout=layout)
        a += k
    assert a == F
    return acc.host()


def _same(got, want):
    assert got.dtype == want.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got, want), f"hist differs at {(got != want).nonzero()[:6].tolist()}"


def _frames(F, n, lo, hi, seed):
    """Calibrated-looking values: neighbouring pixels around the same value (spread about a bin), some
    uniform over a little more than the window, a few specials."""
    g = torch.Generator().manual_seed(seed)
    w = hi - lo
    x = lo + 0.3 * w + torch.randn((F, n), generator=g) * (w / 64.0)
    u = lo - 0.1 * w + torch.rand((F, n), generator=g) * 1.2 * w
    pick = torch.rand((F, n), generator=g) < 0.3
    x = torch.where(pick, u, x)
    flat = x.reshape(-1)
    flat[5::29] = float("nan")
    flat[7::31] = float("inf")
    flat[9::41] = float("-inf")
    flat[11::37] = -0.0
    flat[13::43] = lo
    flat[17::47] = hi
    return x.contiguous()


def test_tile_pixels():
    T = {nb: pixel_hist_tile_pixels(nb) for nb in ALL_BINS}
    assert T[64] == 1024 and T[1024] == 64 and T[256] == 256 and T[1] == 1024 and T[65] == 512
    for nb, t in T.items():
        assert t & (t - 1) == 0 and 64 <= t <= 1024 and t * ((nb + 3) // 4) * 4 <= 65536
    for bad in (0, 1025):
        with pytest.raises(ValueError):
            pixel_hist_tile_pixels(bad)


@pytest.mark.parametrize("nbins", ALL_BINS)
def test_sizes_around_the_tile_and_frame_counts(native, cuda_device, nbins):
    """n in {1, 3, 4, 5, T - 1, T, T + 1, 2 T + 3} x F in {1, 2, 63, 64}: the scalar tail, a partial last
    tile, more than one workgroup, every remainder of the frame groups; nbins % 4 != 0 takes the scalar
    flush.  The golden model runs once per n on 64 frames; a prefix of the frames is a prefix of the sum."""
    T = pixel_hist_tile_pixels(nbins)
    for n in (1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 3):
        x = _frames(64, n, LO, HI, seed=nbins * 7 + n)
        frames = _dev_frames(x, cuda_device)
        for F in (1, 2, 63, 64):
            acc = Acc(n, nbins, cuda_device)
            pixel_hist(frames[:F], LO, HI, nbins, acc.hist)
            _same(acc.host(), reference.pixel_hist_reference(x[:F], LO, HI, nbins))


def _edge_values(lo, hi, nbins):
    na = np.nextafter
    lo32, hi32 = F32(lo), F32(hi)
    vals = [lo32, hi32, na(lo32, F32(-np.inf)), na(hi32, F32(np.inf)), na(lo32, F32(np.inf)), na(hi32, F32(-np.inf)),
            F32(np.nan), F32(np.inf), F32(-np.inf), F32(-0.0), F32(0.0)]
    for k in sorted({0, 1, 2, 3, 4, 5, nbins // 2, nbins - 2, nbins - 1, nbins}):   # computed bin edges +- 1 ulp
        if 0 <= k <= nbins:
            e = F32(np.float64(lo32) + k * (np.float64(hi32) - np.float64(lo32)) / nbins)
            vals += [e, na(e, F32(-np.inf)), na(e, F32(np.inf))]
    return np.array(vals, F32)


@pytest.mark.parametrize("lo,hi,nbins", [(LO, HI, 64), (0.0, 8.0, 4), (0.1, 0.7, 3), (-7.5, 11.25, 255),
                                         (100.0, 1124.0, 1024), (-1.0, 1.0, 1)])
@pytest.mark.parametrize("tail", [0, 3])
def test_special_values_in_every_lane_position(native, cuda_device, lo, hi, nbins, tail):
    """lo and hi exactly, one ulp outside and inside, NaN, +-inf, +-0.0 and the computed bin edges +- 1 ulp,
    each in all four positions of a 4-pixel group (frame f is the list rotated by f) and, with ``tail``, in
    the scalar tail."""
    vals = _edge_values(lo, hi, nbins)
    n = (len(vals) + 3) // 4 * 4 + tail
    row = np.resize(vals, n)
    x = torch.from_numpy(np.stack([np.roll(row, f) for f in range(5)]))
    want = reference.pixel_hist_reference(x, lo, hi, nbins)
    _same(_run(x, lo, hi, nbins, cuda_device), want)
    if lo == 0.0:      # -0.0 with lo = 0 goes to bin 0
        z = torch.tensor([[-0.0, 0.0, -0.0, 0.0, -0.0]])
        got = _run(z, lo, hi, nbins, cuda_device)
        assert got[:, 0].tolist() == [1] * 5 and int(got.sum()) == 5


@pytest.mark.parametrize("nbins", [64, 255, 1024])
def test_64_frames_full_counters_do_not_carry(native, cuda_device, nbins):
    """F = 64: the four pixels of a group have all 64 frames in ONE bin each, the bins being the four bytes
    of one packed word (every byte counter of that word pattern reaches 64); a pixel splits 32 / 32 and one
    16 / 16 / 16 / 16 over the bytes of a word; one pixel's frames go to 64 different bins."""
    F = 64
    T = pixel_hist_tile_pixels(nbins)
    n = T + 12
    w = (HI - LO) / nbins
    centre = lambda b: LO + (b + 0.5) * w   # noqa: E731
    x = np.full((F, n), np.nan, F32)
    for base in (0, T + 4):                                   # a group in the first tile, one in the partial second
        for i in range(4):
            x[:, base + i] = centre(4 + i)
    x[:32, 5], x[32:, 5] = centre(8), centre(9)
    for f in range(F):
        x[f, 6] = centre(12 + f % 4)
        x[f, 9] = centre(f % nbins)
        x[f, T + 9] = centre((nbins - 1 - f) % nbins)
    x = torch.from_numpy(x)
    got = _run(x, LO, HI, nbins, cuda_device)
    _same(got, reference.pixel_hist_reference(x, LO, HI, nbins))
    for base in (0, T + 4):
        for i in range(4):
            assert got[base + i, 4 + i] == 64 and int(got[base + i].sum()) == 64
    assert got[5, 8] == 32 and got[5, 9] == 32 and got[6, 12:16].tolist() == [16] * 4
    if nbins >= 64:
        assert got[9, :64].tolist() == [1] * 64


@pytest.mark.parametrize("nbins", [5, 64])
def test_adds_to_what_the_accumulator_holds(native, cuda_device, nbins):
    """A preloaded bit pattern: the kernel adds and never clears, rows no sample touches keep their
    pattern, and a word preloaded to 2^31 - 1 - 64 reaches exactly 2^31 - 1."""
    F = 64
    T = pixel_hist_tile_pixels(nbins)
    n = T + 7
    x = _frames(F, n, LO, HI, seed=3)
    x[:, 2] = LO + (1.5) * (HI - LO) / nbins                 # pixel 2: all 64 frames in bin 1
    x[:, 8:24] = float("nan")                                 # rows no sample touches
    x[:, T + 1] = float("inf")
    g = torch.Generator().manual_seed(4)
    pre = torch.randint(0, 2 ** 30, (n, nbins), generator=g, dtype=torch.int64).to(torch.int32)
    pre[8:24] = 0x55AA55AA
    pre[2, 1] = 2 ** 31 - 1 - 64
    want = reference.pixel_hist_reference(x, LO, HI, nbins)
    assert int(want[8:24].sum()) == 0 and int(want[T + 1].sum()) == 0 and int(want[2, 1]) == 64
    got = _run(x, LO, HI, nbins, cuda_device, pre=pre)
    _same(got, pre + want)
    assert int(got[2, 1]) == 2 ** 31 - 1 and bool((got[8:24] == 0x55AA55AA).all())


def test_two_streams_two_accumulators(native, cuda_device):
    nbins = 64
    n = 2 * pixel_hist_tile_pixels(nbins) + 3
    xs = [_frames(9, n, LO, HI, seed=20 + k) for k in range(2)]
    frames = [_dev_frames(x, cuda_device) for x in xs]
    accs = [Acc(n, nbins, cuda_device) for _ in range(2)]
    streams = [torch.cuda.Stream(device=cuda_device) for _ in range(2)]
    torch.cuda.synchronize()
    for _ in range(2):
        for k in range(2):
            with torch.cuda.stream(streams[k]):
                pixel_hist(frames[k], LO, HI, nbins, accs[k].hist, stream=streams[k])
    for k in range(2):
        _same(accs[k].host(), 2 * reference.pixel_hist_reference(xs[k], LO, HI, nbins))


@pytest.mark.parametrize("nbins", [37, 256])
def test_repeat_and_split_equal_the_golden_model_of_the_whole(native, cuda_device, nbins):
    """The same launch twice equals the golden model of the doubled batch; 67 frames go as 64 + 3 inside the
    wrapper and as 5 + 62 by the caller."""
    n = pixel_hist_tile_pixels(nbins) + 5
    x = _frames(67, n, LO, HI, seed=nbins)
    want = reference.pixel_hist_reference(x, LO, HI, nbins)
    _same(_run(x, LO, HI, nbins, cuda_device), want)
    _same(_run(x, LO, HI, nbins, cuda_device, split=[5, 62]), want)
    twice = torch.cat([x[:30], x[:30]])
    _same(_run(twice, LO, HI, nbins, cuda_device, split=[30, 30]), reference.pixel_hist_reference(twice, LO, HI, nbins))


@pytest.mark.parametrize("layout", [1, 2])
@pytest.mark.parametrize("nbins", [5, 64, 1024])
def test_measurement_layouts_compute_the_same(native, cuda_device, layout, nbins):
    n = pixel_hist_tile_pixels(nbins) + 6
    x = _frames(64, n, LO, HI, seed=layout)
    _same(_run(x, LO, HI, nbins, cuda_device, layout=layout), reference.pixel_hist_reference(x, LO, HI, nbins))


def test_tiny_epix_frames(native, cuda_device):
    """A detector's frame (3-D tensors, 3072 pixels = three tiles) at the default parameters."""
    from psana_ray_amd.models import get_detector

    shape = get_detector("tiny_epix").frame_shape
    n = int(np.prod(shape))
    x = _frames(11, n, LO, HI, seed=1)
    frames = [x[f].reshape(shape).clone().to(cuda_device) for f in range(11)]
    acc = Acc(n, reference.HIST_BINS, cuda_device)
    pixel_hist(frames, reference.HIST_LO, reference.HIST_HI, reference.HIST_BINS, acc.hist)
    _same(acc.host(), reference.pixel_hist_reference(x, LO, HI, 64))


def test_every_refusal_comes_before_any_launch(native, cuda_device):
    dev = cuda_device
    n, nbins = 20, 8
    x = _frames(3, n, LO, HI, seed=2)
    frames = _dev_frames(x, dev)
    pre = torch.full((n, nbins), 7, dtype=torch.int32)
    acc = Acc(n, nbins, dev, pre)
    ok = dict(lo=LO, hi=HI, nbins=nbins, hist=acc.hist)

    def refused(frames=frames, **kw):
        with pytest.raises(ValueError):
            pixel_hist(frames, **{**ok, **kw})

    for kw in (dict(lo=1.0, hi=1.0), dict(lo=2.0, hi=1.0), dict(hi=float("inf")), dict(lo=float("nan")),
               dict(lo=0.0, hi=1e-45), dict(nbins=0), dict(nbins=1025), dict(nbins=8.0), dict(nbins=4),
               dict(frames_so_far=2 ** 31 - 3), dict(frames_so_far=-1), dict(_layout=3)):
        refused(**kw)
    big = torch.zeros(n * nbins + 4, dtype=torch.int32, device=dev)
    for hist in (acc.hist.to(torch.int64), acc.hist.cpu(), acc.hist.t(), acc.hist.reshape(-1), big[1:n * nbins + 1].view(n, nbins),
                 torch.zeros((n + 1, nbins), dtype=torch.int32, device=dev), None):
        refused(hist=hist)
    refused(frames=[f.cpu() for f in frames])
    refused(frames=[f.to(torch.float64) for f in frames])
    refused(frames=[frames[0], frames[1][:-1]])
    refused(frames=[frames[0], torch.zeros(2 * n, device=dev)[::2]])
    refused(frames=[frames[0], torch.zeros(n + 1, device=dev)[1:]])            # 4-B aligned only
    refused(frames=[x[0].numpy()])
    if torch.cuda.device_count() > 1:
        refused(frames=[f.to("cuda:1") for f in frames])
    pixel_hist([], **ok)                                                       # no frames: nothing to do
    # the launcher takes the scale itself: zero, negative, infinite and NaN are refused there
    C = _ext.load()
    for inv_w in (0.0, -0.5, float("inf"), float("nan")):
        with pytest.raises(RuntimeError, match="scale"):
            C.pixel_hist([int(f.data_ptr()) for f in frames], n, LO, HI, inv_w, nbins, int(acc.hist.data_ptr()),
                         _ext.stream_handle(None), 0)
    with pytest.raises(RuntimeError, match="2\\^31"):
        C.pixel_hist([int(f.data_ptr()) for f in frames], 2 ** 28, LO, HI, 0.5, nbins, int(acc.hist.data_ptr()),
                     _ext.stream_handle(None), 0)
    assert torch.equal(acc.host(), pre), "a refused call wrote the accumulator"
    # and the accepted call still works on the same accumulator
    pixel_hist(frames, **ok)
    _same(acc.host(), pre + reference.pixel_hist_reference(x, LO, HI, nbins))
    assert kernels.pixel_hist is pixel_hist
