"""K-09 dark-statistics kernel (csrc/dark.hip) against the integer golden model, word for word, on the
smallest shapes where each hazard exists."""
import numpy as np
import pytest
import torch

from psana_ray_amd.models import get_detector
from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

NC = {0: 2, 1: 3, 2: 1}


def _u16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.uint16).to(dev)


def _host_u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.uint16)


def _zeros(kind, n, dev):
    return (torch.zeros((NC[kind], n), dtype=torch.int32, device=dev),
            torch.zeros((NC[kind], n), dtype=torch.int64, device=dev),
            torch.zeros((NC[kind], n), dtype=torch.int64, device=dev))


def _accumulate(x_np, kind, lo, hi, dev, acc=None, separate=False):
    """x_np: uint16 [F, n].  Frames are rows of one device tensor (16-B aligned for these n) or, with
    ``separate``, F allocations of their own.  Returns the accumulators on the host."""
    F, n = x_np.shape
    if separate:
        frames = [_u16(x_np[f], dev) for f in range(F)]
    else:
        assert (2 * n) % 16 == 0 or F == 1
        xd = _u16(x_np, dev)
        frames = [xd[f] for f in range(F)]
    acc = _zeros(kind, n, dev) if acc is None else acc
    kernels.dark_accumulate(frames, kind, lo, hi, *acc)
    torch.cuda.synchronize()
    return tuple(t.cpu() for t in acc)


def _same(got, want):
    for g, w, name in zip(got, want, ("cnt", "sum", "sq")):
        assert g.dtype == w.dtype
        assert torch.equal(g, w), f"{name} differs at {(g != w).nonzero()[:4].tolist()}"


def _raw(kind, shape, seed):
    """Raw words with every gain-bit pattern, ADUs spread over the range and its two ends."""
    rng = np.random.default_rng(seed)
    if kind == 2:
        x = rng.integers(0, 65536, size=shape, dtype=np.int64)
        x.reshape(-1)[::7] = 65535
        x.reshape(-1)[3::11] = 0
    else:
        adu = rng.integers(0, 16384, size=shape, dtype=np.int64)
        adu.reshape(-1)[::13] = 16383
        top = rng.integers(0, 4, size=shape, dtype=np.int64)     # epix: bit 15 set in half of them
        x = adu | (top << 14)
    return x.astype(np.uint16)


def test_plain_1027_tail_and_partial_workgroup(native, cuda_device):
    """n = 1027: two 1024-pixel workgroups, the second partial, and the n % 4 = 3 scalar tail; 65535
    samples give sq its largest per-sample add.  Frames of 2054 B are separate allocations."""
    x = _raw(2, (9, 1027), 1)
    x[:, 1024:] = 65535                     # the tail pixels at the maximum in every frame
    x[4, 1026] = 17
    want = reference.dark_accumulate_reference(_host_u16(x), 2, 0, 65535)
    assert int(want[2].max()) >= 8 * 65535 ** 2
    _same(_accumulate(x, 2, 0, 65535, cuda_device, separate=True), want)
    want = reference.dark_accumulate_reference(_host_u16(x), 2, 1, 65534)
    _same(_accumulate(x, 2, 1, 65534, cuda_device, separate=True), want)


@pytest.mark.parametrize("kind,n", [(0, 1027), (1, 1026), (1, 5), (0, 3)])
def test_unaligned_candidate_planes(native, cuda_device, kind, n):
    """n % 4 != 0 with NC > 1: the planes of candidates >= 1 start at c * n, not 16-B aligned."""
    x = _raw(kind, (5, n), 2 + n)
    want = reference.dark_accumulate_reference(_host_u16(x), kind, 100, 16000)
    _same(_accumulate(x, kind, 100, 16000, cuda_device, separate=True), want)


@pytest.mark.parametrize("F", [1, 3, 8, 9, 64])
def test_tiny_epix_unroll_remainders(native, cuda_device, F):
    spec = get_detector("tiny_epix")
    x = _raw(0, (F, spec.npix), 10 + F)
    want = reference.dark_accumulate_reference(_host_u16(x), 0, 5, 16380)
    _same(_accumulate(x, 0, 5, 16380, cuda_device), want)


def test_tiny_epix_67_frames_two_launches(native, cuda_device):
    spec = get_detector("tiny_epix")
    x = _raw(0, (67, spec.npix), 3)
    want = reference.dark_accumulate_reference(_host_u16(x), 0, 0, 65535)
    _same(_accumulate(x, 0, 0, 65535, cuda_device, separate=True), want)


def test_tiny_jungfrau_all_gain_bits_in_every_lane_group(native, cuda_device):
    """Pixel p of frame f carries gain bits (p + f) % 4: every lane's four pixels see all four
    patterns, gb == 2 (invalid) included, in every frame."""
    spec = get_detector("tiny_jungfrau")
    F, n = 6, spec.npix
    rng = np.random.default_rng(4)
    adu = rng.integers(0, 16384, size=(F, n), dtype=np.int64)
    gb = (np.arange(n)[None, :] + np.arange(F)[:, None]) % 4
    x = (adu | (gb << 14)).astype(np.uint16)
    want = reference.dark_accumulate_reference(_host_u16(x), 1, 0, 16383)
    assert int(want[0].sum()) == F * n - int((gb == 2).sum())
    _same(_accumulate(x, 1, 0, 16383, cuda_device), want)


def test_preloaded_accumulators_carry_and_order(native, cuda_device):
    """sum = 2^32 - 5, sq = 2^40 - 3, cnt = 2^20 preloaded: the add carries across the 32-bit
    boundary.  The same call twice accumulates; a permuted frame order gives the same words."""
    spec = get_detector("tiny_epix")
    dev = cuda_device
    F, n = 11, spec.npix
    x = _raw(0, (F, n), 5)
    c, s, q = reference.dark_accumulate_reference(_host_u16(x), 0, 0, 16383)

    def pre():
        return (torch.full((2, n), 2 ** 20, dtype=torch.int32, device=dev),
                torch.full((2, n), 2 ** 32 - 5, dtype=torch.int64, device=dev),
                torch.full((2, n), 2 ** 40 - 3, dtype=torch.int64, device=dev))

    acc = pre()
    _same(_accumulate(x, 0, 0, 16383, dev, acc=acc), (c + 2 ** 20, s + (2 ** 32 - 5), q + (2 ** 40 - 3)))
    assert bool((s > 5).any()) and bool((acc[1].cpu() >= 2 ** 32).any())
    _same(_accumulate(x, 0, 0, 16383, dev, acc=acc), (2 * c + 2 ** 20, 2 * s + (2 ** 32 - 5), 2 * q + (2 ** 40 - 3)))
    perm = np.random.default_rng(6).permutation(F)
    _same(_accumulate(x[perm], 0, 0, 16383, dev, acc=pre()), (c + 2 ** 20, s + (2 ** 32 - 5), q + (2 ** 40 - 3)))


def test_untouched_candidate_is_left_exactly_as_it_was(native, cuda_device):
    """Frames that never hit candidate 1 (bit 14 clear everywhere): its preloaded pattern is unchanged --
    the skipped read-modify-write."""
    spec = get_detector("tiny_epix")
    dev = cuda_device
    n = spec.npix
    x = (_raw(0, (9, n), 7) & 0xBFFF).astype(np.uint16)      # bit 15 stays set in places
    pat = torch.arange(n, dtype=torch.int64)
    acc = _zeros(0, n, dev)
    acc[0][1] = (pat % 1000 - 500).to(torch.int32).to(dev)
    acc[1][1] = (pat * 0x0123456789 - 2 ** 45).to(dev)
    acc[2][1] = (-(pat * 0x1F3D5B79) - 1).to(dev)
    before = tuple(t[1].cpu().clone() for t in acc)
    got = _accumulate(x, 0, 0, 16383, dev, acc=acc)
    want = reference.dark_accumulate_reference(_host_u16(x), 0, 0, 16383)
    assert int(want[0][1].sum()) == 0
    for g, w, b in zip(got, want, before):
        assert torch.equal(g[0], w[0])
        assert torch.equal(g[1], b)


def test_epix10k2m_production_shape(native, cuda_device):
    """7 frames of epix10k2M: 2112 workgroups."""
    spec = get_detector("epix10k2M")
    assert spec.npix // 1024 == 2112
    rng = np.random.default_rng(8)
    x = (rng.integers(2000, 3200, size=(7, spec.npix), dtype=np.int64)
         | (rng.integers(0, 64, size=(7, spec.npix), dtype=np.int64) == 0).astype(np.int64) << 14).astype(np.uint16)
    want = reference.dark_accumulate_reference(_host_u16(x), 0, 0, 16383)
    _same(_accumulate(x, 0, 0, 16383, cuda_device), want)


def test_jungfrau05m_production_panel(native, cuda_device):
    spec = get_detector("jungfrau05M")
    x = _raw(1, (3, spec.npix), 9)
    want = reference.dark_accumulate_reference(_host_u16(x), 1, 10, 16000)
    _same(_accumulate(x, 1, 10, 16000, cuda_device), want)


def test_consumer_over_alternating_streams(native, cuda_device):
    """Three batches through DarkStatsConsumer (its streams alternate, one accumulator set each) ==
    the golden sum over all frames."""
    from psana_ray_amd.pipeline import DarkStatsConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    spec = get_detector("tiny_epix")
    x = _raw(0, (15, spec.npix), 12)
    ring = FrameRing(spec.frame_shape, torch.uint16, cuda_device, 16, 16)
    ep = QueueEndpoint(ring)
    cons = DarkStatsConsumer(ep, spec, adu_lo=3, adu_hi=16000, batch=5)
    assert len(cons._acc) == len(cons.streams) >= 2
    xt = _host_u16(x).reshape(15, *spec.frame_shape)
    for k in range(3):
        slots = [ep.acquire(timeout=5.0) for _ in range(5)]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(xt[5 * k + j])
            ep.commit(s, 0, 5 * k + j, 5 * k + j, None)
        assert cons.poll(timeout=5.0) == 5
    cnt, s, q, frames = cons.synchronize()
    want = reference.dark_accumulate_reference(_host_u16(x), 0, 3, 16000)
    assert frames == 15 and cnt.dtype == np.int64 and s.dtype == np.int64 and q.dtype == np.int64
    assert np.array_equal(cnt, want[0].to(torch.int64).numpy())
    assert np.array_equal(s, want[1].numpy())
    assert np.array_equal(q, want[2].numpy())
    # process_frames (frames that are not queue items) lands in the same run
    extra = [_u16(x[i], cuda_device) for i in range(4)]
    cons.process_frames(extra)
    cnt2, s2, _q2, frames2 = cons.synchronize()
    w4 = reference.dark_accumulate_reference(_host_u16(x[:4]), 0, 3, 16000)
    assert frames2 == 19 and np.array_equal(s2, (want[1] + w4[1]).numpy())
    assert np.array_equal(cnt2, (want[0].to(torch.int64) + w4[0]).numpy())
    ep.close()


def test_consumer_refuses_other_rings(native, cuda_device):
    from psana_ray_amd.pipeline import DarkStatsConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    spec = get_detector("tiny_epix")
    ep = QueueEndpoint(FrameRing(spec.frame_shape, torch.float32, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="uint16"):
        DarkStatsConsumer(ep, spec)
    ep.close()
    ep = QueueEndpoint(FrameRing(get_detector("tiny_jungfrau").frame_shape, torch.uint16, cuda_device, 4, 4))
    with pytest.raises(ValueError, match="pixels"):
        DarkStatsConsumer(ep, spec)
    ep.close()


def test_validation_raises_before_any_launch(native, cuda_device):
    dev = cuda_device
    n = 64
    MARK = 0x5A5A
    frames = [torch.zeros(n, dtype=torch.uint16, device=dev)]

    def acc(nc=1, cdt=torch.int32, sdt=torch.int64, nn=n):
        return (torch.full((nc, nn), MARK, dtype=cdt, device=dev), torch.full((nc, nn), MARK, dtype=sdt, device=dev),
                torch.full((nc, n), MARK, dtype=torch.int64, device=dev))

    good = acc()
    big = torch.zeros(n + 8, dtype=torch.uint16, device=dev)
    cases = [
        dict(frames=[torch.zeros(n, dtype=torch.float32, device=dev)]),          # float frames
        dict(frames=[big[1:n + 1]]),                                              # misaligned frame
        dict(frames=[frames[0], torch.zeros(n + 4, dtype=torch.uint16, device=dev)]),   # unequal numel
        dict(acc=acc(cdt=torch.int64)),                                           # wrong accumulator dtype
        dict(acc=acc(sdt=torch.int32)),
        dict(acc=acc(nc=2)),                                                      # wrong shape (plain has 1 candidate)
        dict(acc=acc(nn=n + 4)),
        dict(lo=9, hi=8),                                                         # lo > hi
        dict(hi=65536),                                                           # hi > 65535
        dict(lo=-1),
        dict(kind=3),
        dict(frames_so_far=2 ** 31 - 1),                                          # the run is full
    ]
    for case in cases:
        a = case.get("acc", good)
        with pytest.raises(ValueError):
            kernels.dark_accumulate(case.get("frames", frames), case.get("kind", 2), case.get("lo", 0),
                                    case.get("hi", 65535), *a, frames_so_far=case.get("frames_so_far", 0))
        torch.cuda.synchronize()
        for t in (*a, *good):
            assert bool((t == MARK).all()), case
    # one below the bound still runs
    kernels.dark_accumulate(frames, 2, 0, 65535, *good, frames_so_far=2 ** 31 - 2)
    torch.cuda.synchronize()
    assert bool((good[0] == MARK + 1).all())
