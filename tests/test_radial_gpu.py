"""K-08 radial profile kernel (csrc/radial.hip) against the integer golden model, bitwise, on the
smallest shapes where each hazard exists."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd.models import RadialBinning, get_detector, make_geometry
from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

S = 8
VMIN, VMAX = -float(2 ** 20), float(2 ** 20)


def _u16(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.uint16).to(dev)


def _run(frames, bins_np, nbins, dev, vmin=VMIN, vmax=VMAX, run=None):
    """frames: list of device tensors.  Returns (sums, counts, profile) on the host."""
    F = len(frames)
    bins = _u16(bins_np, dev)
    sums = torch.full((F, nbins), -7, dtype=torch.int64, device=dev)       # stale contents must be overwritten
    counts = torch.full((F, nbins), -7, dtype=torch.int32, device=dev)
    prof = torch.full((F, nbins), float("nan"), dtype=torch.float32, device=dev)
    kernels.radial_profile(frames, bins, nbins, sums, counts, prof, vmin, vmax, S, run=run)
    torch.cuda.synchronize()
    return sums.cpu(), counts.cpu(), prof.cpu()


def _same(got, want):
    assert torch.equal(got[0], want[0]), "sums differ"
    assert torch.equal(got[1], want[1]), "counts differ"
    assert torch.equal(got[2].view(torch.int32), want[2].view(torch.int32)), "profile words differ"


def _spiky(shape, seed):
    """Detector-like values seeded with every special case of the contract."""
    rng = np.random.default_rng(seed)
    x = rng.normal(30.0, 300.0, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    k = rng.integers(0, flat.size, size=max(8, flat.size // 50))
    special = np.array([np.nan, np.inf, -np.inf, 3.0e6, -3.0e6, (5 + 0.5) / 2 ** S, (6 + 0.5) / 2 ** S,
                        -(5 + 0.5) / 2 ** S, -1234.75, 2.0 ** 20, -2.0 ** 20], np.float32)
    flat[k] = special[np.arange(k.size) % special.size]
    return torch.from_numpy(x)


@pytest.mark.parametrize("layout", ["image", "calib"])
@pytest.mark.parametrize("nbins", [1, 7])
def test_tiny_odd_vector_tail(native, cuda_device, layout, nbins):
    """tiny_odd image frames have 153 elements (not a multiple of 4): the scalar tail path."""
    spec = get_detector("tiny_odd")
    rb = RadialBinning.from_geometry(make_geometry(spec), layout, nbins)
    assert rb.bins.size == (153 if layout == "image" else 144)
    x = _spiky((3, rb.bins.size), 11)
    want = reference.radial_profile_reference(x, rb.bins, nbins, VMIN, VMAX, S)
    assert int(want[1].sum()) > 0
    # one allocation per frame: rows of a [3, 153] tensor would not be 16-B aligned
    _same(_run([x[i].to(cuda_device) for i in range(3)], rb.bins, nbins, cuda_device), want)


@functools.lru_cache(maxsize=None)
def _tiny_epix_case():
    spec = get_detector("tiny_epix")
    rng = np.random.default_rng(21)
    bins = rng.integers(0, 64, size=spec.npix).astype(np.uint16)
    bins[rng.random(spec.npix) < 0.1] = 0xFFFF
    x = _spiky((67, spec.npix), 22)
    return bins, x, reference.radial_profile_reference(x, bins, 64, VMIN, VMAX, S)


def test_tiny_epix_67_separate_frames_two_launches(native, cuda_device):
    bins, x, want = _tiny_epix_case()
    frames = [x[i].to(cuda_device).clone() for i in range(67)]   # separately allocated: scattered pointers
    _same(_run(frames, bins, 64, cuda_device), want)


def test_repeatable_and_frame_order(native, cuda_device):
    bins, x, want = _tiny_epix_case()
    frames = [x[i].to(cuda_device) for i in range(67)]
    a = _run(frames, bins, 64, cuda_device)
    b = _run(frames, bins, 64, cuda_device)
    _same(a, b)
    perm = torch.from_numpy(np.random.default_rng(5).permutation(67))
    c = _run([frames[int(i)] for i in perm], bins, 64, cuda_device)
    _same(c, tuple(t[perm] for t in want))


@functools.lru_cache(maxsize=None)
def _epix_frames():
    spec = get_detector("epix10k2M")
    return _spiky((2, *spec.frame_shape), 31)


@pytest.mark.parametrize("nbins", [1024, 1, 4096])
def test_epix10k2m_calib_layout(native, cuda_device, nbins):
    """Many workgroups per frame; nbins 1 puts every pixel in one bin (worst contention, largest sum)."""
    spec = get_detector("epix10k2M")
    rb = RadialBinning.from_geometry(make_geometry(spec), "calib", nbins)
    x = _epix_frames()
    want = reference.radial_profile_reference(x, rb.bins, nbins, VMIN, VMAX, S)
    if nbins == 1:
        assert int(want[1][0, 0]) > spec.npix * 0.9
    _same(_run([x[0].to(cuda_device), x[1].to(cuda_device)], rb.bins, nbins, cuda_device), want)


@functools.lru_cache(maxsize=None)
def _epix_batch():
    """7 epix10k2M frames: 7 x 528 = 3696 chunks of 16 KB."""
    spec = get_detector("epix10k2M")
    return _spiky((7, *spec.frame_shape), 33)


@pytest.mark.parametrize("nbins", [1024, 4096])
def test_epix10k2m_workgroups_own_many_chunks_across_frames(native, cuda_device, nbins):
    """The regime the consumer runs in: more chunks than resident workgroups, not dividing evenly.
    The grid is min(chunks, CUs x resident workgroups per CU).  A CU holds at most 8 workgroups of
    4 waves, so at 1024 bins the grid is at most 2048 on 256 CUs (1536 at 6 per CU, what the kernel's
    registers allow); at 4096 bins the 48-KiB histogram allows 3 per CU, 768.  The 7 x 528 = 3696
    chunks then give every workgroup a contiguous range of about 2-3 (1024 bins) or 4-5 (4096 bins)
    chunks -- the double-buffered steady state, loading two chunks ahead -- and since 528 k G / 3696
    is no integer for G = 1536, 2048 or 768, ranges straddle every frame boundary: the histogram is
    merged into one frame's rows, cleared, and carried on into the next frame's.  Frames are separate
    allocations with different contents.  nbins arrives as a numpy integer, as from an array."""
    spec = get_detector("epix10k2M")
    rb = RadialBinning.from_geometry(make_geometry(spec), "calib", nbins)
    x = _epix_batch()
    want = reference.radial_profile_reference(x, rb.bins, nbins, VMIN, VMAX, S)
    frames = [x[i].to(cuda_device) for i in range(7)]
    _same(_run(frames, rb.bins, np.int64(nbins), cuda_device), want)


def test_epix10k2m_image_layout(native, cuda_device):
    spec = get_detector("epix10k2M")
    geo = make_geometry(spec)
    rb = RadialBinning.from_geometry(geo, "image", 1024)
    img = reference.assemble_reference(_epix_frames()[:1], geo.rows, geo.cols, geo.image_shape)
    want = reference.radial_profile_reference(img, rb.bins, 1024, VMIN, VMAX, S)
    _same(_run([img[0].to(cuda_device)], rb.bins, 1024, cuda_device), want)


def test_run_accumulator_over_alternating_streams(native, cuda_device):
    """Three batches through RadialProfileConsumer (its two streams alternate) == the int64 sum of
    the per-frame golden sums."""
    from psana_ray_amd.pipeline import RadialProfileConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    spec = get_detector("tiny_epix")
    rb = RadialBinning.from_geometry(make_geometry(spec), "calib", 32)
    x = _spiky((3 * 5, *spec.frame_shape), 41)
    ring = FrameRing(spec.frame_shape, torch.float32, cuda_device, 16, 16)
    ep = QueueEndpoint(ring)
    cons = RadialProfileConsumer(ep, rb, batch=5, keep_results=True)
    for k in range(3):
        slots = [ep.acquire(timeout=5.0) for _ in range(5)]
        for j, s in enumerate(slots):
            ep.slot_tensor(s).copy_(x[5 * k + j])
            ep.commit(s, 0, 5 * k + j, 5 * k + j, None)
        assert cons.poll(timeout=5.0) == 5
    run_sum, run_count, frames = cons.synchronize()
    want = reference.radial_profile_reference(x, rb.bins, 32, cons.vmin, cons.vmax, cons.frac_bits)
    assert frames == 15 and run_sum.dtype == np.int64
    assert np.array_equal(run_sum, want[0].sum(0).numpy())
    assert np.array_equal(run_count, want[1].to(torch.int64).sum(0).numpy())
    got = torch.cat([p.cpu() for p, _ in cons.results])
    assert [m[1] for _, ms in cons.results for m in ms] == list(range(15))
    assert torch.equal(got.view(torch.int32), want[2].view(torch.int32))
    ep.close()


def test_validation_raises_before_any_launch(native, cuda_device):
    dev = cuda_device
    n, nb = 64, 4
    frames = [torch.zeros(n, dtype=torch.float32, device=dev)]
    marker = 12345

    def call(frames=frames, bins=None, nbins=nb, vmin=-1.0, vmax=1.0, frac_bits=S):
        bins = _u16(np.zeros(n, np.uint16), dev) if bins is None else bins
        nbo = max(1, min(int(nbins), 4096))
        sums = torch.full((len(frames), nbo), marker, dtype=torch.int64, device=dev)
        counts = torch.full((len(frames), nbo), marker, dtype=torch.int32, device=dev)
        prof = torch.full((len(frames), nbo), float(marker), dtype=torch.float32, device=dev)
        with pytest.raises(ValueError):
            kernels.radial_profile(frames, bins, nbins, sums, counts, prof, vmin, vmax, frac_bits)
        torch.cuda.synchronize()
        assert bool((sums == marker).all()) and bool((counts == marker).all()) and bool((prof == marker).all())

    bad = np.zeros(n, np.uint16)
    bad[17] = nb                                   # a map entry >= nbins
    call(bins=_u16(bad, dev))
    call(bins=_u16(np.zeros(n - 4, np.uint16), dev))   # wrong map length
    call(nbins=0)
    call(nbins=4097)
    call(vmin=-2.0 ** 40, vmax=2.0 ** 40, frac_bits=12)   # 2^40 * 2^12 * 64 >= 2^53
    call(frames=[torch.zeros(n + 1, dtype=torch.float32, device=dev)[1:]])   # misaligned frame
