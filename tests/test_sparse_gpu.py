"""K-10 zero-suppression kernels (csrc/sparse.hip) against the golden model, word for word, on the
smallest shapes where each hazard exists.  Every run pre-fills the outputs and the scratch with 0xFF
bytes and puts guard words behind pix / val / scratch."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd.models import get_detector, make_geometry
from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

C = kernels.SPARSE_CHUNK
GUARD = 64           # extra words behind pix / val
SCRATCH_GUARD = 256  # extra bytes behind the scratch block
THR, VMAX = 10.0, 1000.0


def _outputs(F, cap, dev):
    """nnz, flags, offs, pix, val -- all 0xFF bytes, pix / val with GUARD words behind F * cap."""
    nnz = torch.full((F,), -1, dtype=torch.int32, device=dev)
    flags = torch.full((F,), 0xFF, dtype=torch.uint8, device=dev)
    offs = torch.full((F + 1,), -1, dtype=torch.int64, device=dev)
    pix = torch.full((F * cap + GUARD,), -1, dtype=torch.int32, device=dev)
    val = torch.full((F * cap + GUARD,), -1, dtype=torch.int32, device=dev).view(torch.float32)
    return nnz, flags, offs, pix, val


def _scratch(n, cap, F, dev):
    return torch.full((kernels.sparsify_scratch_bytes(n, cap, F) + SCRATCH_GUARD,), 0xFF, dtype=torch.uint8, device=dev)


def _launch(frames_dev, thr, vmax, cap, dev, mask=None, keys=None, key_min=0, scratch=None, stream=None):
    F, n = len(frames_dev), frames_dev[0].numel()
    out = _outputs(F, cap, dev)
    if scratch is None:
        scratch = _scratch(n, cap, F, dev)
    kernels.sparsify(frames_dev, thr, vmax, cap, *out, mask=mask, keys=keys, key_min=key_min, scratch=scratch,
                     stream=stream)
    return out, scratch


def _collect(out, scratch, F, n, cap):
    """Host copies (after a synchronize), with the guard checks."""
    nnz, flags, offs, pix, val = (t.cpu() for t in out)
    assert bool((pix[F * cap:] == -1).all()), "guard words behind pix were written"
    assert bool((val.view(torch.int32)[F * cap:] == -1).all()), "guard words behind val were written"
    need = kernels.sparsify_scratch_bytes(n, cap, F)
    assert bool((scratch[need:].cpu() == 0xFF).all()), "guard bytes behind the scratch block were written"
    total = int(offs[F])
    assert 0 <= total <= F * cap
    return nnz, flags, offs, pix[:total], val[:total]


def _same(got, want):
    for g, w, name in zip(got, want, ("nnz", "flags", "offs", "pix")):
        assert g.dtype == w.dtype and torch.equal(g, w), f"{name} differs"
    assert torch.equal(got[4].view(torch.int32), want[4].view(torch.int32)), "val words differ"


def _dev_frames(x, dev):
    """One allocation per frame: ring slots are not contiguous (and rows of an odd n are not 16-B aligned)."""
    return [x[i].to(dev).clone() for i in range(x.shape[0])]


def _check(x, thr, vmax, cap, dev, mask=None, keys=None, key_min=0, scratch=None):
    F, n = x.shape
    want = reference.sparsify_reference(x, thr, vmax, cap, mask=mask, keys=keys, key_min=key_min)
    out, scratch = _launch(_dev_frames(x, dev), thr, vmax, cap, dev, mask=None if mask is None else mask.to(dev),
                           keys=None if keys is None else keys.to(dev), key_min=key_min, scratch=scratch)
    torch.cuda.synchronize()
    got = _collect(out, scratch, F, n, cap)
    _same(got, want)
    return want


def _frames(F, n, seed, where="random", density=0.01):
    """Values below THR everywhere except the chosen pixels, which lie inside [THR, VMAX]."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5.0, 5.0, size=(F, n)).astype(np.float32)
    hot = np.zeros((F, n), bool)
    if where == "random":
        hot = rng.random((F, n)) < density
    elif where == "all":
        hot[:] = True
    elif where == "last_chunk":
        first = (max(1, -(-(n // 4) // (C // 4))) - 1) * C   # first element of the frame's last chunk
        hot[:, first:] = rng.random((F, n - first)) < 0.5
    elif where == "tail":
        hot[:, 4 * (n // 4):] = True
    elif where != "none":
        raise ValueError(where)
    x[hot] = rng.uniform(THR, VMAX, size=int(hot.sum())).astype(np.float32)
    return torch.from_numpy(x), hot


SIZES = [1, 3, 4, C - 1, C, C + 1, 3 * C + 5, 3072]   # 3072: the tiny_epix calib frame


def test_tiny_epix_is_a_listed_size():
    assert get_detector("tiny_epix").npix == 3072


@pytest.mark.parametrize("F", [1, 3, 64])
@pytest.mark.parametrize("n", SIZES)
def test_shapes_and_densities(native, cuda_device, n, F):
    for k, where in enumerate(("none", "all", "random", "last_chunk", "tail")):
        x, hot = _frames(F, n, 100 * n + 10 * F + k, where)
        cap = n if where == "all" else max(1, n // 2)
        want = _check(x, THR, VMAX, cap, cuda_device)
        assert np.array_equal(want[0].numpy(), hot.sum(1)), where   # the case is what it says
        if where == "all":
            assert int(want[2][F]) == F * n and not bool(want[1].any())


def test_special_values(native, cuda_device):
    """NaN, +-inf, -0.0, and values on and next to both window edges."""
    n = C + 7
    thr, vmax = np.float32(0.0), np.float32(50.0)
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, thr, vmax, np.nextafter(vmax, np.float32(np.inf)),
                   np.nextafter(thr, np.float32(-np.inf)), 49.999996, -1.0e-45, 1.0e-45, 3.0e38, -3.0e38], np.float32)
    rng = np.random.default_rng(7)
    x = rng.uniform(-100.0, -1.0, size=(3, n)).astype(np.float32)
    for f in range(3):
        pos = rng.choice(n, size=4 * sp.size, replace=False)
        x[f, pos] = np.tile(sp, 4)
        x[f, n - 1 - f] = -0.0          # one in the scalar tail region
    xt = torch.from_numpy(x)
    want = _check(xt, float(thr), float(vmax), n, cuda_device)
    kept = want[4].view(torch.int32)
    assert bool((kept == np.int32(-2 ** 31)).any()), "-0.0 must be kept with its sign bit when thr <= 0"
    assert not bool(torch.isnan(want[4]).any()) and not bool(torch.isinf(want[4]).any())
    assert bool((want[4] == float(vmax)).any()) and bool((kept == 0).any())
    # thr > 0: neither zero is kept
    thr2 = float(np.float32(1.0e-45))
    want2 = _check(xt, thr2, float(vmax), n, cuda_device)
    assert not bool((want2[4] == 0.0).any()) and bool((want2[4] == thr2).any())


def test_capacity_edge_and_overflow_neighbour(native, cuda_device):
    """nnz == cap is stored; nnz == cap + 1 stores nothing, reports its exact nnz, and the frames
    after it are packed contiguously."""
    F, n, cap = 6, 3 * C + 5, 300
    rng = np.random.default_rng(17)
    x = rng.uniform(-5.0, 5.0, size=(F, n)).astype(np.float32)
    for f, k in enumerate([120, cap, cap, 37, 5 * cap, 0]):
        x[f, rng.choice(n - 8, size=k, replace=False)] = 100.0 + f
    x[0, n - 1] = x[2, n - 2] = 77.0   # pixels of the n % 4 tail count too: frame 2 has cap + 1
    xt = torch.from_numpy(x)
    want = _check(xt, THR, VMAX, cap, cuda_device)
    nnz, flags, offs = want[0].numpy(), want[1].numpy(), want[2].numpy()
    assert nnz.tolist() == [121, cap, cap + 1, 37, 5 * cap, 0]
    assert flags.tolist() == [0, 0, 1, 0, 1, 0]
    assert offs.tolist() == [0, 121, 121 + cap, 121 + cap, 158 + cap, 158 + cap, 158 + cap]


def test_dense_batch_every_chunk_full(native, cuda_device):
    """Everything kept at cap = n over 64 frames: every chunk's compaction is full, the staging rows
    and pix / val are written to their last element (guards checked in _check)."""
    F, n = 64, 2 * C + 3
    x, _ = _frames(F, n, 23, "all")
    want = _check(x, THR, VMAX, n, cuda_device)
    assert int(want[2][F]) == F * n
    assert torch.equal(want[3].view(F, n), torch.arange(n, dtype=torch.int32).expand(F, n))


def test_scratch_reused_without_clearing(native, cuda_device):
    """The same 0xFF-filled scratch block serves a second, different batch: the launch clears what it needs."""
    n, cap = 3 * C + 5, 2000
    scratch = _scratch(n, cap, 64, cuda_device)
    x1, _ = _frames(64, n, 31, "random", 0.05)
    _check(x1, THR, VMAX, cap, cuda_device, scratch=scratch)
    x2, _ = _frames(5, n, 32, "random", 0.001)      # fewer frames: another directory layout
    _check(x2, THR, VMAX, cap, cuda_device, scratch=scratch[:kernels.sparsify_scratch_bytes(n, cap, 5) + SCRATCH_GUARD])
    x3, _ = _frames(64, n, 33, "last_chunk")
    _check(x3, THR, VMAX, cap, cuda_device, scratch=scratch)


@pytest.mark.parametrize("n", [3, C + 1, 3 * C + 5])
def test_mask(native, cuda_device, n):
    rng = np.random.default_rng(41 + n)
    x, hot = _frames(3, n, 42 + n, "random", 0.3)
    mask = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8))
    want = _check(x, THR, VMAX, n, cuda_device, mask=mask)
    assert np.array_equal(want[0].numpy(), (hot & (mask.numpy() != 0)).sum(1))
    all_off = torch.zeros(n, dtype=torch.uint8)
    assert int(_check(x, THR, VMAX, n, cuda_device, mask=all_off)[2][3]) == 0


def test_keys_alternating_at_64_frames(native, cuda_device):
    F, n = 64, 3 * C + 5
    x, hot = _frames(F, n, 51, "random", 0.02)
    keys = torch.tensor([7 if f % 2 == 0 else 6 for f in range(F)], dtype=torch.int32)
    want = _check(x, THR, VMAX, n // 8, cuda_device, keys=keys, key_min=7)
    nnz, flags = want[0].numpy(), want[1].numpy()
    assert np.array_equal(flags, np.where(np.arange(F) % 2 == 0, 0, 2).astype(np.uint8))
    assert np.array_equal(nnz, np.where(np.arange(F) % 2 == 0, hot.sum(1), 0))
    # every frame on the edge: keys[f] == key_min is processed; all skipped: nothing stored
    _check(x, THR, VMAX, n // 8, cuda_device, keys=keys, key_min=6)
    assert int(_check(x, THR, VMAX, n // 8, cuda_device, keys=keys, key_min=8)[2][F]) == 0
    # a skipped frame is not even read for overflow: negative keys, masks and keys together
    mask = torch.from_numpy((np.random.default_rng(52).random(n) < 0.7).astype(np.uint8))
    _check(x, THR, VMAX, 100, cuda_device, mask=mask, keys=-keys, key_min=-6)


def test_repeatable_and_two_streams_in_flight(native, cuda_device):
    dev = cuda_device
    F, n, cap = 64, 3 * C + 5, 1500
    xa, _ = _frames(F, n, 61, "random", 0.05)
    xb, _ = _frames(F, n, 62, "random", 0.08)
    wa = reference.sparsify_reference(xa, THR, VMAX, cap)
    wb = reference.sparsify_reference(xb, THR, VMAX, cap)
    fa, fb = _dev_frames(xa, dev), _dev_frames(xb, dev)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(dev), torch.cuda.Stream(dev)
    runs = []
    for fr, st in ((fa, s1), (fb, s2), (fa, s2), (fb, s1)):   # separate outputs and scratch per launch
        with torch.cuda.stream(st):
            runs.append(_launch(fr, THR, VMAX, cap, dev, stream=st))
    torch.cuda.synchronize()
    got = [_collect(o, s, F, n, cap) for o, s in runs]
    _same(got[0], wa)
    _same(got[1], wb)
    _same(got[2], got[0])
    _same(got[3], got[1])


@functools.lru_cache(maxsize=None)
def _epix_calibrated(dev_str):
    """64 epix10k2M calib frames: the synthetic source through the calibrator (on the GPU), and their
    host copy for the golden model."""
    from psana_ray_amd.models import Calibrator, Mode
    from psana_ray_amd.source import SyntheticRun

    dev = torch.device(dev_str)
    src = SyntheticRun("synthetic", 0, "epix10k2M", pool_frames=16, seed=3)
    pool = torch.from_numpy(src.pool.view(np.int16)).view(torch.uint16)
    raw = [pool[i % pool.shape[0]].to(dev).clone() for i in range(64)]
    out = [torch.empty(src.spec.frame_shape, dtype=torch.float32, device=dev) for _ in range(64)]
    Calibrator(src.consts, dev, Mode.calib).run(raw, out)
    torch.cuda.synchronize()
    return out, torch.stack([t.cpu() for t in out]).reshape(64, -1)


def test_production_shape_default_parameters(native, cuda_device):
    """64 epix10k2M calib frames at the CLI's defaults: thr 20, vmax 2^20, cap n // 16."""
    frames, host = _epix_calibrated(str(cuda_device))
    n = host.shape[1]
    cap = n // 16
    want = reference.sparsify_reference(host, 20.0, 2.0 ** 20, cap)
    out, scratch = _launch(frames, 20.0, 2.0 ** 20, cap, cuda_device)
    torch.cuda.synchronize()
    _same(_collect(out, scratch, 64, n, cap), want)
    assert int(want[0].sum()) > 0


def test_image_layout_batch(native, cuda_device):
    spec = get_detector("epix10k2M")
    geo = make_geometry(spec)
    _, host = _epix_calibrated(str(cuda_device))
    img = reference.assemble_reference(host[:3].reshape(3, *spec.frame_shape), geo.rows, geo.cols, geo.image_shape)
    x = img.reshape(3, -1).contiguous()
    n = x.shape[1]
    want = _check(x, 20.0, 2.0 ** 20, n // 16, cuda_device)
    assert int(want[0].sum()) > 0


def test_validation_raises_before_any_launch(native, cuda_device):
    dev = cuda_device
    n, cap = 64, 8
    good = [torch.full((n,), 100.0, dtype=torch.float32, device=dev) for _ in range(2)]

    def call(frames=good, thr=THR, vmax=VMAX, cap=cap, F_out=None, **kw):
        F = len(frames) if F_out is None else F_out
        c = cap if isinstance(cap, int) and 1 <= cap <= 1024 else 8
        nnz, flags, offs, pix, val = _outputs(max(1, min(F, 64)), c, dev)
        args = {"nnz": nnz, "flags": flags, "offs": offs, "pix": pix, "val": val}
        args.update(kw)
        with pytest.raises(ValueError):
            kernels.sparsify(frames, thr, vmax, cap, args.pop("nnz"), args.pop("flags"), args.pop("offs"),
                             args.pop("pix"), args.pop("val"), **args)
        torch.cuda.synchronize()
        # the sentinel: a launch would have written nnz / flags / offs
        assert bool((nnz == -1).all()) and bool((flags == 0xFF).all()) and bool((offs == -1).all())
        assert bool((pix == -1).all()) and bool((val.view(torch.int32) == -1).all())

    call(frames=[t.to(torch.float64) for t in good])                                  # dtype
    call(frames=[t.cpu() for t in good])                                              # device
    call(frames=[good[0], torch.zeros(n + 4, dtype=torch.float32, device=dev)])       # element count
    call(frames=[torch.zeros(n + 1, dtype=torch.float32, device=dev)[1:]])            # 16-B alignment
    call(frames=[])                                                                   # F = 0
    call(frames=[good[0]] * 65)                                                       # F = 65
    call(cap=0)
    call(cap=2 ** 30)                                                                 # F * cap >= 2^31
    call(cap=1.5)
    call(thr=float("nan"))
    call(vmax=float("inf"))
    call(thr=-float("inf"))
    call(thr=3.0e39)                                                                  # not finite as float32
    call(thr=5.0, vmax=4.0)                                                           # empty window
    call(nnz=torch.zeros(2, dtype=torch.int64, device=dev))
    call(nnz=torch.zeros(3, dtype=torch.int32, device=dev))
    call(flags=torch.zeros(2, dtype=torch.int8, device=dev))
    call(offs=torch.zeros(2, dtype=torch.int64, device=dev))                          # needs F + 1
    call(offs=torch.zeros(3, dtype=torch.int32, device=dev))
    call(pix=torch.zeros(2 * cap - 1, dtype=torch.int32, device=dev))
    call(val=torch.zeros(2 * cap, dtype=torch.int32, device=dev))
    call(pix=torch.zeros(2 * cap, dtype=torch.int32))                                 # on the host
    call(mask=torch.ones(n, dtype=torch.bool, device=dev))
    call(mask=torch.ones(n - 1, dtype=torch.uint8, device=dev))
    call(keys=torch.zeros(2, dtype=torch.int64, device=dev))
    call(keys=torch.zeros(3, dtype=torch.int32, device=dev))
    call(keys=torch.zeros(2, dtype=torch.int32))
    call(scratch=torch.zeros(kernels.sparsify_scratch_bytes(n, cap, 2) - 1, dtype=torch.uint8, device=dev))
    call(scratch=torch.zeros(kernels.sparsify_scratch_bytes(n, cap, 2) + 16, dtype=torch.uint8, device=dev)[1:])
    # and the same arguments, valid, do launch
    out, scratch = _launch(good, THR, VMAX, cap, dev)
    torch.cuda.synchronize()
    nnz, flags, offs, pix, val = _collect(out, scratch, 2, n, cap)
    assert nnz.tolist() == [n, n] and flags.tolist() == [1, 1] and offs.tolist() == [0, 0, 0]


def test_exported_sizes_agree(native):
    assert native.SPARSE_CHUNK == kernels.SPARSE_CHUNK
    for n, cap, F in ((1, 1, 1), (3072, 192, 64), (C + 1, 7, 3), (2162688, 135168, 64), (2 ** 31 - 1, 33554431, 63)):
        assert native.sparsify_scratch_bytes(n, cap, F) == kernels.sparsify_scratch_bytes(n, cap, F)
