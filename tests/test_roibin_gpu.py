"""K-17 roibin kernels (csrc/roibin.hip) against the golden model, bit for bit for every output word, on the
smallest shapes where each path exists: the 16-B path at every codes-per-lane width, the scalar path with even and
odd Wb, ragged blocks, several workgroups; with junk-filled outputs and guard words behind every buffer."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import kernels, reference

from tests._roibin_oracle import make_case

pytestmark = pytest.mark.gpu

f32 = np.float32
GUARD = 64                      # guard bytes behind every buffer
GUARD_BYTE = 0x5E
JUNK_BYTE = 0xFF                # what every output holds before the call
MP = 8
# (2, 6, 8): 16-B path, even Wb at every B.  (1, 7, 10): scalar path, odd Wb and ragged blocks (even Wb at B = 1).
# (3, 9, 12): 16-B path with an odd Wb at B = 4, ragged rows.  (1, 5, 14) / (1, 5, 7): scalar path with an even Wb
# at B = 4 / B = 2.  (2, 70, 388): several workgroups.
SHAPES = [(2, 6, 8), (1, 7, 10), (3, 9, 12), (1, 5, 14), (1, 5, 7), (2, 70, 388)]
WINDOW = dict(step=0.5, vmin=-100.0, vmax=100.0)


def _dev():
    return torch.device("cuda:0")


class Out:
    """Junk-filled outputs on the device, each followed by guard bytes."""
    SPEC = (("codes", torch.int16), ("npk", torch.int32), ("nbox", torch.int32), ("nbad", torch.int32),
            ("nsat", torch.int32), ("flags", torch.uint8), ("offs", torch.int64), ("ctr", torch.int32),
            ("rec", torch.float32), ("box", torch.float32))

    def __init__(self, F, shape, p, dev):
        P, Hb, Wb = reference.roibin_code_shape(shape, p.bin)
        Wn = 2 * p.radius + 1
        shapes = {"codes": (F, P, Hb, Wb), "npk": (F,), "nbox": (F,), "nbad": (F,), "nsat": (F,), "flags": (F,),
                  "offs": (F + 1,), "ctr": (F * p.max_peaks,), "rec": (F * p.max_peaks, 8),
                  "box": (F * p.max_peaks, Wn, Wn)}
        self.raw, self.t, self.nbytes = {}, {}, {}
        for name, dt in self.SPEC:
            nb = int(np.prod(shapes[name])) * torch.empty(0, dtype=dt).element_size()
            raw = torch.full(((nb + 15) // 16 * 16 + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=dev)
            raw[:nb] = JUNK_BYTE
            self.raw[name], self.nbytes[name] = raw, nb
            self.t[name] = raw[:nb].view(dt).view(*shapes[name])

    def host(self):
        torch.cuda.synchronize()
        for name, r in self.raw.items():
            assert bool((r[self.nbytes[name]:].cpu() == GUARD_BYTE).all()), f"guard bytes behind {name} were written"
        return {k: v.cpu().numpy() for k, v in self.t.items()}


def _params(B, R=2, min_peaks=0, max_peaks=MP, **kw):
    return reference.validate_roibin_params(bin=B, radius=R, max_peaks=max_peaks, min_peaks=min_peaks, **{**WINDOW, **kw})


def _launch(x, shape, peaks, counts, p, mask=None, stream=None):
    dev = _dev()
    F = x.shape[0]
    frames = [torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in np.asarray(x, f32).reshape(F, -1)]
    o = Out(F, shape, p, dev)
    m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(dev)
    kernels.roibin(frames, shape, p, torch.from_numpy(peaks).to(dev), torch.from_numpy(np.asarray(counts, np.int32)).to(dev),
                   mask=m, stream=stream, **o.t)
    return o


def _check(got, x, shape, peaks, counts, p, mask=None):
    """Every word against the golden model: header, offs, the boxes up to offs[F] and the codes of kept frames as
    integer views; the code rows of skipped frames and the box rows from offs[F] on still hold the pre-fill."""
    F = x.shape[0]
    g = reference.roibin_reference(torch.from_numpy(np.asarray(x, f32)), shape, torch.from_numpy(peaks),
                                   torch.from_numpy(np.asarray(counts, np.int32)), p, mask=mask)
    for k in ("npk", "nbox", "nbad", "nsat", "flags", "offs"):
        assert np.array_equal(got[k], getattr(g, k).numpy()), (k, got[k], getattr(g, k))
    K = int(g.offs[-1])
    assert np.array_equal(got["ctr"][:K], g.ctr.numpy())
    assert np.array_equal(got["rec"][:K].view(np.uint32), g.rec.numpy().view(np.uint32))
    assert np.array_equal(got["box"][:K].view(np.uint32), g.box.numpy().view(np.uint32))
    for k in ("ctr", "rec", "box"):
        assert bool((got[k][K:].view(np.uint8) == JUNK_BYTE).all()), f"{k}: rows past offs[F] were written"
    kept = (g.flags.numpy() & reference.ROIBIN_FLAG_SKIPPED) == 0
    assert np.array_equal(got["codes"][kept].view(np.uint16), g.codes.numpy().view(np.uint16))
    assert bool((got["codes"][~kept].view(np.uint8) == JUNK_BYTE).all()), "a skipped frame's code rows were written"
    return g


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_golden(shape, B):
    F = 3
    x, mask, peaks, counts = make_case(shape, F, seed=B)
    counts[1] = 0
    p = _params(B, min_peaks=1)
    for m in (None, mask):
        g = _check(_launch(x, shape, peaks, counts, p, m).host(), x, shape, peaks, counts, p, m)
        assert int(g.flags[1]) == 2 and int(g.nbad.sum()) > 0 and int(g.nbox.sum()) > 0


@pytest.mark.parametrize("B", [1, 2, 4])
@pytest.mark.parametrize("shape", [(2, 6, 8), (1, 7, 10)])
def test_every_lane_position(shape, B):
    """The special pixels (NaN, +-inf, the window's edges, masked ones) and the rounding blocks in every position of
    a quad: the frame and the mask rolled by 0 .. 3 pixels along a row."""
    P, H, W = shape
    x, mask, peaks, counts = make_case(shape, 2, seed=5)
    # the rounding cases of the contract as 2 x 2 blocks in the first two rows of frame 0: (S, c) = (-7, 4), (-3, 2),
    # (-1, 2), (1, 2); frame 1 saturates above and below (window +-100 at step 2^-10)
    top = np.asarray([[-1, -2, -1, -2, -1, 0, 1, 0], [-2, -2, 9, 9, 9, 9, 9, 9]], f32)
    keep = np.asarray([[1, 1, 1, 1, 1, 1, 1, 1], [1, 1, 0, 0, 0, 0, 0, 0]], np.uint8)
    x[0, 0, :2, :8] = top
    x[1, 0, :4], x[1, 0, 4:] = 90.0, -90.0     # whole blocks at every B and roll: both clamps at step 2^-10
    mk = mask.reshape(P, H, W).copy()
    mk[0, :2, :8] = keep
    for roll in range(4):
        xr, mr = np.roll(x, roll, axis=3), np.roll(mk, roll, axis=2).reshape(-1)
        for step in (1.0, 2.0 ** -10):
            p = _params(B, step=step)
            g = _check(_launch(xr, shape, peaks, counts, p, mr).host(), xr, shape, peaks, counts, p, mr)
            assert (int(g.nsat.sum()) > 0) == (step < 1.0)


@pytest.mark.parametrize("R", [0, 7])
def test_box_radius_and_record_counts(R):
    shape = (2, 6, 8)
    x, mask, peaks, _ = make_case(shape, 5, seed=9)
    counts = np.asarray([0, 1, MP, MP + 1, -2], np.int32)
    p = _params(2, R=R)
    g = _check(_launch(x, shape, peaks, counts, p, mask).host(), x, shape, peaks, counts, p, mask)
    assert g.flags.tolist()[3] & 1 and g.flags.tolist()[4] == 2 and g.npk.tolist() == [0, 1, MP, MP + 1, 0]


def test_many_records_sorted():
    """A full 4096-slot frame, records in shuffled order with ties and invalid ones: the 12-stage sort."""
    shape = (2, 70, 388)
    rng = np.random.default_rng(2)
    F, mp = 2, 4096
    x = rng.integers(-50, 50, size=(F, *shape)).astype(f32)
    peaks = rng.random((F, mp, 8)).astype(f32)
    counts = np.asarray([mp, 1000], np.int32)
    for f in range(F):
        k = int(counts[f])
        peaks[f, :k, 0] = rng.integers(0, 2, k)
        peaks[f, :k, 1] = rng.integers(0, 70, k)
        peaks[f, :k, 2] = rng.integers(0, 388, k)
        peaks[f, :k:97, 2] = 388.0          # invalid
        peaks[f, 5:k:50, :3] = peaks[f, 4:k:50, :3]   # ties on ctr
    p = _params(4, R=1, max_peaks=mp)
    g = _check(_launch(x, shape, peaks, counts, p).host(), x, shape, peaks, counts, p)
    assert int(g.nbad[0]) > 0 and int(g.nbox[0]) == mp - int(g.nbad[0]) and int(g.nbox[1]) + int(g.nbad[1]) == 1000


@pytest.mark.parametrize("F", [1, 64])
def test_frame_counts(F):
    shape = (2, 6, 8)
    x, mask, peaks, counts = make_case(shape, F, seed=F)
    p = _params(2, min_peaks=3)
    g = _check(_launch(x, shape, peaks, counts, p, mask).host(), x, shape, peaks, counts, p, mask)
    assert F == 1 or (0 < int((g.flags & 2 != 0).sum()) < F)


def test_two_streams_equal_bytes():
    shape = (3, 9, 12)
    x, mask, peaks, counts = make_case(shape, 4, seed=21)
    p = _params(2)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    a = _launch(x, shape, peaks, counts, p, mask, stream=s1)
    b = _launch(x, shape, peaks, counts, p, mask, stream=s2)
    ha, hb = a.host(), b.host()
    for k in ha:
        assert np.array_equal(ha[k].view(np.uint8), hb[k].view(np.uint8)), k
    _check(ha, x, shape, peaks, counts, p, mask)


def test_refusals_before_any_launch():
    dev = _dev()
    shape = (2, 6, 8)
    x, mask, peaks, counts = make_case(shape, 2, seed=1)
    p = _params(2)
    o = Out(2, shape, p, dev)
    frames = [torch.from_numpy(r).to(dev) for r in x.reshape(2, -1)]
    pk, ct = torch.from_numpy(peaks).to(dev), torch.from_numpy(counts).to(dev)
    ok = dict(o.t)
    bad = [
        (dict(ok, codes=o.t["codes"].view(-1)[1:-1]), "codes"), (dict(ok, nsat=o.t["nsat"].long()), "nsat"),
        (dict(ok, box=o.t["box"][:, :3]), "box"), (dict(ok, offs=o.t["offs"][:2]), "offs"),
        (dict(ok, mask=torch.ones(5, dtype=torch.uint8, device=dev)), "mask"),
    ]
    for kw, msg in bad:
        with pytest.raises(ValueError, match=msg):
            kernels.roibin(frames, shape, p, pk, ct, **kw)
    with pytest.raises(ValueError, match="peaks"):
        kernels.roibin(frames, shape, p, pk[:, :4], ct, **ok)
    with pytest.raises(ValueError, match="counts"):
        kernels.roibin(frames, shape, p, pk, ct.cpu(), **ok)
    with pytest.raises(ValueError, match="2\\^25"):
        kernels.roibin(frames, shape, p._replace(vmax=2.0 ** 26), pk, ct, **ok)
    with pytest.raises(ValueError, match="RoibinParams"):
        kernels.roibin(frames, shape, dict(bin=2), pk, ct, **ok)
    with pytest.raises(ValueError, match="elements"):
        kernels.roibin(frames, (2, 6, 9), p, pk, ct, **ok)
    with pytest.raises(ValueError, match="frames"):
        kernels.roibin([], shape, p, pk, ct, **ok)
    torch.cuda.synchronize()
    for name, t in o.t.items():
        assert bool((t.view(-1).view(torch.uint8).cpu() == JUNK_BYTE).all()), f"{name} was written by a refused call"
