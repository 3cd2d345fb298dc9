"""K-16 ROI kernel (csrc/roi.hip) against the golden model, word for word for every output, on the smallest
shapes where each hazard exists: every lanes-per-row tiling, the column chunks, the scalar path, the strip
edges, the clear and the widest words."""
import numpy as np
import pytest
import torch

from psana_ray_amd.ops import kernels, reference

pytestmark = pytest.mark.gpu

GUARD = 64                      # guard words behind every buffer
GUARD_WORD = 0x5EED5EED5EED
JUNK = 0x7777777777777777       # what every output holds before the call
TAIL = 2                        # frames' worth of rows behind the call's own: they must stay junk
f32 = np.float32


def _guarded(shape, dev):
    words = int(np.prod(shape))
    al = (words + 15) // 16 * 16
    raw = torch.full((al + GUARD,), GUARD_WORD, dtype=torch.int64, device=dev)
    v = raw[:words].view(*shape)
    v.fill_(JUNK)
    return raw, v, words


class Bufs:
    """Junk-filled outputs on the device for F + TAIL frames, every tensor followed by guard words."""

    def __init__(self, F, rects, proj, dev):
        R = len(rects)
        want_x, want_y = reference.validate_roi_proj(proj)
        Lx, Ly = sum(r[4] - r[3] for r in rects), sum(r[2] - r[1] for r in rects)
        self.F = F
        self.raw, self.t, self.words = {}, {}, {}
        spec = {"rows": (F + TAIL, R, 8)}
        if want_x:
            spec["proj_x"] = (F + TAIL, Lx)
        if want_y:
            spec["proj_y"] = (F + TAIL, Ly)
        for name, shape in spec.items():
            self.raw[name], self.t[name], self.words[name] = _guarded(shape, dev)

    def arg(self, name, a=0, b=None):
        t = self.t.get(name)
        return None if t is None else t[a:self.F if b is None else b]

    def host(self):
        torch.cuda.synchronize()
        out = {}
        for name, r in self.raw.items():
            assert bool((r[self.words[name]:].cpu() == GUARD_WORD).all()), f"guard words behind {name} were written"
            full = self.t[name].cpu()
            assert bool((full[self.F:] == JUNK).all()), f"{name}: rows behind the call's frames were touched"
            out[name] = full[:self.F]
        return out


def _device_frames(x, dev):
    """x: float32 [F, n] on the host -> F separate 16-B aligned device tensors."""
    return [torch.from_numpy(np.ascontiguousarray(r)).to(dev) for r in np.asarray(x, f32)]


def _launch(frames, shape, rects, dev, vmin, vmax, S, proj="both", mask=None, split=None, stream=None):
    F = len(frames)
    b = Bufs(F, rects, proj, dev)
    m = None if mask is None else torch.from_numpy(np.asarray(mask, np.uint8)).to(dev)
    cuts = [0, *(split or []), F]
    for a, e in zip(cuts[:-1], cuts[1:]):
        kernels.roi_stats(frames[a:e], shape, rects, vmin, vmax, S, b.arg("rows", a, e), b.arg("proj_x", a, e),
                          b.arg("proj_y", a, e), mask=m, stream=stream)
    return b


def _golden(x, shape, rects, vmin, vmax, S, proj, mask):
    rows, px, py = reference.roi_stats_reference(torch.from_numpy(np.asarray(x, f32)), shape, rects, vmin, vmax, S, mask, proj)
    want_x, want_y = reference.validate_roi_proj(proj)
    g = {"rows": rows}
    if want_x:
        g["proj_x"] = px
    if want_y:
        g["proj_y"] = py
    return g


def _check(x, shape, rects, dev, vmin=-100.0, vmax=100.0, S=2, proj="both", mask=None, split=None, golden=None):
    """The kernel's outputs == the golden model's, every word; guards and the rows behind the call intact."""
    x = np.asarray(x, f32).reshape(-1, int(np.prod(shape)))
    got = _launch(_device_frames(x, dev), shape, rects, dev, vmin, vmax, S, proj, mask, split).host()
    want = golden if golden is not None else _golden(x, shape, rects, vmin, vmax, S, proj, mask)
    assert set(got) == set(want)
    for k in want:
        assert got[k].dtype == torch.int64 and got[k].shape == want[k].shape, k
        bad = (got[k] != want[k]).nonzero()
        assert bad.numel() == 0, f"{k}: {bad.shape[0]} words differ, first at {bad[0].tolist()}: " \
                                 f"{got[k][tuple(bad[0])].item()} != {want[k][tuple(bad[0])].item()}"
    return got


def _frames(F, shape, seed, scale=40.0):
    rng = np.random.default_rng(seed)
    # quarters, so that .5 ties of v * 2^S are common at S = 1; about 1 % outside the window of +-100
    return (np.round(rng.normal(0.0, scale, (F, int(np.prod(shape)))) * 4) / 4).astype(f32)


def test_strip_rule(native):
    assert kernels.roi_strip_rows(1) == kernels.roi_strip_rows(8) == 1024 and kernels.roi_strip_rows(16) == 512
    assert kernels.roi_strip_rows(1024) == 8 and kernels.roi_strip_rows(8192) == 1 == kernels.roi_strip_rows(100000)
    # the plan: every row of every rectangle in exactly one strip, strips no taller than the rule
    rects = [(1, 3, 30, 2, 1030), (0, 0, 40, 5, 6)]
    st = np.asarray(native.roi_plan_strips([v for r in rects for v in r], 2, 40, 1100), np.int64).reshape(-1, 8)
    for r, (p, y0, y1, x0, x1) in enumerate(rects):
        mine = st[st[:, 0] == r]
        assert (mine[:, 3] == x0).all() and (mine[:, 4] == x1).all() and (mine[:, 2] <= kernels.roi_strip_rows(x1 - x0)).all()
        ys = np.concatenate([np.arange(y, y + n) for y, n in zip(mine[:, 5], mine[:, 2])])
        assert ys.tolist() == list(range(y0, y1)) and np.array_equal(mine[:, 1], p * 40 + mine[:, 5])
    assert len(st) == 4 + 1


@pytest.mark.parametrize("W", [12, 13])
def test_small_shapes_every_residue_and_special_rectangles(cuda_device, W):
    shape = (2, 5, W)
    P, H = 2, 5
    x = _frames(3, shape, 1)
    residues = [(p, 1, 4, x0, x1) for p, x0, x1 in
                [(0, 0, 1), (0, 1, 6), (0, 2, 7), (0, 3, 8), (1, 0, 4), (1, 4, 9), (1, 5, 11), (1, 3, W), (1, 0, W)]]
    special = [(0, 2, 3, 5, 6), (1, 0, H, 0, W), (P - 1, H - 1, H, W - 1, W), (0, 1, 4, 2, 9), (0, 1, 4, 2, 9),
               (1, 0, 3, 0, 6), (1, 2, 5, 4, 10)]
    for S in (0, 1, 2):
        _check(x, shape, residues, cuda_device, S=S)
    got = _check(x, shape, special, cuda_device)
    assert torch.equal(got["rows"][:, 3], got["rows"][:, 4])
    _check(x[:1], shape, [(1, 1, 3, 2, 7)], cuda_device)           # R = 1


WIDTHS = (1, 4, 5, 255, 256, 257, 1024, 1025, 1030)


@pytest.mark.parametrize("W", [1100, 1101])
@pytest.mark.parametrize("where", ["left", "odd", "right"])
def test_every_width(cuda_device, W, where):
    """Every lanes-per-row tiling (1 .. 256), the column chunks (more than 256 quads) and, at W = 1101, the scalar
    path, with x0 at a quad boundary, off it, and x1 at the frame's edge."""
    shape = (1, 3, W)
    x = _frames(2, shape, W)
    x0 = {"left": lambda w: 0, "odd": lambda w: min(3, W - w), "right": lambda w: W - w}[where]
    rects = [(0, i % 2, 3 - (i // 2) % 2, x0(w), x0(w) + w) for i, w in enumerate(WIDTHS)]
    _check(x, shape, rects, cuda_device)


@pytest.mark.parametrize("W,x0,width", [(8, 0, 4), (9, 2, 5), (1028, 4, 1024), (1029, 3, 1024)])
def test_heights_around_the_strip(cuda_device, W, x0, width):
    s = kernels.roi_strip_rows(width)
    heights = [1, s - 1, s, s + 1, 2 * s + 1]
    H = 2 * s + 3
    shape = (1, H, W)
    x = _frames(1, shape, 5 + W)
    rects = [(0, y0, y0 + h, x0, x0 + width) for y0, h in zip((H - 1, 2, 1, 0, 2), heights)]
    _check(x, shape, rects, cuda_device)


@pytest.mark.parametrize("ahead", [1, 2])
def test_both_load_pipelines(native, cuda_device, ahead):
    """The kernel keeps the loads of 2 row iterations in flight on small grids and of 1 on large ones; either,
    forced, on shapes with several row iterations, a short last one, column chunks and both load paths."""
    native.roi_rows_ahead(ahead)
    try:
        assert native.roi_rows_ahead() == ahead
        for W in (1100, 1101):
            shape = (2, 9, W)
            x = _frames(2, shape, 20 + W)
            rects = [(0, 0, 9, 3, 1033), (1, 1, 8, 0, 16), (1, 0, 9, 1090, W), (0, 4, 5, 7, 8), (1, 0, 9, 0, W)]
            _check(x, shape, rects, cuda_device, mask=(np.arange(2 * 9 * W) % 7 != 0).astype(np.uint8))
        s = kernels.roi_strip_rows(5)
        _check(_frames(1, (1, 2 * s + 3, 9), 4), (1, 2 * s + 3, 9), [(0, 1, 2 * s + 2, 2, 7), (0, 0, s + 1, 0, 9)], cuda_device)
    finally:
        native.roi_rows_ahead(0)
    assert native.roi_rows_ahead() == 0


def test_a_grid_past_the_resident_size(cuda_device):
    """More than 2048 workgroups (strips x frames): the launch takes the one-iteration pipeline by itself."""
    shape = (1, 40, 8200)
    x = _frames(4, shape, 31, scale=30.0)
    rects = [(0, 0, 40, r % 5, 8193 + r % 7) for r in range(16)]   # strips of one row: 16 x 40 x 4 frames = 2560
    assert all(kernels.roi_strip_rows(r[4] - r[3]) == 1 for r in rects)
    _check(x, shape, rects, cuda_device, proj="both")


@pytest.mark.parametrize("F", [1, 2, 63, 64, 70])
def test_frame_counts_with_16_rectangles(cuda_device, F):
    shape = (2, 5, 12)
    x = _frames(F, shape, 10 + F)
    rects = [(i % 2, i % 3, 3 + i % 3, i % 5, 6 + i % 7) for i in range(16)]
    _check(x, shape, rects, cuda_device)


def test_split_calls_equal_one_call(cuda_device):
    shape = (2, 9, 20)
    x = _frames(9, shape, 3)
    rects = [(0, 0, 9, 0, 20), (1, 2, 7, 3, 18), (1, 8, 9, 19, 20)]
    one = _check(x, shape, rects, cuda_device)
    for split in ([1], [4], [8], [2, 3, 7]):
        got = _check(x, shape, rects, cuda_device, split=split)
        assert all(torch.equal(got[k], one[k]) for k in one)


@pytest.mark.parametrize("proj", ["none", "x", "y", "both"])
@pytest.mark.parametrize("W", [20, 21])
def test_projection_selectors_and_mask(cuda_device, proj, W):
    shape = (2, 9, W)
    x = _frames(3, shape, 4)
    rng = np.random.default_rng(11)
    mask = (rng.random(int(np.prod(shape))) < 0.7).astype(np.uint8) * rng.integers(1, 256, int(np.prod(shape))).astype(np.uint8)
    mask.reshape(shape)[1, 2:4, 5:9] = 0                            # an all-masked rectangle
    rects = [(0, 0, 9, 0, W), (1, 2, 4, 5, 9), (1, 1, 8, 3, W - 1)]
    got = _check(x, shape, rects, cuda_device, proj=proj, mask=mask)
    assert got["rows"][:, 1].tolist() == [[0] * 8] * 3
    _check(x, shape, rects, cuda_device, proj=proj)


def test_values_at_the_window_and_ties(cuda_device):
    shape = (1, 4, 8)
    lo, hi = f32(-10.0), f32(10.0)
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, lo, hi, np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf)),
            np.nextafter(lo, f32(0)), np.nextafter(hi, f32(0)), 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.25, 0.75, -0.25, 3.0, 9.75]
    x = np.zeros((1, 32), f32)
    x[0, :len(vals)] = vals
    for S in (0, 1, 2, 16):
        got = _check(x, shape, [(0, 0, 4, 0, 8), (0, 1, 3, 1, 7)], cuda_device, vmin=lo, vmax=hi, S=S)
        assert got["rows"][0, 0, 0].item() == 32 - 5
    # the maximum several times: the lowest index wins; all sums negative
    y = -np.abs(_frames(2, (2, 5, 12), 5)) - 1.0
    y3 = y.reshape(2, 2, 5, 12)
    y3[:, 1, 3, 9] = y3[:, 1, 1, 4] = y3[:, 1, 1, 10] = y3[:, 0, 4, 11] = -0.5
    got = _check(y, (2, 5, 12), [(1, 0, 5, 2, 12), (1, 2, 5, 0, 12)], cuda_device, vmin=-200, vmax=200)
    q, i = reference.roi_key_decode(got["rows"][:, :, 4])
    assert q.tolist() == [[-2, -2]] * 2 and i.tolist() == [[(5 + 1) * 12 + 4, (5 + 3) * 12 + 9]] * 2
    assert bool((got["rows"][:, :, 1:4] < 0).all())


@pytest.mark.parametrize("W", [24, 25])
def test_nan_outside_every_rectangle_changes_nothing(cuda_device, W):
    shape = (2, 7, W)
    x = _frames(2, shape, 6)
    rects = [(0, 1, 5, 3, 17), (1, 0, 7, 20, W), (1, 6, 7, 0, 2)]
    inside = np.zeros(shape, bool)
    for p, y0, y1, x0, x1 in rects:
        inside[p, y0:y1, x0:x1] = True
    poisoned = np.where(inside.reshape(1, -1), x, f32(np.nan))
    clean = _check(x, shape, rects, cuda_device)
    _check(poisoned, shape, rects, cuda_device, golden=clean)


def test_widest_words(cuda_device):
    """S = 0 and the largest window: q = +-2147483520 in a 64-pixel rectangle that ends in the frame's last row and
    column -- the largest |sum|, |sy|, |sx| and both ends of the key's high word."""
    H, W = 65536, 64
    shape = (1, H, W)
    v = 2147483520.0
    reference.validate_roi_params(-v, v, 0, [(0, H - 8, H, W - 8, W)])
    x = np.zeros((3, H * W), f32)
    x3 = x.reshape(3, H, W)
    rng = np.random.default_rng(8)
    x3[0, H - 8:, W - 8:] = v
    x3[1, H - 8:, W - 8:] = -v
    x3[2, H - 8:, W - 8:] = np.where(rng.random((8, 8)) < 0.5, v, -v)
    got = _check(x, shape, [(0, H - 8, H, W - 8, W)], cuda_device, vmin=-v, vmax=v, S=0)
    rows = got["rows"]
    assert rows[0, 0, 1].item() == 64 * 2147483520 and rows[1, 0, 1].item() == -64 * 2147483520
    assert rows[0, 0, 2].item() == 2147483520 * 8 * sum(range(H - 8, H))
    q, i = reference.roi_key_decode(rows[:, 0, 4])
    assert q[:2].tolist() == [2147483520, -2147483520] and i[:2].tolist() == [(H - 8) * W + W - 8] * 2


def test_streams_and_repeats_give_equal_bytes(cuda_device):
    shape = (2, 40, 1100)
    x = _frames(4, shape, 9)
    rects = [(0, 0, 40, 0, 1100), (1, 3, 30, 2, 1030), (0, 5, 6, 7, 8), (1, 0, 40, 1090, 1100)]
    fr = _device_frames(x, cuda_device)
    want = _golden(x, shape, rects, -100.0, 100.0, 2, "both", None)
    s1, s2 = torch.cuda.Stream(cuda_device), torch.cuda.Stream(cuda_device)
    torch.cuda.synchronize()
    runs = [_launch(fr, shape, rects, cuda_device, -100.0, 100.0, 2, stream=s) for s in (s1, s2, s1, None)]
    outs = [b.host() for b in runs]
    for o in outs:
        assert all(torch.equal(o[k], want[k]) for k in want)


def test_refusals_before_any_launch(cuda_device):
    shape = (2, 5, 12)
    fr = _device_frames(_frames(2, shape, 1), cuda_device)
    rects = [(0, 0, 5, 0, 12)]
    rows = torch.zeros((2, 1, 8), dtype=torch.int64, device=cuda_device)
    px = torch.zeros((2, 12), dtype=torch.int64, device=cuda_device)
    ok = dict(frames=fr, shape=shape, rects=rects, vmin=-1.0, vmax=1.0, frac_bits=2, rows=rows)
    kernels.roi_stats(**ok, proj_x=px)
    for bad in (dict(rects=[(0, 0, 6, 0, 12)]), dict(rects=[]), dict(vmin=2.0), dict(frac_bits=17),
                dict(vmax=2.0 ** 31), dict(rows=rows[:1]), dict(rows=rows.to(torch.int32)), dict(rows=rows.cpu()),
                dict(proj_x=px[:, :11]), dict(proj_y=px), dict(shape=(2, 5, 13)),
                dict(mask=torch.ones(119, dtype=torch.uint8, device=cuda_device)),
                dict(frames=[t.double() for t in fr]), dict(frames=[t.cpu() for t in fr])):
        with pytest.raises(ValueError):
            kernels.roi_stats(**{**ok, **bad})
    torch.cuda.synchronize()
