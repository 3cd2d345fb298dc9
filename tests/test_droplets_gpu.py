"""K-14 droplet kernels (csrc/droplets.hip) against the golden model, word for word for every output, on the
smallest shapes where each hazard exists.  Outputs and scratch start as 0xFF; guard words sit behind every
buffer and behind the scratch."""
import functools

import numpy as np
import pytest
import torch

from psana_ray_amd.ops import kernels, reference
from tests._droplets_oracle import patterns, random_frames

pytestmark = pytest.mark.gpu

GUARD = 64            # guard elements behind every buffer
GUARD_BYTE = 0xA5
PER_FRAME = (("nact", torch.int32, 0), ("ndrop", torch.int32, 0), ("flags", torch.uint8, 0), ("offs", torch.int64, 1))
COLS = (("label", torch.int32), ("npix", torch.int32), ("adu", torch.int64), ("sy", torch.int64), ("sx", torch.int64),
        ("qmax", torch.int32))
f32 = np.float32
CHUNK = kernels.SPARSE_CHUNK                      # elements per scan chunk
SHAPE_1C = (1, 37, 111)                           # 4107: just past one chunk per frame, n % 4 == 3
SHAPE_2C = (2, 41, 101)                           # 8282: just past two, a panel edge inside chunk 1
assert CHUNK < np.prod(SHAPE_1C) < CHUNK + 64 and 2 * CHUNK < np.prod(SHAPE_2C) < 2 * CHUNK + 128
SMALL = [(1, 1, 1), (1, 1, 9), (1, 7, 1), (2, 5, 7), (3, 8, 12)]


def _guarded(words, dtype, dev):
    """``words`` elements of 0xFF bytes followed by GUARD elements of 0xA5 bytes."""
    es = torch.empty(0, dtype=dtype).element_size()
    raw = torch.full(((words + GUARD) * es,), GUARD_BYTE, dtype=torch.uint8, device=dev)
    raw[:words * es] = 0xFF
    return raw, raw[:words * es].view(dtype)


class Bufs:
    def __init__(self, F, n, cap_pix, cap, dev):
        self.raw, self.t = {}, {}
        for name, dt, extra in PER_FRAME:
            self.raw[name], self.t[name] = _guarded(F + extra, dt, dev)
        for name, dt in COLS:
            self.raw[name], self.t[name] = _guarded(F * cap, dt, dev)
        self.need = kernels.droplets_scratch_bytes(n, cap_pix, cap, F)
        self.raw["scratch"], self.t["scratch"] = _guarded(self.need, torch.uint8, dev)

    def args(self):
        return [self.t[k] for k, *_ in PER_FRAME] + [self.t[k] for k, _ in COLS]

    def host(self):
        torch.cuda.synchronize()
        for name, r in self.raw.items():
            tail = r[self.t[name].numel() * self.t[name].element_size():].cpu()
            assert tail.numel() >= GUARD and bool((tail == GUARD_BYTE).all()), f"guard words behind {name} were written"
        out = {k: v.cpu() for k, v in self.t.items() if k != "scratch"}
        return out

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((r.cpu()[:self.t[k].numel() * self.t[k].element_size()] == 0xFF).all())
                   for k, r in self.raw.items())


def _caps(shape, cap_pix, cap):
    n = int(np.prod(shape))
    return (max(1, n // 16) if cap_pix is None else cap_pix), (max(1, n // 64) if cap is None else cap)


def _run(x, shape, dev, par, mask=None, cap_pix=None, cap=None, separate=False, stream=None, bufs=None):
    """x: float32 [F, n] on the host.  Returns the outputs on the host (guards checked)."""
    x = torch.as_tensor(np.asarray(x, f32))
    F, n = x.shape
    cap_pix, cap = _caps(shape, cap_pix, cap)
    if separate or (4 * n) % 16:
        frames = [x[f].clone().to(dev) for f in range(F)]
    else:
        xd = x.to(dev)
        frames = [xd[f] for f in range(F)]
    b = Bufs(F, n, cap_pix, cap, dev) if bufs is None else bufs
    md = None if mask is None else torch.as_tensor(mask, dtype=torch.uint8).to(dev)
    kernels.droplets(frames, shape, par, cap_pix, cap, *b.args(), mask=md, scratch=b.t["scratch"], stream=stream)
    return b.host()


def _ref(x, shape, par, mask=None, cap_pix=None, cap=None):
    x = torch.as_tensor(np.asarray(x, f32))
    cap_pix, cap = _caps(shape, cap_pix, cap)
    return reference.droplet_reference(x, shape, par, mask, cap_pix, cap)


def _same(got, want):
    for name, _dt, _e in PER_FRAME:
        g, w = got[name], getattr(want, name)
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert torch.equal(g, w), f"{name}: {g.tolist()[:8]} != {w.tolist()[:8]}"
    k = int(want.offs[-1])
    for name, _dt in COLS:
        g, w = got[name][:k], getattr(want, name)
        assert g.dtype == w.dtype, name
        assert torch.equal(g, w), f"{name} differs at rows {(g != w).nonzero()[:4].reshape(-1).tolist()} of {k}"


def _check(x, shape, dev, par, **kw):
    want = _ref(x, shape, par, **{k: v for k, v in kw.items() if k in ("mask", "cap_pix", "cap")})
    got = _run(x, shape, dev, par, **kw)
    _same(got, want)
    return got, want


@pytest.fixture(scope="module")
def dev(native, cuda_device):
    return cuda_device


PAR = dict(thr_low=5.0, thr_seed=5.0, vmax=100.0, frac_bits=2)


@pytest.mark.parametrize("shape", SMALL + [SHAPE_1C, SHAPE_2C])
def test_patterns(dev, shape):
    pats = patterns(shape)
    x = np.stack([p.reshape(-1) for p in pats.values()])
    n = x.shape[1]
    _got, want = _check(x, shape, dev, PAR, cap_pix=n, cap=n)
    nd = dict(zip(pats, want.ndrop.tolist()))
    for k in ("L", "U", "comb", "spiral", "serpentine"):
        assert nd.get(k, 1) == 1, k
    for k in ("diagonal", "row_end", "panel_edge"):
        assert nd.get(k, 2) == 2, k
    _check(x, shape, dev, dict(PAR, thr_seed=10.5), cap_pix=n, cap=n)   # only clusters with a brighter pixel stay


@pytest.mark.parametrize("shape", [(3, 8, 12), SHAPE_1C])
def test_full_panel_sums_pass_2_32(dev, shape):
    par = dict(thr_low=5.0, vmax=2.0 ** 14, frac_bits=16)     # Q = 2^30
    n = int(np.prod(shape))
    x = np.full((2, n), 2.0 ** 14, f32)
    x[1, 0] = 7.25
    got, want = _check(x, shape, dev, par, cap_pix=n, cap=n)
    assert want.ndrop.tolist() == [shape[0]] * 2 and int(want.npix[0]) == shape[1] * shape[2]
    assert int(got["adu"][0]) == shape[1] * shape[2] * 2 ** 30 > 2 ** 32 and int(got["sx"][0]) > 2 ** 32


def test_chunk_boundary_straddlers(dev):
    for shape in (SHAPE_1C, SHAPE_2C):
        P, H, W = shape
        n = P * H * W
        x = np.zeros((2, n), f32)
        for c in range(1, n // CHUNK + 1):
            b = c * CHUNK
            x[0, b - 3:b + 3] = 10.0                  # a run through the boundary (a row end may cut it)
            x[1, b - W:b + W + 1:W] = 12.0            # a column through it (a panel edge may cut it)
            x[1, b - 1] = 9.0
        x[0, n - 3:] = 11.0                           # the n % 4 tail
        _check(x, shape, dev, PAR, cap_pix=n, cap=n)


def test_mask_and_vmax_cut(dev):
    shape = (2, 5, 7)
    x = np.zeros((2, 70), f32)
    x[:, 14:21] = 10.0
    x[:, 35 + 3:70:7] = 10.0
    x[1, 17] = np.nextafter(f32(100.0), f32(np.inf))
    x[1, 35 + 3 + 14] = 101.0
    m = np.ones(70, np.uint8)
    m[16] = 0
    m[35 + 3 + 21] = 0
    got, _ = _check(x, shape, dev, PAR, cap_pix=70, cap=70)
    assert got["ndrop"].tolist() == [2, 4]
    got, _ = _check(x, shape, dev, PAR, mask=m, cap_pix=70, cap=70)
    assert got["ndrop"].tolist() == [4, 4]


def test_values_in_every_quad_lane(dev):
    lo, hi, seed = f32(5.0), f32(100.0), f32(20.0)
    dn, up = lambda v: np.nextafter(f32(v), f32(-np.inf)), lambda v: np.nextafter(f32(v), f32(np.inf))
    specials = [lo, dn(lo), hi, up(hi), np.nan, np.inf, -np.inf, -0.0, 0.0, -7.0, 5.125, 5.375, 5.625, 5.875, 6.125,
                dn(seed), seed, up(seed)]
    n = 8 * len(specials) + 8
    rows = []
    for e in range(4):
        a = np.zeros(n, f32)
        for j, v in enumerate(specials):
            a[8 * j + e] = v
        rows.append(a)
        b = a.copy()                 # every special with an active neighbour to its right: candidates of two
        for j in range(len(specials)):
            b[8 * j + e + 1] = 6.0
        rows.append(b)
    x = np.stack(rows)
    for shape in ((1, 1, n), (1, n // 8, 8)):
        for par in (PAR, dict(PAR, thr_seed=20.0), dict(PAR, frac_bits=0), dict(PAR, frac_bits=3, thr_seed=20.0)):
            got, want = _check(x, shape, dev, par, cap_pix=n, cap=n)
    # the candidate whose best pixel is one ulp below thr_seed is dropped and not counted
    y = np.zeros((1, 16), f32)
    y[0, 0:2] = [dn(seed), 6.0]
    y[0, 8:10] = [6.0, seed]
    got, _ = _check(y, (1, 1, 16), dev, dict(PAR, thr_seed=20.0), cap_pix=16, cap=16)
    assert got["nact"].tolist() == [4] and got["ndrop"].tolist() == [1] and got["label"][:1].tolist() == [8]


def test_capacity_edges(dev):
    shape = (1, 4, 8)
    x = np.zeros((3, 32), f32)
    x[:, [0, 2, 4, 9]] = 10.0
    x[1, 20] = 11.0                                   # the frame in the middle has one more
    got, _ = _check(x, shape, dev, PAR, cap_pix=32, cap=4)
    assert got["ndrop"].tolist() == [4, 5, 4] and got["flags"].tolist() == [0, 1, 0]
    assert got["offs"].tolist() == [0, 4, 4, 8] and got["label"][:8].tolist() == [0, 2, 4, 9] * 2
    got, _ = _check(x, shape, dev, PAR, cap_pix=4, cap=8)
    assert got["nact"].tolist() == [4, 5, 4] and got["ndrop"].tolist() == [4, 0, 4] and got["flags"].tolist() == [0, 4, 0]
    assert got["label"][:8].tolist() == [0, 2, 4, 9] * 2
    got, _ = _check(x, shape, dev, PAR, cap_pix=5, cap=5)
    assert got["flags"].tolist() == [0, 0, 0]
    got, _ = _check(x[1:2], shape, dev, PAR, cap_pix=1, cap=1)
    assert got["flags"].tolist() == [4] and got["offs"].tolist() == [0, 0]


@functools.lru_cache(maxsize=None)
def _random_case(frac, F, shape, masked):
    n = int(np.prod(shape))
    x = random_frames(shape, F, frac, seed=int(frac * 1000) + F)
    m = (np.random.default_rng(17).random(n) > 0.05).astype(np.uint8) if masked else None
    par = dict(thr_low=2.0, thr_seed=30.0, vmax=55.0, frac_bits=2)
    default = frac < 0.01                       # only the sparse case fits n // 16 pixels and n // 64 droplets
    caps = {} if default else dict(cap_pix=n, cap=n)
    want = _ref(x, shape, par, mask=m, **caps)
    assert not want.flags.any(), "the chosen seed overflows a case that is not meant to"
    return x, m, par, caps, want


@pytest.mark.parametrize("frac", [0.001, 0.05, 0.3, 0.59])
@pytest.mark.parametrize("F,shape,masked", [(1, SHAPE_2C, False), (2, SHAPE_1C, True), (64, (3, 8, 12), True),
                                            (3, SHAPE_2C, True)])
def test_random_frames(dev, frac, F, shape, masked):
    x, m, par, caps, want = _random_case(frac, F, shape, masked)
    got = _run(x, shape, dev, par, mask=m, separate=(F == 2), **caps)
    _same(got, want)


def test_default_caps_overflow_dense_frames(dev):
    x = random_frames(SHAPE_2C, 3, 0.3, seed=9)
    x[1] = 0.0
    x[1, 5] = 40.0
    got, _ = _check(x, SHAPE_2C, dev, dict(thr_low=2.0, vmax=55.0))
    assert got["flags"].tolist() == [4, 0, 4] and got["ndrop"].tolist() == [0, 1, 0] and got["offs"].tolist() == [0, 0, 1, 1]


def test_same_call_twice_same_bytes_and_no_clearing(dev):
    x, m, par, caps, want = _random_case(0.3, 3, SHAPE_2C, True)
    n = x.shape[1]
    b = Bufs(3, n, n, n, dev)
    g1 = _run(x, SHAPE_2C, dev, par, mask=m, bufs=b, **caps)
    _same(g1, want)
    # a second batch through the same, now used, outputs and scratch; then the first again
    x2 = random_frames(SHAPE_2C, 3, 0.59, seed=4)
    _same(_run(x2, SHAPE_2C, dev, par, mask=m, bufs=b, **caps), _ref(x2, SHAPE_2C, par, mask=m, **caps))
    g3 = _run(x, SHAPE_2C, dev, par, mask=m, bufs=b, **caps)
    k = int(want.offs[-1])
    for name in g1:
        cut = k if name in dict(COLS) else None
        assert torch.equal(g1[name][:cut], g3[name][:cut]), name


def test_two_streams_in_flight(dev):
    cases = [_random_case(0.3, 3, SHAPE_2C, True), _random_case(0.59, 3, SHAPE_2C, True)]
    n = cases[0][0].shape[1]
    streams = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    bufs = [Bufs(3, n, n, n, dev), Bufs(3, n, n, n, dev)]
    frames, masks = [], []
    for x, m, *_ in cases:
        xd = torch.as_tensor(x).to(dev)
        frames.append([xd[f] for f in range(3)] if (4 * n) % 16 == 0 else [xd[f].clone() for f in range(3)])
        masks.append(torch.as_tensor(m).to(dev))
    torch.cuda.synchronize()
    for _round in range(3):
        for i in (0, 1):
            with torch.cuda.stream(streams[i]):
                kernels.droplets(frames[i], SHAPE_2C, cases[i][2], n, n, *bufs[i].args(), mask=masks[i],
                                 scratch=bufs[i].t["scratch"], stream=streams[i])
    for i in (0, 1):
        _same(bufs[i].host(), cases[i][4])


def test_value_errors_before_any_launch(dev):
    shape = (2, 5, 7)
    n, F = 70, 2
    x = torch.zeros(F, n, device=dev)
    frames = [x[0].clone(), x[1].clone()]
    b = Bufs(F, n, 8, 4, dev)
    a = dict(zip([k for k, *_ in PER_FRAME] + [k for k, _ in COLS], b.args()))

    def call(frames=frames, shape=shape, par=PAR, cap_pix=8, cap=4, mask=None, scratch=b.t["scratch"], **over):
        kernels.droplets(frames, shape, par, cap_pix, cap, **{**a, **over}, mask=mask, scratch=scratch)

    bad = [
        dict(frames=[]), dict(frames=frames * 33), dict(shape=(2, 5, 8)), dict(shape=(70,)), dict(shape=(1, 2, 5, 7)),
        dict(par=dict(PAR, thr_low=0.0)), dict(par=dict(PAR, thr_low=float("nan"))), dict(par=dict(PAR, thr_seed=4.0)),
        dict(par=dict(PAR, thr_seed=101.0)), dict(par=dict(PAR, vmax=float("inf"))), dict(par=dict(PAR, frac_bits=17)),
        dict(par=dict(PAR, frac_bits=-1)), dict(par=dict(PAR, vmax=2.0 ** 20, frac_bits=11)),
        dict(cap_pix=0), dict(cap=0), dict(cap_pix=2 ** 30), dict(cap=2 ** 30),
        dict(frames=[x[0].double(), x[1].double()]), dict(frames=[x[0].cpu(), x[1].cpu()]),
        dict(frames=[frames[0], torch.zeros(71, device=dev)[1:]]),
        dict(nact=a["nact"][:1]), dict(ndrop=a["ndrop"].long()), dict(flags=a["flags"].int()), dict(offs=a["offs"][:F]),
        dict(label=a["label"][:7]), dict(npix=a["npix"].long()), dict(adu=a["adu"].int()), dict(sy=a["sy"][:3]),
        dict(sx=a["sx"].cpu()), dict(qmax=a["qmax"][::2]),
        dict(mask=torch.ones(69, dtype=torch.uint8, device=dev)), dict(mask=torch.ones(70, dtype=torch.int32, device=dev)),
        dict(mask=torch.ones(71, dtype=torch.uint8, device=dev)[1:]),
        dict(scratch=b.t["scratch"][:b.need - 16]), dict(scratch=b.t["scratch"][1:]), dict(scratch=torch.zeros(b.need)),
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            call(**kw)
    assert b.untouched(), "a refused call wrote an output or the scratch"
    # the sums bound: Q = 2^30 over a panel that could reach 2^63
    with pytest.raises(ValueError):
        reference.validate_droplet_caps((1, 2 ** 15, 2 ** 15), dict(thr_low=5.0, vmax=2.0 ** 14, frac_bits=16), 2 ** 19, 4)
    call()
    assert not b.untouched()
    b.host()
