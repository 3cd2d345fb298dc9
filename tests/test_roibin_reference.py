"""K-17 golden model (ops.reference.roibin_reference) against an independent per-block Python loop
(tests/_roibin_oracle.py), the stated rounding cases, and RoibinFrames.to_dense on top of it.  CPU only."""
import numpy as np
import pytest
import torch

from psana_ray_amd import roibin as rb
from psana_ray_amd.ops import reference

from tests._roibin_oracle import batch_arrays, make_case, roibin_oracle

f32 = np.float32
CASES = [((2, 6, 8), 2), ((1, 7, 10), 4), ((3, 5, 9), 1)]
FIELDS = ("npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "rec", "box", "codes")


def _ref(x, shape, peaks, counts, mask=None, **kw):
    return reference.roibin_reference(torch.from_numpy(np.asarray(x, f32)), shape, torch.from_numpy(peaks),
                                      torch.from_numpy(np.asarray(counts, np.int32)), mask=mask, **kw)


def _same(got, want):
    for k in FIELDS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert np.array_equal(got[k], want[k]), k


def _frames_of(batch, shape, p, F):
    """A RoibinFrames of one batch."""
    kept = (batch.flags.numpy() & 2) == 0
    return rb.RoibinFrames("det", "calib", shape, p.bin, p.step, p.inv, p.vmin, p.vmax, p.radius, p.max_peaks,
                           p.min_peaks, {}, "", rank=np.zeros(F), idx=np.arange(F), gevt=np.arange(F),
                           photon_energy=np.zeros(F), npk=batch.npk.numpy(), nbox=batch.nbox.numpy(),
                           nbad=batch.nbad.numpy(), nsat=batch.nsat.numpy(), flags=batch.flags.numpy(),
                           offs=batch.offs.numpy(), ctr=batch.ctr.numpy(), rec=batch.rec.numpy(), box=batch.box.numpy(),
                           koffs=np.concatenate([[0], np.cumsum(kept)]), codes=batch.codes.numpy())


@pytest.mark.parametrize("shape,B", CASES)
@pytest.mark.parametrize("R", [0, 2, 7])
def test_reference_equals_the_loop(shape, B, R):
    x, mask, peaks, counts = make_case(shape, 4, seed=B * 10 + R)
    kw = dict(bin=B, step=0.5, vmin=-100.0, vmax=100.0, radius=R, max_peaks=8, min_peaks=0)
    for m in (None, mask):
        got = batch_arrays(_ref(x, shape, peaks, counts, m, **kw))
        want = roibin_oracle(x, shape, peaks, counts, B, 0.5, -100.0, 100.0, R, 0, m)
        _same(got, want)
        assert got["nbad"].sum() > 0 and (got["flags"] & 4).any()     # the case holds invalid records
        assert (got["box"] == 0x7FC00000).any() or R == 0            # corner boxes reach outside the panel


@pytest.mark.parametrize("shape,B", CASES)
def test_min_peaks_and_count_edges(shape, B):
    x, mask, peaks, _ = make_case(shape, 6, seed=7, bad=False)
    counts = np.asarray([8, 9, -3, 0, 1, 2], np.int32)   # max_peaks, max_peaks + 1, negative, none, one, two
    for mn in (0, 1, 2):
        kw = dict(bin=B, step=1.0, vmin=-100.0, vmax=100.0, radius=1, max_peaks=8, min_peaks=mn)
        b = _ref(x, shape, peaks, counts, mask, **kw)
        _same(batch_arrays(b), roibin_oracle(x, shape, peaks, counts, B, 1.0, -100.0, 100.0, 1, mn, mask))
        assert b.npk.tolist() == [8, 9, 0, 0, 1, 2]
        assert b.flags[1] == 1 and b.nbox[1] == 0                  # more than max_peaks: no boxes, codes kept
        assert b.flags[2] == 2 and (b.flags[3] == 2) == (mn > 0)    # counts < 0 is below every min_peaks
        assert b.codes.shape[0] == int((counts >= mn).sum())


def test_floor_rounding_of_block_means():
    # B = 2 blocks with chosen (S, c): masked pixels take a value out of the block
    def block(vals, keep):
        x = np.zeros((1, 1, 2, 2), f32)
        x.reshape(-1)[:] = vals
        m = np.asarray(keep, np.uint8)
        z = np.zeros((1, 4, 8), f32)
        b = _ref(x, (1, 2, 2), z, [0], m, bin=2, step=1.0, vmin=-50.0, vmax=50.0, radius=0, max_peaks=4, min_peaks=0)
        return int(b.codes.reshape(-1)[0]), int(b.nsat[0])

    assert block([-1, -2, -2, -2], [1, 1, 1, 1]) == (-2, 0)      # S = -7, c = 4: -1.75 -> -2
    assert block([-1, -2, 9, 9], [1, 1, 0, 0]) == (-1, 0)        # S = -3, c = 2: -1.5 -> -1 (half up)
    assert block([-1, 0, 9, 9], [1, 1, 0, 0]) == (0, 0)          # S = -1, c = 2: -0.5 -> 0, not C's -0
    assert block([1, 0, 9, 9], [1, 1, 0, 0]) == (1, 0)           # S = 1, c = 2: 0.5 -> 1
    assert block([1, 2, 2, 2], [1, 1, 1, 0]) == (2, 0)           # S = 5, c = 3: 1.67 -> 2
    assert block([1, 1, 2, 2], [1, 1, 1, 1]) == (2, 0)           # S = 6, c = 4: 1.5 -> 2
    assert block([9, 9, 9, 9], [0, 0, 0, 0]) == (-32768, 0)      # all masked
    assert block([np.nan, np.inf, -np.inf, 51.0], [1, 1, 1, 1]) == (-32768, 0)   # nothing counts
    assert block([2.5, 99, 99, 99], [1, 0, 0, 0]) == (2, 0)      # ties to even in q: rint(2.5) = 2
    assert block([3.5, 99, 99, 99], [1, 0, 0, 0]) == (4, 0)


def test_saturation_both_ways():
    x = np.asarray([[40000.0, 40000.0, -40000.0, -40000.0, 32767.0, -32767.0, 32768.0, -32768.0]], f32).reshape(1, 1, 1, 8)
    z = np.zeros((1, 4, 8), f32)
    b = _ref(x, (1, 1, 8), z, [0], bin=1, step=1.0, vmin=-1e5, vmax=1e5, radius=0, max_peaks=4, min_peaks=0)
    assert b.codes.reshape(-1).tolist() == [32767, 32767, -32767, -32767, 32767, -32767, 32767, -32767]
    assert int(b.nsat[0]) == 6
    b = _ref(x, (1, 1, 8), z, [0], bin=2, step=1.0, vmin=-1e5, vmax=1e5, radius=0, max_peaks=4, min_peaks=0)
    assert b.codes.reshape(-1).tolist() == [32767, -32767, 0, 0] and int(b.nsat[0]) == 2


@pytest.mark.parametrize("step", [1.0, 0.3, 7.0])
def test_to_dense_bound_at_bin_1(step):
    """|to_dense - v| <= step * (0.5 + |v * inv| * 2^-22): v * inv is rounded once (2^-24 relative), rint adds at most
    a half, and float32(code) * step is rounded once more (2^-24 relative of about the same magnitude); 2^-22 covers
    both roundings and the rounding of inv itself with room to spare.  Derived, not measured."""
    rng = np.random.default_rng(3)
    shape = (3, 5, 9)
    x = (rng.normal(size=(2, *shape)) * 3000.0 * step).astype(f32)
    x = np.clip(x, -32000.0 * step, 32000.0 * step).astype(f32)     # no code saturates
    z = np.zeros((2, 4, 8), f32)
    b = _ref(x, shape, z, [0, 0], bin=1, step=step, vmin=-1e6, vmax=1e6, radius=0, max_peaks=4, min_peaks=0)
    assert int(b.nsat.sum()) == 0
    p = reference.validate_roibin_params(bin=1, step=step, vmin=-1e6, vmax=1e6, radius=0, max_peaks=4, min_peaks=0)
    rf = _frames_of(b, shape, p, 2)
    for i in range(2):
        d = rf.to_dense(i).astype(np.float64)
        v = x[i].astype(np.float64)
        bound = float(f32(step)) * (0.5 + np.abs(v * p.inv) * 2.0 ** -22)
        assert bool((np.abs(d - v) <= bound).all())


@pytest.mark.parametrize("shape,B", CASES)
def test_to_dense_is_the_frame_inside_every_box(shape, B):
    x, mask, peaks, counts = make_case(shape, 4, seed=11)
    counts[2] = 0
    kw = dict(bin=B, step=0.25, vmin=-100.0, vmax=100.0, radius=2, max_peaks=8, min_peaks=1)
    b = _ref(x, shape, peaks, counts, mask, **kw)
    rf = _frames_of(b, shape, reference.validate_roibin_params(**kw), 4)
    P, H, W = shape
    xb = x.view(np.uint32)
    for i in range(4):
        if counts[i] < 1:
            with pytest.raises(ValueError, match="skipped"):
                rf.to_dense(i)
            assert rf.boxes(i)[0].size == 0
            continue
        d = rf.to_dense(i).view(np.uint32)
        inside = np.zeros(shape, bool)
        ctr, rec, box = rf.boxes(i)
        assert np.all(np.diff(ctr) >= 0)
        for c in ctr.tolist():
            p, y, xx = c // (H * W), (c // W) % H, c % W
            inside[p, max(y - 2, 0):y + 3, max(xx - 2, 0):xx + 3] = True
        assert inside.any() and np.array_equal(d[inside], xb[i][inside])   # bit for bit, NaN and inf included
        # outside the boxes: the block's code times step, NaN where nothing counted
        codes = rf.frame_codes(i)
        want = np.repeat(np.repeat(codes.astype(f32) * f32(0.25), B, 1), B, 2)[:, :H, :W]
        none = np.repeat(np.repeat(codes == -32768, B, 1), B, 2)[:, :H, :W]
        got = rf.to_dense(i)
        assert np.array_equal(got[~inside & ~none], want[~inside & ~none]) and np.isnan(got[~inside & none]).all()


@pytest.mark.parametrize("kw,msg", [
    (dict(bin=3), "bin"), (dict(bin=2.0), "integers"), (dict(step=0.0), "step"), (dict(step=-1.0), "step"),
    (dict(step=float("nan")), "step"), (dict(step=float("inf")), "step"), (dict(step=1e-46), "step"),
    (dict(vmin=1.0, vmax=0.0), "empty"), (dict(vmin=float("-inf")), "finite"), (dict(vmax=float("nan")), "finite"),
    (dict(vmax=2.0 ** 25), "2\\^25"), (dict(vmin=-2.0 ** 25), "2\\^25"), (dict(vmax=2.0 ** 20, step=2.0 ** -5), "2\\^25"),
    (dict(radius=8), "radius"), (dict(radius=-1), "radius"), (dict(max_peaks=0), "max_peaks"),
    (dict(max_peaks=4097), "max_peaks"), (dict(min_peaks=-1), "min_peaks"), (dict(step="a"), "numbers"),
])
def test_parameter_refusals(kw, msg):
    with pytest.raises(ValueError, match=msg):
        reference.validate_roibin_params(**kw)


def test_input_refusals():
    x = torch.zeros((2, 1, 4, 4))
    pk, ct = torch.zeros((2, 4, 8)), torch.zeros(2, dtype=torch.int32)
    kw = dict(bin=2, max_peaks=4)
    reference.roibin_reference(x, (1, 4, 4), pk, ct, **kw)
    reference.roibin_reference(x, (4, 4), pk, ct, **kw)   # 2-D frames: one panel
    for args, msg in (((x.double(), (1, 4, 4), pk, ct), "float32"), ((x, (1, 4, 5), pk, ct), "elements"),
                      ((x, (1, 4, 4), pk[:, :3], ct), "peaks"), ((x, (1, 4, 4), pk, ct.long()), "counts"),
                      ((x, (1, 4, 4), pk, ct[:1]), "counts"), ((torch.zeros((65, 16)), (1, 4, 4), pk, ct), "frames")):
        with pytest.raises(ValueError, match=msg):
            reference.roibin_reference(*args, **kw)
    with pytest.raises(ValueError, match="mask"):
        reference.roibin_reference(x, (1, 4, 4), pk, ct, mask=np.ones(15, np.uint8), **kw)
    p = reference.validate_roibin_params(**kw)
    assert p.inv == 1.0 and reference.roibin_reference(x, (1, 4, 4), pk, ct, p).codes.shape == (2, 1, 2, 2)
