"""The K-11 golden model (ops.reference.powder_accumulate_reference) against a plain float64 /
Python-int loop, the float64 views of PowderStats against exact rationals, and the run bound."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from psana_ray_amd import powder
from psana_ray_amd.ops import reference

NONE = -2 ** 31


def _loop(x, vmin, vmax, S, thr, keys=None, key_min=0):
    """The contract, one sample at a time: Python ints, float32 comparisons, round-half-even."""
    F, n = x.shape
    nc = 1 if keys is None else 2
    lo, hi, th = np.float32(vmin), np.float32(vmax), np.float32(thr)
    out = {k: [[0] * n for _ in range(nc)] for k in ("cnt", "sum", "sq", "above")}
    out["qmax"] = [[NONE] * n for _ in range(nc)]
    nfr = [0] * nc
    for f in range(F):
        c = 0 if keys is None else int(keys[f] >= key_min)
        nfr[c] += 1
        for p in range(n):
            v = np.float32(x[f, p])
            if not (lo <= v and v <= hi):
                continue
            q = int(round(Fraction(float(v)) * 2 ** S))     # Python's round of a Fraction: ties to even
            out["cnt"][c][p] += 1
            out["sum"][c][p] += q
            out["sq"][c][p] += q * q
            out["qmax"][c][p] = max(out["qmax"][c][p], q)
            out["above"][c][p] += int(v >= th)
    return nfr, out


def _tiny(F, n, seed):
    rng = np.random.default_rng(seed)
    x = (rng.normal(0, 30, size=(F, n))).astype(np.float32)
    x.reshape(-1)[::5] = np.abs(x.reshape(-1)[::5]) * 50
    x.reshape(-1)[3::7] = np.nan
    x.reshape(-1)[4::11] = np.inf
    x.reshape(-1)[6::13] = -np.inf
    x.reshape(-1)[2::17] = -0.0
    ties = np.array([0.125, -0.125, 0.375, -0.375, 0.625, 20.0, np.nextafter(np.float32(20), np.float32(0))], np.float32)
    x[0, :len(ties)] = ties
    return x


@pytest.mark.parametrize("keys, key_min", [(None, 0), ([0, 3, 1, 2, 5, 2], 2), ([7] * 6, 7), ([6] * 6, 7)])
@pytest.mark.parametrize("window", [(-2.0 ** 20, 2.0 ** 20, 2, 20.0), (-8.0, 1024.0, 12, 0.5), (0.0, 100.0, 0, 50.0)])
def test_golden_model_against_a_python_int_loop(keys, key_min, window):
    x = _tiny(6, 23, 1)
    k = None if keys is None else torch.tensor(keys, dtype=torch.int32)
    nfr, cnt, s, sq, qmax, above = reference.powder_accumulate_reference(torch.from_numpy(x), *window, keys=k,
                                                                         key_min=key_min)
    assert (nfr.dtype, cnt.dtype, s.dtype, sq.dtype, qmax.dtype, above.dtype) == (
        torch.int64, torch.int32, torch.int64, torch.int64, torch.int32, torch.int32)
    wn, w = _loop(x, *window, keys=keys, key_min=key_min)
    assert nfr.tolist() == wn
    for got, name in ((cnt, "cnt"), (s, "sum"), (sq, "sq"), (qmax, "qmax"), (above, "above")):
        assert got.tolist() == w[name], name
    assert int(cnt.sum()) > 0


def _stats(x, S=2, vmin=-2.0 ** 20, vmax=2.0 ** 20, thr=20.0):
    nfr, cnt, s, sq, qmax, above = reference.powder_accumulate_reference(torch.from_numpy(x), vmin, vmax, S, thr)
    return powder.PowderStats("tiny", "calib", (x.shape[1],), vmin, vmax, S, thr, 0, {}, nfr.numpy(), cnt.numpy(),
                              s.numpy(), sq.numpy(), above.numpy(), qmax.numpy())


@pytest.mark.parametrize("S", [0, 2, 12])
def test_mean_from_integers_against_float64_mean(S):
    """Each sample is rounded by at most 2^-(S+1) (K-08's bound), so the mean moves by at most that;
    the float64 division and scaling add at most 2^-52 relative -- far inside the 2^-23 |mean| the
    bound leaves for them."""
    rng = np.random.default_rng(2)
    x = rng.normal(5, 40, size=(50, 64)).astype(np.float32)
    st = _stats(x, S=S, vmin=-1000.0, vmax=1000.0)
    want = x.astype(np.float64).mean(axis=0)
    err = np.abs(st.mean(0) - want)
    assert np.all(err <= 2.0 ** -(S + 1) + 2.0 ** -23 * np.abs(want)), err.max()
    assert np.array_equal(st.mean(None), st.mean(0))


def test_rms_max_and_fraction_against_exact_rationals():
    """rms in units of 2^-S against the exact rational variance of the quantised samples: sum and cnt
    convert to float64 exactly here; the two divisions, the square and the subtraction round once each
    on terms no larger than mean^2 + var (as in tests/test_dark_reference.py), the root once more, and
    squaring it back doubles that: at most 8 roundings of 2^-53, so 2^-50 * (mean^2 + var)."""
    rng = np.random.default_rng(3)
    S = 2
    x = rng.normal(100, 25, size=(40, 16)).astype(np.float32)
    x[:, 3] = 7.25                       # stuck: rms exactly 0
    x[:, 4] = np.nan                     # never contributes
    x[::2, 5] = np.nan
    st = _stats(x, S=S)
    q = np.round(x.astype(np.float64) * 2 ** S)
    rms, mx, fa, mean = st.rms(0), st.max(0), st.fraction_above(0), st.mean(0)
    for p in range(16):
        col = [int(v) for v in q[:, p] if np.isfinite(v)]
        if not col:
            assert np.isnan(rms[p]) and np.isnan(mx[p]) and np.isnan(fa[p]) and np.isnan(mean[p])
            continue
        m = Fraction(sum(col), len(col))
        var = Fraction(sum(v * v for v in col), len(col)) - m * m
        got_var = Fraction(float(rms[p]) * 2 ** S) ** 2
        assert abs(got_var - var) <= Fraction(2.0 ** -50) * (m * m + var), p
        assert mx[p] == max(col) / 2 ** S
        assert fa[p] == sum(v >= 20.0 for v in x[:, p] if np.isfinite(v)) / len(col)
    assert rms[3] == 0.0 and mx[3] == 7.25
    # a constant pixel stays exactly 0 where sq no longer converts to float64 exactly
    big = powder.PowderStats("tiny", "calib", (1,), -2.0 ** 20, 2.0 ** 20, 2, 20.0, 0, {}, [400000], [[400000]],
                             [[400000 * 4194303]], [[400000 * 4194303 ** 2]], [[400000]], [[4194303]])
    assert big.rms(0)[0] == 0.0 and big.max(0)[0] == 4194303 / 4


def test_max_frames_and_the_refusals():
    assert reference.powder_max_frames() == 524287
    assert reference.powder_max_frames(-2.0 ** 20, 2.0 ** 20, 2) == 524287 == (2 ** 63 - 1) // 2 ** 44
    assert reference.powder_max_frames(-1024.0, 1024.0, 12) == 524287
    assert reference.powder_max_frames(-1.0, 1.0, 0) == 2 ** 31 - 1          # the int32 count
    assert reference.powder_max_frames(0.0, 0.0, 16) == 2 ** 31 - 1
    assert reference.powder_max_frames(-0.3, 0.2, 0) == 2 ** 31 - 1           # Q = ceil(0.3) = 1
    assert reference.powder_max_frames(-3.0, 2.0 ** 20, 10) == (2 ** 63 - 1) // 2 ** 60 == 7
    for bad in ((1.0, 0.0, 2), (0.0, float("inf"), 2), (float("nan"), 1.0, 2), (0.0, 1.0, 17), (0.0, 1.0, -1),
                (0.0, 2.0 ** 20, 11), (0.0, 1.0, 1.5)):
        with pytest.raises(ValueError):
            reference.powder_max_frames(*bad)
    # one frame more than the bound is refused (7 frames fit at these parameters, 8 do not)
    x = torch.zeros((8, 4), dtype=torch.float32)
    reference.powder_accumulate_reference(x[:7], -3.0, 2.0 ** 20, 10, 1.0)
    with pytest.raises(ValueError, match="more than the 7"):
        reference.powder_accumulate_reference(x, -3.0, 2.0 ** 20, 10, 1.0)
    with pytest.raises(ValueError):
        reference.powder_accumulate_reference(x[:2].to(torch.float64), -3.0, 3.0, 2, 1.0)
    with pytest.raises(ValueError):
        reference.powder_accumulate_reference(x[:2], -3.0, 3.0, 2, 1.0, keys=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match="max_frames"):
        powder.PowderStats("tiny", "calib", (4,), -3.0, 2.0 ** 20, 10, 1.0, 0, {}, [8], np.zeros((1, 4)),
                           np.zeros((1, 4)), np.zeros((1, 4)), np.zeros((1, 4)), np.zeros((1, 4)))
