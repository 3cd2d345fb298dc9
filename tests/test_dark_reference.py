"""K-09 golden model (ops.reference.dark_accumulate_reference) against a brute-force Python-int loop,
DarkStats' float64 moments against exact rationals, and derive_constants on hand-built accumulators."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from psana_ray_amd import dark
from psana_ray_amd.models import CalibConstants, get_detector
from psana_ray_amd.ops import reference

NC = {0: 2, 1: 3, 2: 1}


def _u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.uint16)


def _brute(x, kind, lo, hi):
    """The issue's decode table, sample by sample, in Python integers."""
    F, n = x.shape
    cnt = [[0] * n for _ in range(NC[kind])]
    s = [[0] * n for _ in range(NC[kind])]
    q = [[0] * n for _ in range(NC[kind])]
    for f in range(F):
        for p in range(n):
            r = int(x[f, p])
            if kind == 0:
                adu, c, valid = r & 0x3FFF, (r >> 14) & 1, True
            elif kind == 1:
                gb = r >> 14
                adu, c, valid = r & 0x3FFF, {0: 0, 1: 1, 3: 2}.get(gb, -1), gb != 2
            else:
                adu, c, valid = r, 0, True
            if valid and lo <= adu <= hi:
                cnt[c][p] += 1
                s[c][p] += adu
                q[c][p] += adu * adu
    return np.array(cnt, np.int64), np.array(s, np.int64), np.array(q, np.int64)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_golden_model_equals_brute_force(kind):
    rng = np.random.default_rng(20 + kind)
    F, n = 9, 300
    lo, hi = (1000, 9000) if kind != 2 else (1000, 65535)
    top = 16384 if kind != 2 else 65536
    x = rng.integers(0, top, size=(F, n), dtype=np.int64)
    edge = np.array([lo - 1, lo, hi, hi + 1 if hi < 65535 else 65535, 0, top - 1], np.int64)
    x[:, :60] = edge[rng.integers(0, edge.size, size=(F, 60))]      # the window's ends, inside and outside
    if kind == 2:
        x[:, 60:70] = 65535
    else:
        x |= rng.integers(0, 4, size=(F, n), dtype=np.int64) << 14     # every gain-bit pattern: jungfrau gb == 2,
        assert ((x >> 14) == 2).any() and ((x >> 15) == 1).any()        # epix bit 15 set
    x = x.astype(np.uint16)
    cnt, s, q = reference.dark_accumulate_reference(_u16(x), kind, lo, hi)
    bc, bs, bq = _brute(x, kind, lo, hi)
    assert cnt.dtype == torch.int32 and s.dtype == torch.int64 and q.dtype == torch.int64
    assert cnt.shape == (NC[kind], n)
    assert np.array_equal(cnt.numpy(), bc) and np.array_equal(s.numpy(), bs) and np.array_equal(q.numpy(), bq)
    if kind == 2:
        assert int(q.max()) == F * 65535 ** 2
    # frames of any layout, and a split batch adds up to the whole
    a = reference.dark_accumulate_reference(_u16(x[:4]).reshape(4, 3, 10, 10), kind, lo, hi)
    b = reference.dark_accumulate_reference(_u16(x[4:]), kind, lo, hi)
    assert torch.equal(a[0] + b[0], cnt) and torch.equal(a[1] + b[1], s) and torch.equal(a[2] + b[2], q)


def test_golden_model_window_ends_one_by_one():
    lo, hi = 100, 200
    x = np.array([[lo - 1, lo, hi, hi + 1, 0x8000 | lo, 0x4000 | hi, 0xC000 | (hi + 1)]], np.uint16)
    cnt, s, q = reference.dark_accumulate_reference(_u16(x), 0, lo, hi)
    assert cnt.tolist() == [[0, 1, 1, 0, 1, 0, 0], [0, 0, 0, 0, 0, 1, 0]]       # epix: bit 15 ignored, bit 14 -> c 1
    assert s.tolist() == [[0, lo, hi, 0, lo, 0, 0], [0, 0, 0, 0, 0, hi, 0]]
    cnt, s, q = reference.dark_accumulate_reference(_u16(x), 1, lo, hi)
    assert cnt.tolist() == [[0, 1, 1, 0, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0], [0] * 7]   # jungfrau: 0x8000 is gb 2
    cnt, s, q = reference.dark_accumulate_reference(_u16(np.array([[65535, 65534, 0]], np.uint16)), 2, 0, 65535)
    assert cnt.tolist() == [[1, 1, 1]] and q.tolist() == [[65535 ** 2, 65534 ** 2, 0]]


def test_golden_model_refuses_bad_arguments():
    x = _u16(np.zeros((1, 8), np.uint16))
    for kind, lo, hi in ((3, 0, 1), (0, 5, 4), (0, 0, 65536), (0, -1, 5)):
        with pytest.raises(ValueError):
            reference.dark_accumulate_reference(x, kind, lo, hi)
    with pytest.raises(ValueError):
        reference.dark_accumulate_reference(torch.zeros((1, 8), dtype=torch.float32), 0, 0, 5)


def test_rms_and_mean_against_exact_rationals():
    """variance() is within the documented cancellation bound, VARIANCE_BOUND * (mean^2 + var), of the
    exact rational variance -- also at the largest ADU, where the cancellation is worst."""
    rng = np.random.default_rng(5)
    n, F = 200, 500
    base = np.concatenate([rng.integers(0, 65536, size=n - 4), [65535, 65535, 0, 16383]])
    x = np.clip(base[None, :] + np.rint(rng.normal(0, 3.0, size=(F, n))).astype(np.int64), 0, 65535)
    x[:, n - 4] = 65535                                   # constant at the top: variance exactly 0
    x[:, 7] = 65535 - (np.arange(F) % 2)                  # +-0.5 around 65534.5
    cnt, s, q = reference.dark_accumulate_reference(_u16(x.astype(np.uint16)), 2, 0, 65535)
    st = dark.DarkStats("tiny_plain", 2, 0, 65535, F, cnt.numpy(), s.numpy(), q.numpy())
    mean, var, rms = st.mean()[0], st.variance()[0], st.rms()[0]
    assert mean.dtype == np.float64 and rms.dtype == np.float64
    worst = 0.0
    for p in range(n):
        c, ss, qq = int(st.cnt[0, p]), int(st.sum[0, p]), int(st.sq[0, p])
        m = Fraction(ss, c)
        v = Fraction(qq, c) - m * m
        assert abs(Fraction(mean[p]) - m) <= Fraction(2.0 ** -52) * m
        bound = Fraction(dark.VARIANCE_BOUND) * (m * m + v)
        assert abs(Fraction(var[p]) - v) <= bound, (p, float(v), var[p])
        assert abs(rms[p] - float(v) ** 0.5) <= 1e-12 + float(bound) / max(2 * float(v) ** 0.5, 1e-3)
        worst = max(worst, float(bound))
    assert var[n - 4] == 0.0 and abs(var[7] - 0.25) <= 4e-6
    assert worst < 4e-6                                    # 2^-50 * 65535^2 = 3.8e-6 ADU^2
    # no sample: NaN
    st0 = dark.DarkStats("tiny_plain", 2, 0, 65535, 0, np.zeros((1, 3)), np.zeros((1, 3)), np.zeros((1, 3)))
    assert np.isnan(st0.mean()).all() and np.isnan(st0.rms()).all()


def test_save_load_merge_exact(tmp_path):
    rng = np.random.default_rng(6)
    x = (rng.integers(0, 16384, size=(10, 64)) | (rng.integers(0, 4, size=(10, 64)) << 14)).astype(np.uint16)
    parts = []
    for i, sl in enumerate((slice(0, 3), slice(3, 10))):
        c, s, q = reference.dark_accumulate_reference(_u16(x[sl]), 1, 10, 16000)
        st = dark.DarkStats("tiny_jungfrau", 1, 10, 16000, sl.stop - sl.start, c.numpy(), s.numpy(), q.numpy())
        parts.append(st.save(tmp_path / f"p{i}.npz"))
    back = dark.DarkStats.load(parts[0])
    assert back.cnt.dtype == np.int64 and back.frames == 3 and back.detector == "tiny_jungfrau"
    m = dark.merge(parts)
    c, s, q = reference.dark_accumulate_reference(_u16(x), 1, 10, 16000)
    assert m.frames == 10 and np.array_equal(m.cnt, c.numpy()) and np.array_equal(m.sum, s.numpy())
    assert np.array_equal(m.sq, q.numpy())
    with np.load(parts[0], allow_pickle=False) as z:      # loads without pickle
        assert str(z["detector"]) == "tiny_jungfrau"
    for other in (dark.DarkStats("tiny_epix", 1, 10, 16000, 1, c.numpy(), s.numpy(), q.numpy()),
                  dark.DarkStats("tiny_jungfrau", 1, 11, 16000, 1, c.numpy(), s.numpy(), q.numpy()),
                  dark.DarkStats("tiny_jungfrau", 1, 10, 16001, 1, c.numpy(), s.numpy(), q.numpy()),
                  dark.DarkStats("tiny_jungfrau", 0, 10, 16000, 1, c.numpy()[:2], s.numpy()[:2], q.numpy()[:2])):
        with pytest.raises(ValueError):
            dark.merge([parts[0], other.save(tmp_path / "other.npz")])


def _flat_stats(spec, kind, frames, level, cand=0):
    """Accumulators in which EVERY pixel of candidate ``cand`` saw ``frames`` samples, half of them
    level - 2 and half level + 2: mean = level and rms = 2 exactly, at every pixel."""
    nc, n = NC[kind], spec.npix
    cnt = np.zeros((nc, n), np.int64)
    s = np.zeros((nc, n), np.int64)
    q = np.zeros((nc, n), np.int64)
    cnt[cand] = frames
    s[cand] = frames * level
    q[cand] = frames // 2 * ((level - 2) ** 2 + (level + 2) ** 2)
    return cnt, s, q


def test_derive_constants_planted_pixels_epix():
    spec = get_detector("tiny_epix")
    base = CalibConstants.random(spec, seed=3, gain_config="FL")       # NOT the configuration of the dark run
    F, level = 100, 2400
    cnt, s, q = _flat_stats(spec, 0, F, level)
    STUCK, NOISY, OFFSET, STARVED = 5, 77, 1000, 3071
    q[0, STUCK] = F * level ** 2                                          # every sample == level: rms 0
    q[0, NOISY] = F // 2 * ((level - 40) ** 2 + (level + 40) ** 2)        # rms 40
    s[0, OFFSET] = F * (level + 900)                                      # mean + 900, the same rms 2
    q[0, OFFSET] = F // 2 * ((level + 898) ** 2 + (level + 902) ** 2)
    cnt[0, STARVED], s[0, STARVED] = 4, 4 * 7000                          # 4 samples, and a wild mean: only "starved"
    q[0, STARVED] = 4 * 7000 ** 2
    st = dark.DarkStats(spec.name, 0, 0, 16383, F, cnt, s, q)
    assert np.all(st.rms()[0][[1, 2, 3]] == 2.0) and st.rms()[0][STUCK] == 0.0
    consts, rep = dark.derive_constants([st], base, gain_config="AHL", min_frames=50)
    status = consts.status.reshape(-1)
    assert status.dtype == np.uint8 and consts.status.shape == spec.frame_shape
    want = np.zeros(spec.npix, np.uint8)
    want[STUCK], want[NOISY], want[OFFSET], want[STARVED] = 2, 1, 4, 8
    assert np.array_equal(status, want)                                   # every planted pixel exactly its bit, no other
    # AHL: candidate 0 is gain range 3; candidate 1 (range 5) was never hit -> not covered
    assert rep["covered"] == [3]
    assert rep["ranges"][3]["median_mean"] == level and rep["ranges"][3]["median_rms"] == 2.0
    assert rep["flagged"] == {1: 1, 2: 1, 4: 1, 8: 1} and rep["bad_pixels"] == 4
    ped = consts.pedestals.reshape(spec.n_gains, -1)
    bped = base.pedestals.reshape(spec.n_gains, -1)
    good = np.ones(spec.npix, bool)
    good[[STUCK, NOISY, OFFSET, STARVED]] = False
    assert ped.dtype == np.float32 and np.all(ped[3, good] == np.float32(level))
    assert ped[3, OFFSET] == np.float32(level + 900) and ped[3, STUCK] == np.float32(level)
    assert ped[3, STARVED].view(np.int32) == bped[3, STARVED].view(np.int32)      # too few samples: base value
    for g in (0, 1, 2, 4, 5, 6):                                                   # uncovered ranges: bitwise the base
        assert np.array_equal(ped[g].view(np.int32), bped[g].view(np.int32))
    assert np.array_equal(consts.gains.view(np.int32), base.gains.view(np.int32))
    assert np.array_equal(consts.gain_config, base.gain_config) and tuple(consts.cm_gains) == tuple(base.cm_gains)
    assert consts.gains is not base.gains
    # the base status enters only on request
    c2, _ = dark.derive_constants(st, base, gain_config="AHL", min_frames=50, include_base_status=True)
    assert np.array_equal(c2.status.reshape(-1), want | base.status.reshape(-1)) and base.status.any()
    # absolute limits replace the robust ones
    c3, r3 = dark.derive_constants(st, base, gain_config="AHL", min_frames=50, rms_hi=100.0, rms_lo=1.0,
                                   mean_lo=0.0, mean_hi=16383.0)
    w3 = np.zeros(spec.npix, np.uint8)
    w3[STUCK], w3[STARVED] = 2, 8
    assert np.array_equal(c3.status.reshape(-1), w3) and r3["ranges"][3]["limits"]["rms_hi"] == 100.0
    # an epix dark run needs its configuration; a wrong detector is refused
    with pytest.raises(ValueError):
        dark.derive_constants(st, base)
    with pytest.raises(ValueError):
        dark.derive_constants(st, CalibConstants.random(get_detector("tiny_jungfrau"), seed=1))


def test_derive_constants_two_runs_fill_their_ranges_and_per_pixel_config():
    spec = get_detector("tiny_epix")
    base = CalibConstants.random(spec, seed=4)
    a = dark.DarkStats(spec.name, 0, 0, 16383, 60, *_flat_stats(spec, 0, 60, 2500))          # FH: range 0
    b = dark.DarkStats(spec.name, 0, 0, 16383, 80, *_flat_stats(spec, 0, 80, 1800, cand=1))  # AML, switched: range 6
    consts, rep = dark.derive_constants([a, b], base, gain_config=["FH", "AML"], min_frames=50)
    assert rep["covered"] == [0, 6] and not consts.status.any()
    assert np.all(consts.pedestals[0] == np.float32(2500)) and np.all(consts.pedestals[6] == np.float32(1800))
    for g in (1, 2, 3, 4, 5):
        assert np.array_equal(consts.pedestals[g].view(np.int32), base.pedestals[g].view(np.int32))
    # per-pixel configuration: the first half FM (range 1), the second half FL (range 2)
    cfg = np.where(np.arange(spec.npix) < spec.npix // 2, 1, 2).astype(np.uint8)
    consts, rep = dark.derive_constants(a, base, gain_config=cfg.reshape(spec.frame_shape), min_frames=50)
    assert rep["covered"] == [1, 2] and rep["ranges"][1]["pixels"] == spec.npix // 2
    p = consts.pedestals.reshape(spec.n_gains, -1)
    bp = base.pedestals.reshape(spec.n_gains, -1)
    h = spec.npix // 2
    assert np.all(p[1, :h] == np.float32(2500)) and np.array_equal(p[1, h:].view(np.int32), bp[1, h:].view(np.int32))
    assert np.all(p[2, h:] == np.float32(2500)) and np.array_equal(p[2, :h].view(np.int32), bp[2, :h].view(np.int32))
    assert not consts.status.any()


def test_derive_constants_jungfrau_uses_candidates_directly():
    spec = get_detector("tiny_jungfrau")
    base = CalibConstants.random(spec, seed=5)
    cnt, s, q = _flat_stats(spec, 1, 64, 3000)
    c1, s1, q1 = _flat_stats(spec, 1, 64, 14000, cand=1)
    st = dark.DarkStats(spec.name, 1, 0, 16383, 128, cnt + c1, s + s1, q + q1)
    consts, rep = dark.derive_constants(st, base, gain_config="ignored for jungfrau", min_frames=50)
    assert rep["covered"] == [0, 1]
    assert np.all(consts.pedestals[0] == np.float32(3000)) and np.all(consts.pedestals[1] == np.float32(14000))
    assert np.array_equal(consts.pedestals[2].view(np.int32), base.pedestals[2].view(np.int32))
    assert consts.gain_config is None and not consts.status.any()
