"""K-16 ROI statistics on the CPU: the golden model against an independent loop oracle word for word, the host
bounds, the rectangle parser and the RoiFrames file (round trip, merge, refusals)."""
import numpy as np
import pytest
import torch

from psana_ray_amd import roi
from psana_ray_amd.ops import reference

from tests._roi_oracle import roi_oracle, rows_as_int64

f32 = np.float32
I32_MIN = -2 ** 31


def _check(x, shape, rects, vmin=-1000.0, vmax=1000.0, S=2, mask=None, proj="both"):
    """Golden model == loop oracle, every word.  Returns the golden rows (numpy int64 [F, R, 8]) and projections."""
    x = np.asarray(x, f32).reshape(-1, int(np.prod(shape)))
    rows, px, py = reference.roi_stats_reference(torch.from_numpy(x), shape, rects, vmin, vmax, S, mask, proj)
    orows, opx, opy = roi_oracle(x, shape, [tuple(r) for r in rects], vmin, vmax, S, mask, proj)
    assert rows.dtype == torch.int64 and tuple(rows.shape) == (x.shape[0], len(rects), 8)
    assert np.array_equal(rows.numpy(), rows_as_int64(orows))
    assert np.array_equal(px.numpy(), np.asarray(opx, np.int64).reshape(x.shape[0], -1))
    assert np.array_equal(py.numpy(), np.asarray(opy, np.int64).reshape(x.shape[0], -1))
    return rows.numpy(), px.numpy(), py.numpy()


def _frames(F, shape, seed, scale=40.0):
    rng = np.random.default_rng(seed)
    # quarters, so that .5 ties of v * 2^S are common at S = 1
    return (np.round(rng.normal(0.0, scale, (F, int(np.prod(shape)))) * 4) / 4).astype(f32)


@pytest.mark.parametrize("W", [12, 13])
def test_every_residue_of_x0_and_x1(W):
    shape = (2, 5, W)
    x = _frames(2, shape, 1)
    rects = [(p, 1, 4, x0, x1) for p, x0, x1 in
             [(0, 0, 1), (0, 1, 6), (0, 2, 7), (0, 3, 8), (1, 0, 4), (1, 4, 9), (1, 5, 11), (1, 3, W), (1, 0, W)]]
    assert {r[3] % 4 for r in rects} == {0, 1, 2, 3} and {r[4] % 4 for r in rects} == {0, 1, 2, 3}
    for S in (0, 1, 2):
        _check(x, shape, rects, -100.0, 100.0, S)


@pytest.mark.parametrize("shape", [(2, 5, 12), (2, 5, 13)])
def test_special_rectangles(shape):
    P, H, W = shape
    x = _frames(3, shape, 2)
    rects = [(0, 2, 3, 5, 6),                       # one pixel
             (1, 0, H, 0, W),                       # a whole panel
             (P - 1, H - 1, H, W - 1, W),           # the last pixel of the last panel
             (0, 1, 4, 2, 9), (0, 1, 4, 2, 9),      # two equal
             (1, 0, 3, 0, 6), (1, 2, 5, 4, 10)]     # two overlapping
    rows, px, py = _check(x, shape, rects, -60.0, 60.0, 2)
    assert np.array_equal(rows[:, 3], rows[:, 4])
    assert px.shape[1] == sum(r[4] - r[3] for r in rects) and py.shape[1] == sum(r[2] - r[1] for r in rects)
    # the one-pixel rectangle: sum == qmax, the index is the pixel's
    q, i = reference.roi_key_decode(rows[:, 0, 4])
    inside = rows[:, 0, 0] == 1
    assert np.array_equal(q[inside], rows[inside, 0, 1]) and set(i[inside]) <= {(0 * H + 2) * W + 5}


def test_2d_frames_are_one_panel():
    x = _frames(2, (5, 12), 3)
    a = reference.roi_stats_reference(torch.from_numpy(x), (5, 12), [(0, 1, 4, 2, 9)], -50, 50, 2, None, "both")
    b = reference.roi_stats_reference(torch.from_numpy(x), (1, 5, 12), [(0, 1, 4, 2, 9)], -50, 50, 2, None, "both")
    assert all(torch.equal(u, v) for u, v in zip(a, b))


def test_values_nan_inf_zero_edges_and_ties():
    shape = (1, 4, 8)
    lo, hi = f32(-10.0), f32(10.0)
    vals = [np.nan, np.inf, -np.inf, -0.0, 0.0, lo, hi, np.nextafter(lo, f32(-np.inf)), np.nextafter(hi, f32(np.inf)),
            np.nextafter(lo, f32(0)), np.nextafter(hi, f32(0)), 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 0.25, 0.75, -0.25, 3.0, 9.75]
    x = np.zeros((1, 32), f32)
    x[0, :len(vals)] = vals
    for S in (0, 1, 2):
        rows, _px, _py = _check(x, shape, [(0, 0, 4, 0, 8)], lo, hi, S)
        assert rows[0, 0, 0] == 32 - 5            # NaN, +-inf and the two values just outside fail
    # S = 0: ties go to even
    rows, px, _py = _check(x[:, 8:16].repeat(4, 0).reshape(1, 32), shape, [(0, 0, 1, 3, 8)], lo, hi, 0, proj="x")
    assert px[0].tolist() == [0, 2, 2, 0, -2]     # 0.5, 1.5, 2.5, -0.5, -1.5


def test_masked_rectangle_has_no_sample():
    shape = (2, 5, 12)
    x = _frames(2, shape, 4)
    mask = np.ones(120, np.uint8)
    m3 = mask.reshape(shape)
    m3[1, 1:3, 2:7] = 0
    m3[0, 0, ::2] = 0
    rows, px, py = _check(x, shape, [(1, 1, 3, 2, 7), (0, 0, 5, 0, 12), (1, 0, 4, 0, 8)], -100, 100, 2, mask)
    assert rows[:, 0].tolist() == [[0] * 8] * 2
    q, i = reference.roi_key_decode(rows[:, 0, 4])
    assert q.tolist() == [I32_MIN] * 2 and i.tolist() == [-1] * 2
    assert not px[:, :5].any() and not py[:, :2].any()
    # a window that nothing reaches
    rows, _px, _py = _check(x, shape, [(0, 0, 5, 0, 12)], 1e6, 2e6, 0)
    assert rows[:, 0].tolist() == [[0] * 8] * 2


def test_ties_of_the_maximum_lowest_index_wins_and_negative_sums():
    shape = (2, 5, 12)
    x = -np.abs(_frames(2, shape, 5)) - 1.0
    x3 = x.reshape(2, 2, 5, 12)
    x3[:, 1, 3, 9] = -0.5
    x3[:, 1, 1, 4] = -0.5
    x3[:, 1, 1, 10] = -0.5       # the same row, later
    x3[:, 0, 4, 11] = -0.5       # not in the rectangle
    rows, _px, _py = _check(x, shape, [(1, 0, 5, 2, 12), (1, 2, 5, 0, 12)], -200, 200, 2)
    q, i = reference.roi_key_decode(rows[:, :, 4])
    assert q.tolist() == [[-2, -2]] * 2
    assert i.tolist() == [[(5 + 1) * 12 + 4, (5 + 3) * 12 + 9]] * 2
    assert (rows[:, :, 1] < 0).all() and (rows[:, :, 2] < 0).all() and (rows[:, :, 3] < 0).all()


def test_key_decode_round_trip():
    q = np.array([-2 ** 31 + 1, -1, 0, 1, 2 ** 31 - 1], np.int64)
    idx = np.array([0, 5, 2 ** 31 - 2, 77, 1], np.int64)
    key = (((q + 2 ** 31).astype(np.uint64) << np.uint64(32)) | (0xFFFFFFFF - idx).astype(np.uint64))
    assert (key != 0).all()
    for k in (key, key.view(np.int64), torch.from_numpy(key.view(np.int64))):
        dq, di = reference.roi_key_decode(k)
        assert dq.dtype == np.int32 and di.dtype == np.int32
        assert np.array_equal(dq, q) and np.array_equal(di, idx)
    dq, di = reference.roi_key_decode(np.zeros(3, np.int64))
    assert dq.tolist() == [I32_MIN] * 3 and di.tolist() == [-1] * 3


def test_bounds_accepted_and_refused():
    big = [(0, 0, 512, 0, 1024)]
    # the default window takes a whole 512 x 1024 Jungfrau panel ...
    lo, hi, S, Q = reference.validate_roi_params(reference.ROI_VMIN, reference.ROI_VMAX, reference.ROI_FRAC_BITS, big)
    assert (lo, hi, S, Q) == (-2.0 ** 20, 2.0 ** 20, 2, 2 ** 22) and Q * 512 * 1024 * 1023 <= 2 ** 63 - 1
    # ... Q < 2^31: 2147483520 = the largest float32 below 2^31 is the last that fits at S = 0
    assert reference.validate_roi_params(-5.0, 2147483520.0, 0)[3] == 2147483520
    with pytest.raises(ValueError, match=r"2\^31"):
        reference.validate_roi_params(-5.0, 2147483648.0, 0)
    with pytest.raises(ValueError, match=r"2\^31"):
        reference.validate_roi_params(-2.0 ** 20, 2.0 ** 20, 11)
    # the moments: Q * area * max(y1 - 1, x1 - 1, 1) <= 2^63 - 1, at the edge
    Q = 2 ** 30
    over = [(0, 0, 2 ** 11, 0, 2 ** 11 + 1)]         # 2^30 * 2^11 * (2^11 + 1) * 2^11 = 2^63 + 2^52
    with pytest.raises(ValueError, match=r"2\^63 - 1"):
        reference.validate_roi_params(-2.0 ** 30, 2.0 ** 30, 0, over)
    fits = [(0, 0, 2 ** 11, 0, 2 ** 11)]             # 2^30 * 2^22 * (2^11 - 1) = 2^63 - 2^52
    assert reference.validate_roi_params(-2.0 ** 30, 2.0 ** 30, 0, fits)[3] == Q
    one = [(0, 0, 1, 0, 1)]                          # the lever of pixel (0, 0) counts as 1
    assert reference.validate_roi_params(-2.0 ** 20, 2.0 ** 20, 10, one)[3] == 2 ** 30
    for bad in ((1.0, 0.0, 2), (0.0, np.inf, 2), (np.nan, 1.0, 2), (0.0, 1.0, 17), (0.0, 1.0, -1), (0.0, 1.0, 1.5)):
        with pytest.raises(ValueError):
            reference.validate_roi_params(*bad)
    with pytest.raises(ValueError, match="proj"):
        reference.validate_roi_proj("z")


def test_rectangles_validated():
    shape = (2, 5, 12)
    ok = reference.validate_roi_rects([(1, 4, 5, 11, 12)] * 16, shape)
    assert ok.dtype == np.int32 and ok.shape == (16, 5)
    for bad in ([], [(0, 0, 1, 0, 1)] * 17, [(2, 0, 1, 0, 1)], [(-1, 0, 1, 0, 1)], [(0, 0, 6, 0, 1)], [(0, 0, 1, 0, 13)],
                [(0, 2, 2, 0, 1)], [(0, 0, 1, 3, 3)], [(0, 3, 2, 0, 1)], [(0, -1, 2, 0, 1)], [(0, 0, 1, 0)],
                [(0.0, 0.0, 1.0, 0.0, 1.0)], "nonsense"):
        with pytest.raises(ValueError):
            reference.validate_roi_rects(bad, shape)
    with pytest.raises(ValueError):
        reference.roi_stats_reference(torch.zeros(1, 120, dtype=torch.float64), shape, [(0, 0, 1, 0, 1)], 0, 1, 0)
    with pytest.raises(ValueError):
        reference.roi_stats_reference(torch.zeros(1, 119), shape, [(0, 0, 1, 0, 1)], 0, 1, 0)


def test_parser():
    P = roi.RoiSet.parse_spec
    assert P("3,10:20,0:384", 3) == (3, 10, 20, 0, 384) and P(" 3 , 10 : 20 , 0:384 ", 3) == (3, 10, 20, 0, 384)
    assert P("10:20,0:384", 2) == (0, 10, 20, 0, 384)
    for bad, nd in (("10:20,0:384", 3), ("3,10:20,0:384", 2), ("3,10:20", 3), ("a,1:2,3:4", 3), ("1,2:3,4", 3),
                    ("1,-2:3,4:5", 3), ("", 2), ("1:2:3,4:5", 2), ("1,2:3,4:5,6", 3), ("1,2:3,4:99999999999", 3)):
        with pytest.raises(ValueError):
            P(bad, nd)
    rs = roi.RoiSet.from_specs(["1,1:3,2:7", "0,0:5,0:12"], (2, 5, 12))
    assert rs.rects.tolist() == [[1, 1, 3, 2, 7], [0, 0, 5, 0, 12]] and rs.R == 2
    assert rs.offx.tolist() == [0, 5, 17] and rs.offy.tolist() == [0, 2, 7]
    assert rs.row_bytes("none") == 128 and rs.row_bytes("x") == 128 + 8 * 17 and rs.row_bytes("both") == 128 + 8 * 24
    assert roi.RoiSet.from_specs(["1:3,2:7"], (5, 12)).rects.tolist() == [[0, 1, 3, 2, 7]]
    assert rs.sha256 == roi.RoiSet(rs.rects, (2, 5, 12)).sha256 != roi.RoiSet(rs.rects[::-1], (2, 5, 12)).sha256
    assert rs.sha256 != roi.RoiSet(rs.rects, (2, 5, 13)).sha256
    for specs, shape in (([], (2, 5, 12)), (["2,0:1,0:1"], (2, 5, 12)), (["0,0:6,0:1"], (2, 5, 12)),
                         (["0,1:1,0:1"], (2, 5, 12)), (["0:1,0:1"], (2, 5, 12)), (["0,0:1,0:1"], (5, 12))):
        with pytest.raises(ValueError):
            roi.RoiSet.from_specs(specs, shape)


def test_rect_files(tmp_path):
    a = np.array([[1, 1, 3, 2, 7], [0, 0, 5, 0, 12]], np.int64)
    np.save(tmp_path / "r5.npy", a)
    np.save(tmp_path / "r4.npy", a[:, 1:].astype(np.int32))
    np.save(tmp_path / "rf.npy", a.astype(np.float64))
    np.save(tmp_path / "r3.npy", a[:, :3])
    assert roi.RoiSet.from_file(tmp_path / "r5.npy", (2, 5, 12)).rects.tolist() == a.tolist()
    assert roi.RoiSet.from_file(tmp_path / "r4.npy", (5, 12)).rects[:, 1:].tolist() == a[:, 1:].tolist()
    for name, shape in (("r4.npy", (2, 5, 12)), ("rf.npy", (2, 5, 12)), ("r3.npy", (2, 5, 12)), ("none.npy", (2, 5, 12)),
                        ("r5.npy", (1, 5, 12))):
        with pytest.raises(ValueError):
            roi.RoiSet.from_file(tmp_path / name, shape)


# ---------------------------------------------------------------------------------------------- RoiFrames
SHAPE = (2, 5, 12)
RECTS = [(1, 1, 3, 2, 7), (0, 0, 5, 0, 12), (1, 0, 4, 3, 4)]


def _roiframes(gevt, proj="both", seed=7, detector="det", shape=SHAPE, rects=RECTS, vmin=-60.0, vmax=60.0, S=2,
               mask=None, layout="calib"):
    gevt = np.asarray(gevt, np.int64)
    n = int(np.prod(shape))
    # a frame's content follows from its gevt alone, so every split of a run sees the same frames
    x = np.stack([_frames(1, shape, 1000 + int(g))[0] for g in gevt]) if len(gevt) else np.zeros((0, n), f32)
    if len(gevt):
        rows, px, py = reference.roi_stats_reference(torch.from_numpy(x), shape, rects, vmin, vmax, S, mask, proj)
        rows, px, py = rows.numpy(), px.numpy(), py.numpy()
    else:
        rows, px, py = np.zeros((0, len(rects), 8), np.int64), None, None
    return roi.RoiFrames.from_rows(detector, layout, shape, vmin, vmax, S, proj, rects, roi.mask_sha256(shape, mask),
                                   rows, px, py, rank=gevt % 3, idx=gevt // 3, gevt=gevt,
                                   photon_energy=np.where(gevt % 2 == 0, 9500.0 + gevt, np.nan))


def _same(a, b):
    assert a.key() == b.key() and np.array_equal(a.rects, b.rects)
    assert np.array_equal(a.offx, b.offx) and np.array_equal(a.offy, b.offy)
    for k in roi.PER_FRAME:
        u, v = a._arr(k), b._arr(k)
        assert u.dtype == v.dtype and u.shape == v.shape and u.tobytes() == v.tobytes(), k


@pytest.mark.parametrize("proj", ["none", "x", "y", "both"])
def test_roiframes_round_trip_is_bitwise(tmp_path, proj):
    st = _roiframes(np.arange(9), proj)
    assert st.proj_x.shape == (9, 18 if proj in ("x", "both") else 0)
    assert st.proj_y.shape == (9, 11 if proj in ("y", "both") else 0)
    p = st.save(tmp_path / "a.npz")
    back = roi.RoiFrames.load(p)
    _same(st, back)
    with np.load(p, allow_pickle=False) as z:
        assert set(z.files) == set(roi._FIELDS)
        assert z["rects"].dtype == np.int32 and z["rects"].shape == (3, 5) and z["offx"].tolist() == [0, 5, 17, 18]
        assert z["npix"].dtype == np.int32 and z["sum"].dtype == np.int64 and z["qmax"].dtype == np.int32
        assert str(z["rects_sha256"]) == st.rects_sha256 and str(z["proj"]) == proj
    # an empty run round-trips too
    _same(_roiframes([], proj), roi.RoiFrames.load(_roiframes([], proj).save(tmp_path / "e.npz")))


def test_roiframes_accessors():
    st = _roiframes(np.arange(5), "both")
    x = np.stack([_frames(1, SHAPE, 1000 + g)[0] for g in range(5)]).reshape(5, *SHAPE)
    raw = x[:, 1, 1:3, 2:7].astype(np.float64)
    ok = np.abs(raw) <= 60                           # the window; quarters, so q * 2^-2 is the value itself
    assert not ok.all() and ok.any(axis=(1, 2)).all()
    sub = np.where(ok, raw, 0.0)
    assert np.array_equal(st.npix[:, 0], ok.sum(axis=(1, 2)))
    assert np.array_equal(st.sum(0), sub.sum(axis=(1, 2)))
    assert np.array_equal(st.mean(0), sub.sum(axis=(1, 2)) / ok.sum(axis=(1, 2)))
    top = np.where(ok, raw, -np.inf).max(axis=(1, 2))
    assert np.array_equal(st.max(0), top)
    am = st.argmax(0)
    assert am.shape == (5, 3) and all(x[f, am[f, 0], am[f, 1], am[f, 2]] == top[f] for f in range(5))
    assert (am[:, 0] == 1).all()
    ys, xs = np.arange(1, 3).reshape(1, 2, 1), np.arange(2, 7).reshape(1, 1, 5)
    com = st.com(0)
    assert np.allclose(com[:, 0], (sub * ys).sum(axis=(1, 2)) / sub.sum(axis=(1, 2)), rtol=1e-12)
    assert np.allclose(com[:, 1], (sub * xs).sum(axis=(1, 2)) / sub.sum(axis=(1, 2)), rtol=1e-12)
    assert np.array_equal(st.projection(0, "x"), sub.sum(axis=1)) and np.array_equal(st.projection(0, "y"), sub.sum(axis=2))
    rp = st.run_projection(0, "x")
    assert rp.dtype == np.int64 and np.array_equal(rp, (sub.sum(axis=1) * 4).sum(axis=0).astype(np.int64))
    with pytest.raises(ValueError):
        st.sum(3)
    with pytest.raises(ValueError):
        _roiframes(np.arange(2), "x").projection(0, "y")
    # no sample: NaN / -1
    em = _roiframes(np.arange(2), "none", vmin=1e6, vmax=2e6, S=0)
    assert np.isnan(em.mean(0)).all() and np.isnan(em.max(0)).all() and np.isnan(em.com(0)).all()
    assert (em.argmax(0) == -1).all() and (em.qmax == I32_MIN).all() and (em.imax == -1).all() and not em.sum(0).any()


def test_merge_equals_one_run_for_any_split(tmp_path):
    gevt = np.arange(23)
    one = _roiframes(gevt, "both")
    rng = np.random.default_rng(0)
    perm = rng.permutation(23)
    parts = [perm[:7], perm[7:8], perm[8:20], perm[20:]]
    paths = [_roiframes(g, "both").save(tmp_path / f"p{i}.npz") for i, g in enumerate(parts)]
    _same(roi.merge(paths), one)
    _same(roi.merge(paths[::-1]), one)
    assert roi.main(["merge", *paths, "--out", str(tmp_path / "m.npz")]) == 0
    _same(roi.RoiFrames.load(tmp_path / "m.npz"), one)


def test_merge_refusals(tmp_path, capsys):
    base = _roiframes(np.arange(4)).save(tmp_path / "base.npz")
    other = {
        "detector": _roiframes(np.arange(4, 8), detector="other"),
        "layout": _roiframes(np.arange(4, 8), layout="image"),
        "shape": _roiframes(np.arange(4, 8), shape=(2, 5, 13)),
        "vmin": _roiframes(np.arange(4, 8), vmin=-61.0),
        "vmax": _roiframes(np.arange(4, 8), vmax=61.0),
        "frac_bits": _roiframes(np.arange(4, 8), S=1),
        "proj": _roiframes(np.arange(4, 8), proj="x"),
        "rects_sha256": _roiframes(np.arange(4, 8), rects=RECTS[::-1]),
        "mask_sha256": _roiframes(np.arange(4, 8), mask=np.arange(120, dtype=np.uint8)),
    }
    for what, st in other.items():
        with pytest.raises(ValueError, match=what):
            roi.merge([base, st.save(tmp_path / f"o_{what}.npz")])
    with pytest.raises(ValueError, match="present twice"):
        roi.merge([base, _roiframes(np.arange(3, 6)).save(tmp_path / "dup.npz")])
    with pytest.raises(ValueError):
        roi.merge([])
    np.savez(tmp_path / "junk.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="not an ROI file"):
        roi.RoiFrames.load(tmp_path / "junk.npz")
    assert roi.main(["merge", str(base), str(tmp_path / "o_proj.npz"), "--out", str(tmp_path / "x.npz")]) == 2
    assert roi.main(["info", str(tmp_path / "junk.npz")]) == 2
    assert roi.main(["export", str(tmp_path / "missing.npz"), "--out_prefix", str(tmp_path / "e")]) == 2
    capsys.readouterr()


def test_info_and_export(tmp_path, capsys):
    import json

    st = _roiframes(np.arange(6), "x")
    p = st.save(tmp_path / "a.npz")
    assert roi.main(["info", p]) == 0
    info = json.loads(capsys.readouterr().out)
    assert info["frames"] == 6 and info["rois"] == 3 and info["proj"] == "x" and info["rects"] == [list(r) for r in RECTS]
    assert info["row_bytes"] == 3 * 64 + 8 * 18
    assert roi.main(["export", p, "--out_prefix", str(tmp_path / "run")]) == 0
    assert np.array_equal(np.load(tmp_path / "run_sum.npy"), np.stack([st.sum(r) for r in range(3)], axis=1))
    assert np.array_equal(np.load(tmp_path / "run_com.npy"), np.stack([st.com(r) for r in range(3)], axis=1), equal_nan=True)
    for r in range(3):
        assert np.array_equal(np.load(tmp_path / f"run_proj_x_r{r}.npy"), st.projection(r, "x"))
    assert not (tmp_path / "run_proj_y_r0.npy").exists()
