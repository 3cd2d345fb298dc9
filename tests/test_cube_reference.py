"""The K-15 golden model against K-11's (an independent, already-tested model) and a Python-integer oracle;
the bin assignment; the CubeStats file, its float64 views and ``merge``."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from psana_ray_amd import cube
from psana_ray_amd.ops import reference

from tests._cube_oracle import cube_oracle

ARRAYS = ("frames", "cnt", "sum", "sq")


def _frames(shape, seed, scale=30.0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * scale
    flat = x.reshape(-1)
    flat[::17] = flat[::17].abs() * 40.0 + 20.0
    flat[5::29] = float("nan")
    flat[7::31] = float("inf")
    flat[11::37] = -0.0
    flat[13::41] = 2.625          # a tie at S = 2
    return x.contiguous()


@pytest.mark.parametrize("params", [(-2.0 ** 20, 2.0 ** 20, 2), (-8.0, 1024.0, 12), (-1.0, 1.0, 0)])
def test_every_bin_equals_the_powder_model_of_its_frames(params):
    F, n, B = 23, 200, 6
    x = _frames((F, n), 1)
    bins = [(f * 5) % (B + 1) - 1 for f in range(F)]          # -1 .. B - 1; bin 4 below is emptied
    bins = [-1 if b == 4 else b for b in bins]
    nfr, cnt, s, sq = reference.cube_accumulate_reference(x, bins, B, *params)
    assert nfr.dtype == torch.int64 and cnt.dtype == torch.int32 and s.dtype == torch.int64 and sq.dtype == torch.int64
    assert nfr.shape == (B,) and cnt.shape == s.shape == sq.shape == (B, n)
    assert int(nfr.sum()) == sum(b >= 0 for b in bins) < F
    for b in range(B):
        sel = [f for f in range(F) if bins[f] == b]
        if not sel:
            assert b == 4 and int(nfr[b]) == 0 and not cnt[b].any() and not s[b].any() and not sq[b].any()
            continue
        pn, pc, ps, pq, _m, _a = reference.powder_accumulate_reference(x[sel], *params, 0.0)
        assert int(pn[0]) == int(nfr[b]) == len(sel)
        assert torch.equal(pc[0], cnt[b]) and torch.equal(ps[0], s[b]) and torch.equal(pq[0], sq[b])


def test_python_integer_oracle_on_tiny_inputs():
    vals = [float("nan"), float("inf"), float("-inf"), -0.0, 0.0, -40.0, 60.0, float(np.nextafter(np.float32(60), np.float32(100))),
            float(np.nextafter(np.float32(-40), np.float32(-100))), 0.125, 0.375, -0.125, -0.375, 2.5625, 59.9375, -39.9375,
            17.3, -5.55]
    vals = [float(np.float32(v)) for v in vals]
    F, n, B = 7, len(vals), 4
    rows = [[vals[(p + 3 * f) % n] for p in range(n)] for f in range(F)]
    x = torch.tensor(rows, dtype=torch.float32)
    for bins in ([0, 3, -1, 3, 1, 0, 3], [2] * F, [-1] * F, [0, 1, 2, 3, -1, -1, -1]):
        got = reference.cube_accumulate_reference(x, bins, B, -40.0, 60.0, 3)
        want = cube_oracle(rows, bins, B, -40.0, 60.0, 3)
        for g, w in zip(got, want):
            assert g.tolist() == w
    # an all-dropped batch adds nothing; a dropped frame's content never matters
    assert all(not t.any() for t in reference.cube_accumulate_reference(x, [-1] * F, B, -40.0, 60.0, 3))
    y = x.clone()
    y[2] = float("nan")
    a = reference.cube_accumulate_reference(x, [0, 3, -1, 3, 1, 0, 3], B, -40.0, 60.0, 3)
    b = reference.cube_accumulate_reference(y, [0, 3, -1, 3, 1, 0, 3], B, -40.0, 60.0, 3)
    assert all(torch.equal(p, q) for p, q in zip(a, b))


def test_reference_refusals():
    x = torch.zeros((3, 8))
    for kw in (dict(bins=[0, 0]), dict(bins=[0, 0, 2]), dict(bins=[0, -2, 0]), dict(bins=[0.0, 1.0, 1.0]),
               dict(nbins=0), dict(nbins=4097), dict(vmin=1.0, vmax=0.0), dict(frac_bits=17),
               dict(vmax=2.0 ** 20, frac_bits=11), dict(x=x.to(torch.float64)), dict(x=torch.zeros((0, 8)), bins=[])):
        with pytest.raises(ValueError):
            reference.cube_accumulate_reference(kw.get("x", x), kw.get("bins", [0, 1, 1]), kw.get("nbins", 2),
                                                kw.get("vmin", -1.0), kw.get("vmax", 1.0), kw.get("frac_bits", 2))
    reference.cube_accumulate_reference(x, np.array([0, 1, -1], np.int16), 4096, -1.0, 1.0, 2)


# ---------------------------------------------------------------------------------------- bin assignment
def test_bin_of_photon_energy_at_every_edge():
    for edges in (np.linspace(9000.0, 9100.0, 8), np.array([-3.5, -1.0, 0.0, 1e-3, 7.0, 7.5])):
        bg = cube.CubeBinning("photon_energy", edges=edges)
        B = edges.size - 1
        assert bg.nbins == B and bg.edges.dtype == np.float64 and bg.table_sha256 == ""
        for i, e in enumerate(edges):
            below, above = np.nextafter(e, -np.inf), np.nextafter(e, np.inf)
            got = bg.bin_of([below, e, above]).tolist()
            want = [i - 1, min(i, B - 1), i if i < B else -1]       # pe == edges[B] goes to B - 1
            assert got == want, (i, got, want)
        out = bg.bin_of([None, float("nan"), float("inf"), float("-inf"), edges[0] - 1.0, edges[B] + 1.0])
        assert out.dtype == np.int32 and out.tolist() == [-1] * 6
        assert cube.bin_of([edges[1]], edges=edges).tolist() == [1]
        assert bg.bin_of([]).shape == (0,)


def test_edges_refused_and_linspace_kept_bitwise():
    for bad in ([1.0, 1.0, 2.0], [3.0, 2.0], [1.0], [0.0, float("nan")], [0.0, float("inf")], [[0.0, 1.0]],
                np.arange(4098.0)):
        with pytest.raises(ValueError):
            cube.CubeBinning("photon_energy", edges=bad)
    with pytest.raises(ValueError):
        cube.CubeBinning("photon_energy")
    with pytest.raises(ValueError):
        cube.CubeBinning("energy", edges=[0.0, 1.0])
    with pytest.raises(ValueError):
        cube.CubeBinning("photon_energy", edges=[0.0, 1.0], table=np.zeros(3, np.int64))
    bg = cube.CubeBinning.linspace(8995.3, 9104.7, 7)
    assert bg.edges.tobytes() == np.linspace(8995.3, 9104.7, 8).tobytes()


def test_bin_of_gevt_table():
    table = np.array([3, -1, 0, 0, 2], np.int32)
    bg = cube.CubeBinning("gevt", table=table)
    assert bg.nbins == 4 and bg.edges.size == 0 and len(bg.table_sha256) == 64
    got = bg.bin_of([0, 1, 2, 3, 4, 5, -1, 10 ** 12])
    assert got.dtype == np.int32 and got.tolist() == [3, -1, 0, 0, 2, -1, -1, -1]
    assert cube.CubeBinning("gevt", table=table, nbins=9).nbins == 9
    assert cube.CubeBinning("gevt", table=table.astype(np.int64)).table_sha256 == bg.table_sha256
    assert cube.CubeBinning("gevt", table=table[::-1].copy()).table_sha256 != bg.table_sha256
    assert bg.bin_of_meta([(0, 7, 4, 9000.0), (0, 8, 1, None)]).tolist() == [2, -1]
    for bad in (dict(table=table, nbins=3), dict(table=np.array([0, -2])), dict(table=np.array([0.0, 1.0])),
                dict(table=np.zeros((2, 2), np.int64)), dict(table=np.zeros(0, np.int64)), dict(table=None),
                dict(table=np.array([-1, -1])), dict(table=np.array([4096])), dict(table=table, edges=[0.0, 1.0])):
        with pytest.raises(ValueError):
            cube.CubeBinning("gevt", **bad)


# ---------------------------------------------------------------------------------------- CubeStats
def _run(n_frames=17, shape=(2, 3, 4), seed=3, by="photon_energy", **kw):
    """A small run through the golden model as a CubeStats, and its frames / energies."""
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.integers(-40, 90, size=(n_frames, n)).astype(np.float32) / 4)
    x[:, 5] = 2.75                  # equal samples
    x[:, 6] = float("nan")          # never a sample
    pe = [None if g % 5 == 4 else 9000.0 + 6.5 * g + float(rng.random()) for g in range(n_frames)]
    gevt = list(range(100, 100 + n_frames))
    if by == "photon_energy":
        bg = cube.CubeBinning.linspace(9010.0, 9090.0, 4)
        bins = bg.bin_of(pe)
    else:
        bg = cube.CubeBinning("gevt", table=np.array([-1] * 100 + [g % 3 for g in range(n_frames - 2)]))
        bins = bg.bin_of(gevt)
    vmin, vmax, S = kw.get("vmin", -8.0), kw.get("vmax", 100.0), kw.get("S", 3)
    nfr, cnt, s, sq = reference.cube_accumulate_reference(x, bins, bg.nbins, vmin, vmax, S)
    st = cube.CubeStats(kw.get("detector", "tiny"), kw.get("layout", "calib"), shape, vmin, vmax, S, bg.by, bg.nbins,
                        bg.edges, bg.table_sha256, nfr.numpy(), int((bins < 0).sum()), cnt.numpy(), s.numpy(),
                        sq.numpy(), rank=[0] * n_frames, idx=list(range(n_frames)), gevt=gevt,
                        photon_energy=[np.nan if e is None else e for e in pe], bin=bins)
    return st, x, pe, bins


def _part(st, x, pe, bins, sel):
    """The CubeStats one consumer would have written over the frames ``sel`` of the run."""
    sel = list(sel)
    nfr, cnt, s, sq = reference.cube_accumulate_reference(x[sel], bins[sel], st.nbins, st.vmin, st.vmax, st.frac_bits)
    return cube.CubeStats(st.detector, st.layout, st.shape, st.vmin, st.vmax, st.frac_bits, st.by, st.nbins, st.edges,
                          st.table_sha256, nfr.numpy(), int((bins[sel] < 0).sum()), cnt.numpy(), s.numpy(), sq.numpy(),
                          rank=st.rank[sel], idx=st.idx[sel], gevt=st.gevt[sel], photon_energy=st.photon_energy[sel],
                          bin=st.bin[sel])


def _same_files(a, b):
    assert a.key() == b.key() and a.dropped == b.dropped
    for k in (*ARRAYS, *cube.PER_FRAME, "edges"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape, k
        assert x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("by", ["photon_energy", "gevt"])
def test_save_load_round_trip(tmp_path, by):
    st, _x, _pe, bins = _run(by=by)
    assert -1 in bins.tolist() and int(st.frames.sum()) + st.dropped == 17
    path = st.save(tmp_path / "a.npz")
    _same_files(cube.CubeStats.load(path), st)
    with np.load(path, allow_pickle=False) as z:                 # plain arrays only: loads without pickle
        assert str(z["format"]) == cube.CUBE_FORMAT and str(z["by"]) == by
        assert z["cnt"].dtype == np.int32 and z["sum"].dtype == np.int64 and z["sq"].dtype == np.int64
        assert z["frames"].dtype == np.int64 and z["frames"].shape == (st.nbins,) and z["dropped"].dtype == np.int64
        assert z["bin"].dtype == np.int16 and z["photon_energy"].dtype == np.float64 and z["gevt"].dtype == np.int64
        assert z["rank"].dtype == np.int64 and z["idx"].dtype == np.int64 and z["bin"].shape == (17,)
        assert (z["edges"].size == st.nbins + 1) == (by == "photon_energy")
        assert (len(str(z["table_sha256"])) == 64) == (by == "gevt")
    np.savez(tmp_path / "x.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="not a cube file"):
        cube.CubeStats.load(tmp_path / "x.npz")
    with pytest.raises(ValueError):                                # rows that do not add up to the frames
        cube.CubeStats(st.detector, st.layout, st.shape, st.vmin, st.vmax, st.frac_bits, st.by, st.nbins, st.edges,
                       st.table_sha256, st.frames + 1, st.dropped, st.cnt, st.sum, st.sq, rank=st.rank, idx=st.idx,
                       gevt=st.gevt, photon_energy=st.photon_energy, bin=st.bin)
    with pytest.raises(ValueError):
        cube.CubeStats(st.detector, st.layout, st.shape, st.vmin, st.vmax, st.frac_bits, st.by, st.nbins, st.edges,
                       st.table_sha256, st.frames, st.dropped, st.cnt[:, :-1], st.sum, st.sq, rank=st.rank, idx=st.idx,
                       gevt=st.gevt, photon_energy=st.photon_energy, bin=st.bin)


def test_mean_rms_diff_against_exact_rationals():
    st, x, _pe, bins = _run()
    S = st.frac_bits
    xs = x.numpy()
    for b in range(st.nbins):
        sel = [f for f in range(x.shape[0]) if bins[f] == b]
        mean, rms = st.mean(b), st.rms(b)
        assert mean.dtype == np.float64 and mean.shape == (st.n,)
        for p in range(st.n):
            q = [Fraction(float(v)) * 2 ** S for v in xs[sel, p] if st.vmin <= v <= st.vmax]
            assert all(v.denominator == 1 for v in q)               # quarters at S = 3: q is exact
            if not q:
                assert np.isnan(mean[p]) and np.isnan(rms[p])
                continue
            m = sum(q) / len(q)
            var = sum(v * v for v in q) / len(q) - m * m
            assert mean[p] == pytest.approx(float(m / 2 ** S), rel=1e-15, abs=0)
            if var == 0:
                assert rms[p] == 0.0
            else:
                assert rms[p] == pytest.approx(float(var) ** 0.5 / 2 ** S, rel=1e-9)
        assert rms[5] == 0.0 and mean[5] == 2.75 and np.isnan(mean[6])
    d = st.diff(1, 0)
    assert np.array_equal(d, st.mean(1) - st.mean(0), equal_nan=True) and d[5] == 0.0
    with pytest.raises(ValueError):
        st.mean(st.nbins)
    with pytest.raises(ValueError):
        st.diff(0, -1)


@pytest.mark.parametrize("by", ["photon_energy", "gevt"])
def test_merge_of_a_split_run_is_the_unsplit_run_in_any_file_order(tmp_path, by):
    st, x, pe, bins = _run(by=by)
    F = x.shape[0]
    whole = st.save(tmp_path / "whole.npz")
    parts = [list(range(0, F, 3)), list(range(1, F, 3)), list(range(2, F, 3))]
    files = [_part(st, x, pe, bins, sel).save(tmp_path / f"p{k}.npz") for k, sel in enumerate(parts)]
    want = cube.merge([whole])
    _same_files(want, st)                                           # one consumer's rows are in gevt order already
    for order in ([0, 1, 2], [2, 0, 1], [1, 2, 0]):
        m = cube.merge([files[k] for k in order])
        _same_files(m, st)
        assert m.mean_energy().tobytes() == st.mean_energy().tobytes()
    me = st.mean_energy()
    for b in range(st.nbins):
        v = [Fraction(e) for e, bb in zip(pe, bins) if bb == b and e is not None]
        if v:
            assert me[b] == pytest.approx(float(sum(v) / len(v)), rel=1e-15)
        else:
            assert np.isnan(me[b])
    out = str(tmp_path / "merged.npz")
    assert cube.main(["merge", *files, "--out", out]) == 0
    _same_files(cube.CubeStats.load(out), st)


def test_merge_refusals(tmp_path):
    st, x, pe, bins = _run()
    a = _part(st, x, pe, bins, range(0, 9)).save(tmp_path / "a.npz")
    b = _part(st, x, pe, bins, range(9, 17)).save(tmp_path / "b.npz")
    cube.merge([a, b])
    others = [dict(detector="other"), dict(layout="image"), dict(shape=(2, 4, 3)), dict(vmin=-7.0), dict(vmax=101.0),
              dict(S=2), dict(by="gevt")]
    for k, kw in enumerate(others):
        pc = _run(**kw)[0].save(tmp_path / f"c{k}.npz")
        with pytest.raises(ValueError, match="differ in"):
            cube.merge([a, pc])
        assert cube.main(["merge", a, pc, "--out", str(tmp_path / "no.npz")]) == 2
    # edges that differ in the last bit; another table
    e2 = st.edges.copy()
    e2[2] = np.nextafter(e2[2], np.inf)
    pe2 = cube.CubeStats(st.detector, st.layout, st.shape, st.vmin, st.vmax, st.frac_bits, st.by, st.nbins, e2, "",
                         np.zeros(st.nbins, np.int64), 0, np.zeros_like(st.cnt), np.zeros_like(st.sum),
                         np.zeros_like(st.sq)).save(tmp_path / "e2.npz")
    with pytest.raises(ValueError, match="differ in edges"):
        cube.merge([a, pe2])
    g = _run(by="gevt")[0]
    g2 = cube.CubeStats(g.detector, g.layout, g.shape, g.vmin, g.vmax, g.frac_bits, g.by, g.nbins, g.edges, "0" * 64,
                        np.zeros(g.nbins, np.int64), 0, np.zeros_like(g.cnt), np.zeros_like(g.sum), np.zeros_like(g.sq))
    with pytest.raises(ValueError, match="differ in table_sha256"):
        cube.merge([g.save(tmp_path / "g.npz"), g2.save(tmp_path / "g2.npz")])
    # a gevt present twice
    with pytest.raises(ValueError, match="present twice"):
        cube.merge([a, b, a])
    # a merged run past max_frames (Q = 2^30: 7 frames), dropped frames included
    def small(n_frames, first):
        n = 24
        return cube.CubeStats("tiny", "calib", (2, 3, 4), -3.0, 2.0 ** 20, 10, "gevt", 2, None, "f" * 64,
                              [n_frames - 1, 0], 1, np.zeros((2, n), np.int32), np.zeros((2, n), np.int64),
                              np.zeros((2, n), np.int64), rank=[0] * n_frames, idx=list(range(n_frames)),
                              gevt=list(range(first, first + n_frames)), photon_energy=[np.nan] * n_frames,
                              bin=[0] * (n_frames - 1) + [-1])
    assert small(4, 0).max_frames == 7
    p4, p3, q4 = (small(4, 0).save(tmp_path / "f4.npz"), small(3, 10).save(tmp_path / "f3.npz"),
                  small(4, 20).save(tmp_path / "g4.npz"))
    m = cube.merge([p4, p3])
    assert int(m.frames.sum()) == 5 and m.dropped == 2
    with pytest.raises(ValueError, match="longer than max_frames = 7"):
        cube.merge([p4, q4])
    with pytest.raises(ValueError):
        cube.merge([])


def test_info_and_export_cli(tmp_path, capsys):
    import json

    st, _x, _pe, _bins = _run()
    path = st.save(tmp_path / "run.npz")
    assert cube.main(["info", path]) == 0
    info = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert info["frames"] == st.frames.tolist() and info["dropped"] == st.dropped and info["by"] == "photon_energy"
    assert info["nbins"] == 4 and info["bins_filled"] == int((st.frames > 0).sum()) and info["edges"] == st.edges.tolist()
    prefix = str(tmp_path / "run")
    assert cube.main(["export", path, "--out_prefix", prefix, "--ref_bin", "1"]) == 0
    mean = np.load(prefix + "_mean.npy")
    assert mean.dtype == np.float32 and mean.shape == (4, 2, 3, 4)
    want = np.stack([st.mean(b) for b in range(4)])
    assert np.array_equal(mean.reshape(4, -1), want.astype(np.float32), equal_nan=True)
    assert np.array_equal(np.load(prefix + "_frames.npy"), st.frames)
    assert np.array_equal(np.load(prefix + "_energy.npy"), st.mean_energy(), equal_nan=True)
    diff = np.load(prefix + "_diff.npy")
    assert diff.dtype == np.float32 and diff.shape == (4, 2, 3, 4)
    assert np.array_equal(diff.reshape(4, -1), (want - want[1]).astype(np.float32), equal_nan=True)
    assert cube.main(["export", path, "--out_prefix", prefix, "--ref_bin", "4"]) == 2
    assert cube.main(["info", str(tmp_path / "missing.npz")]) == 2
