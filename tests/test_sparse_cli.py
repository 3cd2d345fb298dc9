"""``psana-ray-consumer --task sparse`` / ``psana-ray-producer --consumer_task sparse`` as separate
processes on CPU sessions (tiny_epix), and the SparseFrames file format."""
import glob
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9
THR, CAP = 20.0, 450    # tiny_epix frames are spot-rich: 250 .. 630 pixels pass, so some frames overflow


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


def _addr():
    return f"127.0.0.1:{random.randint(30000, 45000)}"


def _producer(extra, rank=0, size=1):
    return subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
         "tiny_epix", "--device", "cpu", "--common_mode", "off", "--timeout", "60", *extra],
        env=_env({"RANK": str(rank), "WORLD_SIZE": str(size), "LOCAL_RANK": "0"}), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)


def _consumer(addr, cid, extra):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", str(cid), "--ray_address", addr,
                             "--device", "cpu", "--timeout", "60", "--task", "sparse", "--metrics_interval", "0", *extra],
                            env=_env(), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _finish(procs, timeout=180):
    outs = []
    try:
        for p in procs:
            out, _ = p.communicate(timeout=timeout)
            outs.append((p.returncode, out))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.communicate()
    return outs


def _golden(n_events, mode="calib", common_mode="off"):
    """The session's calibrated frames [n, ...] from the golden model (the pool is generated as the
    producer process generates it)."""
    from psana_ray_amd.config import resolve_common_mode
    from psana_ray_amd.models import make_geometry
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=0, size=1)
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    cm = None if common_mode == "off" else resolve_common_mode(common_mode, src.spec)
    cal = reference.calibrate_reference(raw, src.consts, None, cm)
    if mode == "image":
        geo = make_geometry(src.spec)
        cal = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)
    return cal, src.pool_pe


def _check_against_golden(sf, frames, thr, vmax=2.0 ** 20, mask=None):
    """Every event once, in gevt order; to_dense == where(keep, frame, 0) bit for bit."""
    from psana_ray_amd import sparse

    n = frames.shape[0]
    assert sf.gevt.tolist() == list(range(n)) and sf.idx.tolist() == list(range(n))
    x = frames.reshape(n, -1).numpy()
    keep = (x >= np.float32(thr)) & (x <= np.float32(vmax))
    if mask is not None:
        keep &= mask.reshape(-1) != 0
    assert np.array_equal(sf.nnz, keep.sum(1))
    assert np.array_equal(sf.flags, np.where(keep.sum(1) > sf.cap, sparse.FLAG_OVERFLOW, 0).astype(np.uint8))
    for i in range(n):
        if sf.flags[i]:
            continue
        want = np.where(keep[i], x[i], np.float32(0)).reshape(sf.shape)
        assert np.array_equal(sf.to_dense(i).view(np.int32), want.view(np.int32)), i
    return keep


def _same_files(a, b):
    assert a.params() == b.params()
    for k in (*a.__class__.__dataclass_fields__,):
        va, vb = getattr(a, k), getattr(b, k)
        if isinstance(va, np.ndarray):
            assert va.dtype == vb.dtype and va.shape == vb.shape, k
            assert np.array_equal(va.view(np.uint8), vb.view(np.uint8)), k   # bitwise (photon_energy may be NaN)


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """Three runs over the same 20 events: two consumers, one consumer writing parts of 8, and the
    co-located consumer of a --local producer."""
    d = tmp_path_factory.mktemp("sparse_cli")
    common = ["--sparse_thr", str(THR), "--sparse_cap", str(CAP), "--batch", "6"]
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    outs = _finish([_producer(["--calib", "--num_events", str(N_EVENTS), "--ray_address", addr, "--num_consumers", "2",
                               "--queue_size", "6"]),
                    *[_consumer(addr, c, [*common, "--out", two[c]]) for c in range(2)]])
    addr1 = _addr()
    parts = str(d / "parts.npz")
    outs += _finish([_producer(["--calib", "--num_events", str(N_EVENTS), "--ray_address", addr1, "--num_consumers", "1",
                                "--queue_size", "6"]),
                     _consumer(addr1, 0, [*common, "--out", parts, "--part_frames", "8"])])
    local = str(d / "local.npz")
    outs += _finish([_producer(["--calib", "--num_events", str(N_EVENTS), "--local", "--consumer_task", "sparse",
                                "--out_sparse", local, "--sparse_thr", str(THR), "--sparse_cap", str(CAP)])])
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, parts=parts, local=local, outs=outs)


def test_two_consumers_merge_to_one_consumer_and_to_the_golden_model(sessions):
    from psana_ray_amd import sparse

    s = sessions
    lines = [l for _, out in s.outs for l in out.splitlines() if " sparse: frames=" in l]
    assert len(lines) == 4 and all("stored=" in l and "skipped=0" in l and "pixels=" in l for l in lines), lines
    each = [sparse.SparseFrames.load(f) for f in s.two]
    assert sum(len(e) for e in each) == N_EVENTS
    m = sparse.merge(s.two)
    frames, pe = _golden(N_EVENTS)
    keep = _check_against_golden(m, frames, THR)
    over = keep.sum(1) > CAP
    assert 0 < int(over.sum()) < N_EVENTS and int(keep[~over].sum()) == int(m.offs[-1]) > 0
    assert [l for l in lines if f"frames={N_EVENTS} " in l and f"overflowed={int(over.sum())} " in l
            and f"stored={N_EVENTS - int(over.sum())} " in l and l.endswith(f"pixels={int(m.offs[-1])}")], lines
    assert m.params() == {"detector": "tiny_epix", "layout": "calib", "shape": [2, 32, 48], "thr": THR,
                          "vmax": 2.0 ** 20, "cap": CAP, "min_peaks": 0, "peak_params": {}}
    assert np.array_equal(m.photon_energy, np.asarray(pe)[np.arange(N_EVENTS) % len(pe)])
    one = sparse.merge([s.local])
    _same_files(m, one)
    # the merge CLI writes the same file content
    out = str(s.dir / "merged.npz")
    assert sparse.main(["merge", *s.two, "--out", out]) == 0
    _same_files(sparse.SparseFrames.load(out), m)
    dense = str(s.dir / "f3.npy")
    assert sparse.main(["dense", out, "--gevt", "3", "--out", dense]) == 0
    assert np.array_equal(np.load(dense).view(np.int32), m.to_dense(3).view(np.int32))
    assert sparse.main(["info", out]) == 0


def test_part_files_concatenate_to_the_same_content(sessions):
    from psana_ray_amd import sparse

    s = sessions
    stem = s.parts[:-4]
    files = sorted(glob.glob(stem + ".*.npz"))
    assert [os.path.basename(f) for f in files] == [f"parts.{k:05d}.npz" for k in range(3)] and not os.path.exists(s.parts)
    assert [len(sparse.SparseFrames.load(f)) for f in files] == [8, 8, 4]
    want = sparse.merge(s.two)
    _same_files(sparse.merge([stem + ".*.npz"]), want)
    for loaded in (sparse.SparseFrames.load(stem + ".*.npz"), sparse.SparseFrames.load(files)):
        assert len(loaded) == N_EVENTS
        _same_files(loaded.select(np.argsort(loaded.gevt, kind="stable")), want)


def test_calibrate_on_read_queue_is_calibrated_then_sparsified(native, tmp_path):
    """A --calibrate_on_read queue carries RAW frames: the consumer calibrates (image mode, common mode)
    and sparsifies the image; a frame-shaped mask is applied."""
    from psana_ray_amd import sparse
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    shape = make_geometry(get_detector("tiny_epix")).image_shape
    mask = (np.random.default_rng(3).random(shape) < 0.8).astype(np.uint8)
    np.save(tmp_path / "mask.npy", mask)
    addr = _addr()
    out = str(tmp_path / "c.npz")
    prod = subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
         "tiny_epix", "--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
         "--device", "cpu", "--common_mode", "default", "--calibrate_on_read", "--timeout", "60"],
        env=_env({"RANK": "0", "WORLD_SIZE": "1", "LOCAL_RANK": "0"}), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True)
    cons = _consumer(addr, 0, ["--sparse_thr", "10", "--sparse_vmax", "400", "--sparse_cap", "500", "--sparse_mask",
                               str(tmp_path / "mask.npy"), "--out", out, "--batch", "4"])
    outs = _finish([prod, cons])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    sf = sparse.SparseFrames.load(out)
    assert sf.layout == "image" and sf.shape == (1, *shape) and sf.cap == 500
    frames, _ = _golden(n, "image", "default")
    keep = _check_against_golden(sf, frames, 10.0, 400.0, mask)
    assert int(keep.sum()) > 0


def test_refusals_exit_2(native, tmp_path):
    """A raw uint16 queue without a recipe, a panel-sharded session, a mask of another shape."""
    np.save(tmp_path / "bad.npy", np.ones((2, 32, 47), np.uint8))
    a_raw, a_shard, a_mask = _addr(), _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)],
             _producer(["--calib", "--num_events", "4", "--ray_address", a_mask, "--num_consumers", "1",
                        "--queue_size", "4"])]
    cons = [_consumer(a_raw, 0, []), _consumer(a_shard, 0, []),
            _consumer(a_mask, 0, ["--sparse_mask", str(tmp_path / "bad.npy")])]
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards", "--sparse_mask is (2, 32, 47)")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task sparse" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # the co-located form refuses the same sessions before it starts
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN),
                            "--detector_name", "tiny_epix", "--device", "cpu", "--num_events", "4", "--local",
                            "--consumer_task", "sparse", *extra], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task sparse needs whole calibrated frames" in r.stderr, r.stderr[-2000:]


def _make(gevts, seed=0, **kw):
    from psana_ray_amd import sparse

    rng = np.random.default_rng(seed)
    N = len(gevts)
    nnz = rng.integers(0, 6, size=N).astype(np.int32)
    flags = np.zeros(N, np.uint8)
    if N > 2:
        flags[1], nnz[1] = sparse.FLAG_OVERFLOW, 99
        flags[2], nnz[2] = sparse.FLAG_SKIPPED, 0
    stored = np.where(flags != 0, 0, nnz)
    offs = np.concatenate([[0], np.cumsum(stored)]).astype(np.int64)
    pix = np.concatenate([np.sort(rng.choice(24, size=k, replace=False)) for k in stored] or [[]]).astype(np.int32)
    val = rng.normal(size=pix.size).astype(np.float32)
    if val.size:
        val[0] = -0.0
    pe = rng.normal(9500, 50, size=N)
    if N:
        pe[0] = np.nan
    args = dict(detector="tiny", layout="calib", shape=(2, 3, 4), thr=-5.0, vmax=5.0, cap=8, min_peaks=0)
    args.update(kw)
    return sparse.SparseFrames(**args, rank=np.zeros(N), idx=np.asarray(gevts), gevt=np.asarray(gevts), photon_energy=pe,
                               nnz=nnz, flags=flags, offs=offs, pix=pix, val=val)


def test_file_round_trip_is_bitwise_and_merge_refuses(tmp_path):
    from psana_ray_amd import sparse

    a = _make([4, 0, 9, 7, 2], seed=1)
    pa = a.save(tmp_path / "a.npz")
    _same_files(sparse.SparseFrames.load(pa), a)
    with np.load(pa, allow_pickle=False) as z:           # plain arrays only: loads without pickle
        assert str(z["format"]) == sparse.SPARSE_FORMAT and z["pix"].dtype == np.int32 and z["offs"].dtype == np.int64
    e = _make([], seed=2)
    _same_files(sparse.SparseFrames.load(e.save(tmp_path / "e.npz")), e)
    b = _make([1, 3, 8], seed=3)
    pb = b.save(tmp_path / "b.npz")
    m = sparse.merge([pa, pb, str(tmp_path / "e.npz")])
    assert m.gevt.tolist() == [0, 1, 2, 3, 4, 7, 8, 9]
    for src in (a, b):
        for i, g in enumerate(src.gevt.tolist()):
            j = m.gevt.tolist().index(g)
            assert m.nnz[j] == src.nnz[i] and m.flags[j] == src.flags[i]
            assert np.array_equal(m.frame(j)[0], src.frame(i)[0])
            assert np.array_equal(m.frame(j)[1].view(np.int32), src.frame(i)[1].view(np.int32))
    with pytest.raises(ValueError, match="overflowed"):
        m.to_dense(m.gevt.tolist().index(0))              # a's second frame
    assert not m.to_dense(m.gevt.tolist().index(9)).any()  # a skipped frame is all zeros
    # other parameters, a gevt twice, nothing at all
    for k, kw in enumerate((dict(thr=-4.0), dict(cap=9), dict(shape=(2, 4, 3)), dict(min_peaks=2), dict(layout="image"),
                            dict(detector="other"), dict(peak_params={"thr_peak": 20.0}))):
        pc = _make([11, 12], seed=4, **kw).save(tmp_path / f"c{k}.npz")
        with pytest.raises(ValueError, match="different parameters"):
            sparse.merge([pa, pc])
        assert sparse.main(["merge", pa, pc, "--out", str(tmp_path / "no.npz")]) == 2
    pd = _make([5, 9], seed=5).save(tmp_path / "d.npz")
    with pytest.raises(ValueError, match="gevt 9 is present twice"):
        sparse.merge([pa, pd])
    with pytest.raises(ValueError):
        sparse.merge([str(tmp_path / "none*.npz")])
    np.savez(tmp_path / "x.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="not a sparse-frames file"):
        sparse.SparseFrames.load(tmp_path / "x.npz")
    with pytest.raises(ValueError):                       # offs that disagree with nnz / flags
        sparse.SparseFrames("tiny", "calib", (2, 3, 4), 0.0, 1.0, 8, rank=[0], idx=[0], gevt=[0], photon_energy=[0.0],
                            nnz=[2], flags=[0], offs=[0, 1], pix=[3], val=[1.0])
