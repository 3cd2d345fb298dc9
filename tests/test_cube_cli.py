"""``psana-ray-consumer --task cube`` / ``psana-ray-producer --consumer_task cube`` as separate processes on
CPU sessions (tiny_epix; the CPU endpoints run the golden models), and ``python -m psana_ray_amd.cube``."""
import os
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9
ARRAYS = ("frames", "cnt", "sum", "sq")


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
         "tiny_epix", "--device", "cpu", "--timeout", "60", *extra],
        env=_env({"RANK": str(rank), "WORLD_SIZE": str(size), "LOCAL_RANK": "0"}), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)


def _consumer(addr, cid, extra):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", str(cid), "--ray_address", addr,
                             "--device", "cpu", "--timeout", "60", "--task", "cube", "--metrics_interval", "0", *extra],
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


def _source():
    from psana_ray_amd.source import SyntheticRun

    return SyntheticRun("synthetic", RUN, "tiny_epix", rank=0, size=1)   # generated as the producer generates it


def _golden_frames(n_events, mode="calib", common_mode="off"):
    """The session's calibrated frames [n, ...] from the golden model."""
    from psana_ray_amd.config import resolve_common_mode
    from psana_ray_amd.models import make_geometry
    from psana_ray_amd.ops import reference

    src = _source()
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    cm = None if common_mode == "off" else resolve_common_mode(common_mode, src.spec)
    cal = reference.calibrate_reference(raw, src.consts, None, cm)
    if mode == "image":
        geo = make_geometry(src.spec)
        cal = reference.assemble_reference(cal, geo.rows, geo.cols, geo.image_shape)
    return cal


def _energies(n_events):
    src = _source()
    return [float(src.pool_pe[g % src.pool_frames]) for g in range(n_events)]


def _want(frames, bins, B, vmin=-2.0 ** 20, vmax=2.0 ** 20, S=2):
    from psana_ray_amd.ops import reference

    n = frames.shape[0]
    nfr, cnt, s, sq = reference.cube_accumulate_reference(frames.reshape(n, -1), bins, B, vmin, vmax, S)
    return {"frames": nfr.numpy(), "cnt": cnt.numpy(), "sum": s.numpy(), "sq": sq.numpy()}


def _same_arrays(st, want):
    for k in ARRAYS:
        got = getattr(st, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k]), k


def _same_files(a, b):
    from psana_ray_amd import cube

    assert a.key() == b.key() and a.dropped == b.dropped
    for k in (*ARRAYS, *cube.PER_FRAME):
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k


TABLE = [2, -1, 0, 2, 4, 4, 0, 1, 2, -1, 3, 3, 0, 1, 4, 2, 0, 1]          # events 18 and 19 are outside it


def _edges():
    """Edges chosen from the run's own energies, so that two frames lie below, one above and one on the last
    edge."""
    s = sorted(_energies(N_EVENTS))
    return np.array([s[2], s[6], s[10], s[15], s[18]], np.float64)


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events four times: two consumers binning by a gevt table, two binning by photon energy (one
    of them with --cube_edges_file), and the co-located consumer of a --local producer for each."""
    d = tmp_path_factory.mktemp("cube_cli")
    table, edges = str(d / "table.npy"), str(d / "edges.npy")
    np.save(table, np.array(TABLE, np.int16))
    np.save(edges, _edges())
    prod = ["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS)]
    a1, a2 = _addr(), _addr()
    by_table = [str(d / f"t{c}.npz") for c in range(2)]
    by_energy = [str(d / f"e{c}.npz") for c in range(2)]
    procs = [_producer([*prod, "--ray_address", a1, "--num_consumers", "2", "--queue_size", "6"]),
             *[_consumer(a1, c, ["--cube_by", "gevt", "--cube_table", table, "--cube_bins", "6", "--batch", "6",
                                 "--out", by_table[c]]) for c in range(2)],
             _producer([*prod, "--ray_address", a2, "--num_consumers", "2", "--queue_size", "6"]),
             *[_consumer(a2, c, ["--cube_edges_file", edges, "--batch", "5", "--cube_vmin", "-8", "--cube_vmax", "1024",
                                 "--cube_frac_bits", "12", "--out", by_energy[c]]) for c in range(2)]]
    local_t, local_e = str(d / "local_t.npz"), str(d / "local_e.npz")
    procs += [_producer([*prod, "--local", "--consumer_task", "cube", "--out_cube", local_t, "--cube_by", "gevt",
                         "--cube_table", table, "--cube_bins", "6"]),
              _producer([*prod, "--local", "--consumer_task", "cube", "--out_cube", local_e, "--cube_edges_file", edges,
                         "--cube_vmin", "-8", "--cube_vmax", "1024", "--cube_frac_bits", "12"])]
    outs = _finish(procs)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, by_table=by_table, by_energy=by_energy, local_t=local_t, local_e=local_e,
                                 outs=outs, table=table, edges=edges)


def test_two_consumers_by_gevt_table_merge_to_the_golden_model(sessions):
    from psana_ray_amd import cube

    s = sessions
    bg = cube.CubeBinning("gevt", table=np.array(TABLE), nbins=6)
    bins = bg.bin_of(range(N_EVENTS))
    want = _want(_golden_frames(N_EVENTS), bins, 6)
    assert want["frames"].tolist() == [TABLE.count(b) for b in range(6)] and want["frames"][5] == 0
    each = [cube.CubeStats.load(f) for f in s.by_table]
    assert sum(int(e.frames.sum()) + e.dropped for e in each) == N_EVENTS
    m = cube.merge(s.by_table)
    _same_arrays(m, want)
    assert m.dropped == 4 and m.gevt.tolist() == list(range(N_EVENTS)) and m.bin.tolist() == bins.tolist()
    assert np.array_equal(m.photon_energy, np.array(_energies(N_EVENTS)))
    assert (m.detector, m.layout, m.shape, m.vmin, m.vmax, m.frac_bits, m.by, m.nbins, m.table_sha256) == (
        "tiny_epix", "calib", (2, 32, 48), -2.0 ** 20, 2.0 ** 20, 2, "gevt", 6, bg.table_sha256)
    _same_files(cube.merge(s.by_table[::-1]), m)
    _same_files(cube.CubeStats.load(s.local_t).by_gevt(), m)               # the single-consumer file
    # the lines of the CLIs: max_frames at start, the counts at the end
    cons_out = [out for _, out in s.outs[1:3]]
    assert all("cube: by=gevt bins=6 max_frames=524287 " in out for out in cons_out), cons_out[0][-2000:]
    finals = [re.search(r"Consumer \d cube: frames=(\d+) binned=(\d+) dropped=(\d+) bins_filled=(\d+)/6", out)
              for out in cons_out]
    assert all(finals), cons_out[0][-2000:]
    got = sorted(tuple(int(v) for v in f.groups()) for f in finals)
    assert got == sorted((int(e.frames.sum()) + e.dropped, int(e.frames.sum()), e.dropped, int((e.frames > 0).sum()))
                         for e in each)
    assert f"Consumer 0 cube: frames={N_EVENTS} binned=16 dropped=4 bins_filled=5/6" in s.outs[6][1], s.outs[6][1][-2000:]
    # the views agree with float64 statistics of the golden frames (quantisation: 2^-3 per sample)
    x = _golden_frames(N_EVENTS).reshape(N_EVENTS, -1).numpy().astype(np.float64)
    for b in (0, 2):
        mu = x[bins == b].mean(axis=0)
        assert np.all(np.abs(m.mean(b) - mu) <= 2.0 ** -3 + 2.0 ** -23 * np.abs(mu))
    assert np.isnan(m.mean(5)).all()


def test_two_consumers_by_photon_energy_with_frames_outside_the_edges(sessions):
    from psana_ray_amd import cube

    s = sessions
    edges = _edges()
    pe = _energies(N_EVENTS)
    bins = cube.CubeBinning("photon_energy", edges=edges).bin_of(pe)
    assert (bins < 0).sum() == 3 and bins[pe.index(edges[4])] == 3
    want = _want(_golden_frames(N_EVENTS), bins, 4, vmin=-8.0, vmax=1024.0, S=12)
    m = cube.merge(s.by_energy)
    _same_arrays(m, want)
    assert m.by == "photon_energy" and m.edges.tobytes() == edges.tobytes() and m.table_sha256 == "" and m.dropped == 3
    assert 0 < int(m.cnt.sum()) < 17 * m.n                                   # the window cuts samples below -8
    one = cube.CubeStats.load(s.local_e).by_gevt()
    _same_files(one, m)
    assert one.mean_energy().tobytes() == m.mean_energy().tobytes()
    assert np.all((m.mean_energy() >= edges[:-1]) & (m.mean_energy() <= edges[1:]))
    # files of another binning do not merge
    with pytest.raises(ValueError, match="differ in"):
        cube.merge([s.by_energy[0], s.by_table[0]])
    # merge / info / export
    out = str(s.dir / "merged.npz")
    assert cube.main(["merge", *s.by_energy, "--out", out]) == 0
    _same_files(cube.CubeStats.load(out), m)
    assert cube.main(["merge", s.by_energy[0], s.by_table[0], "--out", str(s.dir / "no.npz")]) == 2
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.cube", "info", out], env=_env(), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and '"dropped": 3' in r.stdout and '"by": "photon_energy"' in r.stdout, r.stderr[-2000:]
    prefix = str(s.dir / "scan")
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.cube", "export", out, "--out_prefix", prefix, "--ref_bin",
                        "0"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    mean, diff = np.load(prefix + "_mean.npy"), np.load(prefix + "_diff.npy")
    assert mean.shape == diff.shape == (4, 2, 32, 48) and mean.dtype == diff.dtype == np.float32
    assert np.array_equal(mean[2].reshape(-1), m.mean(2).astype(np.float32), equal_nan=True)
    assert np.array_equal(np.load(prefix + "_frames.npy"), m.frames) and not diff[0][~np.isnan(diff[0])].any()
    assert np.array_equal(np.load(prefix + "_energy.npy"), m.mean_energy(), equal_nan=True)


def test_cube_edges_flag_and_calibrate_on_read(native, tmp_path):
    """--cube_edges LO,HI,N, and a --calibrate_on_read queue (RAW frames): the consumer calibrates (image mode,
    common mode) and accumulates the image."""
    from psana_ray_amd import cube
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    shape = make_geometry(get_detector("tiny_epix")).image_shape
    addr = _addr()
    out = str(tmp_path / "c.npz")
    outs = _finish([_producer(["--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                               "--common_mode", "default", "--calibrate_on_read"]),
                    _consumer(addr, 0, ["--out", out, "--batch", "4", "--cube_edges", "9400,9550,3", "--cube_vmin", "-50",
                                        "--cube_vmax", "400"])])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    st = cube.CubeStats.load(out)
    bg = cube.CubeBinning.linspace(9400.0, 9550.0, 3)
    assert st.edges.tobytes() == np.linspace(9400.0, 9550.0, 4).tobytes() == bg.edges.tobytes()
    bins = bg.bin_of(_energies(n))
    assert st.layout == "image" and st.shape == (1, *shape) and int(st.frames.sum()) + st.dropped == n
    assert 0 < int(st.frames.sum()) and st.bin.tolist() == bins.tolist()
    _same_arrays(st, _want(_golden_frames(n, "image", "default"), bins, 3, vmin=-50.0, vmax=400.0))


def test_refusals_exit_2(native, tmp_path, caplog):
    """A raw uint16 queue without a recipe, a panel-sharded session, an unnamed detector, no bin source at all,
    both edge forms at once; the co-located form's refusals; --out_cube without the task."""
    edges = str(tmp_path / "edges.npy")
    np.save(edges, np.array([9000.0, 9500.0, 9900.0]))
    src = ["--cube_edges", "9000,9900,3"]
    a_raw, a_shard = _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)]]
    cons = [_consumer(a_raw, 0, src), _consumer(a_shard, 0, src)]
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task cube" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # the bin source is checked before the queue is joined: no producer needed
    bad = ([], ["--cube_edges", "9000,9900,3", "--cube_edges_file", edges], ["--cube_by", "gevt"],
           ["--cube_edges", "9000,9900"], ["--cube_edges", "9900,9000,3"], ["--cube_edges_file", str(tmp_path / "no.npy")],
           ["--cube_by", "gevt", "--cube_edges", "9000,9900,3"], ["--cube_table", edges])
    words = ("no bin source", "not both", "no bin source", "LO,HI,N", "increasing", "no.npy", "belong to", "belong to")
    for extra, word in zip(bad, words):
        r = subprocess.run([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", _addr(), "--device", "cpu",
                            "--task", "cube", *extra], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--task cube" in r.stderr and word in r.stderr, (extra, r.stderr[-2000:])
        assert "Traceback" not in r.stderr
    # the co-located form refuses the same before it starts, and --out_cube without the task
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "cube", *src, *extra], env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--consumer_task cube needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    for extra, word in (([], "no bin source"), (["--cube_edges", "9000,9900,3", "--cube_edges_file", edges], "not both")):
        r = subprocess.run([*base, "--calib", "--consumer_task", "cube", *extra], env=_env(), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task cube" in r.stderr and word in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_cube", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_cube belongs to --consumer_task cube" in r.stderr, r.stderr[-2000:]
    # a session that does not name its detector (and no --detector_name): rc 2, one line
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 32, 48), torch.float32, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                   session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "cube", *src])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_cube(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_cube(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located cube consumers write PATH as PATH.r<rank>.npz; the files merge to
    the golden model over all events."""
    from psana_ray_amd import cube
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    addr = _addr()
    out = str(tmp_path / "run.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "cube", "--out_cube", out,
                               "--cube_edges", "9400,9550,5"], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"run.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = cube.merge(files)
    assert m.gevt.tolist() == list(range(N_EVENTS))
    # rank r of 2 produces its half of the events (gevt = r + 2 k) from a pool of its own
    frames, pe = [None] * N_EVENTS, [None] * N_EVENTS
    for r in range(2):
        src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=r, size=2, n_events=N_EVENTS)
        raw = np.stack([src.pool[k % src.pool_frames] for k in range(src.n_local_events())]).astype(np.int32)
        cal = reference.calibrate_reference(torch.from_numpy(raw), src.consts, None, None)
        for k in range(src.n_local_events()):
            frames[r + 2 * k], pe[r + 2 * k] = cal[k], float(src.pool_pe[k % src.pool_frames])
    bins = cube.CubeBinning.linspace(9400.0, 9550.0, 5).bin_of(pe)
    _same_arrays(m, _want(torch.stack(frames), bins, 5))
    assert m.bin.tolist() == bins.tolist() and np.array_equal(m.photon_energy, np.array(pe))


def test_help_and_readme_command_lines():
    from psana_ray_amd import consumer, producer

    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--cube_edges_file" in r.stdout and "cube" in r.stdout, r.stderr[-2000:]
    consumer.build_parser().parse_args(["0", "--task", "cube", "--cube_by", "gevt", "--cube_table", "t.npy", "--cube_bins",
                                        "40", "--out", "c.npz"])
    producer.build_parser().parse_args(["--exp", "e", "--run", "1", "--detector_name", "epix10k2M", "--local",
                                        "--consumer_task", "cube", "--cube_edges", "9000,9100,10", "--out_cube", "c.npz"])
    text = open(os.path.join(ROOT, "README.md")).read()
    assert "--task cube" in text and "psana_ray_amd.cube merge" in text
