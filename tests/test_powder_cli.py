"""``psana-ray-consumer --task powder`` / ``psana-ray-producer --consumer_task powder`` as separate
processes on CPU sessions (tiny_epix; the CPU endpoints run the golden models), the PowderStats file
format, ``merge`` and ``derive_mask``."""
import os
import random
import re
import shlex
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9
ARRAYS = ("frames", "cnt", "sum", "sq", "above", "qmax")


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
                             "--device", "cpu", "--timeout", "60", "--task", "powder", "--metrics_interval", "0", *extra],
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


def _golden_frames(n_events, mode="calib", common_mode="off"):
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
    return cal


def _golden_stats(frames, min_peaks=0, vmin=-2.0 ** 20, vmax=2.0 ** 20, S=2, thr=20.0):
    """Golden accumulators of ``frames`` as a dict of numpy arrays with the file's dtypes, and the peak counts."""
    from psana_ray_amd.config import PeakFinderParams
    from psana_ray_amd.ops import reference

    n = frames.shape[0]
    keys = counts = None
    if min_peaks > 0:
        f3 = frames if frames.dim() == 4 else frames.reshape(n, 1, *frames.shape[-2:])
        counts = [int(p.shape[0]) for p in reference.peakfind_reference(f3, PeakFinderParams())[0]]
        keys = torch.tensor(counts, dtype=torch.int32)
    nfr, cnt, s, sq, qmax, above = reference.powder_accumulate_reference(frames.reshape(n, -1), vmin, vmax, S, thr,
                                                                         keys=keys, key_min=min_peaks)
    return {"frames": nfr.numpy(), "cnt": cnt.numpy().astype(np.int64), "sum": s.numpy(), "sq": sq.numpy(),
            "above": above.numpy().astype(np.int64), "qmax": qmax.numpy()}, counts


def _same_arrays(st, want):
    for k in ARRAYS:
        got = getattr(st, k)
        assert got.dtype == want[k].dtype and got.shape == want[k].shape, k
        assert np.array_equal(got, want[k]), k


def _same_files(a, b):
    assert a.key() == b.key()
    _same_arrays(a, {k: getattr(b, k) for k in ARRAYS})


def _n_min():
    """The hit filter of the sessions: the median reference peak count of the run's frames."""
    _, counts = _golden_stats(_golden_frames(N_EVENTS), min_peaks=1)
    n_min = sorted(counts)[len(counts) // 2]
    assert min(counts) < n_min <= max(counts), counts
    return n_min


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers with the hit filter, the co-located consumer of a
    --local producer with the same filter (the single-consumer file), and one consumer without it."""
    d = tmp_path_factory.mktemp("powder_cli")
    n_min = _n_min()
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "2", "--queue_size", "6"]),
                    *[_consumer(addr, c, ["--min_peaks", str(n_min), "--batch", "6", "--out", two[c]])
                      for c in range(2)]])
    local = str(d / "local.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--local",
                                "--consumer_task", "powder", "--out_powder", local, "--min_peaks", str(n_min)])])
    addr1 = _addr()
    plain = str(d / "plain.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address",
                                addr1, "--num_consumers", "1", "--queue_size", "6"]),
                     _consumer(addr1, 0, ["--batch", "7", "--out", plain, "--powder_vmin", "-8", "--powder_vmax", "1024",
                                          "--powder_frac_bits", "12", "--powder_thr", "15.5"])])
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, plain=plain, outs=outs, n_min=n_min)


def test_task_powder_end_to_end_and_two_consumers_merge_to_one(sessions):
    from psana_ray_amd import powder

    s = sessions
    frames = _golden_frames(N_EVENTS)
    want, counts = _golden_stats(frames, min_peaks=s.n_min)
    hits = sum(c >= s.n_min for c in counts)
    assert 0 < hits < N_EVENTS and want["frames"].tolist() == [N_EVENTS - hits, hits]
    each = [powder.PowderStats.load(f) for f in s.two]
    assert sum(int(e.frames.sum()) for e in each) == N_EVENTS
    m = powder.merge(s.two)
    _same_arrays(m, want)
    assert (m.detector, m.layout, m.shape, m.vmin, m.vmax, m.frac_bits, m.thr_above, m.min_peaks, m.peak_params) == (
        "tiny_epix", "calib", (2, 32, 48), -2.0 ** 20, 2.0 ** 20, 2, 20.0, s.n_min,
        {"thr_peak": 20.0, "son_min": 5.0, "radius": 1.0})
    one = powder.PowderStats.load(s.local)
    _same_files(m, one)
    # the lines of the CLIs: max_frames at start, frames=<miss>+<hit> at the end
    cons_out = [out for _, out in s.outs[1:3]]
    assert all("powder: max_frames=524287 " in out for out in cons_out), cons_out[0][-2000:]
    finals = [l for out in cons_out for l in out.splitlines() if re.search(r"Consumer \d powder: frames=\d+\+\d+ ", l)]
    assert len(finals) == 2
    got = [tuple(int(v) for v in re.search(r"frames=(\d+)\+(\d+)", l).groups()) for l in finals]
    assert sorted(got) == sorted((int(e.frames[0]), int(e.frames[1])) for e in each)
    assert f"Consumer 0 powder: frames={N_EVENTS - hits}+{hits} " in s.outs[3][1], s.outs[3][1][-2000:]
    # the merge CLI writes the same content; info / export / mask run on it
    out = str(s.dir / "merged.npz")
    assert powder.main(["merge", *s.two, "--out", out]) == 0
    _same_files(powder.PowderStats.load(out), m)
    assert powder.main(["info", out]) == 0
    assert powder.main(["export", out, "--out_prefix", str(s.dir / "hits"), "--cls", "1"]) == 0
    for name in ("mean", "rms", "max"):
        a = np.load(s.dir / f"hits_{name}.npy")
        assert a.shape == (2, 32, 48) and a.dtype == np.float64
        assert np.array_equal(a, getattr(m, name)(1).reshape(2, 32, 48), equal_nan=True)
    # the views agree with float64 statistics of the golden frames (quantisation: 2^-3 per sample)
    x = frames.reshape(N_EVENTS, -1).numpy().astype(np.float64)
    assert np.all(np.abs(m.mean(None) - x.mean(axis=0)) <= 2.0 ** -3 + 2.0 ** -23 * np.abs(x.mean(axis=0)))
    assert np.all(np.abs(m.max(None) - x.max(axis=0)) <= 2.0 ** -3)


def test_other_window_and_frac_bits_without_a_hit_filter(sessions):
    from psana_ray_amd import powder

    st = powder.PowderStats.load(sessions.plain)
    want, _ = _golden_stats(_golden_frames(N_EVENTS), vmin=-8.0, vmax=1024.0, S=12, thr=15.5)
    _same_arrays(st, want)
    assert st.nc == 1 and st.frames.tolist() == [N_EVENTS] and st.peak_params == {} and st.max_frames == 524287
    assert 0 < int(st.cnt.sum()) < N_EVENTS * st.n          # the window cuts samples below -8
    assert f"frames={N_EVENTS}+0 " in sessions.outs[5][1]
    # files of other parameters do not merge
    with pytest.raises(ValueError, match="differ in"):
        powder.merge([sessions.plain, sessions.local])
    assert powder.main(["merge", sessions.plain, sessions.local, "--out", str(sessions.dir / "no.npz")]) == 2


def _make(n=24, nc=1, seed=0, **kw):
    from psana_ray_amd import powder

    rng = np.random.default_rng(seed)
    cnt = rng.integers(1, 9, size=(nc, n))
    args = dict(detector="tiny", layout="calib", shape=(2, 3, n // 6), vmin=-100.0, vmax=100.0, frac_bits=3,
                thr_above=5.0, min_peaks=0 if nc == 1 else 4, peak_params={} if nc == 1 else {"thr_peak": 20.0},
                frames=np.full(nc, 9), cnt=cnt, sum=rng.integers(-800, 800, size=(nc, n)) * cnt,
                sq=rng.integers(640000, 2 ** 40, size=(nc, n)), above=rng.integers(0, 2, size=(nc, n)) * cnt,
                qmax=rng.integers(-800, 800, size=(nc, n)))
    args.update(kw)
    return powder.PowderStats(**args)


def test_file_round_trip_is_bitwise_and_merge_refuses(tmp_path):
    from psana_ray_amd import powder

    for nc in (1, 2):
        a = _make(nc=nc, seed=nc)
        a.qmax[0, 0] = -2 ** 31
        pa = a.save(tmp_path / f"a{nc}.npz")
        _same_files(powder.PowderStats.load(pa), a)
        with np.load(pa, allow_pickle=False) as z:           # plain arrays only: loads without pickle
            assert str(z["format"]) == powder.POWDER_FORMAT and z["qmax"].dtype == np.int32
            assert all(z[k].dtype == np.int64 for k in ("frames", "cnt", "sum", "sq", "above"))
            assert z["frames"].shape == (nc,) and z["cnt"].shape == (nc, 24)
        b = _make(nc=nc, seed=10 + nc)
        m = powder.merge([pa, b.save(tmp_path / f"b{nc}.npz")])
        assert np.array_equal(m.frames, a.frames + b.frames) and np.array_equal(m.sum, a.sum + b.sum)
        assert np.array_equal(m.cnt, a.cnt + b.cnt) and np.array_equal(m.sq, a.sq + b.sq)
        assert np.array_equal(m.above, a.above + b.above) and np.array_equal(m.qmax, np.maximum(a.qmax, b.qmax))
    pa = str(tmp_path / "a1.npz")
    for k, kw in enumerate((dict(vmin=-99.0), dict(vmax=101.0), dict(frac_bits=2), dict(thr_above=6.0),
                            dict(detector="other"), dict(layout="image"), dict(shape=(2, 4, 3)))):
        pc = _make(seed=4, **kw).save(tmp_path / f"c{k}.npz")
        with pytest.raises(ValueError, match="differ in"):
            powder.merge([pa, pc])
        assert powder.main(["merge", pa, pc, "--out", str(tmp_path / "no.npz")]) == 2
    with pytest.raises(ValueError, match="differ in"):                         # NC 1 with NC 2
        powder.merge([pa, str(tmp_path / "a2.npz")])
    with pytest.raises(ValueError, match="differ in peak_params"):
        powder.merge([str(tmp_path / "a2.npz"), _make(nc=2, peak_params={"thr_peak": 21.0}).save(tmp_path / "p.npz")])
    # a merged run past powder_max_frames (Q = 2^30: 7 frames)
    big = dict(vmin=-3.0, vmax=2.0 ** 20, frac_bits=10, sq=np.zeros((1, 24)), sum=np.zeros((1, 24)))
    p4 = _make(frames=[4], **big).save(tmp_path / "f4.npz")
    p3 = _make(frames=[3], **big).save(tmp_path / "f3.npz")
    assert int(powder.merge([p4, p3]).frames[0]) == 7
    with pytest.raises(ValueError, match="longer than max_frames = 7"):
        powder.merge([p4, p4])
    with pytest.raises(ValueError):
        powder.merge([])
    np.savez(tmp_path / "x.npz", a=np.zeros(3))
    with pytest.raises(ValueError, match="not a powder-statistics file"):
        powder.PowderStats.load(tmp_path / "x.npz")
    with pytest.raises(ValueError):                                            # two classes need a hit filter
        _make(nc=2, min_peaks=0)
    with pytest.raises(ValueError):
        _make(cnt=np.zeros((1, 23)))


def test_derive_mask_hot_dead_stuck_and_the_mask_loads_as_sparse_mask(tmp_path):
    from psana_ray_amd import consumer, powder
    from psana_ray_amd.ops import reference

    rng = np.random.default_rng(5)
    F, shape = 12, (2, 3, 4)
    x = rng.normal(3, 4, size=(F, 24)).astype(np.float32)
    x[:, 5] = np.abs(x[:, 5]) + 50                # hot: above the threshold in every frame
    x[:, 6] = np.nan                              # dead: never a sample
    x[:, 7] = 2.75                                # stuck
    x[:7, 8] = 60.0                               # above in 7 of 12 frames: 0.583 > 0.5
    x[:6, 9] = 60.0                               # above in exactly half: NOT hot (strict)
    x[1:, 10] = np.nan                            # one sample: kept at min_samples 1, dropped at 2
    x[0, 10] = 1.0
    keys = torch.tensor([0, 4] * 6, dtype=torch.int32)
    nfr, cnt, s, sq, qmax, above = reference.powder_accumulate_reference(torch.from_numpy(x), -1000.0, 1000.0, 2, 20.0,
                                                                         keys=keys, key_min=4)
    st = powder.PowderStats("tiny", "calib", shape, -1000.0, 1000.0, 2, 20.0, 4, {"thr_peak": 20.0}, nfr.numpy(),
                            cnt.numpy(), s.numpy(), sq.numpy(), above.numpy(), qmax.numpy())
    m = powder.derive_mask(st)
    assert m.dtype == np.uint8 and m.shape == shape
    want = np.ones(24, np.uint8)
    want[[5, 6, 7, 8]] = 0
    assert np.array_equal(m.reshape(-1), want)
    want[10] = 0
    assert np.array_equal(powder.derive_mask(st, min_samples=2).reshape(-1), want)
    assert powder.derive_mask(st, hot_fraction=0.4).reshape(-1)[9] == 0
    path = st.save(tmp_path / "st.npz")
    out = str(tmp_path / "mask.npy")
    assert powder.main(["mask", path, "--out", out, "--hot_fraction", "0.5"]) == 0
    assert np.array_equal(np.load(out), m)
    assert np.array_equal(consumer.load_sparse_mask(out, shape), m.reshape(-1))
    assert np.load(out, allow_pickle=False).dtype == np.uint8      # what --radial_mask reads


def test_calibrate_on_read_queue_is_calibrated_then_accumulated(native, tmp_path):
    """A --calibrate_on_read queue carries RAW frames: the consumer calibrates (image mode, common mode)
    and accumulates the image."""
    from psana_ray_amd import powder
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    shape = make_geometry(get_detector("tiny_epix")).image_shape
    addr = _addr()
    out = str(tmp_path / "c.npz")
    outs = _finish([_producer(["--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                               "--common_mode", "default", "--calibrate_on_read"]),
                    _consumer(addr, 0, ["--out", out, "--batch", "4", "--powder_vmin", "-50", "--powder_vmax", "400"])])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    st = powder.PowderStats.load(out)
    assert st.layout == "image" and st.shape == (1, *shape) and st.frames.tolist() == [n]
    want, _ = _golden_stats(_golden_frames(n, "image", "default"), vmin=-50.0, vmax=400.0)
    _same_arrays(st, want)


def test_refusals_exit_2(native, tmp_path, caplog):
    """A raw uint16 queue without a recipe, a panel-sharded session, parameters out of range, an unnamed
    detector; the co-located form's refusals; --out_powder without the task."""
    a_raw, a_shard, a_par = _addr(), _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)],
             _producer(["--calib", "--num_events", "4", "--ray_address", a_par, "--num_consumers", "1",
                        "--queue_size", "4"])]
    cons = [_consumer(a_raw, 0, []), _consumer(a_shard, 0, []),
            _consumer(a_par, 0, ["--powder_frac_bits", "11"])]             # Q = 2^31
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards", "below 2^31")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task powder" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # the co-located form refuses the same sessions before it starts, and --out_powder without the task
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "powder", *extra], env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--consumer_task powder needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_powder", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_powder belongs to --consumer_task powder" in r.stderr, r.stderr[-2000:]
    # a session that does not name its detector (and no --detector_name): rc 2, one line
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 32, 48), torch.float32, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                   session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "powder"])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_powder(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_powder(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located powder consumers write PATH as PATH.r<rank>.npz; the files
    merge to the golden model over all events."""
    from psana_ray_amd import powder

    addr = _addr()
    out = str(tmp_path / "run.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "powder", "--out_powder",
                               out], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"run.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = powder.merge(files)
    assert int(m.frames.sum()) == N_EVENTS
    # rank r of 2 produces its half of the events from a pool of its own
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    frames = []
    for r in range(2):
        src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=r, size=2, n_events=N_EVENTS)
        raw = np.stack([src.pool[k % src.pool_frames] for k in range(src.n_local_events())]).astype(np.int32)
        frames.append(reference.calibrate_reference(torch.from_numpy(raw), src.consts, None, None))
    want, _ = _golden_stats(torch.cat(frames))
    _same_arrays(m, want)


def test_the_readmes_command_lines_still_parse():
    """Every psana-ray-producer / psana-ray-consumer command line in the README's code blocks parses
    with the parsers as they are now (the new flags took no existing name or abbreviation)."""
    from psana_ray_amd import consumer, producer

    text = open(os.path.join(ROOT, "README.md")).read().replace("\\\n", " ")
    blocks = re.findall(r"```[a-z]*\n(.*?)```", text, flags=re.S)
    found = {"producer": 0, "consumer": 0}
    for block in blocks:
        for prog, rest in re.findall(r"psana-ray-(producer|consumer)((?: +[^\s&;#|`]+)*)", block):
            argv = shlex.split(rest.replace("$c", "0"))
            if not argv or any(a.startswith(("/", "-consumer")) for a in argv[:1]):
                continue
            parser = producer.build_parser() if prog == "producer" else consumer.build_parser()
            try:
                parser.parse_args(argv)
            except SystemExit:
                pytest.fail(f"psana-ray-{prog} {rest} no longer parses")
            found[prog] += 1
    assert found["producer"] >= 5 and found["consumer"] >= 5, found
    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "powder" in r.stdout, r.stderr[-2000:]
