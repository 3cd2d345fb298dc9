"""``psana-ray-consumer --task hist`` / ``psana-ray-producer --consumer_task hist`` as separate processes
on CPU sessions (tiny_epix; the CPU endpoints run the golden model) and the ``python -m
psana_ray_amd.hist`` CLI on their files."""
import json
import os
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from psana_ray_amd import hist as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9


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
                             "--device", "cpu", "--timeout", "60", "--task", "hist", "--metrics_interval", "0", *extra],
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


def _golden_hist(frames, lo=-32.0, hi=96.0, nbins=64):
    from psana_ray_amd.ops import reference

    return reference.pixel_hist_reference(frames.reshape(frames.shape[0], -1), lo, hi, nbins).numpy()


def _same_files(a, b):
    assert a.key() == b.key() and a.frames == b.frames
    assert a.hist.dtype == b.hist.dtype == np.int32 and np.array_equal(a.hist, b.hist)


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers, the co-located consumer of a --local producer (the
    single-consumer file), and one consumer with another window."""
    d = tmp_path_factory.mktemp("hist_cli")
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "2", "--queue_size", "6"]),
                    *[_consumer(addr, c, ["--batch", "6", "--out", two[c]]) for c in range(2)]])
    local = str(d / "local.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--local",
                                "--consumer_task", "hist", "--out_hist", local])])
    addr1 = _addr()
    plain = str(d / "plain.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address",
                                addr1, "--num_consumers", "1", "--queue_size", "6"]),
                     _consumer(addr1, 0, ["--batch", "7", "--out", plain, "--hist_lo", "-8", "--hist_hi", "1000.5",
                                          "--hist_bins", "37"])])
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, plain=plain, outs=outs)


def test_task_hist_end_to_end_and_two_consumers_merge_to_one(sessions):
    s = sessions
    frames = _golden_frames(N_EVENTS)
    want = _golden_hist(frames)
    each = [H.PixelHist.load(f) for f in s.two]
    assert sum(e.frames for e in each) == N_EVENTS
    m = H.merge(s.two)
    assert m.frames == N_EVENTS and m.hist.dtype == np.int32 and np.array_equal(m.hist, want)
    assert (m.detector, m.layout, m.shape, m.lo, m.hi, m.nbins) == ("tiny_epix", "calib", (2, 32, 48), -32.0, 96.0, 64)
    assert 0 < int(m.hist.sum()) <= N_EVENTS * m.n
    # --local --consumer_task hist gives the same bytes as the merge CLI's file
    one = H.PixelHist.load(s.local)
    _same_files(m, one)
    out = str(s.dir / "merged.npz")
    assert H.main(["merge", *s.two, "--out", out]) == 0
    _same_files(H.PixelHist.load(out), one)
    with np.load(out, allow_pickle=False) as za, np.load(s.local, allow_pickle=False) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes(), k
    # the lines of the CLIs: the accumulator bytes at start, frames at the end
    cons_out = [o for _, o in s.outs[1:3]]
    assert all(f"hist: window=[-32,96] bins=64 accumulator_bytes={m.n * 64 * 4}" in o for o in cons_out), cons_out[0][-2000:]
    finals = [l for o in cons_out for l in o.splitlines() if re.search(r"Consumer \d hist: frames=\d+ ", l)]
    assert sorted(int(re.search(r"frames=(\d+)", l).group(1)) for l in finals) == sorted(e.frames for e in each)
    assert f"Consumer 0 hist: frames={N_EVENTS} " in s.outs[3][1], s.outs[3][1][-2000:]


def test_other_window_and_the_hist_cli(sessions, capsys):
    s = sessions
    st = H.PixelHist.load(s.plain)
    frames = _golden_frames(N_EVENTS)
    assert np.array_equal(st.hist, _golden_hist(frames, -8.0, 1000.5, 37))
    assert (st.lo, st.hi, st.nbins, st.frames) == (-8.0, 1000.5, 37, N_EVENTS)
    with pytest.raises(ValueError, match="differ in"):
        H.merge([s.plain, s.local])
    assert H.main(["merge", s.plain, s.local, "--out", str(s.dir / "no.npz")]) == 2
    capsys.readouterr()
    assert H.main(["info", s.local]) == 0
    info = json.loads(capsys.readouterr().out)
    one = H.PixelHist.load(s.local)
    assert info["frames"] == N_EVENTS and info["nbins"] == 64 and info["shape"] == [2, 32, 48]
    assert info["bin_width"] == 2.0 and info["samples"] == int(one.hist.sum())
    sp = str(s.dir / "s.npy")
    assert H.main(["spectrum", s.local, "--out", sp]) == 0
    spec = np.load(sp)
    assert spec.dtype == np.int64 and np.array_equal(spec, one.hist.sum(axis=0, dtype=np.int64))
    assert H.main(["info", str(s.dir / "missing.npz")]) == 2
    # gain: the base constants divided by expected / centroid, where a pixel has samples in the peak window
    from psana_ray_amd.models.constants import CalibConstants
    from psana_ray_amd.source import SyntheticRun

    base = SyntheticRun("synthetic", RUN, "tiny_epix", rank=0, size=1).consts
    pb, po, pc = base.save(s.dir / "base.npz"), str(s.dir / "consts.npz"), str(s.dir / "corr.npy")
    assert H.main(["gain", s.local, "--peak=-10,10", "--expected", "1.5", "--base", pb, "--gain_range", "0",
                   "--min_count", "3", "--out", po, "--corr_out", pc]) == 0
    corr = np.load(pc)
    assert corr.shape == (2, 32, 48) and corr.dtype == np.float32
    assert np.array_equal(corr.reshape(-1), H.derive_gain_correction(one, -10.0, 10.0, 1.5, 3), equal_nan=True)
    got = CalibConstants.load(po)
    ok = np.isfinite(corr)
    assert ok.any()
    assert np.array_equal(got.gains[0][ok], (base.gains[0][ok] / corr[ok]).astype(np.float32))
    assert np.array_equal(got.gains[0][~ok], base.gains[0][~ok]) and np.array_equal(got.gains[1:], base.gains[1:])
    assert np.array_equal(got.pedestals, base.pedestals) and np.array_equal(got.status, base.status)


def test_calibrate_on_read_queue_is_calibrated_then_histogrammed(native, tmp_path):
    """A --calibrate_on_read queue carries RAW frames: the consumer calibrates (image mode, common mode)
    and histograms the image."""
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    shape = make_geometry(get_detector("tiny_epix")).image_shape
    addr = _addr()
    out = str(tmp_path / "c.npz")
    outs = _finish([_producer(["--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                               "--common_mode", "default", "--calibrate_on_read"]),
                    _consumer(addr, 0, ["--out", out, "--batch", "4", "--hist_lo", "-50", "--hist_hi", "400",
                                        "--hist_bins", "256"])])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    st = H.PixelHist.load(out)
    assert st.layout == "image" and st.shape == (1, *shape) and st.frames == n
    assert np.array_equal(st.hist, _golden_hist(_golden_frames(n, "image", "default"), -50.0, 400.0, 256))


def test_refusals_exit_2(native, tmp_path, caplog):
    """A raw uint16 queue without a recipe, a panel-sharded session, parameters out of range, an unnamed
    detector; the co-located form's refusals; --out_hist without the task."""
    a_raw, a_shard, a_par = _addr(), _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)],
             _producer(["--calib", "--num_events", "4", "--ray_address", a_par, "--num_consumers", "1",
                        "--queue_size", "4"])]
    cons = [_consumer(a_raw, 0, []), _consumer(a_shard, 0, []), _consumer(a_par, 0, ["--hist_bins", "1025"])]
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards", "nbins must be in")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task hist" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # the co-located form refuses the same sessions before it starts, and --out_hist without the task
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "hist", *extra], env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--consumer_task hist needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_hist", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_hist belongs to --consumer_task hist" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "hist", "--hist_lo", "5", "--hist_hi", "5"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "lo < hi" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    # a session that does not name its detector (and no --detector_name): rc 2, one line
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 32, 48), torch.float32, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                   session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "hist"])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_hist(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_hist(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located hist consumers write PATH as PATH.r<rank>.npz; the files merge to
    the golden model over all events."""
    addr = _addr()
    out = str(tmp_path / "hist.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "hist", "--out_hist",
                               out, "--hist_bins", "5"], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"hist.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = H.merge(files)
    assert m.frames == N_EVENTS
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    frames = []
    for r in range(2):
        src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=r, size=2, n_events=N_EVENTS)
        raw = np.stack([src.pool[k % src.pool_frames] for k in range(src.n_local_events())]).astype(np.int32)
        frames.append(reference.calibrate_reference(torch.from_numpy(raw), src.consts, None, None))
    assert np.array_equal(m.hist, _golden_hist(torch.cat(frames), nbins=5))


def test_consumer_refuses_a_run_past_the_frame_bound():
    """The consumer refuses, with a ValueError and before any lease or launch, what would take the run
    past 2^31 - 1 frames."""
    from psana_ray_amd.pipeline import PixelHistConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 3, 4), torch.float32, "cpu", 2, 2))
    try:
        cons = PixelHistConsumer(ep, (2, 3, 4), lo=0.0, hi=8.0, nbins=4, detector="t", batch=4)
        x = [torch.full((2, 3, 4), 3.0) for _ in range(3)]
        cons.process_frames(x)
        assert cons.frames == 3 and cons.synchronize()[:, 1].tolist() == [3] * 24
        cons.frames = 2 ** 31 - 1 - 2
        with pytest.raises(ValueError, match="past 2147483647"):
            cons.process_frames(x)
        cons.frames = 2 ** 31 - 1
        with pytest.raises(ValueError, match="past 2147483647"):
            cons.poll(timeout=0.0)
        with pytest.raises(ValueError, match="batch of at most"):
            cons.frames = 0
            cons.process_frames(x + x)
        for bad in (dict(lo=1.0, hi=1.0), dict(nbins=0), dict(nbins=1025)):
            with pytest.raises(ValueError):
                PixelHistConsumer(ep, (2, 3, 4), **{**dict(lo=0.0, hi=8.0, nbins=4), **bad})
    finally:
        ep.close()


def test_help_names_the_task():
    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "hist" in r.stdout and "--hist_bins" in r.stdout, r.stderr[-2000:]
