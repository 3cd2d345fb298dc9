"""The dark-run workflow through the CLIs, on CPU sessions: ``psana-ray-mkrun --dark`` -> a raw producer
-> two ``--task dark`` consumers -> merge -> derive -> a producer with ``--constants``."""
import os
import random
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
N_DARK = 200
MIN_FRAMES = 100
# detector -> (run file format, the gain range a dark run in the default configuration covers)
CASES = {"tiny_epix": ("praw", 3), "tiny_jungfrau": ("xtc2", 0)}


def _env(extra=None, stub=False):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = os.pathsep.join(([STUBS] if stub else []) + [ROOT, env.get("PYTHONPATH", "")])
    env.update(extra or {})
    return env


def _addr():
    return f"127.0.0.1:{random.randint(30000, 45000)}"


def _producer(args, rank=0, size=1, stub=False):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.producer", "--device", "cpu", "--timeout", "60", *args],
                            env=_env({"RANK": str(rank), "WORLD_SIZE": str(size), "LOCAL_RANK": "0"}, stub=stub),
                            stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)


def _consumer(addr, cid, extra):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", str(cid), "--ray_address", addr,
                             "--device", "cpu", "--timeout", "60", "--task", "dark", "--metrics_interval", "0", *extra],
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


def _run_frames(data_dir, exp, run, det):
    """Every frame of the run file [n, P, H, W] uint16, through the project's own reader."""
    from psana_ray_amd.source import open_source

    src = open_source(exp, run, det, data_dir=data_dir)
    frames = []
    while True:
        evs = src.next_events(32)
        if not evs:
            break
        frames.extend(np.array(e.raw, np.uint16, copy=True) for e in evs)
    return np.stack(frames)


def _u16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint16).view(np.int16)).view(torch.uint16)


@pytest.fixture(scope="module", params=sorted(CASES))
def dark_session(request, native, tmp_path_factory):
    """One dark run per detector: the run file, two consumers' files from a raw session, one
    co-located consumer's file, their merge and the derived constants."""
    from psana_ray_amd import dark, mkrun

    det = request.param
    fmt, g = CASES[det]
    d = tmp_path_factory.mktemp(f"dark_{det}")
    exp, run = "darkexp", 5
    assert mkrun.main(["--data_dir", str(d), "--exp", exp, "--run", str(run), "--detector_name", det,
                       "--num_events", str(N_DARK), "--dark", "--format", fmt]) == 0
    addr = _addr()
    files = [str(d / f"c{c}.npz") for c in range(2)]
    src_args = ["--exp", exp, "--run", str(run), "--detector_name", det, "--data_dir", str(d)]
    prod = _producer([*src_args, "--mode", "raw", "--ray_address", addr, "--num_consumers", "2", "--queue_size", "8"])
    # no --detector_name: the detector comes from the session metadata
    cons = [_consumer(addr, c, ["--out", files[c], "--batch", "16"]) for c in range(2)]
    outs = _finish([prod] + cons)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    lines = [l for _, out in outs[1:] for l in out.splitlines() if " dark: frames=" in l]
    assert len(lines) == 2 and all(f"detector={det}" in l for l in lines), lines
    one = str(d / "one.npz")
    outs1 = _finish([_producer([*src_args, "--mode", "raw", "--local", "--consumer_task", "dark", "--out_dark", one])])
    assert outs1[0][0] == 0 and f"dark statistics of {N_DARK} frames" in outs1[0][1], outs1[0][1][-3000:]
    merged = str(d / "dark.npz")
    assert dark.main(["merge", *files, "--out", merged]) == 0
    consts = str(d / "consts.npz")
    assert dark.main(["derive", merged, "--out", consts, "--exp", exp, "--run", str(run), "--data_dir", str(d),
                      "--gain_config", "AHL", "--min_frames", str(MIN_FRAMES), "--report", str(d / "report.json")]) == 0
    return types.SimpleNamespace(det=det, g=g, dir=str(d), exp=exp, run=run, files=files, one=one, merged=merged,
                                 consts=consts, src_args=src_args)


def test_two_consumers_merge_to_one_consumer_and_to_the_golden_model(dark_session):
    from psana_ray_amd import dark
    from psana_ray_amd.models import get_detector
    from psana_ray_amd.ops import reference

    s = dark_session
    spec = get_detector(s.det)
    m = dark.merge(s.files)
    parts = [dark.DarkStats.load(f) for f in s.files]
    assert sum(p.frames for p in parts) == N_DARK == m.frames
    one = dark.DarkStats.load(s.one)
    frames = _run_frames(s.dir, s.exp, s.run, s.det)
    assert frames.shape == (N_DARK, *spec.frame_shape)
    cnt, sm, sq = reference.dark_accumulate_reference(_u16(frames), spec.kernel_kind, 0, 65535)
    for got in (m, one, dark.DarkStats.load(s.merged)):
        assert got.key() == (s.det, spec.kernel_kind, 0, 65535, spec.npix) and got.frames == N_DARK
        assert np.array_equal(got.cnt, cnt.to(torch.int64).numpy())
        assert np.array_equal(got.sum, sm.numpy())
        assert np.array_equal(got.sq, sq.numpy())
    # a dark run stays in its first candidate: every sample is counted there
    assert int(m.cnt[0].min()) == N_DARK and int(m.cnt[1:].sum()) == 0


def test_pedestals_are_recovered_within_their_own_error(dark_session):
    """|mean - true pedestal| <= 6 * rms / sqrt(cnt) at EVERY pixel of the covered range, each with its
    own rms and cnt; no pixel is excluded.  Measured on these 200-frame runs (the figures the test prints):
    tiny_epix max error 1.86 ADU (rms 6.0-8.7, bound >= 2.56), tiny_jungfrau 0.74 ADU (rms 2.6-3.5,
    bound >= 1.10)."""
    from psana_ray_amd import dark
    from psana_ray_amd.models import CalibConstants, get_detector, run_seed

    s = dark_session
    spec = get_detector(s.det)
    true = CalibConstants.random(spec, seed=run_seed(s.exp, s.run, spec.name))     # what the run was generated from
    st = dark.DarkStats.load(s.merged)
    mean, rms, cnt = st.mean()[0], st.rms()[0], st.cnt[0]
    err = np.abs(mean - true.pedestals[s.g].reshape(-1).astype(np.float64))
    bound = 6.0 * rms / np.sqrt(cnt)
    print(f"{s.det}: max error {err.max():.3f} ADU, rms {rms.min():.2f}-{rms.max():.2f}, bound >= {bound.min():.3f}")
    assert np.all(cnt == N_DARK) and np.all(err <= bound), (float(err.max()), float((err - bound).max()))
    # the derived constants carry float32(mean) in that range and the base values everywhere else
    got = CalibConstants.load(s.consts, spec)
    assert np.array_equal(got.pedestals[s.g].reshape(-1), mean.astype(np.float32))
    for g in range(spec.n_gains):
        if g != s.g:
            assert np.array_equal(got.pedestals[g].view(np.int32), true.pedestals[g].view(np.int32))
    assert np.array_equal(got.gains.view(np.int32), true.gains.view(np.int32))
    assert int((got.status != 0).sum()) <= spec.npix // 100       # robust 6-sigma limits on clean data


def _read_all(addr, n_events, want_calibrator):
    """Every frame of the session through an in-process DataReader: {idx: frame}, and the reader's recipe."""
    from psana_ray_amd.data_reader import DataReader, EndOfStream

    got = {}
    with DataReader(addr, device="cpu", timeout_s=60) as reader:
        assert (reader.calibrator is not None) == want_calibrator
        recipe = (reader.session_meta or {}).get("calibrate_on_read")
        while True:
            try:
                item = reader.read(timeout=1.0)
            except EndOfStream:
                break
            if item is None:
                continue
            rank, idx, data, _pe = item
            got[int(idx)] = torch.as_tensor(data).clone()
    assert sorted(got) == list(range(n_events))
    return got, recipe


@pytest.mark.parametrize("on_read", [False, True], ids=["calib", "calibrate_on_read"])
def test_producer_calibrates_with_the_derived_constants(dark_session, on_read):
    from psana_ray_amd.data_reader import DataReader, DataReaderError
    from psana_ray_amd.models import CalibConstants, get_detector, run_seed
    from psana_ray_amd.models.constants import file_sha256
    from psana_ray_amd.ops import reference

    s = dark_session
    spec = get_detector(s.det)
    n = 10
    addr = _addr()
    prod = _producer([*s.src_args, "--calib", "--common_mode", "off", "--constants", s.consts, "--num_events", str(n),
                      "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                      *(["--calibrate_on_read"] if on_read else [])])
    try:
        got, recipe = _read_all(addr, n, on_read)
    finally:
        (rc, out), = _finish([prod])
    assert rc == 0, out[-3000:]
    assert f"sha256 {file_sha256(s.consts)}" in out and os.path.abspath(s.consts) in out
    raw = torch.from_numpy(_run_frames(s.dir, s.exp, s.run, s.det)[:n].astype(np.int32))
    loaded = CalibConstants.load(s.consts, spec)
    want = reference.calibrate_reference(raw, loaded, None, None)
    rand = reference.calibrate_reference(raw, CalibConstants.random(spec, seed=run_seed(s.exp, s.run, spec.name)),
                                         None, None)
    for i in range(n):
        assert got[i].dtype == torch.float32 and torch.equal(got[i].reshape(want[i].shape), want[i]), i
        assert not torch.equal(got[i].reshape(rand[i].shape), rand[i]), i
    if on_read:
        cf = recipe["constants"]
        assert cf == {"path": os.path.abspath(s.consts), "sha256": file_sha256(s.consts)}
        cal = DataReader._make_calibrator(recipe, torch.device("cpu"))       # the recipe as published: fine
        assert np.array_equal(cal.consts.pedestals, loaded.pedestals)
        with pytest.raises(DataReaderError, match="sha256"):
            DataReader._make_calibrator({**recipe, "constants": {**cf, "sha256": "0" * 64}}, torch.device("cpu"))
        with pytest.raises(DataReaderError, match="cannot be read"):
            DataReader._make_calibrator({**recipe, "constants": {**cf, "path": cf["path"] + ".gone"}},
                                        torch.device("cpu"))


def test_calibrate_on_read_queue_is_read_raw(native, tmp_path):
    """A --calibrate_on_read queue carries RAW items: --task dark reads them as they are (no calibration),
    inside an ADU window."""
    from psana_ray_amd import dark
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    addr, n, out = _addr(), 8, str(tmp_path / "c.npz")
    prod = _producer(["--exp", "synthetic", "--run", "9", "--detector_name", "tiny_epix", "--num_events", str(n),
                      "--calibrate_on_read", "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4"])
    cons = _consumer(addr, 0, ["--out", out, "--adu_min", "2400", "--adu_max", "2600"])
    for rc, text in _finish([prod, cons]):
        assert rc == 0, text[-3000:]
    src = SyntheticRun("synthetic", 9, "tiny_epix", rank=0, size=1)   # pool generated as the producer process generates it
    raw = np.stack([src.pool[i % src.pool_frames] for i in range(n)])
    cnt, sm, sq = reference.dark_accumulate_reference(_u16(raw), 0, 2400, 2600)
    st = dark.DarkStats.load(out)
    assert (st.frames, st.adu_lo, st.adu_hi) == (n, 2400, 2600) and 0 < int(cnt.sum()) < n * src.spec.npix
    assert np.array_equal(st.cnt, cnt.to(torch.int64).numpy()) and np.array_equal(st.sum, sm.numpy())
    assert np.array_equal(st.sq, sq.numpy())


# ------------------------------------------------------------------------------------- refusals
def _one_line(out, tag):
    lines = [l for l in out.splitlines() if tag in l]
    assert len(lines) == 1 and "Traceback" not in out, out[-3000:]
    return lines[0]


def test_producer_refusals_exit_2(native, tmp_path):
    from psana_ray_amd.models import CalibConstants, get_detector

    syn = ["--exp", "synthetic", "--run", "2", "--detector_name", "tiny_epix", "--num_events", "4"]
    jf = CalibConstants.random(get_detector("tiny_jungfrau"), seed=1).save(tmp_path / "jf.npz")
    ep = CalibConstants.random(get_detector("tiny_epix"), seed=1).save(tmp_path / "ep.npz")
    pf = ["--calib", "--local", "--consumer_task", "peakfind", "--constants"]
    procs = [
        _producer([*syn, "--calib", "--local", "--consumer_task", "dark"]),          # dark statistics need raw frames
        _producer([*syn, "--mode", "raw", "--panel_shards", "2", "--local", "--consumer_task", "dark"]),
        _producer([*syn, *pf, jf]),                                                   # constants of another detector
        _producer([*syn, *pf, str(tmp_path / "missing.npz")]),
        _producer(["--exp", "mfxl1038923", "--run", "58", "--detector_name", "tiny_epix", *pf, ep], stub=True),
    ]
    outs = _finish(procs)
    for rc, out in outs:
        assert rc == 2, out[-3000:]
    assert "--mode raw" in _one_line(outs[0][1], "--consumer_task dark")
    assert "--consumer_task dark" in outs[1][1] and "Traceback" not in outs[1][1]
    assert "tiny_jungfrau" in _one_line(outs[2][1], "--constants")
    assert "--constants" in outs[3][1] and "Traceback" not in outs[3][1]
    assert "psana_wrapper" in _one_line(outs[4][1], "--constants")     # a psana_wrapper source keeps psana's constants


def test_consumer_refuses_a_float_queue(native):
    addr = _addr()
    prod = _producer(["--exp", "synthetic", "--run", "2", "--detector_name", "tiny_epix", "--num_events", "4", "--calib",
                      "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4"])
    cons = _consumer(addr, 0, [])
    try:
        out, _ = cons.communicate(timeout=120)
    finally:
        for p in (prod, cons):
            if p.poll() is None:
                p.kill()
        prod.communicate()
    assert cons.returncode == 2, out[-3000:]
    assert "float32" in _one_line(out, "--task dark")


def test_consumer_refuses_panel_shards(native):
    addr = _addr()
    prods = [_producer(["--exp", "synthetic", "--run", "2", "--detector_name", "tiny_epix", "--num_events", "4",
                        "--mode", "raw", "--panel_shards", "2", "--ray_address", addr, "--num_consumers", "1",
                        "--queue_size", "4"], rank=r, size=2) for r in range(2)]
    cons = _consumer(addr, 0, [])
    try:
        out, _ = cons.communicate(timeout=120)
    finally:
        for p in prods + [cons]:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    assert cons.returncode == 2, out[-3000:]
    assert "panel shards" in _one_line(out, "--task dark")


def test_consumer_refuses_an_unnamed_detector_and_a_wrong_one(caplog):
    """A session that does not name its detector (and no --detector_name): rc 2, one line; a named
    detector whose frames are not the ring's: rc 2."""
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 32, 48), torch.uint16, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "dark"])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_dark(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            args.detector_name = "tiny_jungfrau"
            assert consumer.run_dark(args, reader, {"flag": False}, {"n": 0}) == 2
            args.detector_name, args.adu_min, args.adu_max = "tiny_epix", 9, 8
            assert consumer.run_dark(args, reader, {"flag": False}, {"n": 0}) == 2
            reader.endpoint = None
            assert consumer.run_dark(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_dark_module_cli_refusals(native, tmp_path):
    from psana_ray_amd import dark

    a = dark.DarkStats("tiny_plain", 2, 0, 65535, 1, np.ones((1, 256)), np.ones((1, 256)), np.ones((1, 256)))
    b = dark.DarkStats("tiny_plain", 2, 1, 65535, 1, np.ones((1, 256)), np.ones((1, 256)), np.ones((1, 256)))
    fa, fb = a.save(tmp_path / "a.npz"), b.save(tmp_path / "b.npz")
    assert dark.main(["merge", fa, fb, "--out", str(tmp_path / "m.npz")]) == 2          # another window
    assert dark.main(["merge", fa, fa, "--out", str(tmp_path / "m.npz")]) == 0
    assert dark.main(["derive", fa, "--out", str(tmp_path / "c.npz")]) == 2               # no base constants
    assert dark.main(["derive", fa, "--out", str(tmp_path / "c.npz"), "--exp", "nosuchexp", "--run", "1"]) == 2
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.dark", "derive", str(tmp_path / "missing.npz"), "--out",
                        str(tmp_path / "c.npz"), "--base", fa], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "Traceback" not in r.stderr, r.stderr[-2000:]
    assert not (tmp_path / "c.npz").exists()
