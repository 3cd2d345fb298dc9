"""``psana-ray-consumer --task photons`` / ``psana-ray-producer --consumer_task photons`` as separate processes
on CPU sessions (tiny_epix; the CPU endpoints run the golden model) and the ``python -m
psana_ray_amd.photons`` CLI on their files."""
import json
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

from psana_ray_amd import photons as PH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9
ADU = 20.0
PHOT = ["--adu_per_photon", str(ADU)]


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
                             "--device", "cpu", "--timeout", "60", "--task", "photons", "--metrics_interval", "0", *extra],
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


def _golden(frames, shape, mask=None, roi=None, **par):
    from psana_ray_amd.ops import reference

    return reference.photon_count_reference(frames.reshape(frames.shape[0], -1), shape,
                                            dict(adu_per_photon=ADU, **par), mask, roi)


def _equals_golden(st, want):
    for k in ("cnt", "psum", "occ", "pk", "tot"):
        g, w = getattr(st, k), getattr(want, k).numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), k


def _same_bytes(a, b):
    with np.load(a, allow_pickle=False) as za, np.load(b, allow_pickle=False) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), k


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers, the co-located consumer of a --local producer (the
    single-consumer file), and one consumer with a mask, ROIs and other thresholds."""
    d = tmp_path_factory.mktemp("photons_cli")
    rng = np.random.default_rng(4)
    mask = (rng.random((2, 32, 48)) < 0.9).astype(np.uint8)
    roi = rng.choice(np.array([0, 1, 255], np.int64), size=(2, 32, 48))   # integer labels of another dtype load too
    np.save(d / "mask.npy", mask)
    np.save(d / "roi.npy", roi)
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "2", "--queue_size", "6"]),
                    *[_consumer(addr, c, ["--batch", "6", "--out", two[c], *PHOT]) for c in range(2)]])
    local = str(d / "local.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--local",
                                "--consumer_task", "photons", "--out_photons", local, *PHOT])])
    addr1 = _addr()
    plain = str(d / "plain.npz")
    outs += _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address",
                                addr1, "--num_consumers", "1", "--queue_size", "6"]),
                     _consumer(addr1, 0, ["--batch", "7", "--out", plain, *PHOT, "--photon_vmax", "1000", "--photon_seed",
                                          "0.4", "--photon_total", "0.75", "--photon_mask", str(d / "mask.npy"),
                                          "--photon_roi", str(d / "roi.npy")])])
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, plain=plain, outs=outs, mask=mask, roi=roi)


def test_task_photons_end_to_end_and_two_consumers_merge_to_one(sessions):
    s = sessions
    frames = _golden_frames(N_EVENTS)
    want = _golden(frames, (2, 32, 48))
    each = [PH.PhotonStats.load(f) for f in s.two]
    assert sum(e.frames for e in each) == N_EVENTS
    m = PH.merge(s.two)
    assert m.frames == N_EVENTS and m.gevt.tolist() == list(range(N_EVENTS))
    _equals_golden(m, want)
    assert (m.detector, m.layout, m.shape, m.adu_per_photon, m.thr_seed, m.n_roi) == \
        ("tiny_epix", "calib", (2, 32, 48), ADU, 0.5, 1)
    assert m.vmax == 250 * ADU and m.roi_npix.tolist() == [m.n] and 0 < int(m.psum.sum())
    # --local --consumer_task photons gives the same bytes as the merge CLI's file, in every array
    out = str(s.dir / "merged.npz")
    assert PH.main(["merge", *s.two, "--out", out]) == 0
    _same_bytes(out, s.local)
    # the lines of the CLIs: the parameters at start, frames at the end
    cons_out = [o for _, o in s.outs[1:3]]
    assert all("photons: adu_per_photon=20 vmax=5000 seed=0.5 total=0.9 rois=1" in o for o in cons_out), cons_out[0][-2000:]
    finals = [l for o in cons_out for l in o.splitlines() if re.search(r"Consumer \d photons: frames=\d+ ", l)]
    assert sorted(int(re.search(r"frames=(\d+)", l).group(1)) for l in finals) == sorted(e.frames for e in each)
    assert f"Consumer 0 photons: frames={N_EVENTS} " in s.outs[3][1], s.outs[3][1][-2000:]


def test_file_round_trip_is_bitwise(sessions, tmp_path):
    st = PH.PhotonStats.load(sessions.plain)
    again = st.save(tmp_path / "again.npz")
    _same_bytes(again, sessions.plain)
    with np.load(again, allow_pickle=False) as z:
        assert z["inv"].dtype == np.float32 and float(z["inv"]) == float(np.float32(1.0 / np.float64(np.float32(ADU))))
        assert z["roi_npix"].dtype == np.int64 and z["cnt"].dtype == np.int32 and z["psum"].dtype == np.int64
        assert z["pk"].shape == (N_EVENTS, 2, 8) and z["tot"].shape == (N_EVENTS, 2)
        broken = {k: z[k] for k in z.files}
    broken["inv"] = np.float32(0.25)
    with open(tmp_path / "broken.npz", "wb") as f:
        np.savez(f, **broken)
    with pytest.raises(ValueError, match="inv"):
        PH.PhotonStats.load(tmp_path / "broken.npz")
    del broken["occ"]
    with open(tmp_path / "short.npz", "wb") as f:
        np.savez(f, **broken)
    with pytest.raises(ValueError, match="not a photon-statistics file"):
        PH.PhotonStats.load(tmp_path / "short.npz")


def test_mask_rois_other_thresholds_and_the_photons_cli(sessions, capsys):
    s = sessions
    st = PH.PhotonStats.load(s.plain)
    frames = _golden_frames(N_EVENTS)
    roi8 = s.roi.astype(np.uint8).reshape(-1)
    _equals_golden(st, _golden(frames, (2, 32, 48), s.mask.reshape(-1), roi8, vmax=1000.0, thr_seed=0.4, thr_total=0.75))
    assert (st.vmax, st.thr_seed, st.thr_total, st.n_roi, st.frames) == (1000.0, float(np.float32(0.4)), 0.75, 2, N_EVENTS)
    assert st.roi_npix.tolist() == [int(((roi8 == r) & (s.mask.reshape(-1) != 0)).sum()) for r in range(2)]
    assert int(st.cnt[s.mask.reshape(-1) == 0].sum()) == 0
    tab = st.pk_table(1)
    assert tab.shape == (N_EVENTS, 9) and (tab.sum(axis=1) == st.roi_npix[1]).all()
    assert np.array_equal(st.kbar(0), st.tot[:, 0] / st.roi_npix[0])
    # the merge refusals: other parameters / ROI hash, a gevt present twice
    with pytest.raises(ValueError, match="differ in"):
        PH.merge([s.plain, s.local])
    assert PH.main(["merge", s.plain, s.local, "--out", str(s.dir / "no.npz")]) == 2
    with pytest.raises(ValueError, match="present twice"):
        PH.merge([s.local, *s.two])
    assert PH.main(["merge", s.local, *s.two, "--out", str(s.dir / "no.npz")]) == 2
    with pytest.raises(ValueError, match="no files"):
        PH.merge([])
    capsys.readouterr()
    assert PH.main(["info", s.local]) == 0
    info = json.loads(capsys.readouterr().out)
    one = PH.PhotonStats.load(s.local)
    assert info["frames"] == N_EVENTS and info["shape"] == [2, 32, 48] and info["adu_per_photon"] == ADU
    assert info["photons"] == int(one.psum.sum()) and info["roi_npix"] == [one.n] and info["roi_sha256"] == one.roi_sha256
    prefix = str(s.dir / "run")
    assert PH.main(["export", s.local, "--out_prefix", prefix]) == 0
    mp, oc = np.load(prefix + "_mean_photons.npy"), np.load(prefix + "_occupancy.npy")
    assert mp.shape == oc.shape == (2, 32, 48) and mp.dtype == np.float64
    assert np.array_equal(mp.reshape(-1), one.mean_photons(), equal_nan=True)
    assert np.array_equal(oc.reshape(-1), one.occupancy(), equal_nan=True)
    assert PH.main(["info", str(s.dir / "missing.npz")]) == 2


def test_merge_refuses_other_detector_shape_rois_and_a_run_past_the_bound(tmp_path):
    from psana_ray_amd.ops.reference import validate_photon_params

    pp = validate_photon_params(ADU)

    def make(path, detector="t", shape=(2, 3, 4), roi=None, frames=2, g0=0, adu=ADU):
        n = int(np.prod(shape))
        st = PH.PhotonStats.from_maps(detector, "calib", shape, validate_photon_params(adu), None, roi, None, frames,
                                      np.full(n, frames, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32),
                                      rank=[0] * frames, idx=list(range(frames)), gevt=list(range(g0, g0 + frames)),
                                      photon_energy=[1.0] * frames)
        return st.save(tmp_path / path)

    a = make("a.npz")
    assert PH.merge([a, make("b.npz", g0=2)]).frames == 4
    for name, kw in (("detector", dict(detector="u")), ("shape", dict(shape=(2, 4, 3))),
                     ("roi_sha256", dict(roi=np.array([0, 255] * 12, np.uint8))),
                     ("n_roi", dict(roi=np.array([0, 1] * 12, np.uint8))), ("adu_per_photon", dict(adu=ADU + 1))):
        with pytest.raises(ValueError, match=name):
            PH.merge([a, make("c.npz", g0=2, **kw)])
    with pytest.raises(ValueError, match="present twice"):
        PH.merge([a, make("d.npz", g0=1)])
    big = PH.PhotonStats.load(a)
    big.frames = 2 ** 31 - 2
    with pytest.raises(ValueError, match="longer than 2147483647"):
        big.add(PH.PhotonStats.load(make("e.npz", g0=2)))
    assert pp.inv == PH.PhotonStats.load(a).inv


def test_calibrate_on_read_queue_is_calibrated_then_counted(native, tmp_path):
    """A --calibrate_on_read queue carries RAW frames: the consumer calibrates (image mode, common mode)
    and counts photons in the image."""
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    shape = make_geometry(get_detector("tiny_epix")).image_shape
    addr = _addr()
    out = str(tmp_path / "c.npz")
    outs = _finish([_producer(["--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                               "--common_mode", "default", "--calibrate_on_read"]),
                    _consumer(addr, 0, ["--out", out, "--batch", "4", *PHOT])])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    st = PH.PhotonStats.load(out)
    assert st.layout == "image" and st.shape == (1, *shape) and st.frames == n
    _equals_golden(st, _golden(_golden_frames(n, "image", "default"), (1, *shape)))
    assert st.gevt.tolist() == list(range(n))


def test_refusals_exit_2(native, tmp_path, caplog):
    """No --adu_per_photon; a raw uint16 queue without a recipe, a panel-sharded session, parameters out of
    range, an unnamed detector; the co-located form's refusals; --out_photons without the task."""
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", _addr(), "--device", "cpu",
                        "--task", "photons"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--task photons needs --adu_per_photon" in r.stderr and "Traceback" not in r.stderr
    a_raw, a_shard, a_par = _addr(), _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)],
             _producer(["--calib", "--num_events", "4", "--ray_address", a_par, "--num_consumers", "1",
                        "--queue_size", "4"])]
    cons = [_consumer(a_raw, 0, PHOT), _consumer(a_shard, 0, PHOT),
            _consumer(a_par, 0, [*PHOT, "--photon_vmax", str(255 * ADU)])]
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards", "at most 254")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task photons" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # the co-located form refuses the same sessions before it starts, and --out_photons without the task
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "photons", *PHOT, *extra], env=_env(), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task photons needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_photons", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_photons belongs to --consumer_task photons" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "photons"], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--consumer_task photons needs --adu_per_photon" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "photons", *PHOT, "--photon_seed", "0.95"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "thr_seed <= thr_total" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    np.save(tmp_path / "bad_roi.npy", np.zeros((2, 32, 47), np.uint8))
    r = subprocess.run([*base, "--calib", "--consumer_task", "photons", *PHOT, "--photon_roi", str(tmp_path / "bad_roi.npy")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--photon_roi is (2, 32, 47)" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    # a session that does not name its detector (and no --detector_name): rc 2, one line
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 32, 48), torch.float32, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                   session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "photons", *PHOT])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_photons(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_photons(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located photon consumers write PATH as PATH.r<rank>.npz; the files merge to
    the golden model over all events."""
    addr = _addr()
    out = str(tmp_path / "photons.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "photons", "--out_photons",
                               out, *PHOT], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"photons.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = PH.merge(files)
    assert m.frames == N_EVENTS and (np.diff(m.gevt) > 0).all() and sorted(set(m.rank.tolist())) == [0, 1]
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    frames = []
    for r in range(2):
        src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=r, size=2, n_events=N_EVENTS)
        raw = np.stack([src.pool[k % src.pool_frames] for k in range(src.n_local_events())]).astype(np.int32)
        frames.append(reference.calibrate_reference(torch.from_numpy(raw), src.consts, None, None))
    want = _golden(torch.cat(frames), (2, 32, 48))
    for k in ("cnt", "psum", "occ"):
        assert np.array_equal(getattr(m, k), getattr(want, k).numpy()), k
    # the per-frame rows are ordered by gevt, the golden frames by rank: compare as multisets of rows
    rows = lambda pk, tot: sorted(map(tuple, np.concatenate([pk.reshape(len(pk), -1), tot], axis=1).tolist()))   # noqa: E731
    assert rows(m.pk, m.tot) == rows(want.pk.numpy(), want.tot.numpy())


def test_consumer_on_a_cpu_ring_and_the_frame_bound():
    """The consumer's CPU path, and its refusal -- a ValueError before any lease or launch -- of what would
    take the run past 2^31 - 1 frames."""
    from psana_ray_amd.pipeline import PhotonConsumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing((2, 3, 4), torch.float32, "cpu", 2, 2))
    try:
        cons = PhotonConsumer(ep, (2, 3, 4), 2.0, detector="t", batch=4)
        x = [torch.full((2, 3, 4), 6.0) for _ in range(3)]
        cons.process_frames(x, [(0, i, i) for i in range(3)])
        st = cons.stats()
        assert cons.frames == 3 and st.psum.tolist() == [9] * 24 and st.pk[:, 0, 2].tolist() == [24] * 3
        assert st.tot[:, 0].tolist() == [72] * 3 and st.kbar(0).tolist() == [3.0] * 3
        cons.frames = 2 ** 31 - 1 - 2
        with pytest.raises(ValueError, match="past 2147483647"):
            cons.process_frames(x, [(0, i, i) for i in range(3)])
        cons.frames = 2 ** 31 - 1
        with pytest.raises(ValueError, match="past 2147483647"):
            cons.poll(timeout=0.0)
        with pytest.raises(ValueError, match="batch of at most"):
            cons.frames = 0
            cons.process_frames(x + x, [(0, i, i) for i in range(6)])
    finally:
        ep.close()


def test_the_readmes_command_lines_still_parse():
    """Every psana-ray-producer / psana-ray-consumer command line in the README's code blocks parses with the
    parsers as they are now, the photon task's among them."""
    from psana_ray_amd import consumer, producer

    text = open(os.path.join(ROOT, "README.md")).read().replace("\\\n", " ")
    blocks = re.findall(r"```[a-z]*\n(.*?)```", text, flags=re.S)
    found = {"producer": 0, "consumer": 0}
    photons = {"producer": 0, "consumer": 0}
    for block in blocks:
        for prog, rest in re.findall(r"psana-ray-(producer|consumer)((?: +[^\s&;#|`]+)*)", block):
            argv = shlex.split(rest.replace("$c", "0"))
            if not argv or any(a.startswith(("/", "-consumer")) for a in argv[:1]):
                continue
            parser = producer.build_parser() if prog == "producer" else consumer.build_parser()
            try:
                ns = parser.parse_args(argv)
            except SystemExit:
                pytest.fail(f"psana-ray-{prog} {rest} no longer parses")
            found[prog] += 1
            if getattr(ns, "task", None) == "photons" or getattr(ns, "consumer_task", None) == "photons":
                photons[prog] += 1
                assert ns.adu_per_photon is not None
    assert found["producer"] >= 5 and found["consumer"] >= 5, found
    assert photons["producer"] >= 1 and photons["consumer"] >= 1, photons
    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "photons" in r.stdout and "--adu_per_photon" in r.stdout, r.stderr[-2000:]
