"""``psana-ray-consumer --task droplets`` / ``psana-ray-producer --consumer_task droplets`` as separate processes
on CPU sessions (tiny_epix; the CPU endpoints run the golden model), a GPU twin of the end-to-end case over HIP
IPC, and the ``python -m psana_ray_amd.droplets`` CLI on their files."""
import os
import random
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from psana_ray_amd import droplets as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_EVENTS = 20
RUN = 9
SHAPE = (2, 32, 48)
DROP = ["--drop_thr_low", "15", "--drop_thr_seed", "30", "--drop_frac_bits", "3", "--drop_pix_cap", "2048", "--drop_cap", "256"]
PAR = dict(thr_low=15.0, thr_seed=30.0, frac_bits=3)
COLS = ("label", "npix", "adu", "sy", "sx", "qmax")


def _env(extra=None):
    env = dict(os.environ)
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "PSANA_RAY_DATA"):
        env.pop(k, None)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    env.update(extra or {})
    return env


def _addr():
    return f"127.0.0.1:{random.randint(30000, 45000)}"


def _producer(extra, rank=0, size=1, device="cpu"):
    return subprocess.Popen(
        [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
         "tiny_epix", "--device", device, "--timeout", "60", *extra],
        env=_env({"RANK": str(rank), "WORLD_SIZE": str(size), "LOCAL_RANK": "0"}), stdout=subprocess.PIPE,
        stderr=subprocess.STDOUT, text=True)


def _consumer(addr, cid, extra, device="cpu"):
    return subprocess.Popen([sys.executable, "-m", "psana_ray_amd.consumer", str(cid), "--ray_address", addr,
                             "--device", device, "--timeout", "60", "--task", "droplets", "--metrics_interval", "0", *extra],
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


def _golden_frames(n_events):
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=0, size=1)
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    return reference.calibrate_reference(raw, src.consts, None, None)


def _equals_golden(df, frames, mask=None):
    """df: DropletFrames ordered by gevt == frame number; frame by frame against the golden model."""
    from psana_ray_amd.ops import reference

    n = int(np.prod(SHAPE))
    for i in range(len(df)):
        w = reference.droplet_reference(frames[i:i + 1].reshape(1, n), SHAPE, PAR, mask, 2048, 256)
        assert (int(df.nact[i]), int(df.ndrop[i]), int(df.flags[i])) == (int(w.nact[0]), int(w.ndrop[0]), int(w.flags[0]))
        got = df.frame(i)
        for k in COLS:
            assert got[k].dtype == getattr(w, k).numpy().dtype and np.array_equal(got[k], getattr(w, k).numpy()), (k, i)


def _same_bytes(a, b):
    with np.load(a, allow_pickle=False) as za, np.load(b, allow_pickle=False) as zb:
        assert sorted(za.files) == sorted(zb.files)
        for k in za.files:
            assert za[k].dtype == zb[k].dtype and za[k].shape == zb[k].shape and za[k].tobytes() == zb[k].tobytes(), k


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers, the co-located consumer of a --local producer (the
    single-consumer file), and one consumer with a mask."""
    d = tmp_path_factory.mktemp("droplets_cli")
    mask = (np.random.default_rng(4).random(SHAPE) < 0.9).astype(np.uint8)
    np.save(d / "mask.npy", mask)
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    base = ["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS)]
    outs = _finish([_producer([*base, "--ray_address", addr, "--num_consumers", "2", "--queue_size", "6"]),
                    *[_consumer(addr, c, ["--batch", "6", "--out", two[c], *DROP]) for c in range(2)]])
    local = str(d / "local.npz")
    outs += _finish([_producer([*base, "--local", "--consumer_task", "droplets", "--out_droplets", local, *DROP])])
    addr1 = _addr()
    masked = str(d / "masked.npz")
    outs += _finish([_producer([*base, "--ray_address", addr1, "--num_consumers", "1", "--queue_size", "6"]),
                     _consumer(addr1, 0, ["--batch", "7", "--out", masked, *DROP, "--drop_mask", str(d / "mask.npy")])])
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, masked=masked, outs=outs, mask=mask)


def test_task_droplets_end_to_end_and_two_consumers_merge_to_one(sessions):
    s = sessions
    frames = _golden_frames(N_EVENTS)
    each = [DR.DropletFrames.load(f) for f in s.two]
    assert sum(len(e) for e in each) == N_EVENTS
    m = DR.merge(s.two)
    assert len(m) == N_EVENTS and m.gevt.tolist() == list(range(N_EVENTS)) and int(m.offs[-1]) > 100
    _equals_golden(m, frames)
    assert (m.detector, m.layout, m.shape, m.thr_low, m.thr_seed, m.vmax, m.frac_bits, m.pix_cap, m.cap, m.mask_sha256) == \
        ("tiny_epix", "calib", SHAPE, 15.0, 30.0, 2.0 ** 20, 3, 2048, 256, "")
    # --local --consumer_task droplets gives the same bytes as the merge CLI's file, in every array
    out = str(s.dir / "merged.npz")
    assert DR.main(["merge", *s.two, "--out", out]) == 0
    _same_bytes(out, s.local)
    # the spectrum of the merged file is the single file's, through the CLI too
    one = DR.DropletFrames.load(s.local)
    assert np.array_equal(m.spectrum(0.0, 4000.0, 100), one.spectrum(0.0, 4000.0, 100))
    assert int(one.spectrum(0.0, 1e9, 7).sum()) == int(one.offs[-1]) and one.spectrum(0.0, 4000.0, 100).dtype == np.int64
    sa, sb = str(s.dir / "sa.npy"), str(s.dir / "sb.npy")
    assert DR.main(["spectrum", *s.two[::-1], "--lo", "0", "--hi", "4000", "--nbins", "100", "--out", sa]) == 0
    assert DR.main(["spectrum", s.local, "--lo", "0", "--hi", "4000", "--nbins", "100", "--out", sb]) == 0
    assert np.array_equal(np.load(sa), np.load(sb)) and np.array_equal(np.load(sa), one.spectrum(0.0, 4000.0, 100))
    # the lines of the CLIs: the parameters at start, frames and overflowed= at the end
    cons_out = [o for _, o in s.outs[1:3]]
    assert all("droplets: thr_low=15 thr_seed=30 vmax=1.04858e+06 frac_bits=3 pix_cap=2048 cap=256" in o
               for o in cons_out), cons_out[0][-2000:]
    finals = [l for o in cons_out for l in o.splitlines() if re.search(r"Consumer \d droplets: frames=\d+ ", l)]
    assert sorted(int(re.search(r"frames=(\d+)", l).group(1)) for l in finals) == sorted(len(e) for e in each)
    assert all("overflowed=0" in l for l in finals)
    assert f"Consumer 0 droplets: frames={N_EVENTS} " in s.outs[3][1] and "overflowed=0" in s.outs[3][1], s.outs[3][1][-2000:]


def test_mask_file_round_trip_and_views(sessions, tmp_path, capsys):
    df = DR.DropletFrames.load(sessions.masked)
    assert df.mask_sha256 == DR.mask_hash(SHAPE, sessions.mask) != ""
    _equals_golden(df.select(np.argsort(df.gevt)), _golden_frames(N_EVENTS), sessions.mask.reshape(-1))
    again = df.save(tmp_path / "again.npz")
    _same_bytes(again, sessions.masked)
    with np.load(again, allow_pickle=False) as z:
        assert str(z["format"]) == DR.DROPLET_FORMAT and z["thr_low"].dtype == np.float32 and z["adu"].dtype == np.int64
        assert z["label"].dtype == np.int32 and z["offs"].shape == (N_EVENTS + 1,) and z["flags"].dtype == np.uint8
        broken = {k: z[k] for k in z.files}
    # views
    e = df.energy()
    assert e.dtype == np.float64 and np.array_equal(e, df.adu / 8.0)
    assert np.array_equal(df.photons(20.0), np.floor(e / 20.0 + 0.5).astype(np.int64)) and df.photons(20.0).dtype == np.int64
    panel, y, x = df.com(3)
    f3 = df.frame(3)
    assert np.array_equal(panel, f3["label"] // (32 * 48)) and np.allclose(y, f3["sy"] / f3["adu"])
    assert ((y >= 0) & (y <= 31) & (x >= 0) & (x <= 47)).all()
    pm = df.photon_map(3, 20.0)
    assert pm.shape == SHAPE and pm.dtype == np.int32 and int(pm.sum()) == int(df.photons(20.0)[df.offs[3]:df.offs[4]].sum())
    # merge refusals: other parameters, another mask, a gevt twice; a file that is not one
    assert DR.main(["merge", sessions.masked, sessions.local, "--out", str(tmp_path / "x.npz")]) == 2
    assert "mask_sha256" in capsys.readouterr().err
    assert DR.main(["merge", sessions.local, sessions.local, "--out", str(tmp_path / "x.npz")]) == 2
    assert "present twice" in capsys.readouterr().err
    for key, val in (("thr_low", np.float32(16.0)), ("detector", np.asarray("other")), ("frac_bits", np.int64(2))):
        other = dict(broken)
        other[key] = val
        with open(tmp_path / "other.npz", "wb") as f:
            np.savez(f, **other)
        with pytest.raises(ValueError, match=key):
            DR.merge([sessions.masked, str(tmp_path / "other.npz")])
    del broken["sy"]
    with open(tmp_path / "broken.npz", "wb") as f:
        np.savez(f, **broken)
    with pytest.raises(ValueError, match="no sy"):
        DR.DropletFrames.load(tmp_path / "broken.npz")
    assert DR.main(["info", sessions.masked]) == 0
    assert f"frames={N_EVENTS} stored={N_EVENTS} overflowed=0" in capsys.readouterr().out
    out = str(tmp_path / "map.npy")
    assert DR.main(["export", sessions.masked, "--gevt", "3", "--adu_per_photon", "20", "--out", out]) == 0
    i = int(np.flatnonzero(df.gevt == 3)[0])
    assert np.array_equal(np.load(out), df.photon_map(i, 20.0))
    assert DR.main(["export", sessions.masked, "--adu_per_photon", "20", "--out", out]) == 2
    capsys.readouterr()


def test_photon_map_places_photons_at_the_rounded_centre():
    from psana_ray_amd.ops import reference

    x = np.zeros((1, 6, 6), np.float32)
    x[0, 1:3, 1:3] = [[3.0, 3.0], [2.0, 2.0]]      # one photon: centre (1.4, 1.5) -> (1, 2)
    x[0, 4, 4] = 21.0                              # two photons in one pixel
    x[0, 0, 5] = 4.0                               # 0.4 photons: rounds to none
    g = reference.droplet_reference(torch.as_tensor(x).reshape(1, -1), (1, 6, 6), dict(thr_low=1.5), cap_pix=36, cap=36)
    df = DR.DropletFrames.from_lists("t", "calib", (6, 6), reference.validate_droplet_params(1.5), None, [0], [0], [7], [0.0],
                                     g.nact.numpy(), g.ndrop.numpy(), g.flags.numpy(), g.offs.numpy(),
                                     {k: getattr(g, k).numpy() for k in COLS}, pix_cap=36, cap=36)
    assert df.shape == (1, 6, 6) and df.photons(10.0).tolist() == [0, 1, 2]
    pm = df.photon_map(0, 10.0)
    want = np.zeros((1, 6, 6), np.int32)
    want[0, 1, 2] = 1
    want[0, 4, 4] = 2
    assert np.array_equal(pm, want)
    over = DR.DropletFrames("t", "calib", (6, 6), 1.5, 1.5, 100.0, 2, 4, 4, "", [0], [0], [1], [0.0], [9], [0], [4], [0, 0])
    with pytest.raises(ValueError, match="overflowed"):
        over.photon_map(0, 10.0)
    with pytest.raises(ValueError, match="offs disagree"):
        DR.DropletFrames("t", "calib", (6, 6), 1.5, 1.5, 100.0, 2, 4, 4, "", [0], [0], [1], [0.0], [9], [2], [0], [0, 0])


def test_refusals_exit_2(native, tmp_path, caplog):
    """No --drop_thr_low; a raw uint16 queue without a recipe, a panel-sharded session, parameters out of range,
    an unnamed detector; the co-located form's refusals; --out_droplets without the task."""
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", _addr(), "--device", "cpu",
                        "--task", "droplets"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--task droplets needs --drop_thr_low" in r.stderr and "Traceback" not in r.stderr
    a_raw, a_shard, a_par = _addr(), _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)],
             _producer(["--calib", "--num_events", "4", "--ray_address", a_par, "--num_consumers", "1",
                        "--queue_size", "4"])]
    cons = [_consumer(a_raw, 0, DROP), _consumer(a_shard, 0, DROP),
            _consumer(a_par, 0, ["--drop_thr_low", "15", "--drop_thr_seed", "10"])]
    try:
        outs = [c.communicate(timeout=120)[0] for c in cons]
    finally:
        for p in prods + cons:
            if p.poll() is None:
                p.kill()
        for p in prods:
            p.communicate()
    for c, out, word in zip(cons, outs, ("raw uint16", "panel shards", "thr_low <= thr_seed")):
        assert c.returncode == 2, out[-3000:]
        lines = [l for l in out.splitlines() if "--task droplets" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "droplets", *DROP, *extra], env=_env(), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task droplets needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_droplets", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_droplets belongs to --consumer_task droplets" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "droplets"], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--consumer_task droplets needs --drop_thr_low" in r.stderr, r.stderr[-2000:]
    r = subprocess.run([*base, "--calib", "--consumer_task", "droplets", *DROP, "--drop_frac_bits", "17"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "frac_bits must be 0 .. 16" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    np.save(tmp_path / "bad_mask.npy", np.zeros((2, 32, 47), np.uint8))
    r = subprocess.run([*base, "--calib", "--consumer_task", "droplets", *DROP, "--drop_mask", str(tmp_path / "bad_mask.npy")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--drop_mask is (2, 32, 47)" in r.stderr and "Traceback" not in r.stderr, r.stderr[-2000:]
    # a session that does not name its detector (and no --detector_name): rc 2, one line
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    ep = QueueEndpoint(FrameRing(SHAPE, torch.float32, "cpu", 2, 2))
    reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                   session_meta={"detector": None})
    args = consumer.build_parser().parse_args(["--task", "droplets", *DROP])
    args.batch = 4
    try:
        with caplog.at_level("ERROR"):
            assert consumer.run_droplets(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_droplets(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located droplet consumers write PATH as PATH.r<rank>.npz; the files merge."""
    addr = _addr()
    out = str(tmp_path / "droplets.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "droplets",
                               "--out_droplets", out, *DROP], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"droplets.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = DR.merge(files)
    assert len(m) == N_EVENTS and (np.diff(m.gevt) > 0).all() and sorted(set(m.rank.tolist())) == [0, 1]
    assert int(m.offs[-1]) == int(m.ndrop.sum()) > 100 and not m.flags.any()


@pytest.mark.gpu
def test_two_processes_over_hip_ipc_task_droplets(native, cuda_device, tmp_path):
    """The GPU twin: a tiny_epix producer and ``psana-ray-consumer 0 --task droplets --out`` as two GPU processes,
    three batches: the file holds the frames sent and equals the golden model."""
    addr = _addr()
    out = str(tmp_path / "droplets.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "1", "--queue_size", "16"], device="cuda:0"),
                    _consumer(addr, 0, ["--batch", "8", "--out", out, *DROP], device="cuda:0")])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    df = DR.DropletFrames.load(out)
    assert df.detector == "tiny_epix" and df.layout == "calib" and sorted(df.gevt.tolist()) == list(range(N_EVENTS))
    _equals_golden(df.select(np.argsort(df.gevt)), _golden_frames(N_EVENTS))
    assert f"droplets: frames={N_EVENTS} " in outs[1][1] and "overflowed=0" in outs[1][1], outs[1][1][-2000:]
