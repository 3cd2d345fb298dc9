"""``psana-ray-consumer --task roibin`` / ``psana-ray-producer --consumer_task roibin`` as separate processes on CPU
sessions (tiny_epix; the CPU endpoints run the golden models), and ``python -m psana_ray_amd.roibin``."""
import glob
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
SHAPE = (2, 32, 48)                                     # tiny_epix, calib layout
MIN_PEAKS = 24                                          # between the run's smallest and largest peak count
FLAGS = ["--rb_bin", "2", "--rb_step", "0.5", "--rb_box", "2", "--rb_vmin", "-64", "--rb_vmax", "4096", "--min_peaks",
         str(MIN_PEAKS)]
ARRAYS = ("rank", "idx", "gevt", "photon_energy", "npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "rec", "box",
          "koffs", "codes")


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
                             "--device", "cpu", "--timeout", "60", "--task", "roibin", "--metrics_interval", "0", *extra],
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

    src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=0, size=1)   # generated as the producer generates it
    raw = torch.from_numpy(np.stack([src.pool[i % src.pool_frames] for i in range(n_events)]).astype(np.int32))
    return reference.calibrate_reference(raw, src.consts, None, None)


def _want(frames, mask=None):
    """The golden model's batch for frames in gevt order: the peak finder's records, then roibin."""
    from psana_ray_amd.config import PeakFinderParams
    from psana_ray_amd.ops import reference

    pp = PeakFinderParams()
    found, _ = reference.peakfind_reference(frames, pp)
    peaks = torch.zeros((len(found), pp.max_peaks, 8))
    for f, r in enumerate(found):
        peaks[f, :r.shape[0]] = r
    counts = torch.tensor([r.shape[0] for r in found], dtype=torch.int32)
    return reference.roibin_reference(frames, SHAPE, peaks, counts, bin=2, step=0.5, vmin=-64.0, vmax=4096.0, radius=2,
                                      max_peaks=pp.max_peaks, min_peaks=MIN_PEAKS, mask=mask)


def _same_files(a, b, skip=()):
    assert a.params() == b.params()
    for k in ARRAYS:
        if k in skip:
            continue
        x, y = getattr(a, k), getattr(b, k)
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers (a mask, parts of 3 frames for one of them), and the co-located
    consumer of a --local producer with the same flags."""
    d = tmp_path_factory.mktemp("roibin_cli")
    mask = np.ones(SHAPE, np.uint8)
    mask[1, 5:9, 10:30:3] = 0
    mask_file = str(d / "mask.npy")
    np.save(mask_file, mask)
    prod = ["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS)]
    flags = [*FLAGS, "--rb_mask", mask_file]
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    local = str(d / "local.npz")
    procs = [_producer([*prod, "--ray_address", addr, "--num_consumers", "2", "--queue_size", "6"]),
             _consumer(addr, 0, [*flags, "--batch", "5", "--out", two[0]]),
             _consumer(addr, 1, [*flags, "--batch", "6", "--out", two[1], "--part_frames", "3"]),
             _producer([*prod, "--local", "--consumer_task", "roibin", "--out_roibin", local, *flags])]
    outs = _finish(procs)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, outs=outs, mask=mask.reshape(-1), mask_file=mask_file)


def test_two_consumers_merge_to_the_golden_model_and_to_one_consumers_file(sessions):
    from psana_ray_amd import roibin

    s = sessions
    parts = sorted(glob.glob(str(s.dir / "c1.*.npz")))
    assert len(parts) >= 1 and not os.path.exists(s.two[1])                  # --part_frames writes parts only
    c0, c1 = roibin.RoibinFrames.load(s.two[0]), roibin.RoibinFrames.load(str(s.dir / "c1.*.npz"))
    assert len(c0) + len(c1) == N_EVENTS and all(len(roibin.RoibinFrames.load(p)) <= 3 for p in parts)
    m = roibin.merge([s.two[0], str(s.dir / "c1.*.npz")])
    g = _want(_golden_frames(N_EVENTS), s.mask)
    assert m.gevt.tolist() == list(range(N_EVENTS))
    for k in ("npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "codes"):
        assert np.array_equal(getattr(m, k), getattr(g, k).numpy()), k
    assert m.rec.tobytes() == g.rec.numpy().tobytes() and m.box.tobytes() == g.box.numpy().tobytes()
    skipped = int((m.flags & roibin.FLAG_SKIPPED != 0).sum())
    assert 0 < skipped < N_EVENTS and m.codes.shape == (N_EVENTS - skipped, 2, 16, 24) and int(m.koffs[-1]) == N_EVENTS - skipped
    assert (m.detector, m.layout, m.shape, m.bin, m.step, m.inv, m.vmin, m.vmax, m.radius, m.max_peaks, m.min_peaks,
            m.mask_sha256) == ("tiny_epix", "calib", SHAPE, 2, 0.5, 2.0, -64.0, 4096.0, 2, 2048, MIN_PEAKS,
                               roibin.mask_sha256(s.mask))
    assert m.peak_params == {"thr_peak": 20.0, "son_min": 5.0, "radius": 1.0}
    _same_files(roibin.merge([str(s.dir / "c1.*.npz"), s.two[0]]), m)
    one = roibin.RoibinFrames.load(s.local)
    assert one.gevt.tolist() == list(range(N_EVENTS))                        # one consumer: processing order
    _same_files(one, m)
    # a kept frame reconstructs: bit-exact in the boxes, to step / 2 of the block mean elsewhere
    x = _golden_frames(N_EVENTS).numpy()
    i = int(np.flatnonzero((m.flags & roibin.FLAG_SKIPPED) == 0)[0])
    dense = m.to_dense(i)
    ctr, _rec, box = m.boxes(i)
    p, y, xx = (int(v) for v in np.unravel_index(int(ctr[len(ctr) // 2]), SHAPE))
    assert dense[p, y, xx] == x[i, p, y, xx] and box.shape[1:] == (5, 5)
    with pytest.raises(ValueError, match="skipped"):
        m.to_dense(int(np.flatnonzero(m.flags & roibin.FLAG_SKIPPED)[0]))
    # the lines of the CLIs
    for _rc, out in s.outs[1:]:
        assert re.search(rf"Consumer \d roibin: bin=2 step=0.5 window=\[-64,4096\] box=5x5 max_peaks=2048 "
                         rf"min_peaks={MIN_PEAKS} codes=16x24 frame_bytes=1536 batch=\d+", out), out[-2000:]
    finals = [re.search(r"Consumer \d roibin: frames=(\d+) kept=(\d+) skipped=(\d+) boxes=(\d+) overflowed=0 saturated=0",
                        out) for _, out in s.outs[1:]]
    assert all(finals) and [int(f.group(1)) for f in finals] == [len(c0), len(c1), N_EVENTS]
    assert int(finals[2].group(3)) == skipped and int(finals[2].group(4)) == int(m.offs[-1])
    assert int(finals[0].group(4)) + int(finals[1].group(4)) == int(m.offs[-1])


def test_module_cli_merge_info_dense(sessions):
    from psana_ray_amd import roibin

    s = sessions
    out = str(s.dir / "merged.npz")
    c1 = str(s.dir / "c1.*.npz")
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.roibin", "merge", s.two[0], c1, "--out", out], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"frames={N_EVENTS} kept=" in r.stdout, r.stderr[-2000:]
    m = roibin.RoibinFrames.load(out)
    _same_files(m, roibin.merge([s.two[0], c1]))
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.roibin", "info", out, s.two[0]], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.splitlines()) == 2 and "bin=2 step=0.5 codes=16x24" in r.stdout
    kept = int(m.gevt[np.flatnonzero((m.flags & 2) == 0)[0]])
    skipped = int(m.gevt[np.flatnonzero(m.flags & 2)[0]])
    npy = str(s.dir / "f.npy")
    assert roibin.main(["dense", out, "--gevt", str(kept), "--out", npy]) == 0
    assert np.array_equal(np.load(npy), m.to_dense(int(np.flatnonzero(m.gevt == kept)[0])), equal_nan=True)
    # refusals: a skipped frame, an unknown gevt, both selectors, a gevt twice, other parameters, another mask, no file
    assert roibin.main(["dense", out, "--gevt", str(skipped), "--out", npy]) == 2
    assert roibin.main(["dense", out, "--gevt", "999", "--out", npy]) == 2
    assert roibin.main(["dense", out, "--gevt", "1", "--frame", "1", "--out", npy]) == 2
    assert roibin.main(["merge", out, out, "--out", str(s.dir / "no.npz")]) == 2
    assert roibin.main(["info", str(s.dir / "nothing*.npz")]) == 2
    import dataclasses

    for field, value, word in (("step", 0.25, "step"), ("mask_sha256", "", "mask_sha256"), ("detector", "other", "detector"),
                               ("radius", 2, None)):
        other = str(s.dir / f"other_{field}.npz")
        a = roibin.RoibinFrames.load(s.two[0])
        dataclasses.replace(a, **{field: value}).save(other)
        if word is None:
            roibin.merge([other, c1])            # the same value: merges
            continue
        with pytest.raises(ValueError, match=word):
            roibin.merge([other, c1])
    e = roibin.RoibinFrames.load(s.two[0]).select([])
    with pytest.raises(ValueError, match="shape"):
        roibin.concat([e, dataclasses.replace(e, shape=(2, 32, 50), codes=None)])
    np.savez(str(s.dir / "junk.npz"), a=np.zeros(3))
    assert roibin.main(["info", str(s.dir / "junk.npz")]) == 2


def test_refusals_exit_2(native, tmp_path, caplog):
    """A raw uint16 queue without a recipe, a panel-sharded session, an unnamed detector, a bad bound, a mask of
    another shape; the co-located form's refusals; --out_roibin without the task."""
    a_raw, a_shard = _addr(), _addr()
    prods = [_producer(["--mode", "raw", "--num_events", "4", "--ray_address", a_raw, "--num_consumers", "1",
                        "--queue_size", "4"]),
             *[_producer(["--calib", "--num_events", "4", "--panel_shards", "2", "--ray_address", a_shard,
                          "--num_consumers", "1", "--queue_size", "6"], rank=r, size=2) for r in range(2)]]
    cons = [_consumer(a_raw, 0, []), _consumer(a_shard, 0, [])]
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
        lines = [l for l in out.splitlines() if "--task roibin" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    np.save(tmp_path / "m.npy", np.ones((2, 32, 47), np.uint8))
    cases = [(["--rb_vmax", str(2.0 ** 25)], "2^25"), (["--rb_step", "0.001", "--rb_vmax", "65536"], "2^25"),
             (["--rb_step", "0"], "step"), (["--rb_vmin", "5", "--rb_vmax", "4"], "window"), (["--rb_box", "8"], "radius"),
             (["--min_peaks", "-1"], "min_peaks"), (["--rb_mask", str(tmp_path / "m.npy")], "--rb_mask"),
             (["--rb_mask", str(tmp_path / "none.npy")], "none.npy")]
    ep = QueueEndpoint(FrameRing(SHAPE, torch.float32, "cpu", 2, 2))
    try:
        for extra, word in cases:
            reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                           session_meta={"detector": {"name": "tiny_epix", "mode": "calib"}})
            args = consumer.build_parser().parse_args(["--task", "roibin", *extra])
            args.batch = 4
            caplog.clear()
            with caplog.at_level("ERROR"):
                assert consumer.run_roibin(args, reader, {"flag": False}, {"n": 0}) == 2, extra
            lines = [r.getMessage() for r in caplog.records if "--task roibin" in r.getMessage()]
            assert len(lines) == 1 and word in lines[0], (extra, lines)
        caplog.clear()
        reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                       session_meta={"detector": None})
        args = consumer.build_parser().parse_args(["--task", "roibin"])
        args.batch = 4
        with caplog.at_level("ERROR"):
            assert consumer.run_roibin(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_roibin(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--task", "roibin", "--rb_bin", "3"], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--rb_bin" in r.stderr
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "roibin", *extra], env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--consumer_task roibin needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    for extra, word in ((["--rb_vmax", "1e9"], "2^25"), (["--rb_mask", str(tmp_path / "m.npy")], "--rb_mask")):
        r = subprocess.run([*base, "--calib", "--consumer_task", "roibin", *extra], env=_env(), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task roibin" in r.stderr and word in r.stderr, (extra, r.stderr[-2000:])
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_roibin", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_roibin belongs to --consumer_task roibin" in r.stderr, r.stderr[-2000:]


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located roibin consumers write PATH as PATH.r<rank>.npz; the files merge."""
    from psana_ray_amd import roibin

    addr = _addr()
    out = str(tmp_path / "roibin.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "roibin", "--out_roibin",
                               out, "--rb_bin", "4"], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"roibin.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = roibin.merge(files)
    assert m.gevt.tolist() == list(range(N_EVENTS)) and m.codes.shape == (N_EVENTS, 2, 8, 12) and m.bin == 4
    assert set(m.rank.tolist()) == {0, 1} and int(m.offs[-1]) == int(m.nbox.sum()) > 0


def test_help_and_readme_command_lines():
    from psana_ray_amd import consumer, producer

    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--rb_bin" in r.stdout and "--rb_mask" in r.stdout, r.stderr[-2000:]
    a = consumer.build_parser().parse_args(["0", "--task", "roibin", "--min_peaks", "10", "--out", "r.npz"])
    assert (a.rb_bin, a.rb_step, a.rb_box, a.rb_vmin, a.rb_vmax, a.rb_mask) == (2, 1.0, 4, -2.0 ** 20, 2.0 ** 20, None)
    producer.build_parser().parse_args(["--exp", "e", "--run", "1", "--detector_name", "epix10k2M", "--local", "--calib",
                                        "--consumer_task", "roibin", "--rb_bin", "4", "--out_roibin", "r.npz"])
    text = open(os.path.join(ROOT, "README.md")).read()
    assert "--task roibin" in text and "--rb_bin" in text and "python -m psana_ray_amd.roibin merge" in text
    assert "no SZ" in text and "PCIe" in text
    assert "Roibin: the contract" in open(os.path.join(ROOT, "docs", "ARCHITECTURE.md")).read()
