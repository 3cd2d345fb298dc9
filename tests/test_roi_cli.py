"""``psana-ray-consumer --task roi`` / ``psana-ray-producer --consumer_task roi`` as separate processes on CPU
sessions (tiny_epix; the CPU endpoints run the golden models), and ``python -m psana_ray_amd.roi``."""
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
SPECS = ["1,4:20,8:40", "0,0:32,0:48", "1,31:32,47:48", "0,10:11,3:30"]
RECTS = [(1, 4, 20, 8, 40), (0, 0, 32, 0, 48), (1, 31, 32, 47, 48), (0, 10, 11, 3, 30)]
ROI_FLAGS = [a for s in SPECS for a in ("--roi", s)]


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
                             "--device", "cpu", "--timeout", "60", "--task", "roi", "--metrics_interval", "0", *extra],
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


def _want(frames, shape, rects, vmin=-2.0 ** 20, vmax=2.0 ** 20, S=2, mask=None, proj="none"):
    """The golden model's RoiFrames arrays for frames in gevt order."""
    from psana_ray_amd.ops import reference

    n = frames.shape[0]
    rows, px, py = reference.roi_stats_reference(frames.reshape(n, -1), shape, rects, vmin, vmax, S, mask, proj)
    rows = rows.numpy()
    qmax, imax = reference.roi_key_decode(rows[:, :, 4])
    return {"npix": rows[:, :, 0].astype(np.int32), "sum": rows[:, :, 1], "sy": rows[:, :, 2], "sx": rows[:, :, 3],
            "qmax": qmax, "imax": imax, "proj_x": px.numpy(), "proj_y": py.numpy()}


def _same_arrays(st, want):
    for k, w in want.items():
        got = st._arr(k)
        assert got.dtype == w.dtype and got.shape == w.shape, (k, got.dtype, got.shape, w.dtype, w.shape)
        assert np.array_equal(got, w), k


def _same_files(a, b):
    from psana_ray_amd import roi

    assert a.key() == b.key()
    for k in roi.PER_FRAME:
        assert a._arr(k).dtype == b._arr(k).dtype and a._arr(k).tobytes() == b._arr(k).tobytes(), k


@pytest.fixture(scope="module")
def sessions(native, tmp_path_factory):
    """The same 20 events three times: two consumers (rectangles by --roi, both projections, a mask), the
    co-located consumer of a --local producer with the same flags, and a --local producer reading --roi_file."""
    d = tmp_path_factory.mktemp("roi_cli")
    mask = np.ones(SHAPE, np.uint8)
    mask[1, 5:9, 10:30:3] = 0
    mask_file, rect_file = str(d / "mask.npy"), str(d / "rects.npy")
    np.save(mask_file, mask)
    np.save(rect_file, np.array(RECTS, np.int64))
    prod = ["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS)]
    flags = [*ROI_FLAGS, "--roi_proj", "both", "--roi_mask", mask_file, "--roi_vmin", "-8", "--roi_vmax", "1024",
             "--roi_frac_bits", "4"]
    addr = _addr()
    two = [str(d / f"c{c}.npz") for c in range(2)]
    local, from_file = str(d / "local.npz"), str(d / "file.npz")
    procs = [_producer([*prod, "--ray_address", addr, "--num_consumers", "2", "--queue_size", "6"]),
             *[_consumer(addr, c, [*flags, "--batch", str(5 + c), "--out", two[c]]) for c in range(2)],
             _producer([*prod, "--local", "--consumer_task", "roi", "--out_roi", local, *flags]),
             _producer([*prod, "--local", "--consumer_task", "roi", "--out_roi", from_file, "--roi_file", rect_file])]
    outs = _finish(procs)
    for rc, out in outs:
        assert rc == 0, out[-3000:]
    return types.SimpleNamespace(dir=d, two=two, local=local, from_file=from_file, outs=outs, mask=mask.reshape(-1))


def test_two_consumers_merge_to_the_golden_model_and_to_one_consumers_file(sessions):
    from psana_ray_amd import roi

    s = sessions
    want = _want(_golden_frames(N_EVENTS), SHAPE, RECTS, -8.0, 1024.0, 4, s.mask, "both")
    each = [roi.RoiFrames.load(f) for f in s.two]
    assert sum(e.frames for e in each) == N_EVENTS
    m = roi.merge(s.two)
    _same_arrays(m, want)
    assert m.gevt.tolist() == list(range(N_EVENTS)) and np.array_equal(m.photon_energy, np.array(_energies(N_EVENTS)))
    rs = roi.RoiSet(RECTS, SHAPE)
    assert (m.detector, m.layout, m.shape, m.vmin, m.vmax, m.frac_bits, m.proj, m.rects_sha256, m.mask_sha256) == (
        "tiny_epix", "calib", SHAPE, -8.0, 1024.0, 4, "both", rs.sha256, roi.mask_sha256(SHAPE, s.mask))
    assert m.rects.tolist() == [list(r) for r in RECTS] and 0 < int(m.npix[:, 1].min()) < int(m.npix[:, 1].max()) <= 32 * 48   # the window cuts
    _same_files(roi.merge(s.two[::-1]), m)
    one = roi.RoiFrames.load(s.local)
    assert one.gevt.tolist() == list(range(N_EVENTS))                       # one consumer: processing order
    _same_files(one, m)
    # the lines of the CLIs
    rb = 4 * 64 + 8 * (32 + 48 + 1 + 27) + 8 * (16 + 32 + 1 + 1)
    for out in (s.outs[1][1], s.outs[2][1], s.outs[3][1]):
        assert re.search(rf"Consumer \d roi: rois=4 proj=both window=\[-8,1024\] frac_bits=4 batch=\d+ row_bytes={rb}\b", out), \
            out[-2000:]
    finals = [re.search(rf"Consumer \d roi: frames=(\d+) rois=4 row_bytes={rb} ", out) for _, out in s.outs[1:3]]
    assert all(finals) and sorted(int(f.group(1)) for f in finals) == sorted(e.frames for e in each)
    assert f"Consumer 0 roi: frames={N_EVENTS} rois=4 row_bytes={rb} detector=tiny_epix layout=calib" in s.outs[3][1]
    # the views against float64 statistics of the golden frames (quantisation: 2^-5 per sample)
    x = _golden_frames(N_EVENTS).numpy().astype(np.float64)[:, 1, 4:20, 8:40]
    keep = (s.mask.reshape(SHAPE)[1, 4:20, 8:40] != 0) & (x >= -8.0) & (x <= 1024.0)
    assert np.array_equal(m.npix[:, 0], keep.sum(axis=(1, 2)))
    assert np.all(np.abs(m.sum(0) - np.where(keep, x, 0).sum(axis=(1, 2))) <= 2.0 ** -5 * keep.sum(axis=(1, 2)))
    assert np.all(np.abs(m.max(0) - np.where(keep, x, -np.inf).max(axis=(1, 2))) <= 2.0 ** -5)
    assert np.array_equal(m.projection(0, "x").sum(axis=1), m.sum(0)) and m.projection(0, "y").shape == (N_EVENTS, 16)


def test_roi_file_default_window_no_projection(sessions):
    from psana_ray_amd import roi

    st = roi.RoiFrames.load(sessions.from_file)
    _same_arrays(st, _want(_golden_frames(N_EVENTS), SHAPE, RECTS))
    assert st.proj == "none" and st.proj_x.shape == (N_EVENTS, 0) and st.proj_y.shape == (N_EVENTS, 0)
    assert (st.vmin, st.vmax, st.frac_bits) == (-2.0 ** 20, 2.0 ** 20, 2) and st.mask_sha256 == roi.mask_sha256(SHAPE)
    assert "row_bytes=256" in sessions.outs[4][1]
    with pytest.raises(ValueError, match="differ in"):
        roi.merge([sessions.from_file, sessions.two[0]])


def test_module_cli_merge_info_export(sessions):
    from psana_ray_amd import roi

    s = sessions
    out = str(s.dir / "merged.npz")
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.roi", "merge", *s.two, "--out", out], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and f"frames={N_EVENTS} rois=4" in r.stdout, r.stderr[-2000:]
    m = roi.RoiFrames.load(out)
    _same_files(m, roi.merge(s.two))
    assert roi.main(["merge", s.two[0], s.from_file, "--out", str(s.dir / "no.npz")]) == 2
    assert roi.main(["merge", out, out, "--out", str(s.dir / "no.npz")]) == 2                 # a gevt twice
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.roi", "info", out], env=_env(), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0 and f'"frames": {N_EVENTS}' in r.stdout and '"proj": "both"' in r.stdout, r.stderr[-2000:]
    prefix = str(s.dir / "run")
    r = subprocess.run([sys.executable, "-m", "psana_ray_amd.roi", "export", out, "--out_prefix", prefix], env=_env(),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    total, com = np.load(prefix + "_sum.npy"), np.load(prefix + "_com.npy")
    assert total.shape == (N_EVENTS, 4) and com.shape == (N_EVENTS, 4, 2) and total.dtype == com.dtype == np.float64
    assert np.array_equal(total[:, 2], m.sum(2)) and np.array_equal(com[:, 0], m.com(0), equal_nan=True)
    for k, (_p, y0, y1, x0, x1) in enumerate(RECTS):
        assert np.array_equal(np.load(f"{prefix}_proj_x_r{k}.npy"), m.projection(k, "x"))
        assert np.load(f"{prefix}_proj_y_r{k}.npy").shape == (N_EVENTS, y1 - y0)


def test_calibrate_on_read_image_frames_take_2d_rectangles(native, tmp_path):
    """A --calibrate_on_read queue (RAW frames): the consumer calibrates (image mode, common mode), then takes the
    rectangles of the 2-D image."""
    from psana_ray_amd import roi
    from psana_ray_amd.models import get_detector, make_geometry

    n = 7
    H, W = make_geometry(get_detector("tiny_epix")).image_shape
    rects2 = [(3, H - 2, 1, W), (0, H, 0, W), (H - 1, H, W - 1, W)]
    specs = [a for (y0, y1, x0, x1) in rects2 for a in ("--roi", f"{y0}:{y1},{x0}:{x1}")]
    addr = _addr()
    out = str(tmp_path / "r.npz")
    outs = _finish([_producer(["--num_events", str(n), "--ray_address", addr, "--num_consumers", "1", "--queue_size", "4",
                               "--common_mode", "default", "--calibrate_on_read"]),
                    _consumer(addr, 0, ["--out", out, "--batch", "4", *specs, "--roi_proj", "x", "--roi_vmin", "-50",
                                        "--roi_vmax", "400"])])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    st = roi.RoiFrames.load(out)
    assert st.layout == "image" and st.shape == (H, W) and st.frames == n and st.gevt.tolist() == list(range(n))
    assert st.rects.tolist() == [[0, *r] for r in rects2]
    _same_arrays(st, _want(_golden_frames(n, "image", "default"), (H, W), [(0, *r) for r in rects2], -50.0, 400.0, 2, None, "x"))


def test_refusals_exit_2(native, tmp_path, caplog):
    """A raw uint16 queue without a recipe, a panel-sharded session, an unnamed detector; no rectangle at all, both
    sources, a malformed spec, a rectangle outside the frames, a 2-number spec on 3-D frames and the reverse, a
    bound violation; the co-located form's refusals; --out_roi without the task."""
    rect_file = str(tmp_path / "rects.npy")
    np.save(rect_file, np.array(RECTS, np.int64))
    src = ["--roi", SPECS[0]]
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
        lines = [l for l in out.splitlines() if "--task roi" in l]
        assert len(lines) == 1 and word in lines[0] and "Traceback" not in out, out[-3000:]
    # what needs no frame shape is checked before the queue is joined: no producer needed
    bad = ([], [*src, "--roi_file", rect_file], ["--roi", "1,4:20"], ["--roi", "1,4-20,8:40"], ["--roi", "x"],
           [*src, "--roi_vmax", "2147483648", "--roi_frac_bits", "0"], [*src, "--roi_frac_bits", "17"],
           [*src, "--roi_vmin", "5", "--roi_vmax", "4"])
    words = ("no rectangle", "not both", "malformed", "malformed", "malformed", "2^31", "frac_bits", "window")
    for extra, word in zip(bad, words):
        r = subprocess.run([sys.executable, "-m", "psana_ray_amd.consumer", "0", "--ray_address", _addr(), "--device", "cpu",
                            "--task", "roi", *extra], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--task roi" in r.stderr and word in r.stderr, (extra, r.stderr[-2000:])
        assert "Traceback" not in r.stderr
    # what needs the frames' shape, on a calib session (3-D frames) and an image session (2-D frames): rc 2 and one
    # line each, before anything is read
    from psana_ray_amd import consumer
    from psana_ray_amd.queue import FrameRing, QueueEndpoint

    np.save(tmp_path / "r17.npy", np.array([RECTS[0]] * 17, np.int64))
    np.save(tmp_path / "r4.npy", np.array(RECTS, np.int64)[:, 1:])
    cases = [("calib", ["--roi", "2,0:4,0:4"], "outside"), ("calib", ["--roi", "0,0:33,0:4"], "outside"),
             ("calib", ["--roi", "0,4:4,0:4"], "empty"), ("calib", ["--roi", "4:20,8:40"], "names no panel"),
             ("calib", ["--roi_file", str(tmp_path / "r17.npy")], "17 rectangles"),
             ("calib", ["--roi_file", str(tmp_path / "r4.npy")], "2-D frames"),
             ("calib", [*src, "--roi_mask", str(tmp_path / "r4.npy")], "--roi_mask"),
             ("image", ["--roi", "0,4:20,8:40"], "names a panel"), ("image", ["--roi", "4:33,8:40"], "outside")]
    eps = {"calib": QueueEndpoint(FrameRing(SHAPE, torch.float32, "cpu", 2, 2)),
           "image": QueueEndpoint(FrameRing((1, 32, 98), torch.float32, "cpu", 2, 2))}
    try:
        for mode, extra, word in cases:
            reader = types.SimpleNamespace(consumer_id=0, endpoint=eps[mode], panel_shards=1, calibrator=None,
                                           session_meta={"detector": {"name": "tiny_epix", "mode": mode}})
            args = consumer.build_parser().parse_args(["--task", "roi", *extra])
            args.batch = 4
            caplog.clear()
            with caplog.at_level("ERROR"):
                assert consumer.run_roi(args, reader, {"flag": False}, {"n": 0}) == 2, extra
            lines = [r.getMessage() for r in caplog.records if "--task roi" in r.getMessage()]
            assert len(lines) == 1 and word in lines[0], (extra, lines)
    finally:
        for e in eps.values():
            e.close()
    caplog.clear()
    # the moments' bound needs the rectangle: checked on a consumer built by hand (no frame is that large here)
    ep = QueueEndpoint(FrameRing(SHAPE, torch.float32, "cpu", 2, 2))
    try:
        args = consumer.build_parser().parse_args(["--task", "roi", "--roi", "0,0:32,0:48", "--roi_vmin", "0", "--roi_vmax",
                                                   "1073741824", "--roi_frac_bits", "0"])
        consumer.roi_consumer(args, ep, SHAPE, "tiny_epix", "calib", batch=4).synchronize()   # 2^30 * 1536 * 47 fits
        from psana_ray_amd.ops import reference

        with pytest.raises(ValueError, match=r"2\^63 - 1"):
            reference.validate_roi_params(0.0, 2.0 ** 30, 0, [(0, 0, 2 ** 11, 0, 2 ** 11 + 1)])
        # a session that does not name its detector (and no --detector_name): rc 2, one line
        reader = types.SimpleNamespace(consumer_id=0, endpoint=ep, panel_shards=1, calibrator=None,
                                       session_meta={"detector": None})
        args = consumer.build_parser().parse_args(["--task", "roi", *src])
        args.batch = 4
        with caplog.at_level("ERROR"):
            assert consumer.run_roi(args, reader, {"flag": False}, {"n": 0}) == 2
            assert sum("does not name its detector" in r.getMessage() for r in caplog.records) == 1
            reader.endpoint = None
            assert consumer.run_roi(args, reader, {"flag": False}, {"n": 0}) == 2
    finally:
        ep.close()
    # the co-located form refuses the same before it starts, and --out_roi without the task
    base = [sys.executable, "-m", "psana_ray_amd.producer", "--exp", "synthetic", "--run", str(RUN), "--detector_name",
            "tiny_epix", "--device", "cpu", "--num_events", "4", "--local"]
    for extra in (["--mode", "raw"], ["--calib", "--panel_shards", "2"]):
        r = subprocess.run([*base, "--consumer_task", "roi", *src, *extra], env=_env(), capture_output=True, text=True,
                           timeout=120)
        assert r.returncode == 2 and "--consumer_task roi needs whole calibrated frames" in r.stderr, r.stderr[-2000:]
    for extra, word in (([], "no rectangle"), ([*src, "--roi_file", rect_file], "not both"), (["--roi", "1;2"], "malformed"),
                        (["--roi", "2,0:4,0:4"], "outside"), (["--roi", "4:20,8:40"], "names no panel")):
        r = subprocess.run([*base, "--calib", "--consumer_task", "roi", *extra], env=_env(), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 2 and "--consumer_task roi" in r.stderr and word in r.stderr, (extra, r.stderr[-2000:])
    r = subprocess.run([*base, "--calib", "--consumer_task", "peakfind", "--out_roi", str(tmp_path / "p.npz")],
                       env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "--out_roi belongs to --consumer_task roi" in r.stderr, r.stderr[-2000:]


def test_several_ranks_write_one_file_each(native, tmp_path):
    """Two producer ranks with co-located ROI consumers write PATH as PATH.r<rank>.npz; the files merge to the
    golden model over all events."""
    from psana_ray_amd import roi
    from psana_ray_amd.ops import reference
    from psana_ray_amd.source import SyntheticRun

    addr = _addr()
    out = str(tmp_path / "roi.npz")
    outs = _finish([_producer(["--calib", "--common_mode", "off", "--num_events", str(N_EVENTS), "--ray_address", addr,
                               "--num_consumers", "0", "--queue_size", "8", "--consumer_task", "roi", "--out_roi", out,
                               *ROI_FLAGS, "--roi_proj", "y"], rank=r, size=2) for r in range(2)])
    for rc, o in outs:
        assert rc == 0, o[-3000:]
    files = [str(tmp_path / f"roi.r{r}.npz") for r in range(2)]
    assert all(os.path.exists(f) for f in files) and not os.path.exists(out)
    m = roi.merge(files)
    assert m.gevt.tolist() == list(range(N_EVENTS))
    # rank r of 2 produces its half of the events (gevt = r + 2 k) from a pool of its own
    frames = [None] * N_EVENTS
    for r in range(2):
        src = SyntheticRun("synthetic", RUN, "tiny_epix", rank=r, size=2, n_events=N_EVENTS)
        raw = np.stack([src.pool[k % src.pool_frames] for k in range(src.n_local_events())]).astype(np.int32)
        cal = reference.calibrate_reference(torch.from_numpy(raw), src.consts, None, None)
        for k in range(src.n_local_events()):
            frames[r + 2 * k] = cal[k]
    _same_arrays(m, _want(torch.stack(frames), SHAPE, RECTS, proj="y"))


def test_help_and_readme_command_lines():
    from psana_ray_amd import consumer, producer

    for mod in ("psana_ray_amd.producer", "psana_ray_amd.consumer"):
        r = subprocess.run([sys.executable, "-m", mod, "--help"], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "--roi_file" in r.stdout and "--roi_proj" in r.stdout, r.stderr[-2000:]
    a = consumer.build_parser().parse_args(["0", "--task", "roi", "--roi", "3,100:164,0:384", "--roi", "0,0:352,0:384",
                                            "--roi_proj", "x", "--out", "r.npz"])
    assert a.roi == ["3,100:164,0:384", "0,0:352,0:384"] and a.roi_vmin == -2.0 ** 20 and a.roi_vmax == 2.0 ** 20
    assert a.roi_frac_bits == 2 and a.roi_mask is None and a.roi_file is None
    producer.build_parser().parse_args(["--exp", "e", "--run", "1", "--detector_name", "epix10k2M", "--local", "--calib",
                                        "--consumer_task", "roi", "--roi", "3,100:164,0:384", "--out_roi", "r.npz"])
    text = open(os.path.join(ROOT, "README.md")).read()
    assert "--task roi" in text and "--roi_proj" in text and "python -m psana_ray_amd.roi merge" in text
    assert "ROI: the integer contract" in open(os.path.join(ROOT, "docs", "ARCHITECTURE.md")).read()
