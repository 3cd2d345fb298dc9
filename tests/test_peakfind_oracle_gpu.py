"""The K-07 HIP peak finder (csrc/peakfind.hip) directly against the independent float64
per-candidate model of tests/_peakfind_oracle.py, on the fixtures of that module: ties, panel seams
and load alignments, an empty ring, equality at both thresholds, non-finite pixels, offset
backgrounds, the parked / spill / in-stream candidate paths at their smallest shape, a partial last
chunk, and more than 64 frames per call.  Every frame is its own allocation."""
import numpy as np
import pytest
import torch

from psana_ray_amd.config import PeakFinderParams
from psana_ray_amd.ops import kernels
from tests import _peakfind_oracle as orc

pytestmark = pytest.mark.gpu

RADII = (1, 2)


@pytest.fixture(scope="module")
def scratch_block(cuda_device, native):
    """One self-resetting scratch block for the module: every launch must leave its counters zero."""
    return torch.zeros(kernels.PF_SCRATCH_WORDS, dtype=torch.int32, device=cuda_device)


def run_kernel(fx, R, dev, scr, launches=1):
    """-> (records [F, max_peaks, 8], counts [F], summary [F, 2], total) as numpy / int, after
    `launches` identical calls with garbage in counts / summary before each."""
    params = PeakFinderParams(thr_peak=fx.thr_peak, son_min=fx.son_min(R), radius=R, max_peaks=fx.max_peaks)
    frames = [torch.from_numpy(fr.copy()).to(dev) for fr in fx.frames]   # separate allocations
    assert all(t.data_ptr() % 16 == 0 for t in frames)
    F = len(frames)
    peaks = torch.zeros((F, fx.max_peaks, 8), dtype=torch.float32, device=dev)
    counts = torch.zeros(F, dtype=torch.int32, device=dev)
    summary = torch.zeros((F, 2), dtype=torch.float32, device=dev)
    total = torch.zeros((), dtype=torch.int64, device=dev)
    for _ in range(launches):
        counts.fill_(12345)
        summary.fill_(-7.0)
        kernels.peakfind(frames, fx.shape, params, peaks, counts, summary, total=total, scratch=scr)
    torch.cuda.synchronize()
    return peaks.cpu().numpy(), counts.cpu().numpy(), summary.cpu().numpy(), int(total)


def check(fx, R, peaks, counts, summary):
    o = fx.oracle(R)
    worst = dict(bkg=0.0, noise=0.0, intensity=0.0)
    for f in range(len(o)):
        n = int(counts[f])
        assert 0 <= n <= fx.max_peaks, f"{fx.name} R={R} frame {f}: count {n} (fixture sized for <= {fx.max_peaks})"
        w = orc.check_frame(peaks[f, :n], n, summary[f], o[f], fx.son_min(R), R, f"{fx.name} R={R} frame {f}")
        worst = {k: max(worst[k], w[k]) for k in worst}
    print(f"{fx.name} R={R}: worst error / bound {worst}")
    orc.assert_coordinates(fx, R, lambda f: {tuple(int(v) for v in r[:3]) for r in peaks[f, :int(counts[f])]})


@pytest.mark.parametrize("scratch", [False, True])
@pytest.mark.parametrize("R", RADII)
@pytest.mark.parametrize("name", [n for n in orc.FIXTURES if n != "many_frames"])
def test_kernel_vs_float64(cuda_device, native, scratch_block, name, R, scratch):
    """With a scratch block: two launches on the same block, garbage in counts / summary before each,
    so the last workgroup must write them whole and re-zero the block.  The paths_* fixtures run
    parked + in-stream without the block and parked + spill with it."""
    fx = orc.fixture(name)
    fx.assert_precondition(R)
    if name.startswith("paths_"):
        assert all(o["count"] > 512 for o in fx.oracle(R)), "every frame must overflow the parked candidates"
    launches = 2 if scratch else 1
    peaks, counts, summary, total = run_kernel(fx, R, cuda_device, scratch_block if scratch else None, launches)
    check(fx, R, peaks, counts, summary)
    assert total == launches * sum(min(int(c), fx.max_peaks) for c in counts)
    if scratch:
        assert int(scratch_block[:256].abs().sum()) == 0, "scratch counters not re-zeroed by the last workgroup"


@pytest.mark.parametrize("R", RADII)
def test_kernel_threshold_equality(cuda_device, native, R):
    """snr == son_min exactly is kept and one ulp below is dropped (bkg = 0 and noise = 1 are exact
    in any precision on the +-1 checkerboard); the pixel AT thr_peak is not in the summary."""
    fx = orc.fixture("threshold")
    peaks, counts, summary, _ = run_kernel(fx, R, cuda_device, None)
    rec = {tuple(int(v) for v in r[:3]): r for r in peaks[0, :int(counts[0])]}
    r = rec[(0, 5, 6)]
    assert r[7] == np.float32(orc.THR_EQ_SON) and r[5] == 0 and r[6] == 1
    assert (0, 5, 18) not in rec and (0, 15, 10) not in rec and (0, 15, 25) in rec
    assert summary[0, 0] == 4


@pytest.mark.parametrize("R", RADII)
def test_kernel_more_than_64_frames(cuda_device, native, scratch_block, R):
    """67 different frames in one call: the wrapper's two launches (64 + 3) share the scratch block
    and the running total."""
    fx = orc.fixture("many_frames")
    assert len(fx.frames) > kernels.MAX_FRAMES
    fx.assert_precondition(R)
    peaks, counts, summary, total = run_kernel(fx, R, cuda_device, scratch_block)
    check(fx, R, peaks, counts, summary)
    assert total == sum(min(int(c), fx.max_peaks) for c in counts)
    assert all(int(c) > 0 for c in counts)
    assert int(scratch_block[:256].abs().sum()) == 0, "scratch counters not re-zeroed by the last workgroup"
