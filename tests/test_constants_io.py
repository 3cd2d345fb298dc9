"""CalibConstants.save / load: a bitwise round trip, and refusal of files that do not fit the detector."""
import numpy as np
import pytest

from psana_ray_amd.models import CalibConstants, get_detector
from psana_ray_amd.models.constants import file_sha256


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.mark.parametrize("name", ["tiny_epix", "tiny_jungfrau", "tiny_plain"])
def test_round_trip_is_bitwise(tmp_path, name):
    spec = get_detector(name)
    c = CalibConstants.random(spec, seed=11, gain_config="mixed" if spec.kind == "epix10ka" else "AHL")
    c.pedestals.reshape(-1)[:4] = np.array([np.nan, -0.0, np.inf, 1e-42], np.float32)   # words a value compare would miss
    c.status.reshape(-1)[3] = 200
    path = c.save(tmp_path / "consts.npz")
    assert path.endswith("consts.npz")
    for back in (CalibConstants.load(path), CalibConstants.load(path, spec)):
        assert back.spec == spec
        for k in ("pedestals", "gains", "status"):
            a, b = getattr(c, k), getattr(back, k)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), k
        if spec.kind == "epix10ka":
            assert back.gain_config.dtype == np.uint8 and np.array_equal(back.gain_config, c.gain_config)
        else:
            assert back.gain_config is None
        assert tuple(back.cm_gains) == tuple(c.cm_gains)
        # the kernel tables the loaded constants pack are the same words
        for a, b in zip(c.device_tables(), back.device_tables()):
            assert np.array_equal(_bits(a), _bits(b))
    with np.load(path, allow_pickle=False) as z:          # plain arrays, no pickle
        assert str(z["detector"]) == spec.name
    assert len(file_sha256(path)) == 64 and file_sha256(path) == file_sha256(path)


def test_file_of_another_detector_is_refused(tmp_path):
    epix = CalibConstants.random(get_detector("tiny_epix"), seed=1)
    path = epix.save(tmp_path / "epix.npz")
    with pytest.raises(ValueError, match="tiny_epix"):
        CalibConstants.load(path, get_detector("tiny_jungfrau"))       # another kind
    with pytest.raises(ValueError, match="tiny_epix"):
        CalibConstants.load(path, get_detector("epix10ka"))            # the same kind, other shapes
    # shapes that disagree with the detector the file names
    bad = CalibConstants(epix.spec, epix.pedestals[:, :1], epix.gains, epix.status, epix.gain_config, epix.cm_gains)
    with pytest.raises(ValueError, match="pedestals"):
        CalibConstants.load(bad.save(tmp_path / "bad.npz"))
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(ValueError, match="not a constants file"):
        CalibConstants.load(tmp_path / "other.npz")
    (tmp_path / "junk.npz").write_bytes(b"not a zip file at all")
    with pytest.raises(ValueError):
        CalibConstants.load(tmp_path / "junk.npz")
    with pytest.raises(OSError):
        CalibConstants.load(tmp_path / "missing.npz")
