"""The K-10 golden model (ops.reference.sparsify_reference) against an independent numpy oracle
(np.flatnonzero per frame), and the SparseFrames container built from it."""
import numpy as np
import pytest
import torch

from psana_ray_amd import sparse
from psana_ray_amd.ops import kernels, reference

C = kernels.SPARSE_CHUNK


def oracle(x, thr, vmax, cap, mask=None, keys=None, key_min=0):
    """Plain numpy, one frame at a time."""
    x = np.asarray(x, np.float32)
    F = x.shape[0]
    thr, vmax = np.float32(thr), np.float32(vmax)
    nnz, flags, offs, pix, val = np.zeros(F, np.int32), np.zeros(F, np.uint8), [0], [], []
    for f in range(F):
        stored = 0
        if keys is not None and keys[f] < key_min:
            flags[f] = 2
        else:
            with np.errstate(invalid="ignore"):
                k = (x[f] >= thr) & (x[f] <= vmax)
            if mask is not None:
                k &= np.asarray(mask).reshape(-1) != 0
            i = np.flatnonzero(k)
            nnz[f] = i.size
            if i.size > cap:
                flags[f] = 1
            else:
                stored = i.size
                pix.append(i.astype(np.int32))
                val.append(x[f][i])
        offs.append(offs[-1] + stored)
    return (nnz, flags, np.asarray(offs, np.int64), np.concatenate(pix) if pix else np.zeros(0, np.int32),
            np.concatenate(val) if val else np.zeros(0, np.float32))


def same(got, want):
    for g, w, name in zip(got[:4], want[:4], ("nnz", "flags", "offs", "pix")):
        g = g.numpy()
        assert g.dtype == w.dtype and np.array_equal(g, w), name
    assert got[4].dtype == torch.float32
    assert np.array_equal(got[4].numpy().view(np.int32), want[4].view(np.int32)), "val words"


def frames(F, n, seed, density):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-5.0, 5.0, size=(F, n)).astype(np.float32)
    hot = rng.random((F, n)) < density
    x[hot] = rng.uniform(10.0, 1000.0, size=int(hot.sum())).astype(np.float32)
    return x


@pytest.mark.parametrize("F", [1, 3, 64])
@pytest.mark.parametrize("n", [1, 3, 4, C - 1, C, C + 1, 3 * C + 5, 3072])
def test_shapes_and_densities(n, F):
    for k, density in enumerate((0.0, 1.0, 0.01, 0.3)):
        x = frames(F, n, 1000 * n + 10 * F + k, density)
        for cap in (n, max(1, n // 8)):
            same(reference.sparsify_reference(torch.from_numpy(x), 10.0, 1000.0, cap), oracle(x, 10.0, 1000.0, cap))


def test_special_values_and_window_edges():
    sp = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 50.0, np.nextafter(np.float32(50.0), np.float32(np.inf)),
                   np.nextafter(np.float32(0.0), np.float32(-np.inf)), 1.0e-45, 3.0e38, -3.0e38, 7.5], np.float32)
    x = np.tile(sp, (2, 3))
    got = reference.sparsify_reference(torch.from_numpy(x), 0.0, 50.0, x.shape[1])
    same(got, oracle(x, 0.0, 50.0, x.shape[1]))
    kept = set(got[4].numpy().view(np.int32).tolist())
    assert kept == {int(np.float32(v).view(np.int32)) for v in (-0.0, 0.0, 50.0, 1.0e-45, 7.5)}   # -0.0 with its sign
    got = reference.sparsify_reference(torch.from_numpy(x), 1.0e-45, 50.0, x.shape[1])
    assert set(got[4].tolist()) == {float(np.float32(1.0e-45)), 50.0, 7.5}
    # the window is compared as float32: 0.1 (double) rounds up to float32(0.1), which is then kept
    y = np.array([[np.float32(0.1), np.nextafter(np.float32(0.1), np.float32(0))]], np.float32)
    assert reference.sparsify_reference(torch.from_numpy(y), 0.1, 1.0, 2)[3].tolist() == [0]


def test_capacity_mask_and_keys():
    F, n, cap = 6, 3 * C + 5, 300
    rng = np.random.default_rng(17)
    x = rng.uniform(-5.0, 5.0, size=(F, n)).astype(np.float32)
    for f, k in enumerate([120, cap, cap + 1, 37, 5 * cap, 0]):
        x[f, rng.choice(n, size=k, replace=False)] = 100.0 + f
    xt = torch.from_numpy(x)
    got = reference.sparsify_reference(xt, 10.0, 1000.0, cap)
    same(got, oracle(x, 10.0, 1000.0, cap))
    assert got[0].tolist() == [120, cap, cap + 1, 37, 5 * cap, 0] and got[1].tolist() == [0, 0, 1, 0, 1, 0]
    assert got[2].tolist() == [0, 120, 120 + cap, 120 + cap, 157 + cap, 157 + cap, 157 + cap]
    mask = (rng.random(n) < 0.5).astype(np.uint8) * rng.integers(1, 256, size=n).astype(np.uint8)
    keys = np.array([3, 2, 3, 2, 3, -1], np.int32)
    for m in (None, mask, torch.from_numpy(mask)):
        for kk in (None, keys, torch.from_numpy(keys)):
            want = oracle(x, 10.0, 1000.0, cap, mask=None if m is None else np.asarray(m),
                          keys=None if kk is None else np.asarray(kk), key_min=3)
            same(reference.sparsify_reference(xt, 10.0, 1000.0, cap, mask=m, keys=kk, key_min=3), want)
            if kk is not None:
                assert want[1].tolist()[1::2] == [2, 2, 2] and want[0].tolist()[1::2] == [0, 0, 0]


def test_any_frame_layout_is_flattened():
    x = frames(3, 2 * 4 * 6, 5, 0.2)
    a = reference.sparsify_reference(torch.from_numpy(x), 10.0, 1000.0, 48)
    b = reference.sparsify_reference(torch.from_numpy(x).reshape(3, 2, 4, 6), 10.0, 1000.0, 48)
    same(b, tuple(t.numpy() for t in a))


@pytest.mark.parametrize("kw", [dict(thr=float("nan")), dict(vmax=float("inf")), dict(thr=2.0, vmax=1.0), dict(cap=0),
                                dict(cap=2 ** 31), dict(cap=1.5), dict(thr=1e39),
                                dict(mask=np.ones(7, np.uint8)), dict(mask=np.ones(8, np.int32)),
                                dict(keys=np.zeros(3, np.int32)), dict(keys=np.zeros(2, np.int64))])
def test_validation(kw):
    args = dict(thr=0.0, vmax=1.0, cap=4)
    args.update(kw)
    with pytest.raises(ValueError):
        reference.sparsify_reference(torch.zeros(2, 8), **args)


def test_validation_of_the_batch():
    with pytest.raises(ValueError):
        reference.sparsify_reference(torch.zeros(65, 4), 0.0, 1.0, 4)
    with pytest.raises(ValueError):
        reference.sparsify_reference(torch.zeros(2, 4, dtype=torch.float64), 0.0, 1.0, 4)
    with pytest.raises(ValueError):
        reference.sparsify_reference(torch.zeros(0, 4), 0.0, 1.0, 4)


def test_scratch_size_arithmetic():
    """Header 256 B, one 8-B directory entry per chunk and frame (rounded to 16 B), 8 B per staged pixel."""
    assert kernels.sparsify_scratch_bytes(1, 1, 1) == 256 + 16 + 8
    assert kernels.sparsify_scratch_bytes(C, 10, 3) == 256 + 32 + 240
    assert kernels.sparsify_scratch_bytes(C + 4, 10, 3) == 256 + 48 + 240
    assert kernels.sparsify_scratch_bytes(C + 3, 10, 3) == 256 + 32 + 240     # the tail belongs to the last chunk
    assert kernels.sparsify_scratch_bytes(2162688, 135168, 64) == 256 + 528 * 64 * 8 + 64 * 135168 * 8
    for bad in ((0, 1, 1), (8, 0, 1), (8, 1, 0), (8, 1, 65), (8, 2 ** 30, 2)):
        with pytest.raises(ValueError):
            kernels.sparsify_scratch_bytes(*bad)


def test_to_dense_of_the_golden_model():
    x = frames(4, 96, 9, 0.1)
    x[2, :40] = 500.0                                    # overflows cap 20
    nnz, flags, offs, pix, val = (t.numpy() for t in reference.sparsify_reference(torch.from_numpy(x), 10.0, 1000.0, 20))
    z = np.zeros(4)
    sf = sparse.SparseFrames("tiny", "calib", (2, 6, 8), 10.0, 1000.0, 20, rank=z, idx=np.arange(4), gevt=np.arange(4),
                             photon_energy=z, nnz=nnz, flags=flags, offs=offs, pix=pix, val=val)
    for i in (0, 1, 3):
        want = np.where((x[i] >= 10.0) & (x[i] <= 1000.0), x[i], np.float32(0)).reshape(2, 6, 8)
        assert np.array_equal(sf.to_dense(i).view(np.int32), want.view(np.int32))
        p, v = sf.frame(i)
        assert np.array_equal(p, np.flatnonzero(want.reshape(-1) != 0)) and np.all(np.diff(p) > 0)
    assert sf.flags[2] == sparse.FLAG_OVERFLOW and sf.nnz[2] >= 40 and sf.frame(2)[0].size == 0
    with pytest.raises(ValueError, match="overflowed"):
        sf.to_dense(2)
