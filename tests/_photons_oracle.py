"""An independent per-pixel oracle of the K-13 photon-counting contract: plain Python loops over pixels and
numpy float32 SCALARS, no shifted arrays.  Slow on purpose; only for small shapes."""
import numpy as np

F32 = np.float32


def photons_oracle(frames, shape, adu_per_photon, vmax=None, thr_seed=0.5, thr_total=0.9, mask=None, roi=None,
                   n_roi=1):
    """frames: float32 array [F, n].  Returns dict(kmap uint8 [F, n], cnt int32 [n], psum int64 [n], occ int32
    [n], pk int32 [F, R, 8], tot int64 [F, R])."""
    P, H, W = shape
    n = P * H * W
    frames = np.asarray(frames, F32).reshape(-1, n)
    nf = frames.shape[0]
    adu = F32(adu_per_photon)
    inv = F32(1.0 / np.float64(adu))
    vmax = F32(F32(250.0) * adu if vmax is None else vmax)
    ts, tt = F32(thr_seed), F32(thr_total)
    kmap = np.zeros((nf, n), np.uint8)
    cnt, psum, occ = np.zeros(n, np.int32), np.zeros(n, np.int64), np.zeros(n, np.int32)
    pk, tot = np.zeros((nf, n_roi, 8), np.int32), np.zeros((nf, n_roi), np.int64)
    with np.errstate(all="ignore"):
        for f in range(nf):
            w = [0] * n
            r = [F32(0.0)] * n
            for p in range(n):
                v = frames[f, p]
                ok = (mask is None or mask[p] != 0) and bool(v > F32(0.0)) and bool(v <= vmax)
                if ok:
                    x = F32(v * inv)
                    w[p] = int(np.floor(x))
                    r[p] = F32(x - F32(w[p]))
                    cnt[p] += 1
            for p in range(n):
                panel, rest = divmod(p, H * W)
                y, x = divmod(rest, W)
                nb = []
                if y > 0:
                    nb.append(p - W)
                if y < H - 1:
                    nb.append(p + W)
                if x > 0:
                    nb.append(p - 1)
                if x < W - 1:
                    nb.append(p + 1)
                seed = bool(r[p] >= ts)
                rmax = F32(0.0)
                for q in nb:
                    assert q // (H * W) == panel
                    if not (r[p] > r[q] or (r[p] == r[q] and p < q)):
                        seed = False
                    if r[q] > rmax:
                        rmax = r[q]
                k = w[p] + (1 if seed and bool(F32(r[p] + rmax) >= tt) else 0)
                kmap[f, p] = k
                psum[p] += k
                occ[p] += k >= 1
                lab = 0 if roi is None else int(roi[p])
                if k >= 1 and lab < n_roi:
                    pk[f, lab, min(k, 8) - 1] += 1
                    tot[f, lab] += k
    return dict(kmap=kmap, cnt=cnt, psum=psum, occ=occ, pk=pk, tot=tot)
