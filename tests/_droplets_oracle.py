"""An independent oracle of the K-14 droplet contract: a pure-Python flood fill (one BFS per unvisited active
pixel) with numpy float32 SCALARS for the compares and Python integers for the sums.  It shares no labelling
code with the golden model.  Slow on purpose; only for small shapes.

Also the pattern set that the reference and the GPU tests share."""
from collections import deque

import numpy as np

F32 = np.float32


def droplets_oracle(frames, shape, thr_low, thr_seed=None, vmax=2.0 ** 20, frac_bits=2, mask=None, cap_pix=None,
                    cap=None):
    """frames: float32 array [F, n].  Returns dict(nact, ndrop, flags, offs, label, npix, adu, sy, sx, qmax) of
    Python-int lists."""
    P, H, W = shape
    n = P * H * W
    frames = np.asarray(frames, F32).reshape(-1, n)
    lo = F32(thr_low)
    seed_thr = lo if thr_seed is None else F32(thr_seed)
    hi = F32(vmax)
    scale = F32(2 ** frac_bits)
    cap_pix = max(1, n // 16) if cap_pix is None else cap_pix
    cap = max(1, n // 64) if cap is None else cap
    out = dict(nact=[], ndrop=[], flags=[], offs=[0], label=[], npix=[], adu=[], sy=[], sx=[], qmax=[])
    with np.errstate(all="ignore"):
        for x in frames:
            act = [(mask is None or mask[p] != 0) and bool(x[p] >= lo) and bool(x[p] <= hi) for p in range(n)]
            nact = sum(act)
            rows = []
            if nact <= cap_pix:
                seen = [False] * n
                for p0 in range(n):
                    if not act[p0] or seen[p0]:
                        continue
                    seen[p0] = True
                    todo = deque([p0])
                    npix = adu = sy = sx = qmax = 0
                    seeded = False
                    while todo:
                        p = todo.popleft()
                        panel, rest = divmod(p, H * W)
                        y, xx = divmod(rest, W)
                        q = int(np.rint(F32(x[p] * scale)))
                        npix += 1
                        adu += q
                        sy += q * y
                        sx += q * xx
                        qmax = max(qmax, q)
                        seeded = seeded or bool(x[p] >= seed_thr)
                        nb = []
                        if y > 0:
                            nb.append(p - W)
                        if y < H - 1:
                            nb.append(p + W)
                        if xx > 0:
                            nb.append(p - 1)
                        if xx < W - 1:
                            nb.append(p + 1)
                        for t in nb:
                            assert t // (H * W) == panel
                            if act[t] and not seen[t]:
                                seen[t] = True
                                todo.append(t)
                    if seeded:
                        rows.append((p0, npix, adu, sy, sx, qmax))   # p0 is the lowest index: the scan ascends
            ndrop = len(rows)
            flags = (1 if ndrop > cap else 0) | (4 if nact > cap_pix else 0)
            if flags:
                rows = []
            out["nact"].append(nact)
            out["ndrop"].append(ndrop)
            out["flags"].append(flags)
            out["offs"].append(out["offs"][-1] + len(rows))
            for r in rows:
                for k, v in zip(("label", "npix", "adu", "sy", "sx", "qmax"), r):
                    out[k].append(v)
    return out


def same_as_oracle(got, want):
    """got: a DropletList (tensors); want: the oracle's dict of lists."""
    for k, w in want.items():
        g = getattr(got, k).tolist()
        assert g == w, f"{k}: {g[:8]} != {w[:8]}"


# ---- the pattern set ---------------------------------------------------------------------------------------

def _frame(shape):
    return np.zeros(shape, F32)


def patterns(shape, v=10.0):
    """Named frames [P, H, W] (float32) of the shapes the contract speaks about, as far as they fit ``shape``."""
    P, H, W = shape
    out = {}
    a = _frame(shape)
    a[0, 0, 0] = v
    a[-1, -1, -1] = v
    a[0, H // 2, W // 2] = v
    out["lone"] = a
    if W >= 2:
        a = _frame(shape)
        a[0, 0, 0:2] = v
        a[-1, -1, W - 2:W] = v
        out["hpair"] = a
    if H >= 2:
        a = _frame(shape)
        a[0, 0:2, 0] = v
        a[-1, H - 2:H, -1] = v
        out["vpair"] = a
    if H >= 2 and W >= 2:
        a = _frame(shape)
        a[0, 0, 0] = v
        a[0, 1, 1] = v
        out["diagonal"] = a               # two droplets
        a = _frame(shape)
        a[0, 0, W - 1] = v
        a[0, 1, 0] = v
        out["row_end"] = a                # consecutive linear indices, not neighbours
    if P >= 2:
        a = _frame(shape)
        a[0, H - 1, :] = v
        a[1, 0, :] = v
        out["panel_edge"] = a             # last row of panel 0, first row of panel 1
    if H >= 3 and W >= 3:
        a = _frame(shape)
        a[0, 0:3, 0] = v
        a[0, 2, 0:3] = v
        out["L"] = a
        a = _frame(shape)
        a[0, 0:H, 0] = v
        a[0, 0:H, 2] = v + 1
        a[0, H - 1, 1] = v + 2
        out["U"] = a                      # the arms meet only at the bottom
    if H >= 3 and W >= 5:
        a = _frame(shape)
        a[-1, H - 1, :] = v
        a[-1, 0:H, 0::2] = v + 3
        out["comb"] = a                   # teeth that meet only in the last row
    if H >= 5 and W >= 5:
        a = _frame(shape)
        y0, y1, x0, x1 = 0, H - 1, 0, W - 1
        a[0, y0, x0:x1 + 1] = v
        while True:                       # a spiral arm two pixels apart
            a[0, y0:y1 + 1, x1] = v
            a[0, y1, x0:x1 + 1] = v
            if y1 - y0 < 4 or x1 - x0 < 4:
                break
            a[0, y0 + 2:y1 + 1, x0] = v
            a[0, y0 + 2, x0:x1 - 1] = v
            y0, x0, y1, x1 = y0 + 2, x0, y1 - 2, x1 - 2
            if y1 - y0 < 2 or x1 - x0 < 2:
                break
        out["spiral"] = a
    if H >= 3 and W >= 2:
        a = _frame(shape)
        a[-1, 0::2, :] = v                # full even rows ...
        for y in range(1, H, 2):          # ... joined at alternating ends: one long chain
            a[-1, y, W - 1 if (y // 2) % 2 == 0 else 0] = v + 1
        out["serpentine"] = a
    a = _frame(shape)
    yy, xx = np.indices((H, W))
    a[:, (yy + xx) % 2 == 0] = v
    out["checkerboard"] = a
    return out


def random_frames(shape, F, frac, seed, lo=2.0, hi=60.0):
    """F frames with about ``frac`` of the pixels in [lo, hi) (quarter-ADU steps: rounding ties of q at 2 bits
    never; at 0 and 1 bits often), the rest noise below lo, a few specials."""
    rng = np.random.default_rng(seed)
    n = int(np.prod(shape))
    x = (rng.integers(-8, 8, size=(F, n)).astype(F32) * F32(0.125))
    on = rng.random((F, n)) < frac
    x[on] = (rng.integers(int(lo * 8), int(hi * 8), size=int(on.sum())).astype(F32) * F32(0.125))
    s = rng.random((F, n))
    x[s < 0.004] = np.nan
    x[(s >= 0.004) & (s < 0.008)] = np.inf
    x[(s >= 0.008) & (s < 0.012)] = -np.inf
    x[(s >= 0.012) & (s < 0.016)] = -0.0
    x[(s >= 0.016) & (s < 0.02)] = -50.0
    return x
