"""An independent per-pixel oracle of the K-16 ROI contract: plain Python loops over pixels, numpy float32
SCALARS and Python integers, no array arithmetic.  Slow on purpose; only for small shapes."""
import numpy as np

F32 = np.float32
M64 = (1 << 64) - 1


def _rint_half_even(t):
    """Round a float (an exact float32 product) to the nearest integer, ties to even, in Python integers."""
    fl = int(np.floor(t))
    d = float(t) - fl
    if d > 0.5 or (d == 0.5 and fl % 2 != 0):
        return fl + 1
    return fl


def roi_oracle(frames, shape, rects, vmin, vmax, frac_bits, mask=None, proj="none"):
    """frames: float32 array [F, n].  Returns (rows [F][R][8] of Python ints -- the key as an unsigned 64-bit
    value --, proj_x [F][Lx], proj_y [F][Ly])."""
    P, H, W = shape
    n = P * H * W
    frames = np.asarray(frames, F32).reshape(-1, n)
    lo, hi, scale = F32(vmin), F32(vmax), F32(2 ** frac_bits)
    Lx = sum(x1 - x0 for (_p, _y0, _y1, x0, x1) in rects) if proj in ("x", "both") else 0
    Ly = sum(y1 - y0 for (_p, y0, y1, _x0, _x1) in rects) if proj in ("y", "both") else 0
    rows, pxs, pys = [], [], []
    with np.errstate(all="ignore"):
        for f in range(frames.shape[0]):
            frow, px, py = [], [0] * Lx, [0] * Ly
            ox = oy = 0
            for (p, y0, y1, x0, x1) in rects:
                npix = s = sy = sx = key = 0
                for y in range(y0, y1):
                    for x in range(x0, x1):
                        idx = (p * H + y) * W + x
                        v = frames[f, idx]
                        if mask is not None and mask[idx] == 0:
                            continue
                        if not (bool(lo <= v) and bool(v <= hi)):
                            continue
                        q = _rint_half_even(F32(v * scale))
                        npix += 1
                        s += q
                        sy += q * y
                        sx += q * x
                        key = max(key, (((q & 0xFFFFFFFF) ^ 0x80000000) << 32) | (0xFFFFFFFF - idx))
                        if Lx:
                            px[ox + x - x0] += q
                        if Ly:
                            py[oy + y - y0] += q
                ox += x1 - x0
                oy += y1 - y0
                frow.append([npix, s, sy, sx, key, 0, 0, 0])
            rows.append(frow)
            pxs.append(px)
            pys.append(py)
    return rows, pxs, pys


def rows_as_int64(rows):
    """The oracle's rows as the int64 [F, R, 8] array of the golden model (the key's bit pattern)."""
    a = np.array([[[w & M64 for w in r] for r in fr] for fr in rows], dtype=np.uint64)
    return a.view(np.int64)
