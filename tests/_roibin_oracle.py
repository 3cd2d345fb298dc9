"""An independent model of the K-17 roibin contract for the tests: plain Python loops over blocks, pixels and
records, exact integers, numpy float32 for the one multiply.  It shares no code with ops.reference."""
import math

import numpy as np

f32 = np.float32
NAN_BITS = 0x7FC00000


def floor_div(a: int, b: int) -> int:
    """Floor division written out from C truncation, so that Python's // is not what is being tested."""
    q = abs(a) // abs(b)
    if (a < 0) != (b < 0):
        q = -q
        if q * b != a:
            q -= 1
    return q


def quantise(v, inv) -> int:
    """int(round half to even(float32(v) * float32(inv)))."""
    x = float(f32(v) * f32(inv))
    fl = math.floor(x)
    d = x - fl
    if d > 0.5 or (d == 0.5 and fl % 2 != 0):
        fl += 1
    return int(fl)


def record_ok(rec, shape):
    out = []
    for v, dim in zip(rec[:3], shape):
        v = float(v)
        if math.isnan(v) or math.isinf(v) or v != math.floor(v) or not 0 <= v < dim:
            return None
        out.append(int(v))
    return tuple(out)


def roibin_oracle(frames, shape, peaks, counts, B, step, vmin, vmax, R, min_peaks, mask=None):
    """frames float32 [F, P, H, W], peaks float32 [F, max_peaks, 8], counts int [F] -> a dict of numpy arrays named
    as the fields of RoibinBatch (box / rec as uint32 bit patterns)."""
    P, H, W = shape
    frames = np.asarray(frames, f32).reshape(-1, P, H, W)
    F, MP = frames.shape[0], peaks.shape[1]
    inv = f32(1.0 / np.float64(f32(step)))
    vmin, vmax = f32(vmin), f32(vmax)
    keep = np.ones((P, H, W), bool) if mask is None else (np.asarray(mask).reshape(P, H, W) != 0)
    Hb, Wb = -(-H // B), -(-W // B)
    Wn = 2 * R + 1
    bits = frames.view(np.uint32)
    o = {k: np.zeros(F, np.int32) for k in ("npk", "nbox", "nbad", "nsat")}
    o["flags"] = np.zeros(F, np.uint8)
    codes, ctrs, recs, boxes = [], [], [], []
    for f in range(F):
        cnt = int(counts[f])
        o["npk"][f] = max(cnt, 0)
        if cnt < min_peaks:
            o["flags"][f] = 2
            continue
        code = np.zeros((P, Hb, Wb), np.int16)
        for p in range(P):
            for yb in range(Hb):
                for xb in range(Wb):
                    S = c = 0
                    for y in range(yb * B, min(yb * B + B, H)):
                        for x in range(xb * B, min(xb * B + B, W)):
                            v = frames[f, p, y, x]
                            if keep[p, y, x] and vmin <= v and v <= vmax:   # NaN fails both
                                S += quantise(v, inv)
                                c += 1
                    if c == 0:
                        code[p, yb, xb] = -32768
                        continue
                    m = floor_div(2 * S + c, 2 * c)
                    if m > 32767 or m < -32767:
                        o["nsat"][f] += 1
                        m = max(-32767, min(32767, m))
                    code[p, yb, xb] = m
        codes.append(code)
        if o["npk"][f] > MP:
            o["flags"][f] |= 1
            continue
        found = []
        for s in range(o["npk"][f]):
            pyx = record_ok(peaks[f, s], shape)
            if pyx is None:
                o["nbad"][f] += 1
                o["flags"][f] |= 4
            else:
                found.append(((pyx[0] * H + pyx[1]) * W + pyx[2], s, pyx))
        found.sort(key=lambda t: (t[0], t[1]))
        o["nbox"][f] = len(found)
        for ctr, s, (p, y, x) in found:
            b = np.full((Wn, Wn), NAN_BITS, np.uint32)
            for dy in range(Wn):
                for dx in range(Wn):
                    yy, xx = y + dy - R, x + dx - R
                    if 0 <= yy < H and 0 <= xx < W:
                        b[dy, dx] = bits[f, p, yy, xx]
            ctrs.append(ctr)
            recs.append(np.asarray(peaks[f, s], f32).view(np.uint32).copy())
            boxes.append(b)
    o["offs"] = np.concatenate([[0], np.cumsum(o["nbox"])]).astype(np.int64)
    o["ctr"] = np.asarray(ctrs, np.int32)
    o["rec"] = np.stack(recs) if recs else np.zeros((0, 8), np.uint32)
    o["box"] = np.stack(boxes) if boxes else np.zeros((0, Wn, Wn), np.uint32)
    o["codes"] = np.stack(codes) if codes else np.zeros((0, P, Hb, Wb), np.int16)
    return o


def batch_arrays(b):
    """A RoibinBatch as the oracle's dict (numpy; rec / box as bit patterns)."""
    d = {k: getattr(b, k).numpy() for k in ("npk", "nbox", "nbad", "nsat", "flags", "offs", "ctr", "codes")}
    d["rec"] = b.rec.numpy().view(np.uint32)
    d["box"] = b.box.numpy().view(np.uint32)
    return d


def make_case(shape, F, seed, max_peaks=8, bad=True):
    """Frames of quarter-integer values with NaN / +-inf / window-edge pixels, a mask, and hand-made records:
    shuffled, with corner peaks, a tie on ctr, and (``bad``) records that are no pixel of the frame."""
    rng = np.random.default_rng(seed)
    P, H, W = shape
    x = (rng.integers(-400, 400, size=(F, P, H, W)) / 4.0).astype(f32)
    flat = x.reshape(F, -1)
    n = flat.shape[1]
    for f in range(F):
        pos = rng.permutation(n)[:6]
        flat[f, pos[0]] = np.nan
        flat[f, pos[1]] = np.inf
        flat[f, pos[2]] = -np.inf
        flat[f, pos[3]] = 100.0      # vmax of the tests' window: counts
        flat[f, pos[4]] = -100.0     # vmin: counts
        flat[f, pos[5]] = np.nextafter(f32(100.0), f32(np.inf))   # just outside
    mask = (rng.random(n) > 0.15).astype(np.uint8)
    peaks = rng.random((F, max_peaks, 8)).astype(f32)    # junk in the unused slots: fractional, so invalid
    counts = np.zeros(F, np.int32)
    for f in range(F):
        k = int(rng.integers(0, max_peaks + 1)) if f else max_peaks
        recs = []
        corners = [(0, 0, 0), (P - 1, H - 1, W - 1), (0, 0, W - 1), (P - 1, H - 1, 0)]
        for j in range(k):
            if j < 4:
                p, y, xx = corners[j]
            elif j == 4:
                p, y, xx = recs[0][:3]   # a tie on ctr: slot order decides
            else:
                p, y, xx = int(rng.integers(P)), int(rng.integers(H)), int(rng.integers(W))
            recs.append([p, y, xx, *rng.normal(size=5)])
        recs = np.asarray(recs, f32).reshape(k, 8)
        if bad and k >= 8:
            recs[5, 1] = np.nan
            recs[6, 2] = W            # one past the row
            recs[7, 0] = 0.5          # not integral
        if bad and k >= 6 and f % 2:
            recs[5, 1] = -1.0
        order = rng.permutation(k)
        peaks[f, :k] = recs[order]
        counts[f] = k
    return x, mask, peaks, counts
