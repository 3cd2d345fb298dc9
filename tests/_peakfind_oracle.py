"""An independent float64 model of the K-07 peak finder, the per-peak error bounds a correct fp32
evaluation stays inside, and the deterministic fixtures the CPU and GPU oracle tests share.

The model is written from the contract at the top of csrc/peakfind.hip, one candidate at a time with
plain loops over the window offsets; it shares no code with ops/reference.py (the kernel's
vectorised fp32 twin), so a mistake made by both the kernel and its twin shows up here.

Contract
  candidate    v > thr_peak, compared in fp32 (thr_peak reaches the kernel as a float); NaN never is
  local max    for every present, non-NaN neighbour n of the (2R+1)^2 window: v > n when n has the
               lower linear index (dy < 0, or dy == 0 and dx < 0), v >= n otherwise.  Pixels outside
               the panel are absent: the next row and the next panel in memory are outside.
  ring         present, non-NaN pixels at Chebyshev distance R+1 .. R+2: bkg = mean,
               noise = sqrt(mean((n - bkg)^2)) (two-pass); both 0 when the ring is empty
  snr          (v - bkg) / max(noise, 1e-6); a peak iff local max and snr >= son_min (NaN: no peak)
  intensity    sum of n - bkg over the present, non-NaN window pixels, centre included
  +-Inf        ordinary IEEE values: an Inf in the ring makes noise and snr NaN (rejected), a +Inf
               pixel is itself a candidate and makes the summary's sum Inf

Bounds (u = 2^-24; nr, M = max |window value| over the (2R+5)^2 window, noise64 from this model)
  E_b = nr * u * M                     fp32 sequential / FMA mean of nr terms
  E_n = E_b + 64 * u * noise64         an RMS about a centre that is off by E_b moves by at most E_b
  |bkg - bkg64| <= E_b, |noise - noise64| <= E_n,
  |intensity - intensity64| <= W * (E_b + W * u * M), W = (2R+1)^2
  snr inside [(v - bkg64 -+ (E_b + u*M)) / max(noise64 +- E_n, 1e-6)] widened by 4u relative; a
  lower denominator bound <= 1e-6 opens the end the numerator points to (+inf for a positive one)
  summary: count exact, |sum - sum64| <= count * u * sum|v|
These are worst-case summation bounds, fitted to no implementation.  Measured on the CPU with the
numpy float32 two-pass evaluation below (f32_two_pass, sequential row-major sums) over every fixture
and both radii, the worst ratio error / bound was 0.15 (bkg), 0.024 (noise), 0.11 (intensity), and
every fp32 snr lay inside its interval, so the constants stand as stated (nothing widened).
test_peakfind_oracle.py::test_f32_two_pass_within_bounds re-measures and prints these ratios.
"""
from __future__ import annotations

import functools
import math
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

U = 2.0 ** -24
NOISE_FLOOR = 1e-6


def _ring_offsets(R: int) -> List[Tuple[int, int]]:
    h = R + 2
    return [(dy, dx) for dy in range(-h, h + 1) for dx in range(-h, h + 1) if max(abs(dy), abs(dx)) > R]


def _window_offsets(R: int) -> List[Tuple[int, int]]:
    return [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]


def oracle_frame(frame: np.ndarray, thr_peak: float, R: int) -> dict:
    """frame: float32 [P, H, W].  Returns {"cands": [...], "count": int, "sum": float, "sum_abs": float};
    cands holds every LOCAL-MAXIMUM candidate as a dict (panel, row, col, value (np.float32),
    intensity, bkg, noise, snr, nr, M), in linear-index order, all statistics in float64."""
    assert frame.dtype == np.float32 and frame.ndim == 3
    P, H, W = frame.shape
    thr = np.float32(thr_peak)
    h = R + 2
    cands = []
    count, total, total_abs = 0, 0.0, 0.0
    for p in range(P):
        for y in range(H):
            for x in range(W):
                v32 = frame[p, y, x]
                if not (v32 > thr):          # NaN fails
                    continue
                v = float(v32)
                count += 1
                total += v
                total_abs += abs(v)
                is_max = True
                for dy, dx in _window_offsets(R):
                    if dy == 0 and dx == 0:
                        continue
                    yy, xx = y + dy, x + dx
                    if not (0 <= yy < H and 0 <= xx < W):
                        continue
                    n = float(frame[p, yy, xx])
                    if n != n:
                        continue
                    before = dy < 0 or (dy == 0 and dx < 0)
                    if (not v > n) if before else (not v >= n):
                        is_max = False
                        break
                if not is_max:
                    continue
                ring = []
                for dy, dx in _ring_offsets(R):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W:
                        n = float(frame[p, yy, xx])
                        if n == n:
                            ring.append(n)
                nr = len(ring)
                if nr:
                    bkg = sum(ring) / nr
                    noise = math.sqrt(sum((n - bkg) * (n - bkg) for n in ring) / nr) if bkg == bkg else float("nan")
                    if any(math.isinf(n) for n in ring):   # Inf - Inf: the contract's NaN, stated outright
                        noise = float("nan")
                else:
                    bkg = noise = 0.0
                den = noise if (noise != noise or noise >= NOISE_FLOOR) else NOISE_FLOOR
                snr = (v - bkg) / den
                inten = 0.0
                for dy, dx in _window_offsets(R):
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W:
                        n = float(frame[p, yy, xx])
                        if n == n:
                            inten += n - bkg
                M = 0.0
                for dy in range(-h, h + 1):
                    for dx in range(-h, h + 1):
                        yy, xx = y + dy, x + dx
                        if 0 <= yy < H and 0 <= xx < W:
                            n = float(frame[p, yy, xx])
                            if n == n:
                                M = max(M, abs(n))
                cands.append(dict(panel=p, row=y, col=x, value=v32, intensity=inten, bkg=bkg, noise=noise,
                                  snr=snr, nr=nr, M=M))
    return dict(cands=cands, count=count, sum=total, sum_abs=total_abs)


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def bounds(c: dict, R: int) -> Tuple[float, float, float]:
    """(E_b, E_n, E_i) of one candidate."""
    W = (2 * R + 1) ** 2
    E_b = c["nr"] * U * c["M"]
    E_n = E_b + 64 * U * c["noise"]
    E_i = W * (E_b + W * U * c["M"])
    return E_b, E_n, E_i


def snr_interval(c: dict, R: int) -> Optional[Tuple[float, float]]:
    """The interval a correct fp32 snr lies in, or None when snr64 is not finite (then the fp32
    value must be the same non-finite value)."""
    if not math.isfinite(c["snr"]) or not math.isfinite(c["M"]):
        return None
    E_b, E_n, _ = bounds(c, R)
    e = E_b + U * c["M"]
    num = (float(c["value"]) - c["bkg"] - e, float(c["value"]) - c["bkg"] + e)
    d_lo, d_hi = c["noise"] - E_n, c["noise"] + E_n
    open_end = d_lo <= NOISE_FLOOR
    d_lo, d_hi = max(d_lo, NOISE_FLOOR), max(d_hi, NOISE_FLOOR)
    qs = [n / d for n in num for d in (d_lo, d_hi)]
    lo, hi = min(qs), max(qs)
    if open_end:
        if num[1] > 0:
            hi = math.inf
        if num[0] < 0:
            lo = -math.inf
    lo -= 4 * U * abs(lo) if math.isfinite(lo) else 0.0
    hi += 4 * U * abs(hi) if math.isfinite(hi) else 0.0
    return lo, hi


def _key(c: dict) -> Tuple[int, int, int]:
    return (c["panel"], c["row"], c["col"])


def borderline(oracles: Sequence[dict], son_min: float, R: int, exact=frozenset()) -> List[Tuple]:
    """Local-maximum candidates whose snr interval contains son_min (`exact`: (frame, panel, row,
    col) of candidates whose statistics are exact in any precision; their snr is a point)."""
    out = []
    for f, o in enumerate(oracles):
        for c in o["cands"]:
            if (f,) + _key(c) in exact:
                continue
            iv = snr_interval(c, R)
            if iv is not None and iv[0] <= son_min <= iv[1]:
                out.append((f,) + _key(c) + iv)
            if iv is None and math.isfinite(c["snr"]):   # finite snr64 under an infinite M: undecidable
                out.append((f,) + _key(c) + (-math.inf, math.inf))
    return out


def place_son_min(oracles: Sequence[dict], intended: float, R: int, exact=frozenset(), span: float = 0.5) -> float:
    """`intended` if no candidate is borderline there, else the midpoint of the widest gap between
    the sorted snr64 values within `span` of it (float64 model only; returned as an fp32 value)."""
    intended = float(np.float32(intended))
    if not borderline(oracles, intended, R, exact):
        return intended
    s = sorted(c["snr"] for o in oracles for c in o["cands"]
               if math.isfinite(c["snr"]) and abs(c["snr"] - intended) <= span)
    s = [intended - span] + s + [intended + span]
    gap, mid = max((b - a, 0.5 * (a + b)) for a, b in zip(s, s[1:]))
    return float(np.float32(mid))


def _same_nonfinite(a: float, b: float) -> bool:
    return (a != a and b != b) or a == b


def _within(a: float, b: float, tol: float) -> bool:
    """|a - b| <= tol for finite values; non-finite values must be the same value."""
    if not (math.isfinite(a) and math.isfinite(b)):
        return _same_nonfinite(a, b)
    return abs(a - b) <= tol


def accepted(o: dict, son_min: float) -> List[dict]:
    return [c for c in o["cands"] if c["snr"] >= son_min]


def check_frame(records: np.ndarray, count: int, summary: Sequence[float], o: dict, son_min: float, R: int,
                what: str) -> Dict[str, float]:
    """One frame of an fp32 implementation against the float64 model.  records: float32 [n, 8]
    (panel, row, col, value, intensity, bkg, noise, snr) in any order.  Asserts the bounds of the
    module docstring; returns the worst error / bound ratios seen (finite values only)."""
    exp = accepted(o, son_min)
    assert count == len(exp), f"{what}: {count} peaks, float64 model {len(exp)}"
    records = np.asarray(records, dtype=np.float32).reshape(-1, 8)
    assert records.shape[0] == len(exp), f"{what}: {records.shape[0]} records for {len(exp)} peaks"
    order = np.lexsort((records[:, 2], records[:, 1], records[:, 0])) if len(exp) else []
    worst = dict(bkg=0.0, noise=0.0, intensity=0.0)
    for r, c in zip(records[order], exp):
        at = f"{what} peak {_key(c)}"
        assert (int(r[0]), int(r[1]), int(r[2])) == _key(c) and all(float(r[i]).is_integer() for i in range(3)), \
            f"{at}: record at {tuple(r[:3])}"
        assert r[3:4].view(np.int32)[0] == np.asarray([c["value"]], np.float32).view(np.int32)[0], \
            f"{at}: value {r[3]!r} vs {c['value']!r}"
        E_b, E_n, E_i = bounds(c, R)
        for name, got, want, tol in (("intensity", r[4], c["intensity"], E_i), ("bkg", r[5], c["bkg"], E_b),
                                     ("noise", r[6], c["noise"], E_n)):
            got = float(got)
            assert _within(got, want, tol), f"{at}: {name} {got!r} vs {want!r}, |diff| {abs(got - want):.3e} > {tol:.3e}"
            if math.isfinite(got) and math.isfinite(want) and math.isfinite(tol) and tol > 0:
                worst[name] = max(worst[name], abs(got - want) / tol)
        iv = snr_interval(c, R)
        snr = float(r[7])
        if iv is None:
            assert _same_nonfinite(snr, c["snr"]), f"{at}: snr {snr!r} vs {c['snr']!r}"
        else:
            assert iv[0] <= snr <= iv[1], f"{at}: snr {snr!r} outside [{iv[0]!r}, {iv[1]!r}] (float64 {c['snr']!r})"
    assert float(summary[0]) == float(o["count"]), f"{what}: summary count {summary[0]} vs {o['count']}"
    assert _within(float(summary[1]), o["sum"], o["count"] * U * o["sum_abs"]), \
        f"{what}: summary sum {float(summary[1])!r} vs {o['sum']!r} (bound {o['count'] * U * o['sum_abs']:.3e})"
    return worst


def assert_coordinates(fx, R, peaks_of_frame):
    """The fixture's planted winners are peaks and its losers are not (peaks_of_frame(f) -> set of
    (panel, row, col))."""
    for f, ws in fx.winners.items():
        got = peaks_of_frame(f)
        missing = [w for w in ws if w not in got]
        assert not missing, f"{fx.name} R={R} frame {f}: expected peaks missing at {missing}"
    for f, ls in fx.losers.items():
        got = peaks_of_frame(f)
        extra = [l for l in ls if l in got]
        assert not extra, f"{fx.name} R={R} frame {f}: peaks where none may be at {extra}"


# ---------------------------------------------------------------------------------------------
# numpy float32 evaluations of one candidate's ring (sequential row-major sums), for calibrating the
# bounds on the CPU and for keeping the retired one-pass formula in view
# ---------------------------------------------------------------------------------------------
def _ring_f32(frame: np.ndarray, c: dict, R: int) -> List[np.float32]:
    P, H, W = frame.shape
    out = []
    for dy, dx in _ring_offsets(R):
        yy, xx = c["row"] + dy, c["col"] + dx
        if 0 <= yy < H and 0 <= xx < W and not np.isnan(frame[c["panel"], yy, xx]):
            out.append(frame[c["panel"], yy, xx])
    return out


def f32_two_pass(frame: np.ndarray, c: dict, R: int) -> Tuple[float, float, float, float]:
    """(bkg, noise, snr, intensity) of candidate c, every operation rounded to float32."""
    f = np.float32
    ring = _ring_f32(frame, c, R)
    with np.errstate(all="ignore"):
        s = f(0)
        for n in ring:
            s = f(s + n)
        bkg = f(s / f(len(ring))) if ring else f(0)
        ss = f(0)
        for n in ring:
            d = f(n - bkg)
            ss = f(ss + f(d * d))
        noise = f(np.sqrt(f(ss / f(len(ring))))) if ring else f(0)
        den = f(NOISE_FLOOR) if noise < f(NOISE_FLOOR) else noise
        snr = f(f(c["value"] - bkg) / den)
        inten = f(0)
        P, H, W = frame.shape
        for dy, dx in _window_offsets(R):
            yy, xx = c["row"] + dy, c["col"] + dx
            if 0 <= yy < H and 0 <= xx < W and not np.isnan(frame[c["panel"], yy, xx]):
                inten = f(inten + f(frame[c["panel"], yy, xx] - bkg))
    return float(bkg), float(noise), float(snr), float(inten)


def f32_one_pass_noise(frame: np.ndarray, c: dict, R: int) -> float:
    """noise by the RETIRED one-pass formula sqrt(max(s2/nr - bkg^2, 0)) in float32."""
    f = np.float32
    ring = _ring_f32(frame, c, R)
    if not ring:
        return 0.0
    with np.errstate(all="ignore"):
        s, s2 = f(0), f(0)
        for n in ring:
            s = f(s + n)
            s2 = f(s2 + f(n * n))
        nr = f(len(ring))
        bkg = f(s / nr)
        var = f(f(s2 / nr) - f(bkg * bkg))
        return float(np.sqrt(max(var, f(0))))


# ---------------------------------------------------------------------------------------------
# fixtures
# ---------------------------------------------------------------------------------------------
class Fixture:
    """frames: float32 [F, P, H, W]; son_intended: where the snr cut is meant to sit (son_min(R) moves
    it off any borderline candidate); exact: candidates whose snr is exact in any precision;
    winners: {frame: [(panel, row, col), ...]} coordinates that must be peaks; losers likewise must
    not be."""

    def __init__(self, name, frames, thr_peak, son_intended, max_peaks=256, exact=frozenset(), winners=None,
                 losers=None, son_fixed=None):
        self.name = name
        self.frames = np.ascontiguousarray(frames, dtype=np.float32)
        self.frames.setflags(write=False)
        self.thr_peak = float(np.float32(thr_peak))
        self.son_intended = son_intended
        self.son_fixed = son_fixed
        self.max_peaks = max_peaks
        self.exact = frozenset(exact)
        self.winners = winners or {}
        self.losers = losers or {}

    @property
    def shape(self):
        return tuple(self.frames.shape[1:])

    @functools.lru_cache(maxsize=None)
    def oracle(self, R: int) -> Tuple[dict, ...]:
        return tuple(oracle_frame(fr, self.thr_peak, R) for fr in self.frames)

    @functools.lru_cache(maxsize=None)
    def son_min(self, R: int) -> float:
        if self.son_fixed is not None:
            return float(np.float32(self.son_fixed))
        return place_son_min(self.oracle(R), self.son_intended, R, self.exact)

    def assert_precondition(self, R: int):
        b = borderline(self.oracle(R), self.son_min(R), R, self.exact)
        assert not b, f"{self.name} R={R}: son_min {self.son_min(R)!r} inside the snr interval of {b[:4]}"


def _ties_frame(seed: int, extra: bool = False):
    """(2, 24, 32), integer background 0..5; returns (frame, winners, losers)."""
    rng = np.random.default_rng(1000 + seed)
    fr = rng.integers(0, 6, size=(2, 24, 32)).astype(np.float32)
    winners, losers = [], []

    def plateau(p, pix, val):
        for (y, x) in pix:
            fr[p, y, x] = val
        pix = sorted(pix)
        winners.append((p,) + pix[0])
        losers.extend((p,) + q for q in pix[1:])

    # panel 0: the four pair orientations and a 2x3 plateau, every plant > 2 pixels from the next
    plateau(0, [(4, 4), (4, 5)], 200.0)                  # horizontal
    plateau(0, [(4, 11), (5, 11)], 210.0)                # vertical
    plateau(0, [(4, 17), (5, 18)], 220.0)                # diagonal
    plateau(0, [(4, 25), (5, 24)], 230.0)                # anti-diagonal: (5, 24) has dx < 0 but dy > 0, so it is AFTER
    plateau(0, [(12, 8), (12, 9), (12, 10), (13, 8), (13, 9), (13, 10)], 240.0)   # 2x3
    plateau(0, [(18, 20), (18, 21), (19, 20), (19, 21)], 250.0)                    # 2x2
    # panel 1: plateaus in each corner and on each edge
    plateau(1, [(0, 0), (0, 1), (1, 0), (1, 1)], 300.0)
    plateau(1, [(0, 30), (0, 31), (1, 30), (1, 31)], 310.0)
    plateau(1, [(22, 0), (22, 1), (23, 0), (23, 1)], 320.0)
    plateau(1, [(22, 30), (22, 31), (23, 30), (23, 31)], 330.0)
    plateau(1, [(0, 14), (0, 15)], 340.0)                # top edge
    plateau(1, [(23, 15), (23, 16)], 350.0)              # bottom edge
    plateau(1, [(11, 0), (12, 0)], 360.0)                # left edge
    plateau(1, [(11, 31), (12, 31)], 370.0)              # right edge
    if extra:   # a frame-dependent lone peak (the 67-frame fixture: every frame different)
        y, x = 8 + seed % 9, 8 + (seed * 5) % 16
        fr[1, y, x] = 400.0 + seed
        winners.append((1, y, x))
    return fr, winners, losers


def _ties(nframes: int, name: str, extra: bool) -> Fixture:
    frames, winners, losers = [], {}, {}
    for f in range(nframes):
        fr, w, l = _ties_frame(f, extra)
        frames.append(fr)
        winners[f], losers[f] = w, l
    return Fixture(name, np.stack(frames), thr_peak=10.0, son_intended=3.0, max_peaks=64, winners=winners,
                   losers=losers)


def _seams() -> Fixture:
    """(3, 12, 20): cols a multiple of 4, not of 8."""
    rng = np.random.default_rng(2)
    frames = (3.0 * rng.random((2, 3, 12, 20))).astype(np.float32)
    W = 20
    w0, w1 = [], []
    # frame 0: seams and corners
    frames[0, 0, 11, 5] = 50.0    # last row of panel 0 ...
    frames[0, 1, 0, 5] = 80.0     # ... and the larger value directly below it in memory
    frames[0, 1, 5, 19] = 50.0    # last column of a row ...
    frames[0, 1, 6, 0] = 80.0     # ... and the larger value next in memory
    w0 += [(0, 11, 5), (1, 0, 5), (1, 5, 19), (1, 6, 0)]
    for (y, x), v in zip([(0, 0), (0, 19), (11, 0), (11, 19)], (60.0, 61.0, 62.0, 63.0)):
        frames[0, 2, y, x] = v
        w0.append((2, y, x))
    # frame 1: a peak at every column 0..7 and W-8..W-1 (all four `off` alignments at both panel
    # edges, groups that start left of the panel), three per row and side so none suppresses another
    for x in list(range(8)) + list(range(W - 8, W)):
        xs = x if x < 8 else x - (W - 8)
        p, y = xs % 3, 2 + 3 * (xs % 3)
        frames[1, p, y, x] = 70.0 + x
        w1.append((p, y, x))
    return Fixture("seams", frames, thr_peak=10.0, son_intended=2.0, winners={0: w0, 1: w1})


def _empty_ring() -> Fixture:
    """(2, 3, 4): with R = 2 the ring (distance 3..4) of a pixel at x = 1, 2 has no present pixel."""
    rng = np.random.default_rng(3)
    frames = (2.0 * rng.random((1, 2, 3, 4))).astype(np.float32)
    frames[0, 0, 1, 1] = 30.0
    frames[0, 1, 1, 2] = 40.0
    return Fixture("empty_ring", frames, thr_peak=10.0, son_intended=4.0, winners={0: [(0, 1, 1), (1, 1, 2)]})


THR_EQ_SON = 16.0


def _threshold() -> Fixture:
    """(1, 20, 48).  Rows 0..10: three candidates on a +-1 checkerboard (every ring of either radius
    holds +1 and -1 in equal numbers, so bkg = 0, noise = 1 and snr == v exactly in any precision)
    with v = son_min, one ulp below and one ulp above.  Rows 11..: a pixel exactly at thr_peak and
    one at nextafter(thr_peak, +inf) on a small integer background."""
    f32 = np.float32
    rng = np.random.default_rng(4)
    fr = np.zeros((1, 20, 48), dtype=np.float32)
    fr[0, 11:, :] = 0.5 * rng.integers(0, 2, size=(9, 48)).astype(np.float32)
    son = f32(THR_EQ_SON)
    vals = {6: son, 18: np.nextafter(son, f32(-np.inf)), 30: np.nextafter(son, f32(np.inf))}
    for cx, v in vals.items():
        for dy in range(-4, 5):
            for dx in range(-4, 5):
                if max(abs(dy), abs(dx)) >= 2:
                    fr[0, 5 + dy, cx + dx] = 1.0 if (dy + dx) % 2 == 0 else -1.0
        fr[0, 5, cx] = v
    thr = f32(10.0)
    fr[0, 15, 10] = thr
    fr[0, 15, 25] = np.nextafter(thr, f32(np.inf))
    exact = {(0, 0, 5, 6), (0, 0, 5, 18), (0, 0, 5, 30)}
    return Fixture("threshold", fr[None], thr_peak=10.0, son_intended=THR_EQ_SON, son_fixed=THR_EQ_SON, exact=exact,
                   winners={0: [(0, 5, 6), (0, 5, 30), (0, 15, 25)]}, losers={0: [(0, 5, 18), (0, 15, 10)]})


def _nonfinite() -> Fixture:
    """(2, 32, 40), background N(5, 1) clipped below thr_peak, peaks nearby."""
    rng = np.random.default_rng(5)
    frames = np.minimum(5.0 + rng.standard_normal((2, 2, 32, 40)), 9.0).astype(np.float32)
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    winners = {0: [], 1: []}
    losers = {0: [], 1: []}
    for f in range(2):
        fr = frames[f]
        # NaN inside a window (distance 1) and inside a ring (distance 3) of a peak: absent, nr drops
        fr[0, 6, 6] = 60.0
        fr[0, 5, 7] = nan
        fr[0, 6, 9] = nan
        fr[0, 9, 5] = nan
        winners[f].append((0, 6, 6))
        # a NaN where a peak would be, real peaks either side of it
        fr[0, 6, 20] = nan
        fr[0, 6, 17] = 45.0
        fr[0, 6, 23] = 46.0
        winners[f] += [(0, 6, 17), (0, 6, 23)]
        losers[f].append((0, 6, 20))
        # a peak at a corner next to NaNs
        fr[0, 0, 39] = 55.0
        fr[0, 1, 38] = nan
        fr[0, 3, 39] = nan
        winners[f].append((0, 0, 39))
        # +Inf / -Inf at distance 3 (inside the ring at either radius) of a would-be peak: rejected
        fr[0, 20, 10] = 70.0
        fr[0, 20, 13] = inf
        fr[0, 20, 30] = 71.0
        fr[0, 23, 30] = -inf
        losers[f] += [(0, 20, 10), (0, 20, 30)]
        winners[f].append((0, 20, 13))           # the +Inf pixel is itself a peak
        # a +Inf pixel that is a peak on a clean background, and an ordinary peak far from everything
        fr[1, 10, 10] = inf
        fr[1, 24, 30] = 52.0
        winners[f] += [(1, 10, 10), (1, 24, 30)]
    frames[1, 1, 24, 30] = 58.0                  # the two frames differ
    return Fixture("nonfinite", frames, thr_peak=12.0, son_intended=4.0, winners=winners, losers=losers)


def _offset_frames(shape, nframes, offset, seed, npeaks):
    rng = np.random.default_rng(seed)
    frames = (3.0 * rng.standard_normal((nframes,) + shape))
    for f in range(nframes):
        flat = rng.choice(int(np.prod(shape)), size=npeaks, replace=False)
        frames[f].reshape(-1)[flat] += rng.uniform(12.0, 80.0, size=npeaks)
    return (frames + offset).astype(np.float32)


def _offset(offset: float) -> Fixture:
    """(2, 48, 64), N(offset, 3) with 60 planted peaks of +12..+80 per frame.  The same seed for every
    offset: the frames differ only by the offset (and its rounding)."""
    name = f"offset_{int(offset)}"
    return Fixture(name, _offset_frames((2, 48, 64), 2, offset, 6, 60), thr_peak=offset + 12.0, son_intended=4.0)


def _paths(offset: float) -> Fixture:
    """(1, 64, 64) x 3 frames: one 16-KB chunk (the unchecked fast load) and one workgroup per frame,
    ~30 % of the pixels above thr_peak -> more than 512 candidates per workgroup.  N(offset, 20): wide
    enough that at offset 5000 the snr intervals (~ nr * u * 5000 / 20) stay far narrower than the gaps
    between the ~1400 local maxima's snr values, so a clear son_min exists."""
    rng = np.random.default_rng(7)
    frames = (20.0 * rng.standard_normal((3, 1, 64, 64)) + offset).astype(np.float32)
    return Fixture(f"paths_{int(offset)}", frames, thr_peak=offset + 10.4, son_intended=1.5, max_peaks=1024)


def _partial_chunk() -> Fixture:
    """(2, 40, 68): 1360 float4 per frame = one full 1024-float4 chunk and one bounds-checked one."""
    rng = np.random.default_rng(8)
    frames = (3.0 + rng.standard_normal((2, 2, 40, 68))).astype(np.float32)
    w = [(1, 39, 67), (1, 39, 0), (1, 38, 30), (1, 36, 50), (1, 39, 40), (0, 10, 10), (0, 39, 67), (1, 0, 0)]
    for f in range(2):
        for i, (p, y, x) in enumerate(w):
            frames[f, p, y, x] = 40.0 + 3 * i + f
    return Fixture("partial_chunk", frames, thr_peak=12.0, son_intended=4.0, winners={0: w, 1: w})


OFFSETS = (0.0, 1000.0, 5000.0, 20000.0, -5000.0)


@functools.lru_cache(maxsize=None)
def fixture(name: str) -> Fixture:
    if name == "ties":
        return _ties(2, "ties", extra=False)
    if name == "many_frames":
        return _ties(67, "many_frames", extra=True)
    if name.startswith("offset_"):
        return _offset(float(name[len("offset_"):]))
    if name.startswith("paths_"):
        return _paths(float(name[len("paths_"):]))
    return {"seams": _seams, "empty_ring": _empty_ring, "threshold": _threshold, "nonfinite": _nonfinite,
            "partial_chunk": _partial_chunk}[name]()


FIXTURES = ("ties", "seams", "empty_ring", "threshold", "nonfinite") + tuple(f"offset_{int(o)}" for o in OFFSETS) + \
    ("paths_0", "paths_5000", "partial_chunk", "many_frames")
