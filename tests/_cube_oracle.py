"""A Python-integer oracle of the K-15 cube contract: one loop per sample, no torch, no numpy arithmetic."""
import math
import struct


def _f32(v: float) -> float:
    return struct.unpack("<f", struct.pack("<f", v))[0]


def _round_half_even(x: float) -> int:
    f = math.floor(x)
    d = x - f
    if d > 0.5 or (d == 0.5 and f % 2 == 1):
        return int(f) + 1
    return int(f)


def cube_oracle(frames, bins, nbins, vmin, vmax, frac_bits):
    """frames: F lists of n Python floats (float32 values); bins: F ints in -1 .. nbins - 1.  Returns
    (nfr [B], cnt [B][n], sum [B][n], sq [B][n]) as lists of Python ints."""
    lo, hi = _f32(vmin), _f32(vmax)
    n = len(frames[0])
    nfr = [0] * nbins
    cnt = [[0] * n for _ in range(nbins)]
    s = [[0] * n for _ in range(nbins)]
    sq = [[0] * n for _ in range(nbins)]
    for frame, b in zip(frames, bins):
        if b < 0:
            continue
        nfr[b] += 1
        for p, v in enumerate(frame):
            if v != v or not (lo <= v <= hi):
                continue
            q = _round_half_even(v * 2 ** frac_bits)   # a float32 times 2^S is exact in a double
            cnt[b][p] += 1
            s[b][p] += q
            sq[b][p] += q * q
    return nfr, cnt, s, sq
