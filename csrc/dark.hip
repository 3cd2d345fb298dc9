// K-09 dark-run statistics for queue consumers: per-pixel, per-candidate count / sum / sum of squares
// of the raw ADU over a batch of raw uint16 frames, ADDED to run accumulators the caller owns.
//
// Numerics contract (docs/ARCHITECTURE.md, "Dark statistics"): everything is an INTEGER, so the
// result does not depend on frame order, batch split or stream, is word-for-word equal to the golden
// model (ops/reference.py dark_accumulate_reference) and two consumers' accumulators add to exactly
// what one would have produced.
//   decode        epix10ka  adu = r & 0x3FFF, c = (r >> 14) & 1 (bit 15 ignored), always valid
//                 jungfrau  adu = r & 0x3FFF, c = 0, 1, 2 for gb = r >> 14 = 0, 1, 3; gb == 2 invalid
//                 plain     adu = r, c = 0, always valid
//   contributes   valid and adu_lo <= adu <= adu_hi (inclusive)
//   cnt[c, p] += 1 (int32)   sum[c, p] += adu (int64)   sq[c, p] += adu * adu (int64)
// 65535^2 * (2^31 - 1) < 2^63: the only limit is the int32 count, which the callers hold below 2^31
// frames per run.  The kernel never clears the accumulators.
//
// MI355X design: the owner-lane accumulator of accum.h over 8-B raw loads, 8 then 1 loads in flight,
// one plane per candidate.  In-batch partials are 32-bit where the 64-frame bound proves it (cnt <= 64,
// sum <= 64 * 65535 < 2^32); sq (64 * 65535^2 > 2^32) is 64-bit.  A candidate none of the lane's four
// pixels hit is skipped -- its words are neither read nor written (an epix dark run never hits
// candidate 1: half the accumulator traffic).
#include "accum.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

template <int KIND>
struct DarkTraits;
template <>
struct DarkTraits<kEpix10ka> { static constexpr int NC = 2; };
template <>
struct DarkTraits<kJungfrau> { static constexpr int NC = 3; };
template <>
struct DarkTraits<kPlain> { static constexpr int NC = 1; };

// in-batch partials of NP pixels; every index is a compile-time constant after unrolling, so the
// arrays live in VGPRs (a candidate-indexed access would send them to scratch)
template <int NC, int NP>
struct DarkPart {
  uint32_t cnt[NC][NP];
  uint32_t sum[NC][NP];
  uint64_t sq[NC][NP];
};

template <int NC, int NP>
__device__ __forceinline__ void dark_zero(DarkPart<NC, NP>& a) {
#pragma unroll
  for (int c = 0; c < NC; ++c)
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      a.cnt[c][i] = 0u;
      a.sum[c][i] = 0u;
      a.sq[c][i] = 0ull;
    }
}

// one raw word into pixel slot I: a masked add to every candidate (no indexed register access)
template <int KIND, int NC, int NP, int I>
__device__ __forceinline__ void dark_add(DarkPart<NC, NP>& a, const uint32_t raw, const uint32_t lo,
                                         const uint32_t span) {
  bool valid;
  const int cand = decode_cand(raw, KIND, valid);
  const uint32_t adu = KIND == kPlain ? raw : (raw & 0x3FFFu);
  const bool ok = valid && (adu - lo) <= span;   // lo <= adu <= hi, unsigned wrap for adu < lo
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    const uint32_t m = (ok && cand == c) ? 1u : 0u;
    const uint32_t v = m ? adu : 0u;
    a.cnt[c][I] += m;
    a.sum[c][I] += v;
    a.sq[c][I] += (uint64_t)(v * v);   // adu^2 <= 65535^2 < 2^32: the 32-bit product is exact
  }
}

template <int KIND, int NC>
__device__ __forceinline__ void dark_add4(DarkPart<NC, 4>& a, const uint2 r, const uint32_t lo, const uint32_t span) {
  dark_add<KIND, NC, 4, 0>(a, r.x & 0xFFFFu, lo, span);
  dark_add<KIND, NC, 4, 1>(a, r.x >> 16, lo, span);
  dark_add<KIND, NC, 4, 2>(a, r.y & 0xFFFFu, lo, span);
  dark_add<KIND, NC, 4, 3>(a, r.y >> 16, lo, span);
}

template <int KIND>
__global__ __launch_bounds__(256) void dark_kernel(const FramePtrs fp, const int nframes, const int64_t n,
                                                   const uint32_t lo, const uint32_t span,
                                                   int32_t* __restrict__ cnt, unsigned long long* __restrict__ sum,
                                                   unsigned long long* __restrict__ sq) {
  constexpr int NC = DarkTraits<KIND>::NC;
  const int64_t nq = n >> 2;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q < nq) {
    DarkPart<NC, 4> a;
    dark_zero(a);
    int f = 0;
    acc_group<uint2, false>(nframes, q, [&] { return fp.in[f++]; },
                            [&](const uint2 r) { dark_add4<KIND, NC>(a, r, lo, span); });
    const int64_t p0 = q * 4;
    const bool vec = (n & 3) == 0;   // planes of c >= 1 start at c * n: 16-B aligned iff n % 4 == 0
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      if ((a.cnt[c][0] | a.cnt[c][1] | a.cnt[c][2] | a.cnt[c][3]) == 0u) continue;   // untouched: words stay as they are
      const int64_t o = (int64_t)c * n + p0;
      if (c == 0 || vec) {
        Words32 wc;
        Words64 ws, wq;
        wc.load(cnt + o); ws.load(sum + o); wq.load(sq + o);
        wc.add(a.cnt[c]); ws.add(a.sum[c]); wq.add(a.sq[c]);
        wc.store(cnt + o); ws.store(sum + o); wq.store(sq + o);
      } else {
        acc_add(cnt + o, a.cnt[c]); acc_add(sum + o, a.sum[c]); acc_add(sq + o, a.sq[c]);
      }
    }
  } else if (q == nq) {
    // scalar tail: the frame's last n % 4 pixels (the launcher adds this lane only when there are any)
    for (int64_t p = nq * 4; p < n; ++p) {
      DarkPart<NC, 1> a;
      dark_zero(a);
      for (int f = 0; f < nframes; ++f) dark_add<KIND, NC, 1, 0>(a, (uint32_t)gin<uint16_t>(fp.in[f])[p], lo, span);
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (a.cnt[c][0] == 0u) continue;
        const int64_t o = (int64_t)c * n + p;
        acc_add(cnt + o, a.cnt[c]); acc_add(sum + o, a.sum[c]); acc_add(sq + o, a.sq[c]);
      }
    }
  }
}

void launch_dark(const FramePtrs& fp, int nframes, int64_t n, int kind, int adu_lo, int adu_hi, uint64_t cnt,
                 uint64_t sum, uint64_t sq, uint64_t stream) {
  check_nframes(nframes, "dark");
  check_frame_size(n, "dark");
  check(kind >= 0 && kind <= 2, "dark: unknown gain kind");
  check(adu_lo >= 0 && adu_lo <= adu_hi && adu_hi <= 65535, "dark: the ADU window must satisfy 0 <= lo <= hi <= 65535");
  check(cnt != 0 && sum != 0 && sq != 0 && aligned16(cnt) && aligned16(sum) && aligned16(sq),
        "dark: accumulators must be non-null and 16-B aligned");
  check_frames(fp, nframes, "dark");
  const dim3 grid = owner_lane_grid(n);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  int32_t* C = reinterpret_cast<int32_t*>(cnt);
  unsigned long long* S = reinterpret_cast<unsigned long long*>(sum);
  unsigned long long* Q = reinterpret_cast<unsigned long long*>(sq);
  const uint32_t lo = (uint32_t)adu_lo, span = (uint32_t)(adu_hi - adu_lo);
  switch (kind) {
    case kEpix10ka: hipLaunchKernelGGL(dark_kernel<kEpix10ka>, grid, dim3(256), 0, s, fp, nframes, n, lo, span, C, S, Q); break;
    case kJungfrau: hipLaunchKernelGGL(dark_kernel<kJungfrau>, grid, dim3(256), 0, s, fp, nframes, n, lo, span, C, S, Q); break;
    default: hipLaunchKernelGGL(dark_kernel<kPlain>, grid, dim3(256), 0, s, fp, nframes, n, lo, span, C, S, Q); break;
  }
  hip_check(hipGetLastError(), "dark launch");
}

}  // namespace pr
