// K-11 powder statistics for queue consumers: per-pixel, per-class count / sum / sum of squares /
// maximum / count above a threshold of the CALIBRATED float32 value over a batch of frames, ADDED to
// run accumulators the caller owns.
//
// Numerics contract (docs/ARCHITECTURE.md, "Powder statistics"): every word is an INTEGER function of
// the inputs, so the result does not depend on frame order, batch split or stream, is word-for-word
// equal to the golden model (ops/reference.py powder_accumulate_reference) and two consumers'
// accumulators merge to exactly what one would have produced.
//   class         NC == 2: frame f is class 1 ("hit") iff keys[f] >= key_min, else class 0 ("miss");
//                 NC == 1 (no keys): every frame is class 0
//   contributes   vmin <= v && v <= vmax as float32 (NaN fails, +-inf is outside the finite window)
//   q             (int) rintf(v * 2^S): the multiply is exact, ties go to even (K-08's rounding)
//   cnt[c, p] += 1 (int32)      sum[c, p] += q (int64, signed)      sq[c, p] += q * q (int64)
//   qmax[c, p] = max(qmax, q) (int32, INT32_MIN = "no sample")      above[c, p] += (v >= thr) (int32)
//   nfr[c] += frames of class c in the launch (int64, one add by one owner thread)
// The callers hold Q = ceil(max(|vmin|, |vmax|) * 2^S) below 2^31 (q fits an int32) and a run at or
// below min(2^31 - 1, (2^63 - 1) / Q^2) frames, so no word overflows.  The kernel never clears anything.
//
// MI355X design: the owner-lane accumulator of accum.h over 16-B float32 loads, one plane per class.
// A frame's class is the same for the whole grid: every wave reads the (at most 64) keys with ONE
// load, lane f taking keys[f], and a ballot turns them into a 64-bit frame mask per class that lives
// in scalar registers.  The lane then makes one PASS per class over that class's frames only -- the
// frame indices come off the mask with scalar bit operations, the frame pointers with scalar loads
// from the kernel arguments -- with ONE set of partials in registers, then the read-modify-write of
// its words of that class.  A class without a frame in the launch has an empty mask: its pass is
// skipped on a scalar branch and its words are neither read nor written (in steady state most batches
// are all misses: half the accumulator traffic).
//
// In-batch partial widths, from the 64-frame bound: cnt, above <= 64 (32-bit); |sum| <= 64 * Q < 2^37
// (64-bit); sq <= 64 * Q^2, which the run bound keeps below 2^63 for ANY accepted Q (2^50 at the
// default Q = 2^22) (64-bit, the product q * q of two int32 is one v_mad_i64_i32).
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
// powder_kernel: 74 VGPRs, 102 SGPRs, no scratch memory (0 bytes per lane, no spills), no LDS, occupancy
// 6 waves per SIMD.  The frame pointers come by s_load_dwordx2, the frames by global_load_dwordx4 nt.
#include "accum.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

struct PowParams {
  float vmin, vmax, scale, thr;   // scale = 2^S
};

// in-batch partials of NP pixels of ONE class; every index is a compile-time constant after
// unrolling, so the arrays live in VGPRs
template <int NP>
struct PowPart {
  uint32_t cnt[NP];
  uint32_t above[NP];
  int32_t qmax[NP];
  long long sum[NP];
  unsigned long long sq[NP];
};

template <int NP>
__device__ __forceinline__ void pow_zero(PowPart<NP>& a) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    a.cnt[i] = 0u;
    a.above[i] = 0u;
    a.qmax[i] = INT32_MIN;
    a.sum[i] = 0ll;
    a.sq[i] = 0ull;
  }
}

// one sample into pixel slot I
template <int NP, int I>
__device__ __forceinline__ void pow_add(PowPart<NP>& a, const float v, const PowParams& pp) {
  const bool ok = v >= pp.vmin && v <= pp.vmax;
  const int q = ok ? (int)rintf(v * pp.scale) : 0;   // |q| <= Q < 2^31
  a.cnt[I] += ok ? 1u : 0u;
  a.above[I] += (ok && v >= pp.thr) ? 1u : 0u;
  a.qmax[I] = max(a.qmax[I], ok ? q : INT32_MIN);
  a.sum[I] += (long long)q;
  a.sq[I] += (unsigned long long)((long long)q * (long long)q);
}

__device__ __forceinline__ void pow_add4(PowPart<4>& a, const f32x4_t r, const PowParams& pp) {
  pow_add<4, 0>(a, r.x, pp);
  pow_add<4, 1>(a, r.y, pp);
  pow_add<4, 2>(a, r.z, pp);
  pow_add<4, 3>(a, r.w, pp);
}

// the lowest frame of the (wave-uniform, non-empty) mask, removed from it
__device__ __forceinline__ int pow_next(uint64_t& m) {
  const int f = __builtin_ctzll(m);
  m &= m - 1ull;
  return f;
}

__global__ __launch_bounds__(256) void powder_kernel(const FramePtrs fp, const int nframes, const int64_t n,
                                                     const PowParams pp, const int* __restrict__ keys,
                                                     const int key_min, long long* __restrict__ nfr,
                                                     int32_t* __restrict__ cnt, long long* __restrict__ sum,
                                                     unsigned long long* __restrict__ sq,
                                                     int32_t* __restrict__ qmax, int32_t* __restrict__ above) {
  // frame masks per class, before any divergence: lane f of every wave looks at keys[f]
  const uint64_t all = nframes >= 64 ? ~0ull : ((1ull << nframes) - 1ull);
  uint64_t hits = 0ull;
  if (keys != nullptr) {
    const int f = (int)(threadIdx.x & 63u);
    const bool hit = f < nframes && keys[f] >= key_min;
    hits = __ballot(hit);
  }
  const uint64_t cls[2] = {all & ~hits, hits};
  const int64_t nq = n >> 2;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q == 0) {   // the owner of nfr (lane 0 exists for every n >= 1: the tail lane when n < 4)
    if (cls[0] != 0ull) nfr[0] += (long long)__builtin_popcountll(cls[0]);
    if (cls[1] != 0ull) nfr[1] += (long long)__builtin_popcountll(cls[1]);
  }
  if (q < nq) {
    const int64_t p0 = q * 4;
    const bool vec = (n & 3) == 0;   // the planes of class 1 start at n: 16-B aligned iff n % 4 == 0
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      uint64_t m = cls[c];
      if (m == 0ull) continue;   // no frame of this class: its words stay as they are (scalar branch)
      PowPart<4> a;
      pow_zero(a);
      acc_group<f32x4_t, true>(__builtin_popcountll(m), q, [&] { return fp.in[pow_next(m)]; },
                               [&](const f32x4_t r) { pow_add4(a, r, pp); });
      const int64_t o = (int64_t)c * n + p0;
      if (c == 0 || vec) {
        Words32 wc, wa, wm;
        Words64 ws, wq;
        wc.load(cnt + o); wa.load(above + o); wm.load(qmax + o); ws.load(sum + o); wq.load(sq + o);
        wc.add(a.cnt); wa.add(a.above); wm.smax(a.qmax); ws.add(a.sum); wq.add(a.sq);
        wc.store(cnt + o); wa.store(above + o); wm.store(qmax + o); ws.store(sum + o); wq.store(sq + o);
      } else {
        acc_add(cnt + o, a.cnt); acc_add(above + o, a.above); acc_max(qmax + o, a.qmax);
        acc_add(sum + o, a.sum); acc_add(sq + o, a.sq);
      }
    }
  } else if (q == nq) {
    // scalar tail: the frame's last n % 4 pixels (the launcher adds this lane only when there are any)
    for (int64_t p = nq * 4; p < n; ++p) {
#pragma unroll
      for (int c = 0; c < 2; ++c) {
        uint64_t m = cls[c];
        if (m == 0ull) continue;
        PowPart<1> a;
        pow_zero(a);
        while (m != 0ull) pow_add<1, 0>(a, gin<float>(fp.in[pow_next(m)])[p], pp);
        const int64_t o = (int64_t)c * n + p;
        acc_add(cnt + o, a.cnt); acc_add(above + o, a.above); acc_max(qmax + o, a.qmax);
        acc_add(sum + o, a.sum); acc_add(sq + o, a.sq);
      }
    }
  }
}

void launch_powder(const FramePtrs& fp, int nframes, int64_t n, float vmin, float vmax, int frac_bits,
                   float thr_above, int nc, uint64_t keys, int key_min, uint64_t nfr, uint64_t cnt, uint64_t sum,
                   uint64_t sq, uint64_t qmax, uint64_t above, uint64_t stream) {
  check_nframes(nframes, "powder");
  check_frame_size(n, "powder");
  const float scale = quant_bound(vmin, vmax, frac_bits, nframes, "powder");
  check(thr_above == thr_above, "powder: thr_above is NaN");
  check(nc == 1 || nc == 2, "powder: 1 or 2 classes");
  check((nc == 2) == (keys != 0), "powder: keys are given iff there are 2 classes");
  check(keys % 4 == 0, "powder: keys must be 4-B aligned");
  check(nfr != 0 && nfr % 8 == 0, "powder: nfr must be non-null and 8-B aligned");
  check(cnt != 0 && sum != 0 && sq != 0 && qmax != 0 && above != 0 && aligned16(cnt) && aligned16(sum) &&
            aligned16(sq) && aligned16(qmax) && aligned16(above),
        "powder: accumulators must be non-null and 16-B aligned");
  check_frames(fp, nframes, "powder");
  const PowParams pp{vmin, vmax, scale, thr_above};
  hipLaunchKernelGGL(powder_kernel, owner_lane_grid(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), fp, nframes, n, pp,
                     reinterpret_cast<const int*>(keys), key_min, reinterpret_cast<long long*>(nfr),
                     reinterpret_cast<int32_t*>(cnt), reinterpret_cast<long long*>(sum),
                     reinterpret_cast<unsigned long long*>(sq), reinterpret_cast<int32_t*>(qmax),
                     reinterpret_cast<int32_t*>(above));
  hip_check(hipGetLastError(), "powder launch");
}

}  // namespace pr
