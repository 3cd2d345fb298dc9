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
// MI355X design: a lane owns 4 consecutive pixels (one 16-B non-temporal load per frame), one owner
// per pixel per launch, so no atomics.  A frame's class is the same for the whole grid: every wave
// reads the (at most 64) keys with ONE load, lane f taking keys[f], and a ballot turns them into a
// 64-bit frame mask per class that lives in scalar registers.  The lane then makes one PASS per class
// over that class's frames only -- the frame indices come off the mask with scalar bit operations,
// the frame pointers with scalar loads from the kernel arguments -- with 8 (then 4, then 1) loads in
// flight, ONE set of partials in registers, and after the pass ONE read-modify-write of the lane's
// words of that class: 16-B accesses where the plane is 16-B aligned (cnt / qmax / above: one each,
// sum / sq: two each).  A class without a frame in the launch has an empty mask: its pass is skipped
// on a scalar branch and its words are neither read nor written (in steady state most batches are all
// misses: half the accumulator traffic).  The planes of class 1 start at n elements, 16-B aligned iff
// n % 4 == 0; otherwise its words go one by one, as K-09 does for candidates >= 1.  The n % 4 last
// pixels of a frame go to one extra lane that walks them with scalar accesses.
//
// In-batch partial widths, from the 64-frame bound: cnt, above <= 64 (32-bit); |sum| <= 64 * Q < 2^37
// (64-bit); sq <= 64 * Q^2, which the run bound keeps below 2^63 for ANY accepted Q (2^50 at the
// default Q = 2^22) (64-bit, the product q * q of two int32 is one v_mad_i64_i32).
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
// powder_kernel: 74 VGPRs, 102 SGPRs, no scratch memory (0 bytes per lane, no spills), no LDS, occupancy
// 6 waves per SIMD.  The frame pointers come by s_load_dwordx2, the frames by global_load_dwordx4 nt.
#include <cmath>

#include "common.h"
#include "kernels.h"

namespace pr {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

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

// K frames of the mask with K loads in flight
template <int K>
__device__ __forceinline__ void pow_group(PowPart<4>& a, const FramePtrs& fp, uint64_t& m, const int64_t q,
                                          const PowParams& pp) {
  f32x4_t r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = ld_nt_f4(gin<f32x4_t>(fp.in[pow_next(m)]) + q);
#pragma unroll
  for (int k = 0; k < K; ++k) pow_add4(a, r[k], pp);
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
      int left = __builtin_popcountll(m);
      for (; left >= 8; left -= 8) pow_group<8>(a, fp, m, q, pp);
      if (left >= 4) {
        pow_group<4>(a, fp, m, q, pp);
        left -= 4;
      }
      for (; left > 0; --left) pow_group<1>(a, fp, m, q, pp);
      const int64_t o = (int64_t)c * n + p0;
      if (c == 0 || vec) {
        u32x4_t* pc = reinterpret_cast<u32x4_t*>(cnt + o);
        u32x4_t* pa = reinterpret_cast<u32x4_t*>(above + o);
        u32x4_t* pm = reinterpret_cast<u32x4_t*>(qmax + o);
        u64x2_t* ps = reinterpret_cast<u64x2_t*>(sum + o);
        u64x2_t* pq = reinterpret_cast<u64x2_t*>(sq + o);
        u32x4_t vc = *pc, va = *pa, vm = *pm;
        u64x2_t s0 = ps[0], s1 = ps[1], q0 = pq[0], q1 = pq[1];
        vc.x += a.cnt[0]; vc.y += a.cnt[1]; vc.z += a.cnt[2]; vc.w += a.cnt[3];
        va.x += a.above[0]; va.y += a.above[1]; va.z += a.above[2]; va.w += a.above[3];
        vm.x = (uint32_t)max((int32_t)vm.x, a.qmax[0]); vm.y = (uint32_t)max((int32_t)vm.y, a.qmax[1]);
        vm.z = (uint32_t)max((int32_t)vm.z, a.qmax[2]); vm.w = (uint32_t)max((int32_t)vm.w, a.qmax[3]);
        // two's complement: the unsigned 64-bit add of a signed partial is the signed add
        s0.x += (unsigned long long)a.sum[0]; s0.y += (unsigned long long)a.sum[1];
        s1.x += (unsigned long long)a.sum[2]; s1.y += (unsigned long long)a.sum[3];
        q0.x += a.sq[0]; q0.y += a.sq[1]; q1.x += a.sq[2]; q1.y += a.sq[3];
        *pc = vc; *pa = va; *pm = vm;
        ps[0] = s0; ps[1] = s1;
        pq[0] = q0; pq[1] = q1;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          cnt[o + i] += (int32_t)a.cnt[i];
          above[o + i] += (int32_t)a.above[i];
          qmax[o + i] = max(qmax[o + i], a.qmax[i]);
          sum[o + i] += a.sum[i];
          sq[o + i] += a.sq[i];
        }
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
        cnt[o] += (int32_t)a.cnt[0];
        above[o] += (int32_t)a.above[0];
        qmax[o] = max(qmax[o], a.qmax[0]);
        sum[o] += a.sum[0];
        sq[o] += a.sq[0];
      }
    }
  }
}

void launch_powder(const FramePtrs& fp, int nframes, int64_t n, float vmin, float vmax, int frac_bits,
                   float thr_above, int nc, uint64_t keys, int key_min, uint64_t nfr, uint64_t cnt, uint64_t sum,
                   uint64_t sq, uint64_t qmax, uint64_t above, uint64_t stream) {
  check(nframes >= 1 && nframes <= kMaxFrames, "powder: nframes out of range");
  check(n >= 1 && n < (int64_t)1 << 31, "powder: frame size out of range");
  check(std::isfinite(vmin) && std::isfinite(vmax) && vmin <= vmax, "powder: the value window must be finite and ordered");
  check(frac_bits >= 0 && frac_bits <= 16, "powder: frac_bits outside [0, 16]");
  check(thr_above == thr_above, "powder: thr_above is NaN");
  // Q = ceil(max(|vmin|, |vmax|) * 2^S) in doubles: a float32 times 2^16 is exact
  const double Q = std::ceil(std::ldexp(std::max(std::fabs((double)vmin), std::fabs((double)vmax)), frac_bits));
  check(Q < 2147483648.0, "powder: max(|vmin|, |vmax|) * 2^frac_bits must stay below 2^31");
  const unsigned __int128 q2 = (unsigned __int128)(uint64_t)Q * (uint64_t)Q;
  check(q2 * (unsigned)nframes <= (unsigned __int128)INT64_MAX, "powder: more frames than (2^63 - 1) / Q^2");
  check(nc == 1 || nc == 2, "powder: 1 or 2 classes");
  check((nc == 2) == (keys != 0), "powder: keys are given iff there are 2 classes");
  check(keys % 4 == 0, "powder: keys must be 4-B aligned");
  check(nfr != 0 && nfr % 8 == 0, "powder: nfr must be non-null and 8-B aligned");
  check(cnt != 0 && sum != 0 && sq != 0 && qmax != 0 && above != 0 && aligned16(cnt) && aligned16(sum) &&
            aligned16(sq) && aligned16(qmax) && aligned16(above),
        "powder: accumulators must be non-null and 16-B aligned");
  for (int f = 0; f < nframes; ++f) check(fp.in[f] != 0 && aligned16(fp.in[f]), "powder: frames must be 16-B aligned");
  const int64_t lanes = n / 4 + (n % 4 != 0 ? 1 : 0);
  const dim3 grid((unsigned)((lanes + 255) / 256));
  const PowParams pp{vmin, vmax, std::ldexp(1.0f, frac_bits), thr_above};
  hipLaunchKernelGGL(powder_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), fp, nframes, n, pp,
                     reinterpret_cast<const int*>(keys), key_min, reinterpret_cast<long long*>(nfr),
                     reinterpret_cast<int32_t*>(cnt), reinterpret_cast<long long*>(sum),
                     reinterpret_cast<unsigned long long*>(sq), reinterpret_cast<int32_t*>(qmax),
                     reinterpret_cast<int32_t*>(above));
  hip_check(hipGetLastError(), "powder launch");
}

}  // namespace pr
