// K-08 on-GPU azimuthal integration for queue consumers: the radial profile I(r) / I(q) of every
// frame of a batch, and a per-run accumulator, from a static uint16 bin map.
//
// Numerics contract (docs/ARCHITECTURE.md, "Radial profile"): everything is accumulated in
// INTEGERS, so the result does not depend on the order of the adds (float atomics are not
// reproducible run to run), is bitwise equal to the golden model (ops/reference.py
// radial_profile_reference) and two consumers' accumulators add to exactly what one would produce.
//   contributes   bins[i] != 0xFFFF and vmin <= v <= vmax (NaN fails both, +-inf is outside)
//   q             (int64) rintf(v * 2^S)         the multiply is exact, rounding is half-to-even
//   sum[f, b]     int64 sum of q; count[f, b] int32 number of contributing pixels
//   profile[f, b] float32(double(sum) * 2^-S / double(count)), +0 where count == 0
// The host wrapper enforces max(|vmin|, |vmax|) * 2^S * n < 2^53 before any launch, so no partial
// or total sum leaves the int64 range (or the exactly-convertible double range); every accumulator
// here is 64-bit, none is narrower.
//
// MI355X design: the frames are streamed ONCE with 16-B non-temporal loads (4 float4 per lane per
// 16-KB chunk, the next chunk in flight while this one is binned), the bin map with plain 8-B
// loads (2 B per pixel, shared by every frame of the batch, so it stays in L2).  A workgroup owns
// a contiguous range of the batch's (frame, chunk) sequence -- one resident wave of workgroups,
// like the peak finder -- and keeps a PRIVATE LDS histogram (64-bit sums, 32-bit counts) that it
// merges into the global [F, nbins] arrays at each frame boundary: touched bins only, integer
// __hip_atomic_fetch_add (relaxed, agent scope), 64 contiguous bins per wave-instruction.  A
// short second kernel writes the profiles and adds the batch into the run accumulator.
//
// Contention: adjacent pixels of a panel row often share a bin, so a wave's lanes collide on a few
// LDS words, and same-address LDS atomics serialise.  Remedy that ships: REPLICATED histograms --
// lane l adds into copy l & (copies - 1), the copies of a bin in adjacent words (distinct banks),
// copies = the largest power of two <= 16 that keeps the histogram within 24 KiB (so the LDS does
// not cut the occupancy; nbins > 2048 run one copy of up to 48 KiB).
//
// Measured on the MI355X (profiles/radial/README.md): epix10k2M calib frames, 64-frame batch,
// us/frame, medians of interleaved rounds in one process.  Two runs: the three remedies (replication
// under a 48-KiB budget then), and a sweep of the replication budget; the shipped 24-KiB form is a
// column of the second.  read_f32 floor 1.77 / 1.82, peakfind 1.70 / 1.71 in those runs.
//   bin map               one copy      replicated 48 KiB   replicated 24 KiB (ships)   wave combine
//   one bin (worst)       14.45 / 14.44  2.03 / 2.03         1.86 (16 copies)            3.33
//   geometry,   64 bins    6.53 /  6.53  2.07 / 2.01         1.90 (16 copies)            3.67
//   geometry,  256 bins    2.92          2.15                1.76 ( 8 copies)
//   geometry,  512 bins    2.05          2.11                1.84 ( 4 copies)
//   geometry, 1024 bins    1.96 /  1.99  2.18 / 2.23         1.87 ( 2 copies)            3.07
//   geometry, 2048 bins    1.79          2.11                1.80 ( 1 copy)
//   geometry, 4096 bins    2.23 /  2.25  2.21 / 2.23         2.21 ( 1 copy)              3.10
// Replication is what keeps few-bin maps at the streaming rate (256 bins and below: 1.2x to 8x);
// from 1024 bins up it is a wash -- bins are about a pixel wide there, a wave's lanes rarely share
// one, and a run of one and the same single-copy configuration read 1.87 against 1.99 depending on
// where in the round it ran, which is the noise of these numbers.  A 48-KiB budget (3 workgroups per
// CU) costs 0.2-0.4 wherever it is used.  bench/kernels.py --only radial on the shipped tree, 1024
// bins: radial 1.98, read_f32 1.78 (ratio 1.11), peakfind 1.67.
// "wave combine" (retired): the four pixels of a lane's float4 merged in registers, then runs of
// neighbouring lanes with one and the same bin summed by a segmented wave-shuffle scan, one lane per
// run adding -- exact and contention-free, but its ~25 extra VALU / shuffle instructions per float4
// cost more than the collisions it removes (about 1.1 us/frame slower even where nothing collides).
#include "common.h"
#include "kernels.h"
#include "launch.h"

#include <cmath>

#include <algorithm>

namespace pr {

typedef unsigned short u16x4_t __attribute__((ext_vector_type(4)));

constexpr int kRadK = 4;                 // float4 per lane per chunk (16 KB of frame per chunk)
constexpr int kRadLdsBytes = 24 * 1024;  // LDS budget of the REPLICATED histogram (one copy may take 48 KiB)
constexpr int kRadMaxCopies = 16;
constexpr unsigned kRadExcluded = 0xFFFFu;

struct RadParams {
  float vmin, vmax, scale;   // scale = 2^S
  int nbins;
  int copies;                // LDS histogram copies (power of two), copy = lane & (copies - 1)
  int64_t n;                 // elements per frame
  uint64_t bins;             // uint16 [n] bin map (0xFFFF = excluded)
};

// LDS layout: int64 sums[nbins * copies], then int32 counts[nbins * copies]; entry bin * copies +
// copy, so the lanes of a wave that share a bin hit `copies` ADJACENT words (distinct banks).
struct RadHist {
  unsigned long long* sums;
  unsigned int* counts;
};

__device__ __forceinline__ void rad_add(const RadHist& h, int slot, long long q, unsigned int c) {
  __hip_atomic_fetch_add(h.sums + slot, (unsigned long long)q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  __hip_atomic_fetch_add(h.counts + slot, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one pixel: does it contribute, and with which quantised value
__device__ __forceinline__ bool rad_quant(float v, unsigned b, const RadParams& rp, long long& q) {
  const bool ok = b < (unsigned)rp.nbins && v >= rp.vmin && v <= rp.vmax;   // 0xFFFF >= nbins
  q = ok ? (long long)rintf(v * rp.scale) : 0ll;
  return ok;
}

// the four pixels of one float4: one LDS add pair per contributing pixel, into this lane's copy
__device__ __forceinline__ void rad_bin4(const RadHist& h, const f32x4_t v, const u16x4_t b, const RadParams& rp,
                                         int copy) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    long long q;
    if (rad_quant(v[e], b[e], rp, q)) rad_add(h, (int)b[e] * rp.copies + copy, q, 1u);
  }
}

__global__ __launch_bounds__(256) void radial_kernel(const FramePtrs fp, const RadParams rp,
                                                     unsigned long long* __restrict__ sums,
                                                     unsigned int* __restrict__ counts, const int nframes) {
  extern __shared__ unsigned long long rad_lds[];
  constexpr int K = kRadK;
  const int copies = rp.copies;
  const int nslots = rp.nbins * copies;
  RadHist h{rad_lds, reinterpret_cast<unsigned int*>(rad_lds + nslots)};
  const int64_t n4 = rp.n / 4;
  const int ncpf = n4 > 0 ? (int)((n4 + 256 * K - 1) / (256 * K)) : 1;   // a frame of < 4 elements is all tail
  const int64_t T = (int64_t)ncpf * nframes;
  const int64_t g0 = T * blockIdx.x / gridDim.x, g1 = T * (blockIdx.x + 1) / gridDim.x;
  const int copy = (threadIdx.x & 63) & (copies - 1);
  const PR_GLOBAL unsigned short* bins = gin<unsigned short>(rp.bins);
  for (int i = threadIdx.x; i < nslots; i += 256) {
    h.sums[i] = 0ull;
    h.counts[i] = 0u;
  }
  __syncthreads();
  // chunk g: K float4 of the frame and the K x 4 bin entries of the same elements; a float4 past
  // the frame's last whole one gets excluded bins (nothing is loaded)
  auto load_to = [&](f32x4_t(&v)[K], u16x4_t(&b)[K], int64_t g) {
    const int f = (int)(g / ncpf);
    const int64_t c0 = (g - (int64_t)f * ncpf) * 256 * K;   // first float4 of the chunk (uniform)
    const PR_GLOBAL f32x4_t* cp = reinterpret_cast<const PR_GLOBAL f32x4_t*>(gin<float>(fp.in[f])) + c0;
    const PR_GLOBAL u16x4_t* bp = reinterpret_cast<const PR_GLOBAL u16x4_t*>(bins) + c0;
    const uint32_t t = threadIdx.x;
    const u16x4_t none = {(unsigned short)kRadExcluded, (unsigned short)kRadExcluded, (unsigned short)kRadExcluded,
                          (unsigned short)kRadExcluded};
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool in = c0 + t + 256 * k < n4;
      v[k] = in ? ld_nt_f4(cp + t + 256 * k) : f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
      b[k] = in ? bp[t + 256 * k] : none;
    }
  };
  // merge the touched bins of this workgroup's histogram into frame f's global rows and clear them
  auto flush = [&](int f) {
    __syncthreads();
    for (int bin = threadIdx.x; bin < rp.nbins; bin += 256) {
      unsigned long long s = 0ull;
      unsigned int c = 0u;
      for (int r = 0; r < copies; ++r) {
        const int slot = bin * copies + r;
        const unsigned int cr = h.counts[slot];
        if (cr != 0u) {
          s += h.sums[slot];
          c += cr;
          h.sums[slot] = 0ull;
          h.counts[slot] = 0u;
        }
      }
      if (c != 0u) {
        const int64_t o = (int64_t)f * rp.nbins + bin;
        __hip_atomic_fetch_add(sums + o, s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_add(counts + o, c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    __syncthreads();
  };
  int fcur = (int)(g0 / ncpf);
  auto chunk = [&](f32x4_t(&v)[K], u16x4_t(&b)[K], int64_t g) {
    const int f = (int)(g / ncpf);   // workgroup-uniform
    if (f != fcur) {
      flush(fcur);
      fcur = f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) rad_bin4(h, v[k], b[k], rp, copy);
    // scalar tail: the frame's last n % 4 elements, by the workgroup that owns its last chunk
    if (g - (int64_t)f * ncpf == ncpf - 1) {
      const int64_t i = 4 * n4 + threadIdx.x;
      if (i < rp.n) {
        long long q;
        const unsigned bb = bins[i];
        if (rad_quant(gin<float>(fp.in[f])[i], bb, rp, q)) rad_add(h, (int)bb * copies + copy, q, 1u);
      }
    }
  };
  f32x4_t va[K], vb[K];
  u16x4_t ba[K], bb[K];
  if (g0 < g1) load_to(va, ba, g0);
  for (int64_t g = g0; g < g1; g += 2) {
    if (g + 1 < g1) load_to(vb, bb, g + 1);
    chunk(va, ba, g);
    if (g + 1 < g1) {
      if (g + 2 < g1) load_to(va, ba, g + 2);
      chunk(vb, bb, g + 1);
    }
  }
  if (g0 < g1) flush(fcur);
}

// profiles of the batch and its sum into the run accumulator: run = int64 [2 * nbins + 1]
// (run_sum, run_count, frames).  Block (x, y): 256 bins x kRadFinFrames frames; one integer atomic
// pair per (bin, block) -- two consumer streams may finalize at the same time.
constexpr int kRadFinFrames = 8;
__global__ __launch_bounds__(256) void radial_finalize_kernel(const unsigned long long* __restrict__ sums,
                                                              const unsigned int* __restrict__ counts,
                                                              float* __restrict__ profile,
                                                              unsigned long long* __restrict__ run, const int nbins,
                                                              const int nframes, const double inv_scale) {
  const int bin = blockIdx.x * 256 + threadIdx.x;
  const int f0 = blockIdx.y * kRadFinFrames, f1 = min(nframes, f0 + kRadFinFrames);
  if (run != nullptr && bin == 0 && blockIdx.y == 0)
    __hip_atomic_fetch_add(run + 2 * nbins, (unsigned long long)nframes, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (bin >= nbins) return;
  unsigned long long ts = 0ull, tc = 0ull;
  for (int f = f0; f < f1; ++f) {
    const int64_t o = (int64_t)f * nbins + bin;
    const long long s = (long long)sums[o];
    const unsigned int c = counts[o];
    profile[o] = c != 0u ? (float)((double)s * inv_scale / (double)c) : 0.0f;
    ts += (unsigned long long)s;
    tc += c;
  }
  if (run != nullptr && tc != 0ull) {
    __hip_atomic_fetch_add(run + bin, ts, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(run + nbins + bin, tc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

void launch_radial(const FramePtrs& fp, int nframes, int64_t n, uint64_t bins, int nbins, float vmin, float vmax,
                   int frac_bits, uint64_t sums, uint64_t counts, uint64_t profile, uint64_t run, uint64_t stream) {
  check_nframes(nframes, "radial");
  check_frame_size(n, "radial");
  check(nbins >= 1 && nbins <= kRadMaxBins, "radial: nbins must be in [1, 4096]");
  check(frac_bits >= 0 && frac_bits <= 60, "radial: frac_bits out of range");
  check(vmin <= vmax, "radial: empty value window");
  // the int64 -> double conversion of every sum stays exact (and no int64 sum can wrap)
  check(std::ldexp(std::max(std::fabs((double)vmin), std::fabs((double)vmax)), frac_bits) * (double)n <
            9007199254740992.0,
        "radial: max(|vmin|, |vmax|) * 2^frac_bits * n must stay below 2^53");
  check(bins != 0 && bins % 8 == 0, "radial: the bin map must be 8-B aligned");
  check(sums % 8 == 0 && counts % 4 == 0 && profile % 4 == 0 && run % 8 == 0 && sums != 0 && counts != 0 &&
            profile != 0,
        "radial: misaligned or missing output");
  check_frames(fp, nframes, "radial");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RadParams rp{vmin, vmax, std::ldexp(1.0f, frac_bits), nbins, 1, n, bins};
  while (rp.copies < kRadMaxCopies && 2 * rp.copies * nbins * 12 <= kRadLdsBytes) rp.copies *= 2;
  const int lds = rp.copies * nbins * 12;
  const int64_t n4 = n / 4;
  const int64_t chunks = std::max<int64_t>(1, (n4 + 256 * kRadK - 1) / (256 * kRadK)) * nframes;
  auto kern = radial_kernel;
  const int g = (int)std::min<int64_t>(chunks, resident_blocks((const void*)kern, lds, "radial"));
  unsigned long long* S = reinterpret_cast<unsigned long long*>(sums);
  unsigned int* C = reinterpret_cast<unsigned int*>(counts);
  hip_check(hipMemsetAsync(S, 0, (size_t)nframes * nbins * 8, s), "radial clear sums");
  hip_check(hipMemsetAsync(C, 0, (size_t)nframes * nbins * 4, s), "radial clear counts");
  hipLaunchKernelGGL(kern, dim3(g), dim3(256), (size_t)lds, s, fp, rp, S, C, nframes);
  hip_check(hipGetLastError(), "radial launch");
  const dim3 fg((nbins + 255) / 256, (nframes + kRadFinFrames - 1) / kRadFinFrames);
  hipLaunchKernelGGL(radial_finalize_kernel, fg, dim3(256), 0, s, S, C, reinterpret_cast<float*>(profile),
                     reinterpret_cast<unsigned long long*>(run), nbins, nframes, std::ldexp(1.0, -frac_bits));
  hip_check(hipGetLastError(), "radial finalize launch");
}

}  // namespace pr
