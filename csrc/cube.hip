// K-15 cube for queue consumers: per-pixel count / sum / sum of squares of the CALIBRATED float32 value
// over a batch of frames, ADDED to one of B accumulator planes chosen PER FRAME by a host-side bin
// (photon energy, delay bin, laser on / off, scan step).
//
// Numerics contract (docs/ARCHITECTURE.md, "Cube: the integer contract"): K-11's, per bin.  Every word
// is an INTEGER function of the inputs, so the result does not depend on frame order, batch split or
// stream, is word-for-word equal to the golden model (ops/reference.py cube_accumulate_reference) and
// two consumers' accumulators merge to exactly what one would have produced.
//   bin           bins[f] in -1 .. B - 1, a HOST array; -1 = the frame is dropped: not read, adds nothing
//   contributes   vmin <= v && v <= vmax as float32 (NaN fails, +-inf is outside the finite window)
//   q             (int) rintf(v * 2^S): the multiply is exact, ties go to even (K-08's rounding)
//   cnt[b, p] += 1 (int32)      sum[b, p] += q (int64, signed)      sq[b, p] += q * q (int64)
//   nfr[b] += frames of bin b in the launch (int64, one add by one owner thread)
// A bin without a frame in the launch is neither read nor written, nfr[b] included; a launch whose
// frames are all dropped launches nothing.  The callers hold Q = ceil(max(|vmin|, |vmax|) * 2^S) below
// 2^31 and a run at or below min(2^31 - 1, (2^63 - 1) / Q^2) frames, so no word overflows.  The kernel
// never clears anything.
//
// MI355X design: the owner-lane accumulator of accum.h over 16-B float32 loads, one plane per bin, fed
// by a PLAN the launcher makes on the host and passes BY VALUE in the kernel arguments (CubePlan, about
// 1 KB): the kept frames' addresses sorted into GROUPS of equal bin (the groups in the order their bins
// first appear, a group's frames in batch order), the end of every group and its bin.  The sorted
// addresses ARE the frame order: the kernel needs no index of a frame.  All control flow over groups is
// scalar; addresses, ends and bins come by scalar loads.  Per group: one pass over its frames, ONE set
// of partials in registers, then the read-modify-write of the lane's words of plane b.
//
// Single-frame groups (a delay scan with jitter puts nearly every frame of a batch into another bin, G
// close to F) were ALSO built four -- and two -- at a time, the frame loads and the twenty accumulator
// loads of four distinct planes all issued before the first add, with the accumulator loads of the
// larger groups issued ahead of their frame loads.  That took 138 VGPRs (3 waves per SIMD) and was not
// faster anywhere: at G = 64 on epix10k2M 19.38 us / frame four at a time, 19.19 two at a time, 19.30 one
// by one (this loop) in alternating rounds of one process, on jungfrau05M (512 workgroups) 4.60 / 4.53 /
// 4.50.  With 5 waves per SIMD and a grid of thousands of waves the other waves cover a lone load's
// latency: the launch is bound by the bytes it moves.  Retired; the rows are in profiles/cube/.
//
// Bytes per launch: 4 n F_kept of frames plus 2 * 20 n G of accumulators -- 1.16 x the read floor with
// G = 1 at 64 frames, 11 x with G = 64, which is inherent to the product.  Measured on 64 epix10k2M
// frames, nbins = 64, two runs (profiles/cube/README.md): G = 1 1.75-1.80 us / frame, 0.96-0.97 x
// powder(NC=1) of the same run and 1.00-1.06 x the read floor; G = 2 1.85-1.89 (1.05-1.06 x G = 1 for
// 1.135 x its bytes); G = 8 3.15-3.45 (1.80-1.91 x for 1.946 x); G = 64 17.31-17.33 (9.60-9.89 x for
// 9.514 x: 5.5 TB/s, 87 % of the streaming roof, while the one 43-MB plane of G = 1 may sit partly in the
// Infinity Cache of the replayed benchmark).
//
// In-batch partial widths, from the 64-frame bound: cnt <= 64 (32-bit); |sum| <= 64 * Q < 2^37 (64-bit);
// sq <= 64 * Q^2, which the run bound keeps below 2^63 for any accepted Q (64-bit, the product q * q of
// two int32 is one v_mad_i64_i32).
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
// cube_kernel: 94 VGPRs, 106 SGPRs, no scratch memory (0 bytes per lane, no VGPR spills; 22 scalar
// registers parked in vector-register lanes), no LDS, occupancy 5 waves per SIMD.  The frame addresses
// come by s_load_dwordx2, the frames by global_load_dwordx4 nt, no flat access.
#include "accum.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

struct CubeParams {
  float vmin, vmax, scale;   // scale = 2^S
};

// the launch plan, by value in the kernel arguments: group g owns frame[gend[g - 1] .. gend[g]) (from 0
// for g == 0) and adds into plane gbin[g]
struct CubePlan {
  uint64_t frame[kMaxFrames];
  int32_t gend[kMaxFrames];
  int32_t gbin[kMaxFrames];
  int32_t ngroups;
};

// in-batch partials of NP pixels of ONE group; every index is a compile-time constant after
// unrolling, so the arrays live in VGPRs
template <int NP>
struct CubePart {
  uint32_t cnt[NP];
  long long sum[NP];
  unsigned long long sq[NP];
};

template <int NP>
__device__ __forceinline__ void cube_zero(CubePart<NP>& a) {
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    a.cnt[i] = 0u;
    a.sum[i] = 0ll;
    a.sq[i] = 0ull;
  }
}

// one sample into pixel slot I
template <int NP, int I>
__device__ __forceinline__ void cube_add(CubePart<NP>& a, const float v, const CubeParams& pp) {
  const bool ok = v >= pp.vmin && v <= pp.vmax;
  const int q = ok ? (int)rintf(v * pp.scale) : 0;   // |q| <= Q < 2^31
  a.cnt[I] += ok ? 1u : 0u;
  a.sum[I] += (long long)q;
  a.sq[I] += (unsigned long long)((long long)q * (long long)q);
}

__device__ __forceinline__ void cube_add4(CubePart<4>& a, const f32x4_t r, const CubeParams& pp) {
  cube_add<4, 0>(a, r.x, pp);
  cube_add<4, 1>(a, r.y, pp);
  cube_add<4, 2>(a, r.z, pp);
  cube_add<4, 3>(a, r.w, pp);
}

__global__ __launch_bounds__(256) void cube_kernel(const CubePlan pl, const int64_t n, const CubeParams pp,
                                                   long long* __restrict__ nfr, int32_t* __restrict__ cnt,
                                                   long long* __restrict__ sum,
                                                   unsigned long long* __restrict__ sq) {
  const int G = pl.ngroups;
  const int64_t nq = n >> 2;
  const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (q == 0) {   // the owner of nfr (lane 0 exists for every n >= 1: the tail lane when n < 4)
    int f = 0;
    for (int g = 0; g < G; ++g) {
      nfr[pl.gbin[g]] += (long long)(pl.gend[g] - f);
      f = pl.gend[g];
    }
  }
  if (q < nq) {
    const int64_t p0 = q * 4;
    const bool vec = (n & 3) == 0;   // plane b starts at b * n: 16-B aligned for every b iff n % 4 == 0
    int f = 0;
    for (int g = 0; g < G; ++g) {   // scalar: every lane of the grid walks the same plan
      const int b = pl.gbin[g];
      CubePart<4> a;
      cube_zero(a);
      acc_group<f32x4_t, true>(pl.gend[g] - f, q, [&] { return pl.frame[f++]; },
                               [&](const f32x4_t r) { cube_add4(a, r, pp); });
      const int64_t o = (int64_t)b * n + p0;
      if (vec || b == 0) {
        Words32 wc;
        Words64 ws, wq;
        wc.load(cnt + o); ws.load(sum + o); wq.load(sq + o);
        wc.add(a.cnt); ws.add(a.sum); wq.add(a.sq);
        wc.store(cnt + o); ws.store(sum + o); wq.store(sq + o);
      } else {
        acc_add(cnt + o, a.cnt); acc_add(sum + o, a.sum); acc_add(sq + o, a.sq);
      }
    }
  } else if (q == nq) {
    // scalar tail: the frame's last n % 4 pixels (the launcher adds this lane only when there are any)
    for (int64_t p = nq * 4; p < n; ++p) {
      int f = 0;
      for (int g = 0; g < G; ++g) {
        CubePart<1> a;
        cube_zero(a);
        const int end = pl.gend[g];
        for (; f < end; ++f) cube_add<1, 0>(a, gin<float>(pl.frame[f])[p], pp);
        const int64_t o = (int64_t)pl.gbin[g] * n + p;
        acc_add(cnt + o, a.cnt); acc_add(sum + o, a.sum); acc_add(sq + o, a.sq);
      }
    }
  }
}

void launch_cube(const FramePtrs& fp, int nframes, int64_t n, float vmin, float vmax, int frac_bits, int nbins,
                 const int32_t* bins, uint64_t nfr, uint64_t cnt, uint64_t sum, uint64_t sq, uint64_t stream) {
  check_nframes(nframes, "cube");
  check_frame_size(n, "cube");
  const CubeParams pp{vmin, vmax, quant_bound(vmin, vmax, frac_bits, nframes, "cube")};
  check(nbins >= 1 && nbins <= kCubeMaxBins, "cube: nbins outside [1, 4096]");
  check(bins != nullptr, "cube: no bins");
  check(nfr != 0 && nfr % 8 == 0, "cube: nfr must be non-null and 8-B aligned");
  check(cnt != 0 && sum != 0 && sq != 0 && aligned16(cnt) && aligned16(sum) && aligned16(sq),
        "cube: accumulators must be non-null and 16-B aligned");
  for (int f = 0; f < nframes; ++f) {
    check_frame(fp.in[f], "cube");
    check(bins[f] >= -1 && bins[f] < nbins, "cube: a frame's bin is outside -1 .. nbins - 1");
  }
  // the plan: the groups in the order their bins first appear, a group's frames in batch order (stable)
  CubePlan pl{};
  int k = 0;
  for (int f = 0; f < nframes; ++f) {
    const int b = bins[f];
    if (b < 0) continue;   // dropped: never read
    bool seen = false;
    for (int g = 0; g < pl.ngroups; ++g) seen = seen || pl.gbin[g] == b;
    if (seen) continue;
    for (int e = f; e < nframes; ++e)
      if (bins[e] == b) pl.frame[k++] = fp.in[e];
    pl.gbin[pl.ngroups] = b;
    pl.gend[pl.ngroups] = k;
    ++pl.ngroups;
  }
  if (pl.ngroups == 0) return;   // every frame dropped: nothing is launched, nothing is written
  hipLaunchKernelGGL(cube_kernel, owner_lane_grid(n), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), pl, n, pp,
                     reinterpret_cast<long long*>(nfr), reinterpret_cast<int32_t*>(cnt),
                     reinterpret_cast<long long*>(sum), reinterpret_cast<unsigned long long*>(sq));
  hip_check(hipGetLastError(), "cube launch");
}

}  // namespace pr
