// K-13 photon counting for queue consumers: the number of photons per pixel of CALIBRATED float32 frames
// (psana's det.photons: whole photons by floor, then the fractional remainders of neighbouring pixel
// pairs merged), as a per-frame map, per-pixel run accumulators and per-frame, per-ROI P(k) counts.
//
// Numerics contract (docs/ARCHITECTURE.md, "Photon counting: the integer contract"): every word is a
// function of the inputs alone and equals the golden model (ops/reference.py photon_count_reference).
//   ok      (no mask or mask[p] != 0) && v > 0 && v <= vmax as float32 (NaN fails, +inf is outside)
//   x       ok ? v * inv : 0, ONE float32 multiply (never contracted: -ffp-contract=off)
//   w, r    w = (int) floorf(x) <= 254, r = x - (float) w (exact)
//   seed    r >= thr_seed, and for every 4-connected neighbour q of the SAME panel
//           r_p > r_q || (r_p == r_q && p < q); a missing or masked neighbour reads as r = 0
//   k       w + (seed && r + rmax >= thr_total), rmax = the largest neighbour r, the add in float32
//   cnt[p] += ok (int32)    psum[p] += k (int64)    occ[p] += (k >= 1) (int32): ADDED, never cleared
//   pk[f, roi, min(k, 8) - 1] += 1 and tot[f, roi] += k for k >= 1 and a label < R (cleared by the launcher)
//   kmap[f, p] = k (uint8), only when asked for
//
// MI355X design (register-only stencil): a lane owns NP = 4 consecutive pixels of a row (NP = 1 when
// W % 4 != 0) for the whole launch, so the run accumulators need no atomics: the in-launch partials are
// 32-bit registers (64 * 255 fits) and there is ONE 16-B read-modify-write of the lane's words after
// the frame loop.  Per frame the lane loads its own quad (16-B non-temporal), the quads of the rows
// above and below and the two pixels beside it; the four extra loads hit lines that this or a
// neighbouring wave fetches at the same time, so HBM sees a frame byte about once.  Which neighbours
// exist (row, column and panel edges) and which pixels the mask keeps is the same for every frame: it
// is folded ONCE per launch into the upper bound each of the lane's 3 * NP + 2 values is compared with
// (vmax, or -1 for "never ok"), and the address of a missing neighbour is redirected to the lane's own
// quad, so the frame loop has neither branches nor out-of-range addresses.  Four frames' loads (20 per
// lane) are in flight at a time.
//
// pk / tot: pixels with k >= 1 are rare, so they count into LDS words [F][R][8 bins + total] (at most
// 18 KiB; 8 / R copies of them where that fits, lane by lane, for frames where they are NOT rare) with
// ds_add_u32; a workgroup owns several pixel blocks (the grid is at most kPhotGrid
// workgroups, blocks dealt round-robin so that neighbouring blocks run at the same time, XCD by XCD),
// and at its end adds only the non-zero words to global memory with relaxed agent-scope integer
// atomics (64-bit for tot).  A workgroup owns at most 2^21 pixels, so its 32-bit totals hold 255 each.
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
// photons_kernel<4, 4> (W % 4 == 0, 4 frames in flight): 141 VGPRs, 106 SGPRs, no scratch memory (0 bytes per
// lane, no spills), 18432 B LDS, occupancy 3 waves per SIMD; photons_kernel<1, 4> (the scalar path): 72
// VGPRs, 91 SGPRs, no scratch, 18432 B LDS, occupancy 7; photons_kernel<4, 2> (measurements only, 2 frames
// in flight): 103 VGPRs, no scratch, occupancy 4 -- and 2-3 % slower.
//
// What bounds it (profiles/photons/README.md): the vector ALU, not memory.  A lane computes the remainder
// of 14 values for its 4 pixels (3.5 per pixel), and the seed / merge / accumulate step is about 14
// instructions per pixel: a counter run of the first version gave 188 vector instructions per wave and
// frame (about 150 in this one, counted in the ISA), which keeps the SIMDs busy for most of the kernel's
// time at 2.75 waves per SIMD, so the kernel runs at about 1.9-2.0 x the read floor for 1.125 x its bytes.  The LDS row-block shape (each remainder computed once,
// neighbours read from LDS) would remove up to a third of those instructions; it has not been built.
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

constexpr int kPhotThreads = 256;
constexpr int kPhotGrid = 1024;    // workgroups at most: each merges its LDS counters once
constexpr int kPhotCell = 9;       // LDS words per (frame, ROI): 8 bins and the total

struct PhotParams {
  float inv, vmax, thr_seed, thr_total;
};

// what a lane knows about its NP pixels for the whole launch
template <int NP>
struct PhotLane {
  int64_t own, up, down, left, right;   // element offsets into a frame (always inside it)
  // the upper bound of "ok" per value the lane reads: vmax where the pixel exists and the mask keeps it, -1
  // otherwise (no v is > 0 and <= -1), so a missing or masked pixel costs the frame loop nothing
  float vo[NP], vu[NP], vd[NP], vl, vr;
  uint32_t lab[NP];                     // ROI label, 255 = none
};

template <int NP>
struct PhotIn {
  float o[NP], u[NP], d[NP], l, r;
};

template <int NP>
__device__ __forceinline__ void phot_load(PhotIn<NP>& in, const uint64_t frame, const PhotLane<NP>& ln) {
  const PR_GLOBAL float* b = gin<float>(frame);
  if constexpr (NP == 4) {
    const f32x4_t o = ld_nt_f4(reinterpret_cast<const PR_GLOBAL f32x4_t*>(b + ln.own));
    const f32x4_t u = *reinterpret_cast<const PR_GLOBAL f32x4_t*>(b + ln.up);
    const f32x4_t d = *reinterpret_cast<const PR_GLOBAL f32x4_t*>(b + ln.down);
    in.o[0] = o.x; in.o[1] = o.y; in.o[2] = o.z; in.o[3] = o.w;
    in.u[0] = u.x; in.u[1] = u.y; in.u[2] = u.z; in.u[3] = u.w;
    in.d[0] = d.x; in.d[1] = d.y; in.d[2] = d.z; in.d[3] = d.w;
  } else {
    in.o[0] = b[ln.own];
    in.u[0] = b[ln.up];
    in.d[0] = b[ln.down];
  }
  in.l = b[ln.left];
  in.r = b[ln.right];
}

// x = ok ? v * inv : 0 of one sample; `&` on purpose: `&&` makes the compiler branch around a compare
__device__ __forceinline__ float phot_x(const float v, const float vm, const float inv, bool& ok) {
  ok = (v > 0.0f) & (v <= vm);
  return ok ? v * inv : 0.0f;
}

// the remainder x - floorf(x) of 0 <= x < 255: v_fract_f32 is exactly that difference
__device__ __forceinline__ float phot_fract(const float x) { return __builtin_amdgcn_fractf(x); }

template <int NP>
struct PhotPart {
  uint32_t cnt[NP], ps[NP], occ[NP];
};

// one frame of the lane's pixels: partials, LDS counters, kmap
template <int NP>
__device__ __forceinline__ void phot_frame(PhotPart<NP>& a, const PhotIn<NP>& in, const PhotLane<NP>& ln,
                                           const PhotParams& pp, uint32_t* cell, const int R,
                                           uint8_t* __restrict__ kout) {
  float ro[NP], ru[NP], rd[NP];
  uint32_t w[NP];
  bool ok[NP], okn;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const float x = phot_x(in.o[i], ln.vo[i], pp.inv, ok[i]);
    w[i] = (uint32_t)(int)x;   // x >= 0: the truncation is floorf
    ro[i] = phot_fract(x);
    ru[i] = phot_fract(phot_x(in.u[i], ln.vu[i], pp.inv, okn));
    rd[i] = phot_fract(phot_x(in.d[i], ln.vd[i], pp.inv, okn));
  }
  const float rl = phot_fract(phot_x(in.l, ln.vl, pp.inv, okn));
  const float rr = phot_fract(phot_x(in.r, ln.vr, pp.inv, okn));
  uint32_t kk[NP], packed = 0u;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const float r = ro[i];
    const float left = i > 0 ? ro[i > 0 ? i - 1 : 0] : rl;
    const float right = i < NP - 1 ? ro[i < NP - 1 ? i + 1 : 0] : rr;
    // up and left have the lower index (they win a tie), right and down the higher one
    // (no r is NaN, so the maxima are plain)
    const float lower = fmaxf(ru[i], left);                            // must be beaten
    const float higher = fmaxf(fmaxf(right, rd[i]), pp.thr_seed);      // must be reached (thr_seed too)
    const bool seed = (r > lower) & (r >= higher);
    const float rmax = fmaxf(fmaxf(right, rd[i]), lower);
    const uint32_t k = w[i] + ((seed & (r + rmax >= pp.thr_total)) ? 1u : 0u);
    a.cnt[i] += ok[i] ? 1u : 0u;
    a.ps[i] += k;
    a.occ[i] += k >= 1u ? 1u : 0u;
    kk[i] = k;
    packed |= k << (8 * i);
  }
  if (packed != 0u) {   // rare: one branch per lane and frame
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (kk[i] >= 1u && ln.lab[i] < (uint32_t)R) {
        uint32_t* c = cell + ln.lab[i] * kPhotCell;
        atomicAdd(c + (min(kk[i], 8u) - 1u), 1u);
        atomicAdd(c + 8, kk[i]);
      }
    }
  }
  if (kout != nullptr) {
    if constexpr (NP == 4) *reinterpret_cast<uint32_t*>(kout + ln.own) = packed;
    else kout[ln.own] = (uint8_t)packed;
  }
}

template <int NP, int K>
__device__ __forceinline__ void phot_group(PhotPart<NP>& a, const FramePtrs& fp, const int f0, const PhotLane<NP>& ln,
                                           const PhotParams& pp, uint32_t* lds, const int R,
                                           uint8_t* __restrict__ kmap, const int64_t n) {
  PhotIn<NP> in[K];
#pragma unroll
  for (int k = 0; k < K; ++k) phot_load<NP>(in[k], fp.in[f0 + k], ln);
#pragma unroll
  for (int k = 0; k < K; ++k)
    phot_frame<NP>(a, in[k], ln, pp, lds + (f0 + k) * R * kPhotCell, R,
                   kmap != nullptr ? kmap + (int64_t)(f0 + k) * n : nullptr);
}

template <int NP, int KF>
__global__ __launch_bounds__(kPhotThreads) void photons_kernel(
    const FramePtrs fp, const int nframes, const uint32_t n, const uint32_t W, const uint32_t H, const PhotParams pp,
    const uint8_t* __restrict__ mask, const uint8_t* __restrict__ roi, const int R, uint8_t* __restrict__ kmap,
    int32_t* __restrict__ cnt, unsigned long long* __restrict__ psum, int32_t* __restrict__ occ,
    int32_t* __restrict__ pk, unsigned long long* __restrict__ tot, const uint32_t nblk) {
  __shared__ uint32_t lds_all[kMaxFrames * 8 * kPhotCell];
  const int nw = nframes * R * kPhotCell;
  // with fewer than 5 ROIs the block holds 8 / R (a power of two) copies of the counters and neighbouring
  // lanes count into different copies: where MANY pixels have photons, all lanes of a wave add to the same
  // few words, and same-address LDS adds are served one after the other
  const int copies = R == 1 ? 8 : R == 2 ? 4 : R <= 4 ? 2 : 1;
  for (int i = threadIdx.x; i < nw * copies; i += kPhotThreads) lds_all[i] = 0u;
  __syncthreads();
  uint32_t* lds = lds_all + (threadIdx.x & (copies - 1)) * nw;
  const uint32_t nl = n / NP;   // lanes with pixels (NP == 4 only when W % 4 == 0, so n % 4 == 0)
  const uint32_t first = (uint32_t)xcd_swizzle((int)blockIdx.x, (int)gridDim.x);
  for (uint32_t b = first; b < nblk; b += gridDim.x) {
    const uint32_t q = b * kPhotThreads + threadIdx.x;
    if (q >= nl) continue;
    const uint32_t p0 = q * NP;
    const uint32_t row = p0 / W, col = p0 - row * W, y = row % H;
    const bool has_up = y > 0u, has_down = y + 1u < H, has_left = col > 0u, has_right = col + NP < W;
    PhotLane<NP> ln;
    ln.own = (int64_t)p0;
    ln.up = has_up ? (int64_t)p0 - W : (int64_t)p0;
    ln.down = has_down ? (int64_t)p0 + W : (int64_t)p0;
    ln.left = has_left ? (int64_t)p0 - 1 : (int64_t)p0;
    ln.right = has_right ? (int64_t)p0 + NP : (int64_t)p0 + (NP - 1);
    const float none = -1.0f;
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      const bool mo = mask == nullptr || mask[ln.own + i] != 0;
      const bool mu = has_up && (mask == nullptr || mask[ln.up + i] != 0);
      const bool md = has_down && (mask == nullptr || mask[ln.down + i] != 0);
      ln.vo[i] = mo ? pp.vmax : none;
      ln.vu[i] = mu ? pp.vmax : none;
      ln.vd[i] = md ? pp.vmax : none;
      ln.lab[i] = roi == nullptr ? 0u : (uint32_t)roi[ln.own + i];
    }
    ln.vl = has_left && (mask == nullptr || mask[ln.left] != 0) ? pp.vmax : none;
    ln.vr = has_right && (mask == nullptr || mask[ln.right] != 0) ? pp.vmax : none;

    PhotPart<NP> a;
#pragma unroll
    for (int i = 0; i < NP; ++i) a.cnt[i] = a.ps[i] = a.occ[i] = 0u;
    int f = 0;
    for (; f + KF <= nframes; f += KF) phot_group<NP, KF>(a, fp, f, ln, pp, lds, R, kmap, (int64_t)n);
    for (; f < nframes; ++f) phot_group<NP, 1>(a, fp, f, ln, pp, lds, R, kmap, (int64_t)n);

    if constexpr (NP == 4) {
      u32x4_t* pc = reinterpret_cast<u32x4_t*>(cnt + p0);
      u32x4_t* po = reinterpret_cast<u32x4_t*>(occ + p0);
      u64x2_t* ps = reinterpret_cast<u64x2_t*>(psum + p0);
      u32x4_t vc = *pc, vo = *po;
      u64x2_t s0 = ps[0], s1 = ps[1];
      vc.x += a.cnt[0]; vc.y += a.cnt[1]; vc.z += a.cnt[2]; vc.w += a.cnt[3];
      vo.x += a.occ[0]; vo.y += a.occ[1]; vo.z += a.occ[2]; vo.w += a.occ[3];
      s0.x += a.ps[0]; s0.y += a.ps[1]; s1.x += a.ps[2]; s1.y += a.ps[3];
      *pc = vc; *po = vo;
      ps[0] = s0; ps[1] = s1;
    } else {
      cnt[p0] += (int32_t)a.cnt[0];
      occ[p0] += (int32_t)a.occ[0];
      psum[p0] += a.ps[0];
    }
  }
  __syncthreads();
  // only the non-zero words go to global memory
  for (int i = threadIdx.x; i < nw; i += kPhotThreads) {
    uint32_t v = 0u;
    for (int c = 0; c < copies; ++c) v += lds_all[c * nw + i];
    if (v == 0u) continue;
    const int c = i / kPhotCell, j = i - c * kPhotCell;   // c = f * R + roi
    if (j < 8) __hip_atomic_fetch_add(pk + c * 8 + j, (int32_t)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else __hip_atomic_fetch_add(tot + c, (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

int photons_lane_pixels(int W) { return W % 4 == 0 ? 4 : 1; }
int photons_block_pixels(int W) { return kPhotThreads * photons_lane_pixels(W); }
int photons_max_grid() { return kPhotGrid; }

void launch_photons(const FramePtrs& fp, int nframes, int P, int H, int W, float inv, float vmax, float thr_seed,
                    float thr_total, uint64_t mask, uint64_t roi, int n_roi, uint64_t kmap, uint64_t cnt,
                    uint64_t psum, uint64_t occ, uint64_t pk, uint64_t tot, uint64_t stream, int variant) {
  check_nframes(nframes, "photons");
  check(P >= 1 && H >= 1 && W >= 1, "photons: the shape must be positive");
  const int64_t n = (int64_t)P * H * W;
  check((int64_t)P * H < ((int64_t)1 << 31) && n < ((int64_t)1 << 31), "photons: frame size out of range");
  check(std::isfinite(inv) && inv > 0.0f, "photons: the scale 1 / adu_per_photon must be finite and positive");
  check(vmax == vmax && std::floor(vmax * inv) <= 254.0f, "photons: floor(vmax / adu_per_photon) must be at most 254");
  check(thr_seed > 0.0f && thr_seed <= thr_total && thr_total < 2.0f, "photons: 0 < thr_seed <= thr_total < 2");
  check(n_roi >= 1 && n_roi <= 8, "photons: 1 to 8 ROIs");
  check(roi != 0 || n_roi == 1, "photons: several ROIs need labels");
  check(aligned16(mask) && aligned16(roi), "photons: mask and labels must be 16-B aligned");
  check(kmap % 4 == 0 || W % 4 != 0, "photons: kmap must be 4-B aligned");   // the quad path stores words
  check(cnt != 0 && psum != 0 && occ != 0 && aligned16(cnt) && aligned16(psum) && aligned16(occ),
        "photons: accumulators must be non-null and 16-B aligned");
  check(pk != 0 && tot != 0 && pk % 4 == 0 && tot % 8 == 0, "photons: pk / tot must be non-null and aligned");
  check_frames(fp, nframes, "photons");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_check(hipMemsetAsync(reinterpret_cast<void*>(pk), 0, (size_t)nframes * n_roi * 8 * 4, st), "photons clear pk");
  hip_check(hipMemsetAsync(reinterpret_cast<void*>(tot), 0, (size_t)nframes * n_roi * 8, st), "photons clear tot");
  const int np = photons_lane_pixels(W);
  const int64_t lanes = n / np;
  const int64_t nblk = (lanes + kPhotThreads - 1) / kPhotThreads;
  check(variant >= 0 && (variant >> 8) <= 1 << 15, "photons: unknown variant");
  const int64_t cap = (variant >> 8) != 0 ? (variant >> 8) : kPhotGrid;   // measurements only
  const int64_t per_wg = (nblk + cap - 1) / cap;   // blocks a workgroup owns
  const dim3 grid((unsigned)((nblk + per_wg - 1) / per_wg));
  const PhotParams pp{inv, vmax, thr_seed, thr_total};
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kPhotThreads), 0, st, fp, nframes, (uint32_t)n, (uint32_t)W, (uint32_t)H, pp,
                       reinterpret_cast<const uint8_t*>(mask), reinterpret_cast<const uint8_t*>(roi), n_roi,
                       reinterpret_cast<uint8_t*>(kmap), reinterpret_cast<int32_t*>(cnt),
                       reinterpret_cast<unsigned long long*>(psum), reinterpret_cast<int32_t*>(occ),
                       reinterpret_cast<int32_t*>(pk), reinterpret_cast<unsigned long long*>(tot), (uint32_t)nblk);
  };
  if (np == 4 && (variant & 1) != 0) go(photons_kernel<4, 2>);   // measurements only: 2 frames in flight
  else if (np == 4) go(photons_kernel<4, 4>);
  else go(photons_kernel<1, 4>);
  hip_check(hipGetLastError(), "photons launch");
}

}  // namespace pr
