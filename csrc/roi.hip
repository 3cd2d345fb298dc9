// K-16 ROI statistics for queue consumers: per frame and rectangle of CALIBRATED float32 frames the pixel
// count, the sum, the first moments in y and x, the maximum with its position, and (when asked for) the
// projections of the rectangle onto its x and y axes.
//
// Numerics contract (docs/ARCHITECTURE.md, "ROI: the integer contract"): every word is an integer function
// of the inputs and equals the golden model (ops/reference.py roi_stats_reference) word for word.
//   ok      (no mask or mask[idx] != 0) && vmin <= v && v <= vmax as float32 (NaN fails, +-inf is outside)
//   q       (int) rintf(v * 2^S): the multiply is exact, ties go to even (K-08's rounding)
//   row     per (frame, rectangle) eight 64-bit words: npix, sum q, sum q * y, sum q * x, key, 0, 0, 0
//           (y, x: row and column inside the panel)
//   key     max over the ok pixels of ((uint32) q ^ 0x80000000) << 32 | (0xFFFFFFFF - idx), idx the pixel's
//           linear index in the frame: the largest q, and among equals the LOWEST index; 0 = no sample
//   proj_x  [f, offx[r] + x - x0] = sum over y of q     proj_y [f, offy[r] + y - y0] = sum over x of q (int64)
// The launcher clears the rows and projection words of its frames on the stream; the kernel only adds
// (integers: the order of arrival does not matter) or, where a word has one owner, stores.
//
// MI355X design: the rectangles are static for a run, so the launcher-side PLAN (RoiPlan) is built once and
// stays on the device: every rectangle cut into strips of roi_strip_rows(width) rows (about 8192 pixels), one
// strip per workgroup, the grid strips x frames.  Only the rectangles are read: the cost follows their area,
// not the detector.  A workgroup of 256 lanes tiles its strip with LPR lanes per row, LPR the power of two that
// covers the row's 16-B quads (at most 256; wider rows take column chunks of 1024 columns), so 256 / LPR rows
// are in flight: a 16-column stripe keeps 64 rows busy.  With W % 4 == 0 a lane loads frame-aligned quads
// (16-B non-temporal) and applies x0 <= x < x1 per element; otherwise it loads single pixels.  No load has a
// predicate: a lane without a pixel reads the strip's first unit, so no branch waits on a load.  While every
// workgroup of the launch is resident at once (up to 2048: small rectangles) the loads of TWO row iterations
// are issued before the first is used, since nothing else hides a strip's chain of dependent loads; beyond
// that the loop takes one iteration at a time (occupancy hides the latency, and fewer registers win).
//   scalars  per lane a 32-bit count, the maximum as (q, lowest index) in 32-bit words, and 64-bit sum q * y;
//            sum q and sum q * x come from the lane's column sums after the rows (no 64-bit multiply per pixel);
//            a shuffle reduction per wave (the key by max), LDS over the four waves, then ONE set of relaxed
//            agent-scope integer atomics per workgroup into the 64-B row: four adds and one 64-bit max (none
//            where the strip has no sample)
//   proj_x   a lane keeps its quad's four column sums over the strip's rows in registers; the lanes of equal
//            column meet in an LDS tile [256 / LPR][4 LPR] and one 64-bit add per column and workgroup goes
//            out, consecutive lanes to consecutive words
//   proj_y   a shuffle reduction over the min(LPR, 64) lanes of a row; where a row is one wave segment and
//            one chunk the word has a single owner and is stored, otherwise added
// No float atomics anywhere.
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage), <pixels per
// lane and load, row iterations in flight>: roi_kernel<4, 2>: 67 VGPRs, 98 SGPRs, no scratch memory (0 bytes per
// lane, no spills), 8352 B LDS, occupancy 7 waves per SIMD; roi_kernel<4, 1>: 50 VGPRs, 96 SGPRs, no scratch,
// 8352 B LDS, occupancy 8; the scalar path roi_kernel<1, 2>: 42 VGPRs, 73 SGPRs, no scratch, 2208 B LDS,
// occupancy 8; roi_kernel<1, 1>: 37 VGPRs, 69 SGPRs, no scratch, 2208 B LDS, occupancy 8.
//
// What it costs (profiles/roi/README.md; 64 epix10k2M frames per batch, two runs): one 64 x 384 stripe with
// proj_x 14.7-14.9 us per batch and one 352 x 16 stripe with proj_y 12.8-12.9 us, against 6.8-7.0 us for the
// smallest launch (one pixel): those two are bound by the launch and by the chain of a strip's dependent loads,
// not by bytes.  All 16 panels as 16 rectangles: 146-147 us, 1.26-1.33 x the read floor of the same run
// (1.21-1.28 x powder with one class); 224-226 us (1.94-2.03 x) with both projections.  In the same process:
// two row iterations in flight are worth 11 % on the stripes (14.9 against 16.6 us, 12.8 against 13.9) and cost
// 12 % on whole panels with projections (253 against 225 us), hence the choice by the grid's size.  Strips of
// 16384 pixels make whole panels 8 % faster and the 64 x 384 stripe 33 % slower; the small rectangles are what
// the kernel is for, so 8192 stays.  A variant that capped LPR at 64 and gave a lane up to four quads of a row
// (eight loads in flight, a row never leaves its wave) was built, measured and retired: 174 VGPRs, 32 KiB of
// LDS, 2 waves per SIMD, 2.5 x the floor on whole panels (14.0 us on the stripe).
#include <cmath>
#include <memory>
#include <vector>

#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

constexpr int kRoiThreads = 256;
constexpr int kRoiStripPixels = 8192;   // pixels of a strip, about: 8 quads per lane
constexpr int kRoiStripRowsMax = 1024;
// Row iterations whose loads are in flight together: 2 while every workgroup of the launch is resident at once
// (nothing else hides a strip's chain of dependent loads), 1 once workgroups queue behind each other (occupancy
// hides it, and the projections run 12 % faster with fewer registers): both measured in one process.
constexpr int kRoiResidentGrid = 2048;  // workgroups: about 8 per CU
constexpr int kRoiStripWords = 8;       // int32 words of a RoiStrip

// one strip of a rectangle, as the kernel reads it (32 B)
struct RoiStrip {
  int32_t r;      // rectangle
  int32_t row0;   // first row, counted over the whole frame: p * H + y
  int32_t ny;     // rows
  int32_t x0, x1;
  int32_t y0;     // first row inside the panel
  int32_t px;     // proj_x word of column x0: offx[r]
  int32_t py;     // proj_y word of the strip's first row: offy[r] + (y - rect y0)
};
static_assert(sizeof(RoiStrip) == kRoiStripWords * 4, "RoiStrip layout");

struct RoiParams {
  float vmin, vmax, scale;   // scale = 2^S
};

__device__ __forceinline__ long long roi_wave_sum(long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
  return v;
}

// what a lane has gathered: 32-bit where a lane's share cannot overflow (a strip is at most 2^31 pixels)
struct RoiAcc {
  uint32_t npix, bi;   // bi: the lowest frame index that attains bq
  int bq;              // the largest q; INT32_MIN = none (|q| <= Q < 2^31, so every sample beats it)
  long long sum, sy, sx;
};

template <int NP, int U>
__global__ __launch_bounds__(kRoiThreads) void roi_kernel(
    const FramePtrs fp, const RoiStrip* __restrict__ strips, const uint32_t W, const uint8_t* __restrict__ mask,
    const RoiParams pp, unsigned long long* __restrict__ rows, const int R, unsigned long long* __restrict__ projx,
    const long long Lx, unsigned long long* __restrict__ projy, const long long Ly) {
  __shared__ long long tile[kRoiThreads * NP];   // proj_x: [256 / LPR][NP * LPR]
  __shared__ unsigned long long red[4 * 5];      // the four waves' scalars
  const RoiStrip s = strips[blockIdx.x];
  const int f = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const PR_GLOBAL float* frame = gin<float>(fp.in[f]);

  // units (quads, or pixels on the scalar path) of a row, the lanes per row and the rows in flight
  const int u0 = s.x0 / NP, nu = (s.x1 + NP - 1) / NP - u0;
  int lg = 0;
  while ((1 << lg) < nu && lg < 8) ++lg;
  const int lpr = 1 << lg, rif = kRoiThreads >> lg;
  const int lr = tid >> lg, lc = tid & (lpr - 1);
  const int iters = (s.ny + rif - 1) / rif;      // the same for every lane: the loops hold shuffles and barriers
  const int nchunks = (nu + lpr - 1) >> lg;
  const int seg = lpr < kWave ? lpr : kWave;     // lanes of one row inside a wave
  const bool own_y = lpr <= kWave && nchunks == 1;
  // an element of the strip that always exists: a lane without a pixel loads from it, so no load has a predicate
  const long long fallback = (long long)s.row0 * W + (long long)u0 * NP;
  unsigned long long* projy_row = projy == nullptr ? nullptr : projy + (long long)f * Ly + s.py;

  RoiAcc a;
  a.npix = 0u; a.bi = 0xFFFFFFFFu; a.bq = INT32_MIN; a.sum = a.sy = a.sx = 0;
  for (int c = 0; c < nchunks; ++c) {
    const int x = (u0 + c * lpr + lc) * NP;       // x + NP - 1 >= x0 always
    const bool colok = x < s.x1;
    long long px[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) px[i] = 0;
    // the loads of U row iterations are issued before the first is used
    for (int it = 0; it < iters; it += U) {
      float v[U][NP];
      uint32_t m[U];
      long long base[U];
      bool rowok[U];
#pragma unroll
      for (int h = 0; h < U; ++h) {
        const int yy = (it + h) * rif + lr;
        rowok[h] = colok & (yy < s.ny);
        base[h] = (long long)(s.row0 + yy) * W;   // < 2^31 where rowok
        const long long idx = rowok[h] ? base[h] + x : fallback;
        if constexpr (NP == 4) {
          const f32x4_t q4 = ld_nt_f4(reinterpret_cast<const PR_GLOBAL f32x4_t*>(frame + idx));
          v[h][0] = q4.x; v[h][1] = q4.y; v[h][2] = q4.z; v[h][3] = q4.w;
          m[h] = mask != nullptr ? *reinterpret_cast<const uint32_t*>(mask + idx) : 0x01010101u;
        } else {
          v[h][0] = frame[idx];
          m[h] = mask != nullptr ? (uint32_t)mask[idx] : 1u;
        }
      }
#pragma unroll
      for (int h = 0; h < U; ++h) {
        const int yy = (it + h) * rif + lr;
        long long rs = 0;
#pragma unroll
        for (int i = 0; i < NP; ++i) {
          const int xi = x + i;
          const bool ok = rowok[h] & (xi >= s.x0) & (xi < s.x1) & (((m[h] >> (8 * i)) & 0xFFu) != 0u) &
                          (v[h][i] >= pp.vmin) & (v[h][i] <= pp.vmax);
          const int q = ok ? (int)rintf(v[h][i] * pp.scale) : 0;   // |q| <= Q < 2^31
          const uint32_t idx = (uint32_t)base[h] + (uint32_t)xi;
          const bool better = ok & ((q > a.bq) | ((q == a.bq) & (idx < a.bi)));
          a.bq = better ? q : a.bq;
          a.bi = better ? idx : a.bi;
          a.npix += ok ? 1u : 0u;
          px[i] += q;
          rs += q;
        }
        a.sy += rs * (long long)(s.y0 + yy);
        if (projy_row != nullptr) {
          for (int d = seg >> 1; d > 0; d >>= 1) rs += __shfl_xor(rs, d);
          if ((lane & (seg - 1)) == 0 && yy < s.ny) {
            unsigned long long* w = projy_row + yy;
            if (own_y) *w = (unsigned long long)rs;   // the launcher's clear has run; nobody else writes it
            else if (rs != 0)
              __hip_atomic_fetch_add(w, (unsigned long long)rs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
        }
      }
    }
    // sum and sx from the column sums: no 64-bit multiply per pixel
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      a.sum += px[i];
      a.sx += px[i] * (long long)(x + i);   // px is 0 for a column outside the rectangle
    }
    if (projx != nullptr) {
      __syncthreads();   // the tile's readers of the chunk before
#pragma unroll
      for (int i = 0; i < NP; ++i) tile[tid * NP + i] = px[i];   // = [lr][lc * NP + i]
      __syncthreads();
      const int ncol = lpr * NP, xc = (u0 + c * lpr) * NP;
      for (int col = tid; col < ncol; col += kRoiThreads) {
        long long sumc = 0;
        for (int j = 0; j < rif; ++j) sumc += tile[j * ncol + col];
        const int xg = xc + col;
        if (xg >= s.x0 && xg < s.x1 && sumc != 0)
          __hip_atomic_fetch_add(projx + (long long)f * Lx + s.px + (xg - s.x0), (unsigned long long)sumc,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
  }

  unsigned long long npix = (unsigned long long)roi_wave_sum((long long)a.npix);
  const long long sum = roi_wave_sum(a.sum), sy = roi_wave_sum(a.sy), sx = roi_wave_sum(a.sx);
  unsigned long long key =
      a.npix == 0u ? 0ull : ((unsigned long long)((uint32_t)a.bq ^ 0x80000000u) << 32) | (0xFFFFFFFFull - a.bi);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    const unsigned long long o = __shfl_xor(key, d);
    key = o > key ? o : key;
  }
  if (lane == 0) {
    unsigned long long* w = red + (tid >> 6) * 5;
    w[0] = npix; w[1] = (unsigned long long)sum; w[2] = (unsigned long long)sy; w[3] = (unsigned long long)sx;
    w[4] = key;
  }
  __syncthreads();
  if (tid == 0) {
    unsigned long long r[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) r[k] = red[k];
#pragma unroll
    for (int wv = 1; wv < 4; ++wv) {
#pragma unroll
      for (int k = 0; k < 4; ++k) r[k] += red[wv * 5 + k];
      r[4] = red[wv * 5 + 4] > r[4] ? red[wv * 5 + 4] : r[4];
    }
    if (r[0] != 0ull) {   // a strip without a sample adds nothing
      unsigned long long* row = rows + ((long long)f * R + s.r) * 8;
#pragma unroll
      for (int k = 0; k < 4; ++k) __hip_atomic_fetch_add(row + k, r[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_fetch_max(row + 4, r[4], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

static int g_roi_strip_pixels = kRoiStripPixels;
static int g_roi_rows_ahead = 0;   // 0 = by the grid's size

int roi_rows_ahead(int set) {
  if (set >= 0) {
    check(set <= 2, "roi_rows_ahead: 0 (by the grid's size), 1 or 2");
    g_roi_rows_ahead = set;
  }
  return g_roi_rows_ahead;
}

int roi_strip_pixels(int set) {
  if (set != 0) {
    check(set >= 256 && set <= (1 << 24), "roi_strip_pixels: 256 .. 2^24");
    g_roi_strip_pixels = set;
  }
  return g_roi_strip_pixels;
}

int roi_strip_rows(int width) {
  check(width >= 1, "roi_strip_rows: the width must be positive");
  const int s = g_roi_strip_pixels / width;
  return s < 1 ? 1 : s > kRoiStripRowsMax ? kRoiStripRowsMax : s;
}

std::vector<int32_t> roi_plan_strips(const std::vector<int32_t>& rects, int P, int H, int W) {
  check(P >= 1 && H >= 1 && W >= 1 && (int64_t)P * H * W < ((int64_t)1 << 31), "roi: frame size out of range");
  check(!rects.empty() && rects.size() % 5 == 0 && rects.size() / 5 <= (size_t)kRoiMaxRects,
        "roi: 1 to 16 rectangles of (p, y0, y1, x0, x1)");
  std::vector<int32_t> out;
  int64_t offx = 0, offy = 0;
  for (size_t r = 0; r < rects.size() / 5; ++r) {
    const int32_t p = rects[5 * r], y0 = rects[5 * r + 1], y1 = rects[5 * r + 2], x0 = rects[5 * r + 3],
                  x1 = rects[5 * r + 4];
    check(p >= 0 && p < P && y0 >= 0 && y0 < y1 && y1 <= H && x0 >= 0 && x0 < x1 && x1 <= W,
          "roi: a rectangle lies outside the frame or is empty");
    const int s = roi_strip_rows(x1 - x0);
    for (int y = y0; y < y1; y += s) {
      const int32_t ny = std::min(s, y1 - y);
      const int32_t strip[kRoiStripWords] = {(int32_t)r, p * H + y, ny, x0, x1, y, (int32_t)offx,
                                             (int32_t)(offy + (y - y0))};
      out.insert(out.end(), strip, strip + kRoiStripWords);
    }
    offx += x1 - x0;
    offy += y1 - y0;
  }
  return out;
}

RoiPlan::RoiPlan(const std::vector<int32_t>& rects_, int P_, int H_, int W_, int device_)
    : P(P_), H(H_), W(W_), device(device_), rects(rects_) {
  const std::vector<int32_t> host = roi_plan_strips(rects, P, H, W);
  R = (int)(rects.size() / 5);
  nstrips = (int)(host.size() / kRoiStripWords);
  Lx = Ly = 0;
  for (int r = 0; r < R; ++r) {
    Lx += rects[5 * r + 4] - rects[5 * r + 3];
    Ly += rects[5 * r + 2] - rects[5 * r + 1];
  }
  DeviceGuard g(device);
  void* d = nullptr;
  hip_check(hipMalloc(&d, host.size() * 4), "roi plan hipMalloc");
  const hipError_t e = hipMemcpy(d, host.data(), host.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) (void)hipFree(d);
  hip_check(e, "roi plan copy");
  strips = reinterpret_cast<uint64_t>(d);
}

RoiPlan::~RoiPlan() {
  if (strips != 0) {
    DeviceGuard g(device);
    (void)hipFree(reinterpret_cast<void*>(strips));
  }
}

void launch_roi(const FramePtrs& fp, int nframes, const RoiPlan& plan, float vmin, float vmax, int frac_bits,
                uint64_t mask, uint64_t rows, uint64_t projx, uint64_t projy, uint64_t stream) {
  check_nframes(nframes, "roi");
  check(plan.strips != 0 && plan.nstrips >= 1, "roi: empty plan");
  check(std::isfinite(vmin) && std::isfinite(vmax) && vmin <= vmax, "roi: the value window must be finite, vmin <= vmax");
  check(frac_bits >= 0 && frac_bits <= 16, "roi: frac_bits must be in [0, 16]");
  // Q < 2^31 (q is an int32) and, per rectangle, Q * area * max(y1 - 1, x1 - 1, 1) <= 2^63 - 1 (the moments)
  const double qd = std::ceil(std::fmax(std::fabs((double)vmin), std::fabs((double)vmax)) * (double)(1 << frac_bits));
  check(qd < 2147483648.0, "roi: max(|vmin|, |vmax|) * 2^frac_bits must stay below 2^31");
  const unsigned __int128 Q = (unsigned __int128)(uint64_t)qd;
  for (int r = 0; r < plan.R; ++r) {
    const int32_t* c = plan.rects.data() + 5 * r;
    const unsigned __int128 area = (unsigned __int128)(c[2] - c[1]) * (unsigned)(c[4] - c[3]);
    const unsigned lever = (unsigned)std::max(std::max(c[2] - 1, c[4] - 1), 1);
    check(Q * area * lever <= (unsigned __int128)INT64_MAX, "roi: Q * area * max(y1 - 1, x1 - 1, 1) must fit 2^63 - 1");
  }
  check(rows != 0 && rows % 64 == 0, "roi: rows must be non-null and 64-B aligned");
  check(projx % 8 == 0 && projy % 8 == 0, "roi: projections must be 8-B aligned");
  check(mask % 16 == 0, "roi: the mask must be 16-B aligned");
  check_frames(fp, nframes, "roi");
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  hip_check(hipMemsetAsync(reinterpret_cast<void*>(rows), 0, (size_t)nframes * plan.R * 64, st), "roi clear rows");
  if (projx != 0)
    hip_check(hipMemsetAsync(reinterpret_cast<void*>(projx), 0, (size_t)nframes * plan.Lx * 8, st), "roi clear proj_x");
  if (projy != 0)
    hip_check(hipMemsetAsync(reinterpret_cast<void*>(projy), 0, (size_t)nframes * plan.Ly * 8, st), "roi clear proj_y");
  const dim3 grid((unsigned)plan.nstrips, (unsigned)nframes);
  const RoiParams pp{vmin, vmax, (float)(1 << frac_bits)};
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, dim3(kRoiThreads), 0, st, fp, reinterpret_cast<const RoiStrip*>(plan.strips),
                       (uint32_t)plan.W, reinterpret_cast<const uint8_t*>(mask), pp,
                       reinterpret_cast<unsigned long long*>(rows), plan.R, reinterpret_cast<unsigned long long*>(projx),
                       (long long)plan.Lx, reinterpret_cast<unsigned long long*>(projy), (long long)plan.Ly);
  };
  const bool one = g_roi_rows_ahead != 0 ? g_roi_rows_ahead == 1   // forced: tests and measurements only
                                         : (int64_t)plan.nstrips * nframes > kRoiResidentGrid;
  if (plan.W % 4 == 0) one ? go(roi_kernel<4, 1>) : go(roi_kernel<4, 2>);
  else one ? go(roi_kernel<1, 1>) : go(roi_kernel<1, 2>);
  hip_check(hipGetLastError(), "roi launch");
}

}  // namespace pr
