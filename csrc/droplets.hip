// K-14 droplets for queue consumers: the connected clusters of active pixels of every frame of a batch,
// each with its label, pixel count, summed charge, charge-weighted row / column sums and largest pixel.
//
// Contract (docs/ARCHITECTURE.md, "Droplets: the contract"; golden model ops/reference.py droplet_reference):
//   active        (mask absent or mask[i] != 0) and thr_low <= v and v <= vmax   (K-10's window: NaN fails,
//                 +-inf and v <= 0 are outside; a pixel above vmax is inactive and splits a cluster)
//   candidate     a maximal 4-connected set of active pixels of one panel (no join across a row end, a
//                 panel edge or a diagonal);  droplet = a candidate with a pixel v >= thr_seed
//   q             (int64) rintf(v * 2^S) per active pixel;  per droplet label = lowest linear index,
//                 npix, adu = sum q, sy / sx = sum q * row / q * column (in-panel), qmax = max q
//   nact[f]       exact number of active pixels, also past cap_pix;  flags bit 2 = nact > cap_pix
//   ndrop[f]      exact number of droplets, also past cap (0 when bit 2 is set);  flags bit 0 = ndrop > cap
//   offs[F + 1]   int64 exclusive scan of the stored counts (a frame with a flag bit stores nothing); the
//                 six columns hold frame f's droplets at offs[f] .. offs[f + 1], label strictly ascending
// Every output word is a function of the inputs alone: integer atomics only, and no position in any
// list depends on workgroup order.
//
// MI355X design.  The frames are streamed from HBM once, by K-10's own scan: launch_droplets calls
// launch_sparsify (csrc/sparse.hip, unchanged: memset, sparse_scan_kernel, sparse_pack_kernel) with the
// window [thr_low, vmax] and cap_pix, which leaves in the scratch block the canonical list of every
// frame's active pixels -- (index, value) rows in ascending index order at koffs[f] .. koffs[f + 1] -- and
// writes nact.  A row's position in that list is its slot; slot order is index order, so the lowest slot
// of a cluster is its lowest pixel.  Four more launches touch active pixels only (grid (blocks, F), a
// block owns a contiguous range of its frame's rows):
//   droplet_index_kernel   parent[s] = s, joined[s] = 0, clears the row's accumulators (planar arrays: one
//     64-B record per row, tried first, made the reduce three times slower -- five atomics into one line).
//   droplet_link_kernel    left neighbour: the previous row when its index is pix - 1 and x > 0;  up
//     neighbour: the row of index pix - W when y > 0, searched in the list itself: the rows between the two
//     are the active pixels of less than one detector row, so a gallop back from s in doubling steps and
//     a bisection find it within a few cache lines next to s (dr_row_of; both loops counted).  No dense
//     slot map is kept, and no launch after the scan reads a frame or the mask.  Neighbours found are
//     united in a lock-free union-find: atomicMin on parent, relaxed, agent scope; both rows get joined = 1.
//   droplet_reduce_kernel  a row that was never joined is a droplet of one pixel and writes its own
//     accumulators with plain stores.  Every other row finds its root (and points itself at it), adds q,
//     q * y, q * x and (1 | seed << 32) and takes max q at the root: at most five relaxed agent-scope
//     integer atomics per pixel.
//   droplet_count_kernel / droplet_pack_kernel   a row is a droplet iff parent[s] == s and its seed count
//     is not zero.  Every block counts its range; the pack rebuilds ndrop / flags / offs from the (F, blocks)
//     counts in every workgroup and writes the columns in slot order, which is label order.
// Kernel boundaries are the only ordering between phases.  No workgroup waits for another, nothing spins
// on a value another workgroup writes, there is no grid-wide barrier.
//
// Termination of the union-find.  parent[s] <= s holds from the index kernel on: the only writes are
// atomicMin with a value below s and the reduce kernel's store of a root found by walking down.
// dr_find follows parent strictly downward and is a counted loop of at most x steps.  dr_unite's loop is
// counted by a + b, which strictly falls every round (a is replaced by an older parent below it): both
// loops end whatever another workgroup does, and whatever the scratch block held.
//
// Resources (hipcc -O3, gfx950; every kernel 8 waves per SIMD, no scratch memory):
//   droplet_index_kernel  22 VGPRs, 0 B scratch, 0 B LDS     droplet_link_kernel   20 VGPRs, 0 B scratch, 0 B LDS
//   droplet_reduce_kernel 22 VGPRs, 0 B scratch, 0 B LDS     droplet_count_kernel  10 VGPRs, 0 B scratch, 16 B LDS
//   droplet_pack_kernel   42 VGPRs, 0 B scratch, 288 B LDS   (K-10's two kernels: csrc/sparse.hip)
//
// Measured on the MI355X (profiles/droplets/README.md): epix10k2M, 64-frame batch, pix_cap = cap = n / 16,
// us/frame, median of five interleaved rounds in one process, two runs.
//   active pixels        droplets        scan (K-10)     index + link    reduce          count + pack    sparsify        read_f32 floor
//   2.1 % (photons)      6.021 / 6.040   3.331 / 3.334   0.981 / 0.993   0.960 / 0.955   0.801 / 0.837   3.327 / 3.314   1.807 / 1.790
//   1.0 %                4.538 / 4.536   3.235 / 3.247   0.505 / 0.507   0.380 / 0.384   0.465 / 0.473   3.233 / 3.210
//   5.0 % (noise)        13.05 / 12.36   3.506 / 3.510   2.843 / 2.767   4.282 / 4.106   2.044 / 1.873   3.506 / 3.489
// The scan costs what sparsify costs, by construction.  A dense slot_of [F, n] map for the up neighbour
// (9.13 / 5.61 / 17.8 in all; index + link 2.77 / 0.91 / 6.14) and one 48-B accumulator record per row
// (reduce 7.78 / 3.76 / 19.1) were measured and not kept; without the joined flag the reduce took
// 1.88 / 0.81 / 6.04.  Not built: an in-wave combine of equal-root neighbours before the atomics.
#include "common.h"
#include "kernels.h"
#include "launch.h"

#include <algorithm>
#include <cmath>

namespace pr {

constexpr int kDrMaxBlocks = 32;       // workgroups per frame of the four row kernels, at most
constexpr int kDrRowsPerBlock = 2048;  // rows of cap_pix that ask for one more workgroup per frame
constexpr int kDrHeader = 1024;        // K-10's flags [64] at 0 and offs int64 [65] at 64
constexpr int kDrCntBytes = kMaxFrames * kDrMaxBlocks * 4;

struct DrParams {
  int W, HW;
  int64_t n;
  float scale;      // 2^S
  float thr_seed;
  int cap;          // droplets per frame
  int cap_pix;
  int nb;           // gridDim.x of the row kernels
  uint64_t kflags;  // uint8 [F]       K-10: bit 0 = nact > cap_pix
  uint64_t koffs;   // int64 [F + 1]   K-10: rows of frame f
  uint64_t pix;     // int32 [rows]
  uint64_t val;     // float [rows]
  uint64_t parent;  // int32 [rows]
  uint64_t joined;  // int32 [rows]    1 = the row was united with a neighbour
  uint64_t qmax;    // int32 [rows]
  uint64_t adu;     // uint64 [rows]   accumulators, valid at roots
  uint64_t sy;      // uint64 [rows]
  uint64_t sx;      // uint64 [rows]
  uint64_t npk;     // uint64 [rows]   low word: pixels; high word: pixels with v >= thr_seed (each <= cap_pix < 2^31)
  uint64_t cnt;     // uint32 [F, nb]
};

// rows [lo, hi) of frame f that block b of nb owns; bounded by the rows the scratch block holds
__device__ __forceinline__ void dr_range(const DrParams& dp, int f, int b, int nframes, int64_t& o0, int64_t& lo,
                                         int64_t& hi) {
  const PR_GLOBAL long long* koffs = gin<long long>(dp.koffs);
  const int64_t lim = (int64_t)nframes * dp.cap_pix;
  int64_t a = koffs[f], e = koffs[f + 1];
  a = a < 0 ? 0 : (a > lim ? lim : a);
  e = e < a ? a : (e > lim ? lim : e);
  const int64_t c = e - a;
  o0 = a;
  lo = a + c * b / dp.nb;
  hi = a + c * (b + 1) / dp.nb;
}

__device__ __forceinline__ int dr_load(const PR_GLOBAL int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// root of x.  parent[s] <= s: every step goes strictly down, so x steps are enough; the loop is counted.
__device__ __forceinline__ int dr_find(const PR_GLOBAL int* parent, int x) {
  for (int steps = x; steps > 0; --steps) {
    const int p = dr_load(parent + x);
    if (p >= x || p < 0) break;   // a root (p > x or p < 0 cannot be after the index kernel)
    x = p;
  }
  return x;
}

// joins the sets of a and b under the lower root.  Every round either ends or replaces a by a value below
// it, so a + b strictly falls: the loop is counted by it.
__device__ __forceinline__ void dr_unite(PR_GLOBAL int* parent, int a, int b) {
  a = dr_find(parent, a);
  b = dr_find(parent, b);
  for (int64_t budget = (int64_t)a + b; a != b && budget >= 0; --budget) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old >= a) break;   // a was a root and now hangs under b
    // a had a parent old < a already: parent[a] is now min(old, b), and old's set and b's must still meet
    a = dr_find(parent, old);
    b = dr_find(parent, b);
  }
}

// the row of pixel index `target` among the frame's rows [o0, g), or -1.  pix ascends and pix[g] > target, and
// the rows between the two are the active pixels of less than one detector row: gallop back from g in
// doubling steps, then bisect.  Both loops are counted (g - o0 < 2^31).
__device__ __forceinline__ int64_t dr_row_of(const PR_GLOBAL int* pix, int64_t o0, int64_t g, int target) {
  int64_t hi = g, lo = g - 1, step = 1;
  for (int it = 0; it < 32; ++it) {
    if (lo < o0) {
      lo = o0 - 1;
      break;
    }
    if (pix[lo] <= target) break;
    hi = lo;
    step *= 2;
    lo = hi - step;
  }
  if (lo < o0) lo = o0 - 1;
  // pix[hi] > target, and lo == o0 - 1 or pix[lo] <= target
  for (int it = 0; it < 32 && hi - lo > 1; ++it) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (pix[mid] <= target) lo = mid; else hi = mid;
  }
  return (lo >= o0 && pix[lo] == target) ? lo : -1;
}

__global__ __launch_bounds__(256) void droplet_index_kernel(const DrParams dp, const int nframes) {
  const int f = blockIdx.y;
  int64_t o0, lo, hi;
  dr_range(dp, f, blockIdx.x, nframes, o0, lo, hi);
  for (int64_t g = lo + threadIdx.x; g < hi; g += 256) {
    gout<int>(dp.parent)[g] = (int)g;
    gout<int>(dp.joined)[g] = 0;
    gout<int>(dp.qmax)[g] = 0;
    gout<unsigned long long>(dp.adu)[g] = 0ull;
    gout<unsigned long long>(dp.sy)[g] = 0ull;
    gout<unsigned long long>(dp.sx)[g] = 0ull;
    gout<unsigned long long>(dp.npk)[g] = 0ull;
  }
}

__global__ __launch_bounds__(256) void droplet_link_kernel(const DrParams dp, const int nframes) {
  const int f = blockIdx.y;
  int64_t o0, lo, hi;
  dr_range(dp, f, blockIdx.x, nframes, o0, lo, hi);
  const PR_GLOBAL int* pix = gin<int>(dp.pix);
  PR_GLOBAL int* parent = gout<int>(dp.parent);
  PR_GLOBAL int* joined = gout<int>(dp.joined);
  for (int64_t g = lo + threadIdx.x; g < hi; g += 256) {
    const int p = pix[g];
    if (p < 0 || p >= dp.n) continue;   // never after a scan of this batch
    const int r = p % dp.HW;
    const int y = r / dp.W, x = r - y * dp.W;
    const bool left = x > 0 && g > o0 && pix[g - 1] == p - 1;
    const int64_t t = y > 0 ? dr_row_of(pix, o0, g, p - dp.W) : -1;
    if (left) {
      joined[g - 1] = 1;   // several lanes may store the same 1
      dr_unite(parent, (int)g, (int)g - 1);
    }
    if (t >= 0) {
      joined[t] = 1;
      dr_unite(parent, (int)g, (int)t);
    }
    if (left || t >= 0) joined[g] = 1;
  }
}

__global__ __launch_bounds__(256) void droplet_reduce_kernel(const DrParams dp, const int nframes) {
  const int f = blockIdx.y;
  int64_t o0, lo, hi;
  dr_range(dp, f, blockIdx.x, nframes, o0, lo, hi);
  const PR_GLOBAL int* pix = gin<int>(dp.pix);
  const PR_GLOBAL float* val = gin<float>(dp.val);
  PR_GLOBAL int* parent = gout<int>(dp.parent);
  for (int64_t g = lo + threadIdx.x; g < hi; g += 256) {
    const int p = pix[g];
    const float v = val[g];
    const int r = p % dp.HW;
    const int y = r / dp.W, x = r - y * dp.W;
    const int q = (int)__builtin_rintf(v * dp.scale);   // 0 <= q <= Q < 2^31 (checked by the launcher)
    const unsigned long long uq = (unsigned long long)(unsigned)q;
    const unsigned long long one = 1ull + (v >= dp.thr_seed ? 1ull << 32 : 0ull);
    if (gin<int>(dp.joined)[g] == 0) {
      // a pixel without an active neighbour is its own droplet and nobody else adds to its row: plain stores
      gout<unsigned long long>(dp.adu)[g] = uq;
      gout<unsigned long long>(dp.sy)[g] = uq * (unsigned)y;
      gout<unsigned long long>(dp.sx)[g] = uq * (unsigned)x;
      gout<unsigned long long>(dp.npk)[g] = one;
      gout<int>(dp.qmax)[g] = q;
      continue;
    }
    int root = dr_find(parent, (int)g);
    if (root < o0) root = (int)g;       // never after a link of this batch: keeps the adds inside the frame
    if (root != (int)g) parent[g] = root;   // a root keeps parent == itself; any reader still sees an ancestor
    __hip_atomic_fetch_add(gout<unsigned long long>(dp.adu) + root, uq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (y != 0)
      __hip_atomic_fetch_add(gout<unsigned long long>(dp.sy) + root, uq * (unsigned)y, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    if (x != 0)
      __hip_atomic_fetch_add(gout<unsigned long long>(dp.sx) + root, uq * (unsigned)x, __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(gout<unsigned long long>(dp.npk) + root, one, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_max(gout<int>(dp.qmax) + root, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__device__ __forceinline__ bool dr_is_droplet(const DrParams& dp, int64_t g) {
  return gin<int>(dp.parent)[g] == (int)g && (gin<unsigned long long>(dp.npk)[g] >> 32) != 0ull;
}

__global__ __launch_bounds__(256) void droplet_count_kernel(const DrParams dp, const int nframes) {
  __shared__ unsigned s_w[4];
  const int f = blockIdx.y;
  int64_t o0, lo, hi;
  dr_range(dp, f, blockIdx.x, nframes, o0, lo, hi);
  unsigned c = 0u;
  for (int64_t g = lo + threadIdx.x; g < hi; g += 256) c += dr_is_droplet(dp, g) ? 1u : 0u;
#pragma unroll
  for (int d = 32; d >= 1; d /= 2) c += __shfl_xor(c, d, 64);
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = c;
  __syncthreads();
  if (threadIdx.x == 0u) gout<unsigned>(dp.cnt)[f * dp.nb + blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

__device__ __forceinline__ unsigned dr_wave_incl(unsigned x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const unsigned y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

__global__ __launch_bounds__(256) void droplet_pack_kernel(const DrParams dp, const int nframes, int* __restrict__ ndrop,
                                                           unsigned char* __restrict__ flags,
                                                           long long* __restrict__ offs, int* __restrict__ label,
                                                           int* __restrict__ npix, long long* __restrict__ adu,
                                                           long long* __restrict__ sy, long long* __restrict__ sx,
                                                           int* __restrict__ qmax) {
  __shared__ unsigned s_off[kMaxFrames + 1];
  __shared__ unsigned s_w[4];
  const uint32_t t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  const int f = blockIdx.y, b = blockIdx.x;
  const unsigned cap = (unsigned)dp.cap;
  const PR_GLOBAL unsigned* cnt = gin<unsigned>(dp.cnt);
  if (w == 0) {
    // ndrop[], the stored counts and the batch-level offsets, rebuilt by every workgroup (F <= 64 lanes;
    // a frame's count is at most cap_pix and F * cap < 2^31)
    unsigned c = 0u;
    unsigned kf = 0u;
    if (lane < nframes) {
      for (int j = 0; j < dp.nb; ++j) c += cnt[lane * dp.nb + j];
      kf = gin<unsigned char>(dp.kflags)[lane] & 1u;
    }
    const unsigned st = (kf == 0u && c <= cap) ? c : 0u;
    const unsigned incl = dr_wave_incl(st);
    s_off[lane + 1] = incl;
    if (lane == 0) s_off[0] = 0u;
    if (b == 0 && f == 0) {
      if (lane < nframes) {
        ndrop[lane] = (int)c;
        flags[lane] = (unsigned char)((c > cap ? 1u : 0u) | (kf << 2));
        offs[lane + 1] = (long long)incl;
      }
      if (lane == 0) offs[0] = 0ll;
    }
  }
  __syncthreads();
  const unsigned end = s_off[f + 1];
  if (end == s_off[f]) return;   // empty or overflowing frame: nothing to write
  unsigned run = s_off[f];
  for (int j = 0; j < b; ++j) run += cnt[f * dp.nb + j];
  int64_t o0, lo, hi;
  dr_range(dp, f, b, nframes, o0, lo, hi);
  const PR_GLOBAL int* pix = gin<int>(dp.pix);
  for (int64_t g0 = lo; g0 < hi; g0 += 256) {
    __syncthreads();   // s_w of the previous round has been read
    const int64_t g = g0 + t;
    const bool d = g < hi && dr_is_droplet(dp, g);
    const unsigned long long bal = __ballot(d);
    const unsigned rank =
        __builtin_amdgcn_mbcnt_hi((unsigned)(bal >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)bal, 0u));
    if (lane == 0) s_w[w] = (unsigned)__popcll(bal);
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const unsigned x = s_w[ww];
      if (ww < w) before += x;
      all += x;
    }
    const unsigned o = run + before + rank;
    if (d && o < end) {   // o < end always after a count of this batch
      label[o] = pix[g];
      npix[o] = (int)(unsigned)gin<unsigned long long>(dp.npk)[g];
      adu[o] = (long long)gin<unsigned long long>(dp.adu)[g];
      sy[o] = (long long)gin<unsigned long long>(dp.sy)[g];
      sx[o] = (long long)gin<unsigned long long>(dp.sx)[g];
      qmax[o] = gin<int>(dp.qmax)[g];
    }
    run += all;
  }
}

static int64_t dr_align16(int64_t x) { return (x + 15) / 16 * 16; }
static int64_t dr_rows(int64_t cap_pix, int frames) { return (cap_pix * frames + 3) / 4 * 4; }

int64_t droplets_scratch_bytes(int64_t n, int64_t cap_pix, int64_t cap, int frames) {
  check_frame_size(n, "droplets");
  check_nframes(frames, "droplets");
  check(cap_pix >= 1 && cap_pix * frames < (int64_t)1 << 31, "droplets: cap_pix out of range");
  check(cap >= 1 && cap * frames < (int64_t)1 << 31, "droplets: cap out of range");
  return kDrHeader + kDrCntBytes + dr_align16(sparsify_scratch_bytes(n, cap_pix, frames)) +
         52 * dr_rows(cap_pix, frames);
}

void launch_droplets(const FramePtrs& fp, int nframes, int P, int H, int W, float thr_low, float thr_seed, float vmax,
                     int frac_bits, int64_t cap_pix, int64_t cap, uint64_t mask, uint64_t nact, uint64_t ndrop,
                     uint64_t flags, uint64_t offs, uint64_t label, uint64_t npix, uint64_t adu, uint64_t sy, uint64_t sx,
                     uint64_t qmax, uint64_t scratch, int64_t scratch_bytes, uint64_t stream, int phases) {
  check(phases >= 1 && phases <= 15, "droplets: phases is a mask of 1 (scan), 2 (index + link), 4 (reduce), 8 (pack)");
  check_nframes(nframes, "droplets");
  check(P >= 1 && H >= 1 && W >= 1 && (int64_t)P * H * W < (int64_t)1 << 31, "droplets: shape out of range");
  const int64_t n = (int64_t)P * H * W, hw = (int64_t)H * W;
  check(cap_pix >= 1 && cap_pix * nframes < (int64_t)1 << 31, "droplets: cap_pix must be >= 1 and F * cap_pix < 2^31");
  check(cap >= 1 && cap * nframes < (int64_t)1 << 31, "droplets: cap must be >= 1 and F * cap < 2^31");
  check(std::isfinite(thr_low) && std::isfinite(thr_seed) && std::isfinite(vmax) && 0.0f < thr_low &&
            thr_low <= thr_seed && thr_seed <= vmax,
        "droplets: need finite 0 < thr_low <= thr_seed <= vmax");
  check(frac_bits >= 0 && frac_bits <= 16, "droplets: frac_bits must be 0 .. 16");
  const double qd = std::ceil((double)vmax * (double)((int64_t)1 << frac_bits));   // exact: a float32 times 2^S
  check(qd < 2147483648.0, "droplets: ceil(vmax * 2^frac_bits) must be below 2^31");
  const __int128 bound = (__int128)(int64_t)qd * (std::max(H, W) - 1) * std::min<int64_t>(hw, cap_pix);
  check(bound <= (__int128)INT64_MAX, "droplets: the weighted sums of a droplet could pass 2^63 - 1");
  check(mask % 4 == 0, "droplets: mask must be 4-B aligned");
  check(nact != 0 && ndrop != 0 && flags != 0 && offs != 0 && label != 0 && npix != 0 && adu != 0 && sy != 0 && sx != 0 &&
            qmax != 0 && nact % 4 == 0 && ndrop % 4 == 0 && offs % 8 == 0 && label % 4 == 0 && npix % 4 == 0 &&
            adu % 8 == 0 && sy % 8 == 0 && sx % 8 == 0 && qmax % 4 == 0,
        "droplets: misaligned or missing output");
  check(scratch != 0 && scratch % 16 == 0, "droplets: the scratch block must be 16-B aligned");
  check(scratch_bytes >= droplets_scratch_bytes(n, cap_pix, cap, nframes), "droplets: scratch block too small");
  check_frames(fp, nframes, "droplets");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int64_t rows = dr_rows(cap_pix, nframes);
  const int64_t sps = dr_align16(sparsify_scratch_bytes(n, cap_pix, nframes));
  DrParams dp{};
  dp.W = W;
  dp.HW = (int)hw;
  dp.n = n;
  dp.scale = (float)((int64_t)1 << frac_bits);
  dp.thr_seed = thr_seed;
  dp.cap = (int)cap;
  dp.cap_pix = (int)cap_pix;
  dp.nb = (int)std::max<int64_t>(1, std::min<int64_t>(kDrMaxBlocks, (cap_pix + kDrRowsPerBlock - 1) / kDrRowsPerBlock));
  dp.kflags = scratch;
  dp.koffs = scratch + 64;
  dp.cnt = scratch + kDrHeader;
  const uint64_t k10 = dp.cnt + kDrCntBytes;
  dp.pix = k10 + (uint64_t)sps;
  dp.val = dp.pix + (uint64_t)rows * 4;
  dp.parent = dp.val + (uint64_t)rows * 4;
  dp.joined = dp.parent + (uint64_t)rows * 4;
  dp.qmax = dp.joined + (uint64_t)rows * 4;
  dp.adu = dp.qmax + (uint64_t)rows * 4;
  dp.sy = dp.adu + (uint64_t)rows * 8;
  dp.sx = dp.sy + (uint64_t)rows * 8;
  dp.npk = dp.sx + (uint64_t)rows * 8;
  if (phases & 1)   // K-10: nact, and the canonical (index, value) rows of the frames that fit cap_pix
    launch_sparsify(fp, nframes, n, thr_low, vmax, cap_pix, mask, 0, 0, nact, dp.kflags, dp.koffs, dp.pix, dp.val, k10, sps,
                    stream, 3);
  const dim3 grid((unsigned)dp.nb, (unsigned)nframes);
  if (phases & 2) {
    hipLaunchKernelGGL(droplet_index_kernel, grid, dim3(256), 0, s, dp, nframes);
    hip_check(hipGetLastError(), "droplets index launch");
    hipLaunchKernelGGL(droplet_link_kernel, grid, dim3(256), 0, s, dp, nframes);
    hip_check(hipGetLastError(), "droplets link launch");
  }
  if (phases & 4) {
    hipLaunchKernelGGL(droplet_reduce_kernel, grid, dim3(256), 0, s, dp, nframes);
    hip_check(hipGetLastError(), "droplets reduce launch");
  }
  if (phases & 8) {
    hipLaunchKernelGGL(droplet_count_kernel, grid, dim3(256), 0, s, dp, nframes);
    hip_check(hipGetLastError(), "droplets count launch");
    hipLaunchKernelGGL(droplet_pack_kernel, grid, dim3(256), 0, s, dp, nframes, reinterpret_cast<int*>(ndrop),
                       reinterpret_cast<unsigned char*>(flags), reinterpret_cast<long long*>(offs),
                       reinterpret_cast<int*>(label), reinterpret_cast<int*>(npix), reinterpret_cast<long long*>(adu),
                       reinterpret_cast<long long*>(sy), reinterpret_cast<long long*>(sx), reinterpret_cast<int*>(qmax));
    hip_check(hipGetLastError(), "droplets pack launch");
  }
}

}  // namespace pr
