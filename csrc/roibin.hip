// K-17 roibin for queue consumers: every kept frame of a batch as a small LOSSLESS box around each peak
// the peak finder (K-07) reported, plus the whole frame binned B x B and quantised to int16 codes.
//
// Contract (docs/ARCHITECTURE.md, "Roibin: the contract"; golden model ops/reference.py roibin_reference).
// Inputs: F frames [P, H, W] float32, the finder's peaks float32 [F, max_peaks, 8] and counts int32 [F].
//   kept        counts[f] >= min_peaks; a skipped frame is neither read nor written (its code rows stay as
//               they were): flags[f] = 2, nbox = nsat = nbad = 0
//   counts      a pixel counts iff (no mask or mask[i] != 0) && vmin <= v && v <= vmax as float32 (NaN and
//               +-inf never count); it gives q = (int) rintf(v * inv), ONE float32 multiply (never
//               contracted: -ffp-contract=off), ties to even
//   code        block sum S, count c over the block clipped to the panel: -32768 when c == 0, otherwise
//               clamp(floor_div(2 S + c, 2 c), -32767, 32767) -- round half up with FLOOR division; a
//               clamped block adds 1 to nsat[f].  max(|vmin|, |vmax|) * inv < 2^25 (the caller's check, and
//               the launcher's), so 2 S + c fits an int32 at B = 4
//   npk         max(counts[f], 0); nrec = min(npk, max_peaks); npk > max_peaks: flags bit 0, nbox = 0
//   valid       a record's (p, y, x) floats are finite, integral and inside the frame; every other record of
//               the nrec adds 1 to nbad[f] (flags bit 2) and never forms an address
//   boxes       the valid records ordered by ctr = (p * H + y) * W + x, ties by slot: ctr int32, rec = bit
//               copy of the record's 8 words, box [2R+1, 2R+1] = bit copies of the frame inside the panel,
//               0x7FC00000 outside; frame f's boxes at offs[f] .. offs[f + 1], offs = exclusive scan of nbox
// Every output word is a function of the inputs alone.  One call is complete in itself: nsat is cleared on
// the stream, nothing else needs clearing; nothing is written past F * max_peaks boxes.
//
// MI355X design, two launches per batch:
//   roibin_bin_kernel<B, NC, VEC, U>   grid (x, F).  A lane owns CELLS of B rows x NC * B columns = NC codes;
//     NC * B is a multiple of 4 on the VEC path (W % 4 == 0: 16-B non-temporal loads, the mask as 4-B words;
//     NC = 4 / 2 / 2 for B = 1 / 2 / 4, or NC = 1 at B = 4 when Wb is odd), so a row of cells never ends in a
//     partial cell and a lane stores its NC codes with ONE 8- / 4- / 2-B store.  The scalar path (W % 4 != 0)
//     loads pixel by pixel and owns NC = 2 codes where Wb is even, else 1.  U cells per lane are loaded
//     before the first is used (4 to 8 16-B loads in flight per lane).  Cell index -> (row of blocks,
//     cell) -> (panel, block row) by two multiply-high divisions whose constants the launcher makes.  A
//     full block (c == B * B) divides by a shift; only a lane with a masked, clipped or out-of-window pixel
//     takes the integer division.  nsat: lanes count their clamped codes in a register, one wave reduction
//     and ONE relaxed agent-scope atomicAdd per workgroup that clamped anything.  Block x == 0 of frame f
//     first validates the frame's records and writes npk / nbox / nbad / flags (also for a skipped frame).
//   roibin_box_kernel   grid F, after the kernel boundary.  Rebuilds offs from the F nbox words in one wave,
//     builds the 64-bit keys (ctr << 32 | slot; ~0 for an invalid record or padding) of the frame's nrec
//     records in LDS, sorts them with a bitonic network (at most 4096 keys, 32 KiB), then one WAVE per box
//     copies ctr, the record's 8 words and the (2R+1)^2 window: nbox * (2R+1)^2 pixels are read, not the frame.
// No float atomics, no workgroup waits for another.
//
// Resources (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage): no instance uses scratch memory (0 bytes
// per lane, no spills).  roibin_bin_kernel<B, NC, VEC, U>: 16 B of LDS; VGPRs <1,4,vec,4> 42, <2,2,vec,4> 58,
// <4,2,vec,1> 52 (7 waves per SIMD), <4,1,vec,2> 54, the scalar instances 26 .. 45; 8 waves per SIMD unless said.
// roibin_box_kernel: 32 VGPRs, 33056 B of LDS (the keys; 4 workgroups per CU).
//
// Measured on the MI355X (profiles/roibin/README.md): epix10k2M calib frames, 64-frame batch, us/frame, median of
// five interleaved rounds in one process, one run; about 100 hand-made records per frame unless said.
//   read_f32 floor 1.830    powder(NC=1) 1.822
//   bin B=1  1.976 (1.08 x the floor for 1.5 x its bytes)     bin B=2  1.658 (0.91 x for 1.125 x)
//   bin B=4  1.623 (0.89 x for 1.03 x)
//   boxes, ~100 peaks, R=4   0.446 (28.6 us per batch)        boxes, 2048 peaks  10.71 (686 us per batch)
//   whole call, B=2, ~100 peaks  2.403
// The binning kernel is at or below the floor row at B = 2 and 4 (that row is a plain read kernel, not a hardware bound);
// B = 1 costs its 0.5 x extra store bytes.  The box kernel is one workgroup per frame by design: 2048 boxes per
// frame are 512 serial boxes per wave, so it is bound by its own latency (0.02 of the HBM roof).  The whole call is
// 0.3 us/frame more than its two parts: supposed to be the box kernel's dependence on the binning kernel, which
// keeps the next launch's binning from overlapping this one's tail in the replayed graph; not measured apart.
// No A/B variants were run.
#include "common.h"
#include "kernels.h"
#include "launch.h"

#include <cmath>

namespace pr {

// n / d for n < 2^31 by one multiply-high (Granlund & Montgomery: m = ceil(2^(31 + L) / d), L = ceil(log2 d))
struct RbDiv {
  uint32_t mul, shr, one;
};

static RbDiv rb_div_make(uint32_t d) {
  RbDiv r{0u, 0u, d == 1u ? 1u : 0u};
  if (d == 1u) return r;
  uint32_t L = 0;
  while ((1ull << L) < d) ++L;
  const uint64_t p = 31 + L;
  r.mul = (uint32_t)(((1ull << p) + d - 1) / d);
  r.shr = (uint32_t)(p - 32);
  return r;
}

__device__ __forceinline__ uint32_t rb_div(const uint32_t n, const RbDiv& d) {
  return d.one ? n : __umulhi(n, d.mul) >> d.shr;
}

struct RbParams {
  float inv, vmin, vmax;
  int P, H, W, Hb, Wb;
  int Cw;            // cells per row of blocks
  uint32_t T;        // cells per frame: P * Hb * Cw
  RbDiv dCw, dHb;
  int min_peaks, max_peaks;
  uint64_t mask;     // uint8 [n] or 0
  uint64_t peaks;    // float [F, max_peaks, 8]
  uint64_t counts;   // int32 [F]
  uint64_t codes;    // int16 [F, P, Hb, Wb]
  uint64_t npk, nbox, nbad, nsat;   // int32 [F]
  uint64_t flags;    // uint8 [F]
};

// one coordinate of a record: finite, integral, 0 <= v < dim.  The int is formed only from a float in
// [0, 2^31), so nothing out of range is ever converted (or turned into an address).
__device__ __forceinline__ bool rb_coord(const float v, const int dim, int& out) {
  out = 0;
  if (!(v >= 0.0f && v < 2147483648.0f)) return false;   // NaN fails
  const unsigned u = (unsigned)v;
  if ((float)u != v || u >= (unsigned)dim) return false;
  out = (int)u;
  return true;
}

__device__ __forceinline__ bool rb_valid(const RbParams& rp, const PR_GLOBAL float* rec, int& ctr) {
  int p, y, x;
  const bool ok = rb_coord(rec[0], rp.P, p) & rb_coord(rec[1], rp.H, y) & rb_coord(rec[2], rp.W, x);
  ctr = (p * rp.H + y) * rp.W + x;   // < P * H * W < 2^31 when ok; 0 otherwise
  return ok;
}

__device__ __forceinline__ int rb_wave_sum(int x) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d, 64);
  return x;
}

// all 256 threads; the sum is returned to every thread
__device__ __forceinline__ int rb_block_sum(int x, int* s_red) {
  x = rb_wave_sum(x);
  __syncthreads();   // s_red of an earlier sum has been read
  if ((threadIdx.x & 63u) == 0u) s_red[threadIdx.x >> 6] = x;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// the header words of frame f, by one workgroup
__device__ __forceinline__ void rb_header(const RbParams& rp, const int f, const int cnt, int* s_red) {
  const int npk = cnt > 0 ? cnt : 0;
  const bool kept = cnt >= rp.min_peaks, over = npk > rp.max_peaks;
  int bad = 0;
  if (kept && !over) {   // workgroup-uniform
    const PR_GLOBAL float* rec = gin<float>(rp.peaks) + (int64_t)f * rp.max_peaks * 8;
    for (int i = threadIdx.x; i < npk; i += 256) {
      int ctr;
      bad += !rb_valid(rp, rec + (int64_t)i * 8, ctr);
    }
  }
  bad = rb_block_sum(bad, s_red);
  if (threadIdx.x == 0u) {
    gout<int>(rp.npk)[f] = npk;
    gout<int>(rp.nbox)[f] = kept && !over ? npk - bad : 0;
    gout<int>(rp.nbad)[f] = bad;
    gout<unsigned char>(rp.flags)[f] = (unsigned char)((kept && over ? 1u : 0u) | (kept ? 0u : 2u) | (bad ? 4u : 0u));
  }
}

__device__ __forceinline__ int rb_floor_div(const int num, const int den) {   // den > 0
  int q = num / den;
  if (num - q * den < 0) --q;
  return q;
}

template <int B>
__device__ __forceinline__ int rb_code(const int S, const int c, int& sat) {
  constexpr int kShift = B == 1 ? 1 : (B == 2 ? 3 : 5);   // log2(2 * B * B)
  if (c == 0) return -32768;
  const int num = 2 * S + c;
  int m;
  if (c == B * B)
    m = num >> kShift;   // arithmetic shift = floor
  else
    m = rb_floor_div(num, 2 * c);
  const bool hi = m > 32767, lo = m < -32767;
  sat += (int)(hi | lo);
  return hi ? 32767 : (lo ? -32767 : m);
}

template <int B, int NC, bool VEC, int U>
__global__ __launch_bounds__(256) void roibin_bin_kernel(const FramePtrs fp, const RbParams rp) {
  constexpr int C = NC * B;             // columns of a cell
  constexpr int MW = VEC ? C / 4 : C;   // mask words per row of a cell: 4 pixels' bytes, or one pixel's
  static_assert(!VEC || C % 4 == 0, "a vector cell is whole float4");
  __shared__ int s_red[4];
  const int f = blockIdx.y;
  const int cnt = gin<int>(rp.counts)[f];
  if (blockIdx.x == 0) rb_header(rp, f, cnt, s_red);
  if (cnt < rp.min_peaks) return;   // workgroup-uniform: a skipped frame is neither read nor written
  const PR_GLOBAL float* frame = gin<float>(fp.in[f]);
  const PR_GLOBAL unsigned char* mask = gin<unsigned char>(rp.mask);
  PR_GLOBAL unsigned short* codes = gout<unsigned short>(rp.codes) + (int64_t)f * rp.P * rp.Hb * rp.Wb;
  const float qnan = __int_as_float(0x7FC00000);
  int sat = 0;
  const uint32_t step = gridDim.x * 256u * U;   // <= T + 256 U: c0 stays below 2^32
  for (uint32_t c0 = blockIdx.x * 256u * U; c0 < rp.T; c0 += step) {
    float v[U][B][C];
    uint32_t m[U][B][MW];
    int64_t dst[U];   // the cell's first code, -1 = no cell
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint32_t c = c0 + u * 256u + threadIdx.x;
      const bool live = c < rp.T;
      const uint32_t cc = live ? c : 0u;
      const uint32_t r = rb_div(cc, rp.dCw), xc = cc - r * rp.Cw;     // r = p * Hb + yb
      const uint32_t p = rb_div(r, rp.dHb), yb = r - p * rp.Hb;
      const int y0 = (int)yb * B, x0 = (int)xc * C;
      const int64_t base = ((int64_t)p * rp.H + y0) * rp.W + x0;
      dst[u] = live ? (int64_t)r * rp.Wb + (int64_t)xc * NC : -1;
#pragma unroll
      for (int dy = 0; dy < B; ++dy) {
        const bool row = live && y0 + dy < rp.H;
        const int64_t o = base + (int64_t)dy * rp.W;
        if constexpr (VEC) {
#pragma unroll
          for (int k = 0; k < MW; ++k) {   // W % 4 == 0 and C | 4-column grid: the float4 is inside the row
            const f32x4_t q = row ? ld_nt_f4(reinterpret_cast<const PR_GLOBAL f32x4_t*>(frame + o) + k)
                                  : f32x4_t{qnan, qnan, qnan, qnan};
            v[u][dy][4 * k + 0] = q.x; v[u][dy][4 * k + 1] = q.y;
            v[u][dy][4 * k + 2] = q.z; v[u][dy][4 * k + 3] = q.w;
            m[u][dy][k] = row ? (rp.mask != 0 ? reinterpret_cast<const PR_GLOBAL uint32_t*>(mask + o)[k] : 0x01010101u) : 0u;
          }
        } else {
#pragma unroll
          for (int dx = 0; dx < C; ++dx) {
            const bool in = row && x0 + dx < rp.W;
            v[u][dy][dx] = in ? frame[o + dx] : qnan;
            m[u][dy][dx] = in ? (rp.mask != 0 ? (uint32_t)mask[o + dx] : 1u) : 0u;
          }
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      int code[NC];
#pragma unroll
      for (int k = 0; k < NC; ++k) {
        int S = 0, c = 0;
#pragma unroll
        for (int dy = 0; dy < B; ++dy) {
#pragma unroll
          for (int dx = 0; dx < B; ++dx) {
            const int col = k * B + dx;
            const uint32_t mb = VEC ? (m[u][dy][col / 4] >> (8 * (col % 4))) & 0xFFu : m[u][dy][col];
            const float x = v[u][dy][col];
            const bool ok = (mb != 0u) & (x >= rp.vmin) & (x <= rp.vmax);
            S += (int)rintf((ok ? x : 0.0f) * rp.inv);
            c += (int)ok;
          }
        }
        code[k] = rb_code<B>(S, c, sat) & 0xFFFF;
      }
      if (dst[u] >= 0) {
        if constexpr (NC == 4)
          *reinterpret_cast<PR_GLOBAL u32x2_t*>(codes + dst[u]) =
              u32x2_t{(unsigned)(code[0] | (code[1] << 16)), (unsigned)(code[2] | (code[3] << 16))};
        else if constexpr (NC == 2)
          *reinterpret_cast<PR_GLOBAL uint32_t*>(codes + dst[u]) = (unsigned)(code[0] | (code[1] << 16));
        else
          codes[dst[u]] = (unsigned short)code[0];
      }   // a lane without a cell read NaN with mask 0: c == 0, nothing clamped
    }
  }
  sat = rb_block_sum(sat, s_red);
  if (threadIdx.x == 0u && sat != 0)
    __hip_atomic_fetch_add(gout<int>(rp.nsat) + f, sat, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

constexpr int kRbMaxPeaks = kRoibinMaxPeaks;

__global__ __launch_bounds__(256) void roibin_box_kernel(const FramePtrs fp, const RbParams rp, const int nframes,
                                                         const int R, long long* __restrict__ offs,
                                                         int* __restrict__ ctr_out, uint32_t* __restrict__ rec_out,
                                                         uint32_t* __restrict__ box_out) {
  __shared__ unsigned long long s_key[kRbMaxPeaks];
  __shared__ unsigned s_off[kMaxFrames + 1];
  __shared__ int s_red[4];
  const uint32_t t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  const int f = blockIdx.x;
  if (w == 0) {
    // the batch's offsets, rebuilt by every workgroup (F <= 64); a word the bin kernel did not write
    // cannot take a box past F * max_peaks
    int nb = lane < nframes ? gin<int>(rp.nbox)[lane] : 0;
    nb = nb < 0 ? 0 : (nb > rp.max_peaks ? rp.max_peaks : nb);
    unsigned incl = (unsigned)nb;
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
      const unsigned y = __shfl_up(incl, d, 64);
      if (lane >= d) incl += y;
    }
    s_off[lane + 1] = incl;
    if (lane == 0) s_off[0] = 0u;
    if (f == 0) {
      if (lane < nframes) offs[lane + 1] = (long long)incl;
      if (lane == 0) offs[0] = 0ll;
    }
  }
  __syncthreads();
  const int cnt = gin<int>(rp.counts)[f];
  const int nrec = cnt > 0 ? cnt : 0;
  if (cnt < rp.min_peaks || nrec > rp.max_peaks || nrec == 0) return;   // workgroup-uniform
  const PR_GLOBAL float* recs = gin<float>(rp.peaks) + (int64_t)f * rp.max_peaks * 8;
  int npow = 1;
  while (npow < nrec) npow <<= 1;   // <= 4096
  int nval = 0;
  for (int i = t; i < npow; i += 256) {
    unsigned long long key = ~0ull;
    if (i < nrec) {
      int ctr;
      if (rb_valid(rp, recs + (int64_t)i * 8, ctr)) {
        key = ((unsigned long long)(unsigned)ctr << 32) | (unsigned)i;
        ++nval;
      }
    }
    s_key[i] = key;
  }
  for (int k = 2; k <= npow; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      __syncthreads();
      for (int i = t; i < npow; i += 256) {
        const int l = i ^ j;
        if (l > i) {
          const unsigned long long a = s_key[i], b = s_key[l];
          if ((a > b) == ((i & k) == 0)) {
            s_key[i] = b;
            s_key[l] = a;
          }
        }
      }
    }
  nval = rb_block_sum(nval, s_red);   // its barriers also end the sort
  const int room = (int)(s_off[f + 1] - s_off[f]);
  const int nb = nval < room ? nval : room;   // equal after the bin kernel of this batch
  const int64_t o0 = (int64_t)s_off[f];
  const int Wn = 2 * R + 1, A = Wn * Wn;            // A <= 225
  const unsigned magic = 65536u / (unsigned)Wn + 1u;   // e / Wn = (e * magic) >> 16 for e < 256, Wn <= 15
  const PR_GLOBAL uint32_t* frame = gin<uint32_t>(fp.in[f]);
  const int HW = rp.H * rp.W;
  for (int j = w; j < nb; j += 4) {   // one wave per box
    const unsigned long long key = s_key[j];
    const int ctr = (int)(key >> 32), slot = (int)(key & 0xFFFFFFFFull);
    const int p = ctr / HW, rem = ctr - p * HW;
    const int y = rem / rp.W, x = rem - y * rp.W;
    if (lane == 0) ctr_out[o0 + j] = ctr;
    if (lane < 8) rec_out[(o0 + j) * 8 + lane] = reinterpret_cast<const PR_GLOBAL uint32_t*>(recs)[(int64_t)slot * 8 + lane];
    for (int e = lane; e < A; e += 64) {
      const int dy = (int)(((unsigned)e * magic) >> 16), dx = e - dy * Wn;
      const int yy = y + dy - R, xx = x + dx - R;
      const bool in = yy >= 0 && yy < rp.H && xx >= 0 && xx < rp.W;
      box_out[(o0 + j) * A + e] = in ? frame[((int64_t)p * rp.H + yy) * rp.W + xx] : 0x7FC00000u;
    }
  }
}

template <int B, int NC, bool VEC, int U>
static void rb_launch_bin(const FramePtrs& fp, RbParams rp, int nframes, hipStream_t s) {
  rp.Cw = (rp.Wb + NC - 1) / NC;
  rp.T = (uint32_t)((int64_t)rp.P * rp.Hb * rp.Cw);
  rp.dCw = rb_div_make((uint32_t)rp.Cw);
  rp.dHb = rb_div_make((uint32_t)rp.Hb);
  const uint32_t per = 256u * U;
  const dim3 grid((rp.T + per - 1) / per, (unsigned)nframes);
  hipLaunchKernelGGL((roibin_bin_kernel<B, NC, VEC, U>), grid, dim3(256), 0, s, fp, rp);
}

void launch_roibin(const FramePtrs& fp, int nframes, int P, int H, int W, int B, float inv, float vmin, float vmax,
                   int R, int min_peaks, int max_peaks, uint64_t mask, uint64_t peaks, uint64_t counts, uint64_t codes,
                   uint64_t npk, uint64_t nbox, uint64_t nbad, uint64_t nsat, uint64_t flags, uint64_t offs,
                   uint64_t ctr, uint64_t rec, uint64_t box, uint64_t stream, int phases) {
  check(phases >= 1 && phases <= 3, "roibin: phases must be 1 (bin), 2 (boxes) or 3");
  check_nframes(nframes, "roibin");
  check(P >= 1 && H >= 1 && W >= 1 && (int64_t)P * H * W < (int64_t)1 << 31, "roibin: frame shape out of range");
  check(B == 1 || B == 2 || B == 4, "roibin: bin must be 1, 2 or 4");
  check(R >= 0 && R <= kRoibinMaxRadius, "roibin: box radius out of range");
  check(max_peaks >= 1 && max_peaks <= kRoibinMaxPeaks, "roibin: max_peaks out of range");
  check(min_peaks >= 0, "roibin: min_peaks must be >= 0");
  check(std::isfinite(vmin) && std::isfinite(vmax) && vmin <= vmax, "roibin: the value window must be finite, vmin <= vmax");
  check(std::isfinite(inv) && inv > 0.0f && std::fmax(std::fabs(vmin), std::fabs(vmax)) * inv < 33554432.0f,
        "roibin: max(|vmin|, |vmax|) * inv must stay below 2^25");
  check(mask % 4 == 0, "roibin: the mask must be 4-B aligned");
  check(peaks != 0 && counts != 0 && peaks % 4 == 0 && counts % 4 == 0, "roibin: misaligned or missing peaks / counts");
  check(codes != 0 && codes % 8 == 0, "roibin: codes must be 8-B aligned");
  check(npk != 0 && nbox != 0 && nbad != 0 && nsat != 0 && flags != 0 && offs != 0 && ctr != 0 && rec != 0 && box != 0 &&
            npk % 4 == 0 && nbox % 4 == 0 && nbad % 4 == 0 && nsat % 4 == 0 && offs % 8 == 0 && ctr % 4 == 0 &&
            rec % 4 == 0 && box % 4 == 0,
        "roibin: misaligned or missing output");
  check_frames(fp, nframes, "roibin");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RbParams rp{};
  rp.inv = inv; rp.vmin = vmin; rp.vmax = vmax;
  rp.P = P; rp.H = H; rp.W = W;
  rp.Hb = (H + B - 1) / B; rp.Wb = (W + B - 1) / B;
  rp.min_peaks = min_peaks; rp.max_peaks = max_peaks;
  rp.mask = mask; rp.peaks = peaks; rp.counts = counts; rp.codes = codes;
  rp.npk = npk; rp.nbox = nbox; rp.nbad = nbad; rp.nsat = nsat; rp.flags = flags;
  if (phases & 1) {
    hip_check(hipMemsetAsync(reinterpret_cast<void*>(nsat), 0, (size_t)nframes * 4, s), "roibin clear nsat");
    const bool even = rp.Wb % 2 == 0;
    if (W % 4 == 0) {
      if (B == 1) rb_launch_bin<1, 4, true, 4>(fp, rp, nframes, s);
      else if (B == 2) rb_launch_bin<2, 2, true, 4>(fp, rp, nframes, s);
      else if (even) rb_launch_bin<4, 2, true, 1>(fp, rp, nframes, s);
      else rb_launch_bin<4, 1, true, 2>(fp, rp, nframes, s);
    } else if (even) {
      if (B == 1) rb_launch_bin<1, 2, false, 4>(fp, rp, nframes, s);
      else if (B == 2) rb_launch_bin<2, 2, false, 2>(fp, rp, nframes, s);
      else rb_launch_bin<4, 2, false, 1>(fp, rp, nframes, s);
    } else {
      if (B == 1) rb_launch_bin<1, 1, false, 4>(fp, rp, nframes, s);
      else if (B == 2) rb_launch_bin<2, 1, false, 2>(fp, rp, nframes, s);
      else rb_launch_bin<4, 1, false, 1>(fp, rp, nframes, s);
    }
    hip_check(hipGetLastError(), "roibin bin launch");
  }
  if (!(phases & 2)) return;
  hipLaunchKernelGGL(roibin_box_kernel, dim3((unsigned)nframes), dim3(256), 0, s, fp, rp, nframes, R,
                     reinterpret_cast<long long*>(offs), reinterpret_cast<int*>(ctr), reinterpret_cast<uint32_t*>(rec),
                     reinterpret_cast<uint32_t*>(box));
  hip_check(hipGetLastError(), "roibin box launch");
}

}  // namespace pr
