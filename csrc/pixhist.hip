// K-12 per-pixel histograms for queue consumers: how often every pixel read every value, over a batch
// of CALIBRATED float32 frames, ADDED to a run accumulator hist int32 [n, nbins] the caller owns
// (pixel-major: one pixel's spectrum is contiguous).
//
// Numerics contract (docs/ARCHITECTURE.md, "Pixel histograms: the integer contract"): every word is an
// INTEGER function of the inputs, so the result does not depend on frame order, batch split or stream,
// is word-for-word equal to the golden model (ops/reference.py pixel_hist_reference) and two consumers'
// accumulators add to exactly what one would have produced.
//   contributes   lo <= v && v <= hi as float32 (NaN fails, +-inf is outside the finite window)
//   bin           b = min(nbins - 1, (int) floorf((v - lo) * inv_w)): a float32 subtraction, then a float32
//                 multiply, each rounded to nearest and NOT contracted (the build passes -ffp-contract=off);
//                 inv_w = float32(nbins / (hi - lo)) comes from the host.  v - lo >= 0, the last bin is
//                 closed on the right, -0.0 with lo = 0 goes to bin 0.
//   hist[p, b] += 1 (int32)
// A bin gains at most 1 per frame: the callers hold a run at or below 2^31 - 1 frames, so no word
// overflows.  The kernel never clears the accumulator.
//
// MI355X design.  The accumulator is nbins times larger than a frame and a lane cannot keep 4 pixels x
// nbins counters in registers, so the in-launch histogram lives in LDS.  A 256-thread workgroup owns a
// TILE of T consecutive pixels (T a power of two from nbins, 64 .. 1024, so that T * ceil(nbins / 4)
// words fit 64 KiB: two workgroups per CU) and streams the launch's frames over it: 16-B non-temporal
// loads, 8 (then 4, then 1) in flight per lane, as powder_kernel does.  The tile's T / 4 quads of pixels
// go to the threads' low bits and the frames to the high bits, so a small tile (many bins) still keeps
// all 256 threads loading; with T >= 256 the frame index is wave-uniform and the frame pointers come by
// scalar loads.
//   LDS counters  BYTE counters packed four to a word: a launch has at most 64 frames, so a byte never
//                 passes 64 and ONE no-return ds_add_u32 of 1 << 8 * (b & 3) on word b >> 2 adds a
//                 sample without a carry into the neighbouring byte.  LDS atomics, because with T < 1024
//                 several threads (other frames) add to the same pixel.
//   layout        pixel 4 * q + i of the tile is ROW i * (T / 4) + q, so the 64 lanes of a wave, which
//                 hold 64 consecutive quads, hit 64 consecutive rows with their i-th sample.  Neighbouring
//                 pixels mostly fall into the same bin: the row pitch is padded to an ODD number of words
//                 (layout 0), which spreads those 64 rows over the 64 banks.  Layouts 1 (word-major: word w
//                 of row r at w * T + r) and 2 (unpadded pitch) exist for the A/B in profiles/hist/ only;
//                 measured, 0 and 2 are equal within 0.3 % and 1 is 0 - 8 % slower: the kernel waits on
//                 memory, not on the LDS.
//   flush         after the frame loop the threads walk the tile's words in the accumulator's order:
//                 consecutive lanes take consecutive words of a pixel's row, unpack 4 counts and do ONE 16-B
//                 read-modify-write of hist.  A lane whose word is zero touches no memory, so lines of the
//                 accumulator no sample fell into are neither read nor written.  The tile's part of hist is
//                 addressed as a BUFFER whose range check does that skip: such a lane's offset lies past
//                 the buffer's end, the load returns 0 and the store is dropped.  The pass therefore has no
//                 branch and a lane has 8 reads of hist in flight before its first write; with a branch
//                 around each access the compiler waits for every access in turn, and the kernel took
//                 1.5 x (64 bins) to 2.2 x (256 bins) as long.  nbins % 4 != 0 leaves a row's words 4-B
//                 aligned only: scalar accesses there, one per non-zero count.
//   tails         the last tile is partial; the n % 4 last pixels of a frame are read with scalar loads.
// One workgroup owns a pixel per launch and there are no global atomics: two launches in flight must
// not share an accumulator.
//
// Compiler's resource usage (hipcc -O3 --offload-arch=gfx950, -Rpass-analysis=kernel-resource-usage):
// pixel_hist_kernel: 60 VGPRs, 60 SGPRs, no scratch memory (0 bytes per lane, no spills), 69632 B of LDS
// per workgroup (1024 rows of 17 words: two workgroups per CU), occupancy 2 waves per SIMD, set by the
// LDS.  The frames come by global_load_dwordx4 nt, the counters by ds_add_u32 without return, hist by
// buffer_load_dwordx4 / buffer_store_dwordx4.
#include <cmath>

#include "common.h"
#include "kernels.h"
#include "launch.h"

namespace pr {

constexpr int kHistBlock = 256;
constexpr int kHistFlush = 8;   // chunks of the flush a lane has in flight
constexpr int kHistNowhere = 0x7FFFFF00;   // a byte offset past the end of any tile's part of hist
constexpr int kHistTileWords = 16384;   // T * ceil(nbins / 4) <= 64 KiB
constexpr int kHistMaxTile = 1024;
// the largest padded tile: 1024 rows of 16 + 1 words (57 .. 64 bins)
constexpr int kHistLdsWords = kHistMaxTile * 17;

struct HistParams {
  float lo, hi, inv_w;
  int nbins;
  int W;        // words per row: ceil(nbins / 4)
  int lq;       // log2(T / 4): the quads of a tile
  int rs, ws;   // LDS word of (row r, word w) = r * rs + w * ws
  int dq, dr;   // 256 / W and 256 % W: the flush's step
  int zero4;    // 16-B words of LDS to clear
};

__device__ __forceinline__ void ph_add(uint32_t* lds, const int base, const float v, const HistParams& hp) {
  if (v >= hp.lo && v <= hp.hi) {
    const float d = v - hp.lo;        // float32, rounded to nearest
    const float x = d * hp.inv_w;     // float32, rounded to nearest; never fused with the subtraction
    const int b = min(hp.nbins - 1, (int)floorf(x));
    (void)__hip_atomic_fetch_add(lds + base + (b >> 2) * hp.ws, 1u << ((b & 3) * 8), __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_WORKGROUP);
  }
}

// K frames f, f + G, ... of one quad with K loads in flight
template <int K>
__device__ __forceinline__ void ph_group(uint32_t* lds, const int (&base)[4], const FramePtrs& fp, const int f,
                                         const int G, const int64_t q16, const HistParams& hp) {
  f32x4_t r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = ld_nt_f4(gin<f32x4_t>(fp.in[f + k * G]) + q16);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    ph_add(lds, base[0], r[k].x, hp);
    ph_add(lds, base[1], r[k].y, hp);
    ph_add(lds, base[2], r[k].z, hp);
    ph_add(lds, base[3], r[k].w, hp);
  }
}

// the frames g, g + G, ... < F of one whole quad
__device__ __forceinline__ void ph_walk(uint32_t* lds, const int (&base)[4], const FramePtrs& fp, const int g,
                                        const int G, const int F, const int64_t q16, const HistParams& hp) {
  int f = g;
  for (; f + 7 * G < F; f += 8 * G) ph_group<8>(lds, base, fp, f, G, q16, hp);
  if (f + 3 * G < F) {
    ph_group<4>(lds, base, fp, f, G, q16, hp);
    f += 4 * G;
  }
  for (; f < F; f += G) ph_group<1>(lds, base, fp, f, G, q16, hp);
}

__global__ __launch_bounds__(kHistBlock) void pixel_hist_kernel(const FramePtrs fp, const int nframes, const int64_t n,
                                                                const HistParams hp, int32_t* __restrict__ hist) {
  __shared__ __attribute__((aligned(16))) uint32_t lds[kHistLdsWords];
  const int t = (int)threadIdx.x;
  {
    const u32x4_t z = {0u, 0u, 0u, 0u};
    for (int i = t; i < hp.zero4; i += kHistBlock) reinterpret_cast<u32x4_t*>(lds)[i] = z;
  }
  __syncthreads();

  const int Q = 1 << hp.lq;   // quads of the tile (16 .. 256); T = 4 * Q
  const int64_t p0 = (int64_t)blockIdx.x * (4 * Q);
  const int64_t left = n - p0;   // >= 1: pixels from the tile's first to the frame's end
  {
    const int q = t & (Q - 1);
    const int G = kHistBlock >> hp.lq;   // threads per quad: each takes every G-th frame
    int g = t >> hp.lq;
    const int64_t pix = p0 + 4 * (int64_t)q;
    int base[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) base[i] = ((i << hp.lq) + q) * hp.rs;
    if (4 * q + 3 < left) {
      const int64_t q16 = pix >> 2;
      if (Q >= kWave) {
        g = __builtin_amdgcn_readfirstlane(g);   // a wave holds 64 quads of ONE frame group
        ph_walk(lds, base, fp, g, G, nframes, q16, hp);
      } else {
        ph_walk(lds, base, fp, g, G, nframes, q16, hp);
      }
    } else if (4 * q < left) {
      // the frame's last n % 4 pixels
      for (int f = g; f < nframes; f += G) {
        const PR_GLOBAL float* in = gin<float>(fp.in[f]);
#pragma unroll
        for (int i = 0; i < 3; ++i)
          if (4 * q + i < left) ph_add(lds, base[i], in[pix + i], hp);
      }
    }
  }
  __syncthreads();

  // flush: chunk c = p * W + w is word w of the tile's pixel p; the chunks are consecutive in hist
  const int rows = (int)(left < (int64_t)(4 * Q) ? left : (int64_t)(4 * Q));
  const bool vec = (hp.nbins & 3) == 0;
  int p = t / hp.W, w = t - p * hp.W;
  PR_GLOBAL int32_t* const hbase = gout<int32_t>((uint64_t)hist) + p0 * hp.nbins;
  if (vec) {
    // The tile's words of hist as a buffer: a lane with nothing to add gives an offset past the buffer's
    // end, for which the hardware returns 0 and drops the store WITHOUT touching memory.  That keeps
    // the pass free of branches, so kHistFlush reads of hist are in flight per lane before the first
    // write (with a branch around each access the compiler waits for every one of them in turn).
    const __amdgpu_buffer_rsrc_t rsrc =
        __builtin_amdgcn_make_buffer_rsrc((void*)(hist + p0 * hp.nbins), 0, rows * hp.nbins * 4, 0x00020000);
    while (p < rows) {
      uint32_t c[kHistFlush];
      int o[kHistFlush];   // byte offset in the tile's part of hist
      u32x4_t v[kHistFlush];
#pragma unroll
      for (int u = 0; u < kHistFlush; ++u) {
        c[u] = 0u;
        if (p < rows) c[u] = lds[(((p & 3) << hp.lq) + (p >> 2)) * hp.rs + w * hp.ws];
        o[u] = c[u] != 0u ? (p * hp.nbins + 4 * w) * 4 : kHistNowhere;
        p += hp.dq;
        w += hp.dr;
        if (w >= hp.W) {
          w -= hp.W;
          ++p;
        }
      }
#pragma unroll
      for (int u = 0; u < kHistFlush; ++u) v[u] = __builtin_amdgcn_raw_buffer_load_b128(rsrc, o[u], 0, 0);
#pragma unroll
      for (int u = 0; u < kHistFlush; ++u) {
        v[u].x += c[u] & 0xFFu;
        v[u].y += (c[u] >> 8) & 0xFFu;
        v[u].z += (c[u] >> 16) & 0xFFu;
        v[u].w += c[u] >> 24;
        __builtin_amdgcn_raw_buffer_store_b128(v[u], rsrc, o[u], 0, 0);
      }
    }
  } else {
    for (; p < rows; p += hp.dq) {
      const uint32_t c = lds[(((p & 3) << hp.lq) + (p >> 2)) * hp.rs + w * hp.ws];
      // bins past nbins - 1 of the row's last word never get a sample: their bytes are 0
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t ck = (c >> (8 * k)) & 0xFFu;
        if (ck != 0u) hbase[p * hp.nbins + 4 * w + k] += (int32_t)ck;
      }
      w += hp.dr;
      if (w >= hp.W) {
        w -= hp.W;
        ++p;
      }
    }
  }
}

int pixel_hist_tile_pixels(int nbins) {
  check(nbins >= 1 && nbins <= kHistMaxBins, "pixel_hist: nbins outside [1, 1024]");
  const int W = (nbins + 3) / 4;
  int T = kHistMaxTile;
  while (T * W > kHistTileWords) T >>= 1;
  return T;
}

void launch_pixel_hist(const FramePtrs& fp, int nframes, int64_t n, float lo, float hi, float inv_w, int nbins,
                       uint64_t hist, uint64_t stream, int layout) {
  check_nframes(nframes, "pixel_hist");
  check(nbins >= 1 && nbins <= kHistMaxBins, "pixel_hist: nbins outside [1, 1024]");
  check(n >= 1 && n < (int64_t)1 << 31 && n * (int64_t)nbins < (int64_t)1 << 31,
        "pixel_hist: n * nbins must stay below 2^31");
  check(std::isfinite(lo) && std::isfinite(hi) && lo < hi, "pixel_hist: the window must be finite with lo < hi");
  check(std::isfinite(inv_w) && inv_w > 0.0f, "pixel_hist: the scale must be finite and positive");
  check(hist != 0 && aligned16(hist), "pixel_hist: hist must be non-null and 16-B aligned");
  check(layout >= 0 && layout <= 2, "pixel_hist: layout 0, 1 or 2");
  check_frames(fp, nframes, "pixel_hist");
  const int T = pixel_hist_tile_pixels(nbins);
  HistParams hp;
  hp.lo = lo;
  hp.hi = hi;
  hp.inv_w = inv_w;
  hp.nbins = nbins;
  hp.W = (nbins + 3) / 4;
  hp.lq = 0;
  while ((4 << hp.lq) < T) ++hp.lq;
  if (layout == 1) {
    hp.rs = 1;
    hp.ws = T;
  } else {
    hp.rs = layout == 0 ? (hp.W | 1) : hp.W;
    hp.ws = 1;
  }
  hp.dq = kHistBlock / hp.W;
  hp.dr = kHistBlock % hp.W;
  const int words = layout == 1 ? hp.W * T : T * hp.rs;   // T is a multiple of 64
  check(words <= kHistLdsWords && words % 4 == 0, "pixel_hist: tile does not fit the LDS");
  hp.zero4 = words / 4;
  const dim3 grid((unsigned)((n + T - 1) / T));
  hipLaunchKernelGGL(pixel_hist_kernel, grid, dim3(kHistBlock), 0, reinterpret_cast<hipStream_t>(stream), fp, nframes, n,
                     hp, reinterpret_cast<int32_t*>(hist));
  hip_check(hipGetLastError(), "pixel_hist launch");
}

}  // namespace pr
