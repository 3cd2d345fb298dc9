// K-10 on-GPU zero suppression for queue consumers: the (pixel index, value) pairs of every frame of
// a batch whose calibrated value lies in a window, packed frame after frame in index order.
//
// Contract (docs/ARCHITECTURE.md, "Sparse frames"; golden model ops/reference.py sparsify_reference):
//   kept          (mask absent or mask[i] != 0) and thr <= v and v <= vmax   (NaN fails, +-inf is
//                 outside a finite window, -0.0 is kept iff thr <= 0 and keeps its sign bit)
//   processed     keys absent or keys[f] >= key_min; otherwise SKIPPED: nnz[f] = 0, flag bit 1
//   nnz[f]        exact number of kept pixels, also past cap;  flags[f] bit 0 = nnz[f] > cap
//   stored[f]     nnz[f] if nnz[f] <= cap, else 0 (an overflowing frame stores nothing)
//   offs[F + 1]   int64 exclusive scan of stored;  pix / val [offs[f] .. offs[f + 1]) = frame f's kept
//                 pixels, linear indices strictly ascending, values as bit copies
// Every output word is a function of the inputs alone: nothing depends on workgroup order.
//
// MI355X design, two launches per batch, frames read once:
//   sparse_scan_kernel   one resident wave of workgroups walks the batch's (frame, 16-KB chunk)
//     sequence, the next chunk's 16-B non-temporal loads in flight (the schedule of radial_kernel).
//     Keep bits go through __ballot, the in-wave rank is mbcnt, the 16 (float4 row, wave) totals of
//     a chunk go through LDS: a chunk's kept pixels are laid out in ascending index order.  Thread 0
//     reserves a segment of the frame's staging row [cap] with ONE relaxed agent-scope atomicAdd of
//     the chunk's count on the frame's cursor and records (offset, count) in the directory
//     [F, chunks per frame]; the chunk writes its segment only when the reservation ends within cap.
//     Counts are always added, so the cursor ends as the exact nnz.  A chunk without a kept pixel
//     does no atomic and takes one barrier instead of two.  The n % 4 tail is walked by thread 0 of
//     the frame's last chunk.  A skipped frame's chunks are dropped on a workgroup-uniform keys[f].
//   sparse_pack_kernel   touches the sparse data only: every workgroup rebuilds stored / offs from
//     the F cursors, takes the exclusive scan of its frame's directory counts and copies each
//     segment to offs[f] + prefix[chunk] -- canonical, whatever order the reservations arrived in.
// No workgroup waits for another: ordering between the phases is the kernel boundary.  The cursors
// are cleared by a memset on the stream; every directory entry of a processed frame is written by
// the scan, so nothing else needs clearing.  Nothing is written past F * cap elements of pix / val
// or outside the scratch block.
//
// Resources (hipcc -O3, gfx950): sparse_scan_kernel 84 VGPRs (5 waves per SIMD), sparse_pack_kernel
// 45 VGPRs, no scratch memory (private spills), 132 B / 4.3 KiB of LDS (asking for 6 waves per SIMD
// makes the scan spill 28 B per lane).
//
// Measured on the MI355X (profiles/sparse/README.md): epix10k2M calib frames, 64-frame batch, default
// cap n / 16, us/frame, median of five interleaved rounds in one process, two runs.
//   kept pixels     sparsify        of which pack   read_f32 floor   radial (1024 bins)
//   0.02 %          1.863 / 1.814   0.099 / 0.098   1.724 / 1.731    1.822 / 1.770
//   0.99 %          3.221 / 3.233   0.163 / 0.165
//   5.00 %          3.494 / 3.505   0.385 / 0.384
//   all skipped     0.616 / 0.600
// At 0.02 % clear + scan run at the read floor; the distance to the radial row (2.5 %) is the pack
// launch.  From 1 % on every chunk holds a kept pixel and pays the reservation (atomic, second
// barrier, directory entry, scattered stores): the cost is per chunk, not per pixel (5 x the pixels
// cost 0.05 more).
#include "common.h"
#include "kernels.h"
#include "launch.h"

#include <algorithm>
#include <cmath>

namespace pr {

constexpr int kSpK = 4;   // float4 per lane per chunk
static_assert(256 * kSpK * 4 == kSparseChunk, "chunk = 256 lanes x kSpK float4");

struct SpParams {
  float thr, vmax;
  int cap;            // entries per frame in the staging rows
  int key_min;
  int64_t n;          // elements per frame
  uint64_t mask;      // uint8 [n] or 0
  uint64_t keys;      // int32 [F] or 0
  uint64_t cursor;    // uint32 [kMaxFrames]
  uint64_t dir;       // uint2 [F, ncpf]: (offset in the frame's staging row, count)
  uint64_t spix;      // int32 [F, cap]
  uint64_t sval;      // float [F, cap]
};

__device__ __forceinline__ bool sp_live(const SpParams& sp, int f) {
  return sp.keys == 0 || gin<int>(sp.keys)[f] >= sp.key_min;
}

__device__ __forceinline__ unsigned sp_lane_rank(unsigned long long b) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
}

__global__ __launch_bounds__(256) void sparse_scan_kernel(const FramePtrs fp, const SpParams sp, const int nframes) {
  constexpr int K = kSpK;
  __shared__ unsigned s_tot[2][4 * K];   // (row k, wave w) totals, double-buffered by chunk parity
  __shared__ unsigned s_base;
  const int64_t n4 = sp.n / 4;
  const int ncpf = n4 > 0 ? (int)((n4 + 256 * K - 1) / (256 * K)) : 1;   // a frame of < 4 elements is all tail
  const int64_t T = (int64_t)ncpf * nframes;
  const int64_t g0 = T * blockIdx.x / gridDim.x, g1 = T * (blockIdx.x + 1) / gridDim.x;
  const uint32_t t = threadIdx.x;
  const int w = t >> 6;
  const PR_GLOBAL unsigned char* mask = gin<unsigned char>(sp.mask);
  // keys[f] is read once per frame and stage (the loads run two chunks ahead of the compaction): a
  // range of skipped chunks then costs no dependent scalar load per chunk
  int lf = -1, cf = -1;
  bool llive = true, clive = true;
  // chunk g: K float4 of the frame and the mask bytes of the same elements; a float4 past the
  // frame's last whole one, or of a skipped frame, gets mask 0 (nothing is loaded)
  auto load_to = [&](f32x4_t(&v)[K], uint32_t(&m)[K], int64_t g) {
    const int f = (int)(g / ncpf);
    const int64_t c0 = (g - (int64_t)f * ncpf) * 256 * K;   // first float4 of the chunk (uniform)
    const PR_GLOBAL f32x4_t* cp = reinterpret_cast<const PR_GLOBAL f32x4_t*>(gin<float>(fp.in[f])) + c0;
    const PR_GLOBAL uint32_t* mp = reinterpret_cast<const PR_GLOBAL uint32_t*>(mask) + c0;
    if (f != lf) {
      lf = f;
      llive = sp_live(sp, f);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const bool in = llive && c0 + t + 256 * k < n4;
      v[k] = in ? ld_nt_f4(cp + t + 256 * k) : f32x4_t{0.0f, 0.0f, 0.0f, 0.0f};
      m[k] = in ? (sp.mask != 0 ? mp[t + 256 * k] : 0x01010101u) : 0u;
    }
  };
  int par = 0;
  auto keep = [&](float v, uint32_t mbyte) { return mbyte != 0u && v >= sp.thr && v <= sp.vmax; };
  auto chunk = [&](f32x4_t(&v)[K], uint32_t(&m)[K], int64_t g) {
    const int f = (int)(g / ncpf);   // workgroup-uniform
    if (f != cf) {
      cf = f;
      clive = sp_live(sp, f);
    }
    if (!clive) return;
    const int c = (int)(g - (int64_t)f * ncpf);
    // alternates over the chunks that reach the barrier below: a wave may still read the totals of
    // the previous such chunk while another, one barrier ahead, writes this one's
    par ^= 1;
    unsigned kb[K];     // keep bits of the lane's 4 pixels of row k
    unsigned rank[K];   // kept pixels of row k in the wave's lower lanes
#pragma unroll
    for (int k = 0; k < K; ++k) {
      unsigned r = 0u, tot = 0u;
      kb[k] = 0u;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const bool kp = keep(v[k][e], (m[k] >> (8 * e)) & 0xFFu);
        const unsigned long long b = __ballot(kp);
        r += sp_lane_rank(b);
        tot += (unsigned)__popcll(b);
        kb[k] |= (unsigned)kp << e;
      }
      rank[k] = r;
      if ((t & 63u) == 0u) s_tot[par][k * 4 + w] = tot;
    }
    __syncthreads();
    // pre[k]: kept pixels of the chunk before this wave's part of row k (rows before k, then the
    // row's lower waves)
    unsigned pre[K], total = 0u;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      pre[k] = total;
#pragma unroll
      for (int ww = 0; ww < 4; ++ww) {
        const unsigned x = s_tot[par][k * 4 + ww];
        if (ww < w) pre[k] += x;
        total += x;
      }
    }
    const bool last = c == ncpf - 1;
    const int ntail = last ? (int)(sp.n - 4 * n4) : 0;
    if (total == 0u && ntail == 0) {   // workgroup-uniform: no atomic, one barrier
      if (t == 0u) gout<u32x2_t>(sp.dir)[(int64_t)f * ncpf + c] = u32x2_t{0u, 0u};
      return;
    }
    const PR_GLOBAL float* frame = gin<float>(fp.in[f]);
    unsigned tk = 0u;   // thread 0: keep bits of the n % 4 tail
    if (t == 0u) {
      for (int e = 0; e < ntail; ++e) {
        const int64_t i = 4 * n4 + e;
        tk |= (unsigned)keep(frame[i], sp.mask != 0 ? (uint32_t)mask[i] : 1u) << e;
      }
      const unsigned cnt = total + (unsigned)__popc(tk);
      unsigned base = 0u;
      if (cnt != 0u)
        base = __hip_atomic_fetch_add(gout<unsigned>(sp.cursor) + f, cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      gout<u32x2_t>(sp.dir)[(int64_t)f * ncpf + c] = u32x2_t{base, cnt};
      // cnt <= n < 2^31 and base + cnt <= n: no wrap
      s_base = (cnt != 0u && base + cnt <= (unsigned)sp.cap) ? base : 0xFFFFFFFFu;
    }
    __syncthreads();
    const unsigned base = s_base;
    if (base == 0xFFFFFFFFu) return;   // nothing kept, or the frame overflows: store nothing
    PR_GLOBAL int* spix = gout<int>(sp.spix) + (int64_t)f * sp.cap + base;
    PR_GLOBAL float* sval = gout<float>(sp.sval) + (int64_t)f * sp.cap + base;
    const int64_t c0 = (int64_t)c * 256 * K;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      unsigned o = pre[k] + rank[k];
      const int i0 = (int)(4 * (c0 + t + 256 * k));
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if ((kb[k] >> e) & 1u) {
          spix[o] = i0 + e;
          sval[o] = v[k][e];
          ++o;
        }
    }
    if (t == 0u) {
      unsigned o = total;
      for (int e = 0; e < ntail; ++e)
        if ((tk >> e) & 1u) {
          const int64_t i = 4 * n4 + e;
          spix[o] = (int)i;
          sval[o] = frame[i];
          ++o;
        }
    }
  };
  f32x4_t va[K], vb[K];
  uint32_t ma[K], mb[K];
  if (g0 < g1) load_to(va, ma, g0);
  for (int64_t g = g0; g < g1; g += 2) {
    if (g + 1 < g1) load_to(vb, mb, g + 1);
    chunk(va, ma, g);
    if (g + 1 < g1) {
      if (g + 2 < g1) load_to(va, ma, g + 2);
      chunk(vb, mb, g + 1);
    }
  }
}

// inclusive scan over the 64 lanes of a wave
__device__ __forceinline__ unsigned sp_wave_incl(unsigned x) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d *= 2) {
    const unsigned y = __shfl_up(x, d, 64);
    if (lane >= d) x += y;
  }
  return x;
}

// grid (kSpPackBlocks or fewer, F): block (bx, f) packs a contiguous range of frame f's chunks
__global__ __launch_bounds__(256) void sparse_pack_kernel(const SpParams sp, const int nframes, const int ncpf,
                                                          int* __restrict__ nnz, unsigned char* __restrict__ flags,
                                                          long long* __restrict__ offs, int* __restrict__ pix,
                                                          float* __restrict__ val) {
  __shared__ unsigned s_off[kMaxFrames + 1];
  __shared__ unsigned s_w[4];
  __shared__ uint4 s_ent[256];   // (source offset, count, destination offset, -)
  const uint32_t t = threadIdx.x;
  const int lane = t & 63, w = t >> 6;
  const int f = blockIdx.y;
  const unsigned cap = (unsigned)sp.cap;
  const PR_GLOBAL unsigned* cursor = gin<unsigned>(sp.cursor);
  if (w == 0) {
    // stored[] and the batch-level offsets, rebuilt by every workgroup (F <= 64; F * cap < 2^31)
    const unsigned c = lane < nframes ? cursor[lane] : 0u;
    const unsigned st = c <= cap ? c : 0u;
    const unsigned incl = sp_wave_incl(st);
    s_off[lane + 1] = incl;
    if (lane == 0) s_off[0] = 0u;
    if (blockIdx.x == 0 && blockIdx.y == 0) {
      if (lane < nframes) {
        nnz[lane] = (int)c;
        flags[lane] = (unsigned char)((c > cap ? 1u : 0u) | (sp_live(sp, lane) ? 0u : 2u));
        offs[lane + 1] = (long long)incl;
      }
      if (lane == 0) offs[0] = 0ll;
    }
  }
  __syncthreads();
  const unsigned cf = cursor[f];
  if (cf == 0u || cf > cap) return;   // empty, skipped or overflowing frame: nothing to copy
  const int c_lo = (int)((int64_t)ncpf * blockIdx.x / gridDim.x);
  const int c_hi = (int)((int64_t)ncpf * (blockIdx.x + 1) / gridDim.x);
  const PR_GLOBAL u32x2_t* dir = gin<u32x2_t>(sp.dir) + (int64_t)f * ncpf;
  // kept pixels of the frame's chunks before this block's range
  unsigned part = 0u;
  for (int j = t; j < c_lo; j += 256) part += dir[j].y;
  part = sp_wave_incl(part);
  if (lane == 63) s_w[w] = part;
  __syncthreads();
  unsigned run = s_off[f] + s_w[0] + s_w[1] + s_w[2] + s_w[3];   // destination of chunk c_lo's segment
  const PR_GLOBAL int* spix = gin<int>(sp.spix) + (int64_t)f * sp.cap;
  const PR_GLOBAL float* sval = gin<float>(sp.sval) + (int64_t)f * sp.cap;
  for (int cb = c_lo; cb < c_hi; cb += 256) {
    __syncthreads();   // s_w / s_ent of the previous round have been read
    const int j = cb + (int)t;
    const u32x2_t e = j < c_hi ? dir[j] : u32x2_t{0u, 0u};
    const unsigned incl = sp_wave_incl(e.y);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    unsigned before = 0u, all = 0u;
#pragma unroll
    for (int ww = 0; ww < 4; ++ww) {
      const unsigned x = s_w[ww];
      if (ww < w) before += x;
      all += x;
    }
    s_ent[t] = make_uint4(e.x, e.y, run + before + incl - e.y, 0u);
    __syncthreads();
    // wave w copies the segments of entries w, w + 4, ...: coalesced, 64 entries per step
    const int ne = min(256, c_hi - cb);
    for (int q = w; q < ne; q += 4) {
      const uint4 se = s_ent[q];
      // never taken after a scan of this batch; keeps a stale or foreign scratch block from sending
      // a copy outside the staging row or the frame's packed range
      if (se.x + se.y > cap || se.z + se.y > s_off[f + 1]) continue;
      for (unsigned i = lane; i < se.y; i += 64u) {
        pix[se.z + i] = spix[se.x + i];
        val[se.z + i] = sval[se.x + i];
      }
    }
    run += all;
  }
}

constexpr int kSpPackBlocks = 16;   // pack workgroups per frame, at most

static int64_t sp_chunks_per_frame(int64_t n) { return std::max<int64_t>(1, (n / 4 + 256 * kSpK - 1) / (256 * kSpK)); }

static int64_t sp_dir_bytes(int64_t n, int frames) {
  return (sp_chunks_per_frame(n) * frames * 8 + 15) / 16 * 16;
}

int64_t sparsify_scratch_bytes(int64_t n, int64_t cap, int frames) {
  check_frame_size(n, "sparsify");
  check_nframes(frames, "sparsify");
  check(cap >= 1 && cap * frames < (int64_t)1 << 31, "sparsify: cap out of range");
  return kSparseScratchHeader + sp_dir_bytes(n, frames) + (int64_t)frames * cap * 8;
}

void launch_sparsify(const FramePtrs& fp, int nframes, int64_t n, float thr, float vmax, int64_t cap, uint64_t mask,
                     uint64_t keys, int key_min, uint64_t nnz, uint64_t flags, uint64_t offs, uint64_t pix,
                     uint64_t val, uint64_t scratch, int64_t scratch_bytes, uint64_t stream, int phases) {
  check(phases >= 1 && phases <= 3, "sparsify: phases must be 1 (scan), 2 (pack) or 3");
  check_nframes(nframes, "sparsify");
  check_frame_size(n, "sparsify");
  check(cap >= 1 && cap * nframes < (int64_t)1 << 31, "sparsify: cap must be >= 1 and F * cap < 2^31");
  check(std::isfinite(thr) && std::isfinite(vmax) && thr <= vmax, "sparsify: the value window must be finite, thr <= vmax");
  check(mask % 4 == 0 && keys % 4 == 0, "sparsify: mask / keys must be 4-B aligned");
  check(nnz != 0 && flags != 0 && offs != 0 && pix != 0 && val != 0 && nnz % 4 == 0 && offs % 8 == 0 && pix % 4 == 0 &&
            val % 4 == 0,
        "sparsify: misaligned or missing output");
  check(scratch != 0 && scratch % 16 == 0, "sparsify: the scratch block must be 16-B aligned");
  check(scratch_bytes >= sparsify_scratch_bytes(n, cap, nframes), "sparsify: scratch block too small");
  check_frames(fp, nframes, "sparsify");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int ncpf = (int)sp_chunks_per_frame(n);
  SpParams sp{thr, vmax, (int)cap, key_min, n, mask, keys, 0, 0, 0, 0};
  sp.cursor = scratch;
  sp.dir = scratch + kSparseScratchHeader;
  sp.spix = sp.dir + sp_dir_bytes(n, nframes);
  sp.sval = sp.spix + (uint64_t)nframes * cap * 4;
  if (phases & 1) {
    hip_check(hipMemsetAsync(reinterpret_cast<void*>(scratch), 0, kSparseScratchHeader, s), "sparsify clear cursors");
    const int64_t chunks = (int64_t)ncpf * nframes;
    const int g = (int)std::min<int64_t>(chunks, resident_blocks((const void*)sparse_scan_kernel, 0, "sparsify"));
    hipLaunchKernelGGL(sparse_scan_kernel, dim3(g), dim3(256), 0, s, fp, sp, nframes);
    hip_check(hipGetLastError(), "sparsify scan launch");
  }
  if (!(phases & 2)) return;
  const dim3 pg((unsigned)std::max(1, std::min(kSpPackBlocks, ncpf / 32)), (unsigned)nframes);
  hipLaunchKernelGGL(sparse_pack_kernel, pg, dim3(256), 0, s, sp, nframes, ncpf, reinterpret_cast<int*>(nnz),
                     reinterpret_cast<unsigned char*>(flags), reinterpret_cast<long long*>(offs),
                     reinterpret_cast<int*>(pix), reinterpret_cast<float*>(val));
  hip_check(hipGetLastError(), "sparsify pack launch");
}

}  // namespace pr
