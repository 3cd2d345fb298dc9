// The owner-lane accumulator shared by the run-statistics kernels (K-09 dark, K-11 powder, K-15 cube).
//
// A lane owns 4 consecutive pixels: one owner per pixel per launch, so no atomics.  It takes ONE
// non-temporal load per frame (16 B of float32, 8 B of raw uint16) with 8, then 4, then 1 loads in
// flight, keeps its in-batch partials in registers, and after the frames of a plane does ONE
// read-modify-write of its words of that plane with 16-B accesses, all loads issued before the first
// store.  Plane c starts at element c * n, 16-B aligned for c >= 1 iff n % 4 == 0; otherwise its words
// go one by one.  The n % 4 last pixels of a frame go to one extra lane (q == n / 4, added by launch.h's
// owner_lane_grid) that walks them with scalar accesses.  All control flow over frames is scalar.
// A kernel supplies its partials and its add (the numerics), where the next frame's address comes
// from, which planes it touches and which it skips, and the owner of its per-launch counters.
#pragma once

#include "common.h"

namespace pr {

typedef unsigned long long u64x2_t __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x4_t acc_ld(const PR_GLOBAL f32x4_t* p) { return ld_nt_f4(p); }
__device__ __forceinline__ uint2 acc_ld(const PR_GLOBAL uint2* p) { return ld_nt_u2(p); }

// K frames with K loads in flight: next() yields a frame's address, add(u) takes the lane's unit U of
// it; every load is issued before the first add
template <typename U, int K, typename Next, typename Add>
__device__ __forceinline__ void acc_frames(const int64_t q, Next& next, Add& add) {
  U r[K];
#pragma unroll
  for (int k = 0; k < K; ++k) r[k] = acc_ld(gin<U>(next()) + q);
#pragma unroll
  for (int k = 0; k < K; ++k) add(r[k]);
}

// a group of `left` (wave-uniform) frames: 8 at a time, then (FOUR) 4, then one by one
template <typename U, bool FOUR, typename Next, typename Add>
__device__ __forceinline__ void acc_group(int left, const int64_t q, Next next, Add add) {
  for (; left >= 8; left -= 8) acc_frames<U, 8>(q, next, add);
  if (FOUR && left >= 4) {
    acc_frames<U, 4>(q, next, add);
    left -= 4;
  }
  for (; left > 0; --left) acc_frames<U, 1>(q, next, add);
}

// A lane's four words of an aligned plane.  Use them load-all, merge-all, store-all, so every read of
// the read-modify-write is in flight before the first write.  The adds are two's complement: the
// unsigned add of a signed partial is the signed add.
struct Words32 {
  u32x4_t v;
  __device__ __forceinline__ void load(const void* p) { v = *reinterpret_cast<const u32x4_t*>(p); }
  __device__ __forceinline__ void store(void* p) const { *reinterpret_cast<u32x4_t*>(p) = v; }
  template <typename T>
  __device__ __forceinline__ void add(const T (&a)[4]) {
    v.x += (uint32_t)a[0]; v.y += (uint32_t)a[1]; v.z += (uint32_t)a[2]; v.w += (uint32_t)a[3];
  }
  __device__ __forceinline__ void smax(const int32_t (&a)[4]) {   // signed maximum
    v.x = (uint32_t)max((int32_t)v.x, a[0]); v.y = (uint32_t)max((int32_t)v.y, a[1]);
    v.z = (uint32_t)max((int32_t)v.z, a[2]); v.w = (uint32_t)max((int32_t)v.w, a[3]);
  }
};

struct Words64 {
  u64x2_t lo, hi;
  __device__ __forceinline__ void load(const void* p) {
    lo = reinterpret_cast<const u64x2_t*>(p)[0];
    hi = reinterpret_cast<const u64x2_t*>(p)[1];
  }
  __device__ __forceinline__ void store(void* p) const {
    reinterpret_cast<u64x2_t*>(p)[0] = lo;
    reinterpret_cast<u64x2_t*>(p)[1] = hi;
  }
  template <typename T>
  __device__ __forceinline__ void add(const T (&a)[4]) {
    lo.x += (unsigned long long)a[0]; lo.y += (unsigned long long)a[1];
    hi.x += (unsigned long long)a[2]; hi.y += (unsigned long long)a[3];
  }
};

// the same merges word by word: NP = 4 for an unaligned plane, NP = 1 for a pixel of the tail lane
template <typename W, typename T, int NP>
__device__ __forceinline__ void acc_add(W* p, const T (&a)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) p[i] += (W)a[i];
}

template <int NP>
__device__ __forceinline__ void acc_max(int32_t* p, const int32_t (&a)[NP]) {
#pragma unroll
  for (int i = 0; i < NP; ++i) p[i] = max(p[i], a[i]);
}

}  // namespace pr
