// Host-side pieces the launchers share: the refusals every frame consumer makes in the same words,
// the quantisation bound of the integer accumulators, and the grid sizes that are computed the same
// way in more than one file.  `name` is the launcher's message prefix ("powder", "pixel_hist", ...).
#pragma once

#include <algorithm>
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>

#include "common.h"

namespace pr {

// refuses with "<name>: <what>"; the text is put together only when it is needed
inline void check_named(bool ok, const char* name, const char* what) {
  if (!ok) check(false, std::string(name) + ": " + what);
}

inline void check_nframes(int nframes, const char* name) {
  check_named(nframes >= 1 && nframes <= kMaxFrames, name, "nframes out of range");
}

// n pixels per frame: a pixel index fits an int32
inline void check_frame_size(int64_t n, const char* name) {
  check_named(n >= 1 && n < (int64_t)1 << 31, name, "frame size out of range");
}

// one input frame: 16-B aligned and, unless the launcher never asked for that, non-null
inline void check_frame(uint64_t p, const char* name, bool nonnull = true) {
  check_named((p != 0 || !nonnull) && aligned16(p), name, "frames must be 16-B aligned");
}

inline void check_frames(const FramePtrs& fp, int nframes, const char* name, bool nonnull = true) {
  for (int f = 0; f < nframes; ++f) check_frame(fp.in[f], name, nonnull);
}

// The value window and fixed-point scale of the integer accumulators (K-11 powder, K-15 cube):
// q = rint(v * 2^frac_bits) fits an int32 and `nframes` squares of it an int64.  Returns 2^frac_bits.
inline float quant_bound(float vmin, float vmax, int frac_bits, int nframes, const char* name) {
  check_named(std::isfinite(vmin) && std::isfinite(vmax) && vmin <= vmax, name, "the value window must be finite and ordered");
  check_named(frac_bits >= 0 && frac_bits <= 16, name, "frac_bits outside [0, 16]");
  // Q = ceil(max(|vmin|, |vmax|) * 2^S) in doubles: a float32 times 2^16 is exact
  const double Q = std::ceil(std::ldexp(std::max(std::fabs((double)vmin), std::fabs((double)vmax)), frac_bits));
  check_named(Q < 2147483648.0, name, "max(|vmin|, |vmax|) * 2^frac_bits must stay below 2^31");
  const unsigned __int128 q2 = (unsigned __int128)(uint64_t)Q * (uint64_t)Q;
  check_named(q2 * (unsigned)nframes <= (unsigned __int128)INT64_MAX, name, "more frames than (2^63 - 1) / Q^2");
  return std::ldexp(1.0f, frac_bits);
}

// grid of the owner-lane accumulators (accum.h): 256-thread workgroups over one lane per 4 pixels
// plus, when n % 4 != 0, the lane that walks the tail
inline dim3 owner_lane_grid(int64_t n) {
  const int64_t lanes = n / 4 + (n % 4 != 0 ? 1 : 0);
  return dim3((unsigned)((lanes + 255) / 256));
}

// Resident workgroups of a 256-thread kernel with `lds` bytes of dynamic LDS on the CURRENT device,
// queried once per (device, kernel, lds) under a lock: a process that drives several GPUs, or
// launches from several threads, sizes every grid from its own device's answer.  Speed only: no
// kernel here needs co-residency.  `what` prefixes the HIP error texts.
inline int resident_blocks(const void* kernel, int lds, const char* what) {
  static std::mutex mu;
  static std::map<std::tuple<int, const void*, int>, int> cache;
  auto ok = [what](hipError_t e, const char* step) {
    if (e != hipSuccess) hip_check(e, (std::string(what) + step).c_str());
  };
  int dev = 0;
  ok(hipGetDevice(&dev), " device");
  std::lock_guard<std::mutex> lk(mu);
  int& n = cache[{dev, kernel, lds}];
  if (n == 0) {
    int cus = 0, per = 0;
    ok(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev), " cu count");
    ok(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, 256, (size_t)lds), " occupancy");
    n = std::max(1, cus * std::max(1, per));
  }
  return n;
}

}  // namespace pr
