// Host tools of the entry points that stage one call's inputs and results through a device block and a pinned mirror each (the bootstrap's
// RANSAC units): the handle behind the C ABI's opaque pointer, its creation and destruction, and the argument checks the units share.
#pragma once
#include "common.hpp"

#include <cfloat>
#include <cmath>
#include <memory>

namespace dsopp_hip {

inline bool finite(double v) { return std::fabs(v) <= DBL_MAX; }

/** the stream of a handle and the four buffers of its calls: the inputs and the results, one device block and one pinned mirror each,
 *  laid out by the unit; they grow geometrically and never shrink */
struct StagedCall {
  StreamRef sr;
  Event done;
  DeviceMem<uint8_t> d_in, d_out;
  PinnedMem<uint8_t> h_in, h_out;
  size_t in_capacity = 0, out_capacity = 0;

  static size_t grown(size_t capacity, size_t need) {
    size_t cap = capacity ? capacity : 4096;
    while (cap < need) cap *= 2;
    return cap;
  }
  /** room for in_bytes and out_bytes; a capacity is zero while its buffers are replaced, so a failed allocation leaves the object usable */
  void ensure(size_t in_bytes, size_t out_bytes) {
    grow(in_capacity, d_in, h_in, in_bytes);
    grow(out_capacity, d_out, h_out, out_bytes);
  }

 private:
  static void grow(size_t &capacity, DeviceMem<uint8_t> &d, PinnedMem<uint8_t> &h, size_t need) {
    if (capacity >= need) return;
    const size_t cap = grown(capacity, need);
    capacity = 0;
    d.alloc(cap);
    h.reserve(cap);
    capacity = cap;
  }
};

/** every sample of K indices lies in [0, n) and repeats none.  A sample that does both wrong is reported as each unit always has:
 *  kRangeFirst looks at the ranges of all K before any repeat (the triples' units), otherwise index by index (the two-view unit) */
template <int K, bool kRangeFirst>
void checkSamples(const int32_t *samples, int iterations, int n, const char *what) {
  if (!samples) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  for (int i = 0; i < iterations; ++i) {
    const int32_t *s = samples + K * static_cast<size_t>(i);
    const auto repeated = [&](int k) {
      for (int l = 0; l < k; ++l)
        if (s[l] == s[k]) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "sample %d repeats an index", i);
    };
    for (int k = 0; k < K; ++k) {
      if (s[k] < 0 || s[k] >= n) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "sample %d holds index %d of %d %s", i, s[k], n, what);
      if (!kRangeFirst) repeated(k);
    }
    for (int k = 1; kRangeFirst && k < K; ++k) repeated(k);
  }
}

/** the body of a dsopp_hip_*_create: H is a StagedCall */
template <typename H>
int createHandle(int device, void *stream, H **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    auto r = std::make_unique<H>();
    r->sr.init(device, stream);
    *out = r.release();
  });
}

/** the body of a dsopp_hip_*_destroy: the stream's work ends before the buffers go */
template <typename H>
void destroyHandle(H *r) {
  if (!r) return;
  (void)hipSetDevice(r->sr.device);
  if (r->sr.stream) (void)hipStreamSynchronize(r->sr.stream);
  delete r;
}

}  // namespace dsopp_hip
