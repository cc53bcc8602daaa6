// ActiveTrackingLandmark::semanticTypeId (src/track/landmarks/src/active_tracking_landmark.cpp:71-88) of one landmark's 256 counters: the
// device code dsopp_hip_window_get_semantic_types (semantic_observation_kernels.hpp) and dsopp_hip_map_update (point_cloud.hip) share.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace dsopp_hip {

constexpr int kSemClasses = 256;

/** `row` = the landmark's 256 counters (16-byte aligned), weights 256 x uint64 or null */
__device__ __forceinline__ uint8_t semanticTypeOfRow(const uint8_t *row_, const unsigned long long *__restrict__ weights) {
  const uint4 *row = reinterpret_cast<const uint4 *>(row_);
  unsigned best_count = 0, best_i = 0;              // std::max_element: the first maximal count
  unsigned long long best_w = 0;                    // max_weight, max_weight_element
  unsigned best_wi = 0;
  for (int q = 0; q < kSemClasses / 16; ++q) {
    const uint4 w4 = row[q];
    const unsigned words[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
    for (int b = 0; b < 16; ++b) {
      const unsigned i = static_cast<unsigned>(16 * q + b);
      const unsigned count = (words[b >> 2] >> (8 * (b & 3))) & 255u;
      if (count > best_count) {
        best_count = count;
        best_i = i;
      }
      if (weights) {
        const unsigned long long wgt = count * weights[i];  // size_t arithmetic, as the reference
        if (wgt > best_w) {
          best_w = wgt;
          best_wi = i;
        }
      }
    }
  }
  return static_cast<uint8_t>((weights && best_w != 0) ? best_wi : best_i);
}

}  // namespace dsopp_hip
