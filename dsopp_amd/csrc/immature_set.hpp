// The immature landmarks of one keyframe, resident on the device across frames (track::landmarks::ImmatureTrackingLandmark as
// struct-of-arrays, src/track/landmarks/include/track/landmarks/immature_tracking_landmark.hpp:93-106).  Shared by
// depth_estimation.hip (owner: the per-frame depth estimator) and pba.hip (the landmark activator reads the estimator
// state and writes the refined inverse depth back).
#pragma once
#include "common.hpp"

#include <memory>

struct dsopp_hip_immature_set {
  dsopp_hip::StreamRef sr;
  int n = 0;
  dsopp_hip::DeviceBuffer<double> d_in;      // projection 2n | direction 3n | patch 8n | gradient 2n
  dsopp_hip::DeviceBuffer<double> d_io;      // idepth_min | idepth_max | uniqueness | search_pixel_interval
  dsopp_hip::DeviceBuffer<uint8_t> d_flags;  // status | traced
  dsopp_hip::PinnedMem<void> h_stage;       // read-back staging
  dsopp_hip::PinnedMem<void> h_tables;      // descriptor tables of a batched estimate led by this set
  dsopp_hip::DeviceBuffer<char> d_tables;
  dsopp_hip::Event tables_copied;            // the previous batch's table upload has left the pinned buffer
};

namespace dsopp_hip {
// ImmatureStatus (immature_tracking_landmark.hpp:14-22) as the sets' status bytes hold it
enum : uint8_t { kImmGood = 0, kImmOutOfBoundary = 1, kImmOutlier = 2, kImmSkipped = 3, kImmIllConditioned = 4, kImmDelete = 6 };
/** ImmatureTrackingLandmark::readyForActivation (src/track/landmarks/src/immature_tracking_landmark.cpp:46-52); idepth = the mean of the
 *  landmark's interval, ImmatureTrackingLandmark::idepth() */
__host__ __device__ inline bool immatureReadyForActivation(uint8_t status, double search_pixel_interval, double uniqueness, double idepth) {
  return (status == kImmGood || status == kImmSkipped || status == kImmIllConditioned || status == kImmOutOfBoundary) &&
         (search_pixel_interval < 8.0) && (uniqueness > 3.0) && (idepth > 0);
}
struct ImmatureSetDeleter {
  void operator()(dsopp_hip_immature_set *s) const { dsopp_hip_immature_set_destroy(s); }
};
using ImmatureSetPtr = std::unique_ptr<dsopp_hip_immature_set, ImmatureSetDeleter>;
/** A set of n landmarks in the ImmatureTrackingLandmark constructor state (depth_estimation.hip), synchronised on return.  The input
 *  planes (projection 2n | direction 3n | patch 8n | gradient 2n of d_in) are uploaded from the host arrays that are not NULL; the
 *  others are left for the caller to write on the set's stream (dsopp_hip_immature_set_create_from_features, features.hip). */
ImmatureSetPtr newImmatureSet(int device, void *stream, int32_t n, const double *projection, const double *direction, const double *patch,
                              const double *gradient);
}  // namespace dsopp_hip
