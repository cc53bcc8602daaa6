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
