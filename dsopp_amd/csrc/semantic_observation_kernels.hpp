// Class observations of the window's landmarks (semantic segmentation): the kernels behind
// dsopp_hip_window_add_semantic_observations / _get_semantic_types.
//   addSemanticObservations                         src/tracker/tracker/src/monocular_tracker.cpp:263-305
//   the checked pinhole reprojection                 src/energy/projector/include/energy/projector/camera_reproject.hpp:270-293
//   ActiveTrackingLandmark::semanticTypeId           src/track/landmarks/src/active_tracking_landmark.cpp:71-88
//
// One work item per landmark of a reference frame.  It walks the frame's partner frames itself and is the only writer of the landmark's
// 256 counters, so the counts need no atomics and do not depend on any order.  The counters are rows of the CALLER's landmark index:
// the internal tile order of the landmark arrays (HostFrame::to_internal) may change under them without a row moving.
#pragma once
#include "device_geom.hpp"
#include "pba_kernels.hpp"
#include "semantic_type.hpp"

namespace dsopp_hip {

constexpr int kSemBlock = 256;

/** one direction (reference -> target) of a frame pair */
struct SemPartner {
  double M[12];          // K_t [R | t] Kinv_r of T_target^-1 T_reference at the current estimates (camera_reproject.hpp:256), rows of 4
  const hbm_u8 *status;  // connection statuses reference -> target, the device's landmark order
  const hbm_u8 *cls;     // the target's undistorted class image
  int n_res;             // entries of `status`
  int width, height;     // of the target
  int pad;
};

/** one reference frame and the range of its partners */
struct SemJob {
  const hbm_f64 *uv, *idepth;  // the device's landmark order
  const hbm_i32 *to_internal;  // caller index -> device index; null = identity
  hbm_u8 *hist;                // n x 256 counters, the caller's landmark order
  int n;                       // landmarks
  int first_block;             // first workgroup of the launch that works on this frame
  int first_partner, n_partners;
  int width, height;           // of the reference
};

__global__ void __launch_bounds__(kSemBlock) semanticObservationsKernel(const SemJob *__restrict__ jobs, int n_jobs,
                                                                        const SemPartner *__restrict__ partners) {
  int j = 0;
  for (int i = 1; i < n_jobs; ++i)
    if (jobs[i].first_block <= static_cast<int>(blockIdx.x)) j = i;
  const SemJob job = jobs[j];
  const int c = (static_cast<int>(blockIdx.x) - job.first_block) * kSemBlock + static_cast<int>(threadIdx.x);
  if (c >= job.n) return;
  const int p = job.to_internal ? job.to_internal[c] : c;
  const double u = job.uv[2 * p], v = job.uv[2 * p + 1], d = job.idepth[p];
  // kCheckSuccess: validIdepth and the reference pattern inside the ROI (camera_reproject.hpp:278-280)
  bool inside = validIdepth<double>(d);
#pragma unroll
  for (int k = 0; k < kPat; ++k) inside = inside && insideROI<double>(u + kPatX[k], v + kPatY[k], job.width, job.height);
  if (!inside) return;
  hbm_u8 *row = job.hist + static_cast<size_t>(c) * kSemClasses;
  for (int q = 0; q < job.n_partners; ++q) {
    const SemPartner *pt = partners + job.first_partner + q;
    if (p >= pt->n_res || pt->status[p] != DSOPP_HIP_STATUS_OK) continue;
    const double m0 = pt->M[2] + pt->M[3] * d, m1 = pt->M[6] + pt->M[7] * d, m2 = pt->M[10] + pt->M[11] * d;
    double tu[kPat], tv[kPat];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < kPat; ++k) {
      const double pu = u + kPatX[k], pv = v + kPatY[k];
      const double x = pt->M[0] * pu + pt->M[1] * pv + m0, y = pt->M[4] * pu + pt->M[5] * pv + m1, z = pt->M[8] * pu + pt->M[9] * pv + m2;
      tu[k] = x / z;
      tv[k] = y / z;
      valid = valid && z > 0.0 && insideROI<double>(tu[k], tv[k], pt->width, pt->height);
    }
    if (!valid) continue;
#pragma unroll
    for (int k = 0; k < kPat; ++k) {
      // inside the ROI: 4 <= coordinate <= size - 5, so the truncated index is inside the class image
      const int cls = pt->cls[static_cast<size_t>(static_cast<int>(tv[k])) * pt->width + static_cast<int>(tu[k])];
      row[cls] = static_cast<uint8_t>(row[cls] + 1);  // std::array<uint8_t, 256>: wraps modulo 256
    }
  }
}

/** semanticTypeId of n landmarks: hist n x 256 counters, weights 256 x uint64 or null */
__global__ void __launch_bounds__(kSemBlock) semanticTypesKernel(const uint8_t *__restrict__ hist, int n, const unsigned long long *__restrict__ weights,
                                                                 uint8_t *__restrict__ type) {
  const int c = static_cast<int>(blockIdx.x) * kSemBlock + static_cast<int>(threadIdx.x);
  if (c >= n) return;
  type[c] = semanticTypeOfRow(hist + static_cast<size_t>(c) * kSemClasses, weights);
}

}  // namespace dsopp_hip
