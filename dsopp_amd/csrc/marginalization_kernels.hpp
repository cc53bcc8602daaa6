// Kernels of the marginalisation unit (marginalization.hip).  Two launches, no host wait between them and no workgroup waiting for another:
//   1. margCountAndChooseKernel — one thread per landmark / immature landmark of the active frames counts what
//      numberOfActiveAndImmatureLandmarks and numberOfMarginalizedLandmarks count (integer sums: any order gives the same); the workgroup
//      that draws the last ticket (lastWorkgroup, ransac_device.hpp) then walks the frames as the reference does, one lane, in the
//      reference's order: findFramesWithSmallNumberOfActivePoints reads the set it is growing, findFramesToMarginalize sums its score in
//      window order, and the erase loop runs against the shrinking list.
//   2. margLandmarksKernel — one thread per landmark of every frame of the window, in the CALLER's order: marginalizeLandmarks for the
//      active frames but the last, ActiveKeyframe::marginalize for the frames that leave, the new flag byte of every landmark.
// binary64 throughout, products and sums unfused (the unit is compiled with -ffp-contract=off), as tests/marginalization_model.py takes them.
#pragma once
#include <hip/hip_runtime.h>

#include "immature_set.hpp"
#include "marginalization.hpp"
#include "ransac_device.hpp"

namespace dsopp_hip {

/** the window slot whose block range holds this workgroup (every frame owns at least one workgroup) */
__device__ __forceinline__ int margSlotOfBlock(const MargArgs &a) {
  int slot = 0;
  for (int f = 1; f < a.n_frames; ++f)
    if (a.frame[f].first_block <= static_cast<int>(blockIdx.x)) slot = f;
  return slot;
}

/** the serial part: sparse_frame_marginalization_strategy.cpp:38-53 (small number of active points), :101-140 (the score), :165-167 with
 *  ActiveOdometryTrack::marginalizeFrame (the erase loop); maximum_size_frame_marginalization_strategy.cpp:16-20 */
__device__ inline void margChoose(const MargArgs &a) {
  constexpr int kKeepFramesFromStart = 2;
  constexpr long long kMinFrameAge = 1;
  const double kEps = 1e-5;
  MargDecision &d = *a.decision;
  int slot_of[kMaxFrames];
  int A = 0;
  for (int f = 0; f < a.n_frames; ++f)
    if (a.frame[f].active >= 0) slot_of[A++] = f;
  bool in_set[kMaxFrames];
  for (int i = 0; i < kMaxFrames; ++i) {
    in_set[i] = false;
    d.score[i] = __builtin_nan("");
    d.n_kept[i] = d.n_gone[i] = 0;
    d.in_set[i] = d.frame_goes[i] = 0;
  }
  for (int i = 0; i < A; ++i) {
    d.n_kept[i] = ransac::freshLoad(a.counts + 2 * slot_of[i]);
    d.n_gone[i] = ransac::freshLoad(a.counts + 2 * slot_of[i] + 1);
  }
  int n_set = 0, n_gone_frames = 0;
  if (a.strategy == DSOPP_HIP_MARGINALIZATION_SPARSE) {
    for (int i = 0; i + kKeepFramesFromStart < A; ++i) {
      const double kept = static_cast<double>(d.n_kept[i]);
      const double all = kept + static_cast<double>(d.n_gone[i]);
      if (kept < (1 - a.maximum_share_marginalized) * all && A - n_set > a.minimum_size) {
        in_set[i] = true;
        ++n_set;
      }
    }
    if (A > a.maximum_size + n_set) {
      double max_score = 0;
      int chosen = 0;
      const MargFrame &last = a.frame[slot_of[A - 1]];
      for (int r = 0; r + kKeepFramesFromStart < A; ++r) {
        const MargFrame &ref = a.frame[slot_of[r]];
        if (static_cast<long long>(ref.camera_id) + kMinFrameAge > static_cast<long long>(last.camera_id)) continue;
        double score = 0;
        for (int t = 0; t + kKeepFramesFromStart < A; ++t) {
          const MargFrame &tgt = a.frame[slot_of[t]];
          if (static_cast<long long>(tgt.camera_id) + kMinFrameAge > static_cast<long long>(last.camera_id) + 1 || r == t) continue;
          const double dx = ref.t[0] - tgt.t[0], dy = ref.t[1] - tgt.t[1], dz = ref.t[2] - tgt.t[2];
          score += 1 / (kEps + sqrt(dx * dx + dy * dy + dz * dz));
        }
        const double dx = ref.t[0] - last.t[0], dy = ref.t[1] - last.t[1], dz = ref.t[2] - last.t[2];
        score *= sqrt(sqrt(dx * dx + dy * dy + dz * dz));
        d.score[r] = score;
        if (score > max_score) {
          max_score = score;
          chosen = r;
        }
      }
      if (!in_set[chosen]) {  // (std::set::insert)
        in_set[chosen] = true;
        ++n_set;
      }
    }
    // the erase loop: ascending indices against the list as it shrinks — a second index lands on a later frame
    int list[kMaxFrames];
    int len = A;
    for (int i = 0; i < A; ++i) list[i] = i;
    for (int s = 0; s < A; ++s) {
      if (!in_set[s]) continue;
      d.selected[d.n_selected++] = s;
      if (s >= len) continue;  // (past the end of the shrunken list: undefined in the reference, nothing leaves here)
      d.marginalized_slot[n_gone_frames++] = slot_of[list[s]];
      for (int k = s; k + 1 < len; ++k) list[k] = list[k + 1];
      --len;
    }
  } else {
    for (int i = 0; A - i > a.maximum_size && i < A; ++i) {  // marginalizeFrame(0) until the size fits
      d.selected[d.n_selected++] = i;
      d.marginalized_slot[n_gone_frames++] = slot_of[i];
    }
  }
  for (int i = 0; i < A; ++i) d.in_set[slot_of[i]] = in_set[i] ? 1 : 0;
  for (int k = 0; k < n_gone_frames; ++k) d.frame_goes[d.marginalized_slot[k]] = 1;
  d.n_active = A;
  d.n_marginalized = n_gone_frames;
}

__global__ void __launch_bounds__(kMargBlock) margCountAndChooseKernel(MargArgs a) {
  __shared__ unsigned s_last;
  __shared__ int s_count[2];
  if (threadIdx.x < 2) s_count[threadIdx.x] = 0;
  __syncthreads();
  const int slot = margSlotOfBlock(a);
  const MargFrame &f = a.frame[slot];
  if (f.active >= 0) {
    const int i = (static_cast<int>(blockIdx.x) - f.first_block) * kMargBlock + static_cast<int>(threadIdx.x);
    bool kept = false, gone = false, ready = false;
    if (i < f.n) {
      const uint8_t fl = f.flags[i];
      gone = (fl & (kFlagOutlier | kFlagMarginalized)) != 0;
      kept = !gone;
    }
    if (i < f.n_immature) {
      const size_t N = static_cast<size_t>(f.n_immature);
      const double idepth = f.imm_io[N + i] * 0.5 + f.imm_io[i] * 0.5;  // ImmatureTrackingLandmark::idepth()
      ready = immatureReadyForActivation(f.imm_status[i], f.imm_io[3 * N + i], f.imm_io[2 * N + i], idepth);
    }
    const int n_kept = __popcll(__ballot(kept)) + __popcll(__ballot(ready)), n_gone = __popcll(__ballot(gone));
    if ((threadIdx.x & 63) == 0) {
      if (n_kept) atomicAdd(&s_count[0], n_kept);
      if (n_gone) atomicAdd(&s_count[1], n_gone);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (s_count[0]) atomicAdd(a.counts + 2 * slot, s_count[0]);
      if (s_count[1]) atomicAdd(a.counts + 2 * slot + 1, s_count[1]);
    }
  }
  if (!ransac::lastWorkgroup(a.ticket, s_last)) return;
  if (threadIdx.x == 0) margChoose(a);
}

/** ActiveTrackingLandmark::marginalize (active_tracking_landmark.cpp:55-63) on the window's own variance (1 / H_dd) and inverse depth:
 *  a zero inverse depth makes the quotient inf (marked) or, with a zero variance, NaN (not marked) */
__device__ __forceinline__ void margMarginalizeLandmark(double variance, double idepth, bool &marginalized, bool &outlier) {
  if (variance / idepth > 1e-3 || idepth < 0) outlier = true;
  marginalized = true;
}

__global__ void __launch_bounds__(kMargBlock) margLandmarksKernel(MargArgs a) {
  const int slot = margSlotOfBlock(a);
  const MargFrame &f = a.frame[slot];
  const MargDecision &d = *a.decision;
  const int i = (static_cast<int>(blockIdx.x) - f.first_block) * kMargBlock + static_cast<int>(threadIdx.x);
  bool newly_marginalized = false, newly_outlier = false;
  if (i < f.n) {
    const int p = f.to_internal ? f.to_internal[i] : i;
    const uint8_t fl = f.flags[p];
    const bool was_marginalized = fl & kFlagMarginalized, was_outlier = fl & kFlagOutlier;
    bool marginalized = was_marginalized, outlier = was_outlier;
    if (f.active >= 0) {
      // marginalizeLandmarks (:56-91): every active frame but the last, landmarks that are neither marginalised nor outlier
      if (a.strategy == DSOPP_HIP_MARGINALIZATION_SPARSE && d.n_active > 2 && f.active < d.n_active - 1 && !marginalized && !outlier) {
        const bool ok_in_last = i < f.n_last && f.status_last[p] == DSOPP_HIP_STATUS_OK;  // (no entry: the reference's .at() would throw)
        const bool out_of_boundary = d.in_set[slot] || !ok_in_last;
        const int successes = f.successes ? f.successes[i] : 0;
        const bool valid = f.n_inliers[p] >= (a.minimum_size + 1) / 2 && successes > 2 * a.maximum_size;
        const bool sufficient = successes > 0;
        if (out_of_boundary && !sufficient) {
          outlier = true;
        } else if (out_of_boundary || valid) {
          margMarginalizeLandmark(f.inv_hdd[p], f.idepth[p], marginalized, outlier);
        }
      }
      // ActiveKeyframe::marginalize (active_keyframe.cpp:176-184): every landmark of a frame that leaves, whatever its flags
      if (d.frame_goes[slot]) margMarginalizeLandmark(f.inv_hdd[p], f.idepth[p], marginalized, outlier);
    }
    a.new_flags[f.flags_offset + i] = static_cast<uint8_t>((marginalized ? 1 : 0) | (outlier ? 2 : 0));
    newly_marginalized = marginalized && !was_marginalized;
    newly_outlier = outlier && !was_outlier;
  }
  const int n_marginalized = __popcll(__ballot(newly_marginalized)), n_outlier = __popcll(__ballot(newly_outlier));
  if ((threadIdx.x & 63) == 0) {
    if (n_marginalized) atomicAdd(&a.decision->newly_marginalized, n_marginalized);
    if (n_outlier) atomicAdd(&a.decision->newly_outlier, n_outlier);
  }
}

/** the counting half of updateFrame (photometric_bundle_adjustment.cpp:256 with active_tracking_landmark.cpp:42-49) */
// (plain pointer parameters: a kernel's name carries its parameter types, and the address-space ones differ between the host and the device pass)
__global__ void __launch_bounds__(kMargBlock) margNoteOptimizationKernel(const uint8_t *__restrict__ flags, const int32_t *__restrict__ n_inliers,
                                                                         const int32_t *__restrict__ to_internal, int32_t *__restrict__ successes, int n) {
  const int i = static_cast<int>(blockIdx.x) * kMargBlock + static_cast<int>(threadIdx.x);
  if (i >= n) return;
  const int p = to_internal ? to_internal[i] : i;
  if (flags[p] & kFlagMarginalized) return;
  if (n_inliers[p] > 3) successes[i] += 1;
}

}  // namespace dsopp_hip
