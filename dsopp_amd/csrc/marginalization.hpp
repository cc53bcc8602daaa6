// What the window's glue (pba.hip) hands to the marginalisation unit (marginalization.hip): plain device pointers of the window's frames,
// no window types.  The unit chooses the keyframes and landmarks that leave the window —
//   SparseFrameMarginalizationStrategy       src/marginalization/src/sparse_frame_marginalization_strategy.cpp:16-168
//   MaximumSizeFrameMarginalizationStrategy  src/marginalization/src/maximum_size_frame_marginalization_strategy.cpp:16-20
//   ActiveTrackingLandmark::marginalize      src/track/landmarks/src/active_tracking_landmark.cpp:55-63
// — and keeps the landmarks' count of successful optimisations (setNumberOfInlierResidualsInTheLastOptimization, :42-49).
#pragma once
#include "pba_types.hpp"

namespace dsopp_hip {

constexpr int kMargBlock = 256;

/** one frame of the window, in window order */
struct MargFrame {
  int n;             // landmarks
  int n_immature;    // landmarks of the frame's immature set (0: none given)
  int n_last;        // entries of the connection towards the last active keyframe (0: none)
  int active;        // index among the active frames (those not flagged marginalised), -1 for a flagged frame
  int camera_id;     // the id of the age test
  int first_block;   // first workgroup of the frame in both launches
  int flags_offset;  // the frame's first byte in the flag output
  int pad;
  double t[3];       // tWorldAgent().translation()
  const hbm_u8 *flags;         // device order
  const hbm_i32 *n_inliers;    // device order
  const hbm_f64 *idepth, *inv_hdd;  // device order
  const hbm_u8 *status_last;   // device order
  const hbm_i32 *to_internal;  // caller -> device index (nullptr: identity)
  const hbm_i32 *successes;    // caller's order (nullptr: every count 0)
  const hbm_u8 *imm_status;    // status n_immature | traced n_immature
  const hbm_f64 *imm_io;       // idepth_min | idepth_max | uniqueness | search_pixel_interval
};

/** the decision as the device leaves it (one read-back: the flag bytes follow it) */
struct MargDecision {
  int n_active;
  int n_selected, n_marginalized;
  int newly_marginalized, newly_outlier;  // summed by the landmark pass
  int pad;
  int selected[kMaxFrames];            // indices among the active frames, ascending
  int marginalized_slot[kMaxFrames];   // window slots, in erase order
  int n_kept[kMaxFrames], n_gone[kMaxFrames];  // by active index: active + ready immature landmarks | outlier or marginalised ones
  double score[kMaxFrames];            // by active index; NaN where findFramesToMarginalize computes none
  // what the landmark pass reads, by window slot
  int in_set[kMaxFrames], frame_goes[kMaxFrames];
};

struct MargArgs {
  MargFrame frame[kMaxFrames];
  int n_frames;
  int strategy;  // DSOPP_HIP_MARGINALIZATION_*
  int minimum_size, maximum_size;
  double maximum_share_marginalized;
  int last_slot;  // window slot of the last active keyframe
  int n_blocks;
  unsigned *ticket;        // zero before the call
  int *counts;             // 2 per window slot, zero before the call
  MargDecision *decision;  // newly_* zero before the call
  hbm_u8 *new_flags;       // bit0 marginalised, bit1 outlier; frame after frame in the caller's order
};

/** both launches on `stream`; nothing waits on the host */
void launchChooseMarginalization(const MargArgs &args, hipStream_t stream);

/** successes[i] += n_inliers[internal(i)] > 3 for every landmark i (caller's order) that is not flagged marginalised */
void launchNoteOptimization(const uint8_t *flags, const int32_t *n_inliers, const int32_t *to_internal, int32_t *successes, int n, hipStream_t stream);

}  // namespace dsopp_hip
