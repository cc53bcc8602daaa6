// What the window's glue (pba.hip) hands to the map unit (point_cloud.hip): plain device pointers of the window's frames and their
// poses at the current estimate, no window types.
#pragma once
#include "common.hpp"

struct dsopp_hip_window;

namespace dsopp_hip {

/** one frame of the window, in window order */
struct MapWindowFrame {
  int id;
  int n;                      // landmarks
  double intr[4];             // fx, fy, cx, cy
  double T_world_agent[7];    // tWorldAgent at the current estimate (qx, qy, qz, qw, tx, ty, tz)
  const double *uv, *idepth, *inv_hdd, *relative_baseline;  // the device's landmark order
  const uint8_t *flags;       // the device's landmark order
  const int *to_internal;     // caller index -> device index (nullptr: identity)
  const uint8_t *sem_hist;    // n x 256 class counters, the caller's order (nullptr: no observation has reached the frame)
};

struct MapWindowView {
  int device = 0;
  hipStream_t stream = nullptr;  // the window's: its arrays are valid behind what this stream holds now
  int n_frames = 0;
  MapWindowFrame frame[DSOPP_HIP_MAX_FRAMES];
};

/** pending appends flushed, the host's state brought up to date; fails on a null window and on a landmark shard of a window group */
void mapWindowView(dsopp_hip_window *w, MapWindowView &view);

}  // namespace dsopp_hip
