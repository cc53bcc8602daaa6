// One float map entry -> one entry of the undistorter's device table (undistort.hip: the entry's layout), for the host loop of
// dsopp_hip_undistorter_create and the kernel of dsopp_hip_undistorter_create_from_model (camera_remap.hip): both run this code.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "undistort.hpp"

namespace dsopp_hip {

/** BORDER_REFLECT_101 of any integer: period 2 (n - 1), ... c b | a b c d | c b ... */
__host__ __device__ inline int reflect101(long c, int n) {
  const long period = 2L * (n - 1);
  long r = c % period;
  if (r < 0) r += period;
  return static_cast<int>(r >= n ? period - r : r);
}

/** one map coordinate -> the two reflected tap coordinates and the 5-bit fraction */
__host__ __device__ inline void splitCoordinate(float c, int n, int &c0, int &c1, int &fraction) {
  const long s = static_cast<long>(rintf(c * 32.0f));  // exact product, rounded half to even (cvRound)
  const long i = s >> kRemapFractionBits;             // arithmetic shift: the floor, also below zero
  fraction = static_cast<int>(s & (kRemapOne - 1));
  c0 = reflect101(i, n);
  c1 = reflect101(i + 1, n);
}

/** the two table words of the map entry (cx, cy) into an in_w x in_h image */
__host__ __device__ inline void foldMapEntry(float cx, float cy, int in_w, int in_h, uint32_t &offset, uint32_t &bits) {
  int x0, x1, fx, y0, y1, fy;
  splitCoordinate(cx, in_w, x0, x1, fx);
  splitCoordinate(cy, in_h, y0, y1, fy);
  offset = static_cast<uint32_t>(y0) * static_cast<uint32_t>(in_w) + static_cast<uint32_t>(x0);
  bits = static_cast<uint32_t>(fx) | (static_cast<uint32_t>(fy) << kRemapFyShift) | (x1 < x0 ? kRemapFlipX : 0u) | (y1 < y0 ? kRemapFlipY : 0u);
}

}  // namespace dsopp_hip
