// The undistorter handle (undistort.hip) and what pyramid.hip needs of it for dsopp_hip_pyramid_build_undistorted.
#pragma once
#include <cstdint>

#include "common.hpp"

struct dsopp_hip_undistorter {
  dsopp_hip::StreamRef sr;
  int in_w = 0, in_h = 0, out_w = 0, out_h = 0;
  dsopp_hip::DeviceMem<uint32_t> table;      // two words per output pixel (undistort.hip: the entry's layout)
  dsopp_hip::DeviceMem<uint8_t> d_in, d_out;  // the blocking form's images (dsopp_hip_undistorter_undistort), allocated by its first call
};

namespace dsopp_hip {
// the table entry's second word (undistort.hip: the entry's layout), shared with the colour kernels of colour.hip
constexpr int kRemapFractionBits = 5;  // INTER_BITS
constexpr int kRemapOne = 1 << kRemapFractionBits;
constexpr unsigned kRemapFyShift = 8, kRemapFlipX = 1u << 16, kRemapFlipY = 1u << 17;
/** enqueue the remap of `in_dev` (in_w x in_h bytes) into `out_dev` (out_w x out_h bytes, 4-byte aligned) on `stream` */
void enqueueUndistort(const dsopp_hip_undistorter *u, const uint8_t *in_dev, uint8_t *out_dev, hipStream_t stream);
}  // namespace dsopp_hip
