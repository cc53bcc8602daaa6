// The image transformer handle (transform.hip) and what pyramid.hip and semantics.hip need of it for
// dsopp_hip_pyramid_build_transformed and dsopp_hip_semantics_create_transformed.
#pragma once
#include <cstdint>

#include "common.hpp"

struct dsopp_hip_transformer {
  dsopp_hip::StreamRef sr;
  int in_w = 0, in_h = 0, resized_w = 0, resized_h = 0, out_w = 0, out_h = 0;
  // two words per output column, then two per output row (transform.hip: the entry's layout); [0] = linear, [1] = nearest.
  // Both are null when there is nothing to do (ratio 1 and nothing to crop): no kernel is launched then.
  dsopp_hip::DeviceMem<uint32_t> table[2];
  dsopp_hip::DeviceMem<uint8_t> d_in, d_out;  // the blocking forms' images, allocated by their first call
  bool identity() const { return !table[0]; }
};

namespace dsopp_hip {
constexpr int kTransformLinear = 0, kTransformNearest = 1;
// the table entry's second word (transform.hip: the entry's layout), shared with the colour kernels of colour.hip
constexpr int kResizeCoefBits = 11;  // INTER_RESIZE_COEF_BITS
constexpr int kResizeCoefOne = 1 << kResizeCoefBits;
constexpr unsigned kResizeWeightMask = 0xfffu, kResizeFirstWeightShift = 12, kResizeStep = 1u << 24;
/** enqueue resize + crop of `in_dev` (in_w x in_h bytes) into `out_dev` (out_w x out_h bytes) on `stream`; both 4-byte aligned.  The
 *  identity is a device-to-device copy (none at all when in_dev == out_dev). */
void enqueueTransform(const dsopp_hip_transformer *t, const uint8_t *in_dev, uint8_t *out_dev, int interpolation, hipStream_t stream);
}  // namespace dsopp_hip
