// The colour forms of the two image stages and the grey conversion (colour.hip), and what pyramid.hip needs of them for
// dsopp_hip_pyramid_build_colour.
#pragma once
#include <cstddef>
#include <cstdint>

#include "transform.hpp"
#include "undistort.hpp"

namespace dsopp_hip {
// Images are 8-bit BGR, interleaved: channel c of pixel o is byte 3 * o + c.  An input may have any alignment; an output must be 4-byte
// aligned and may be null (not both of a call).  `bgr_out_dev` takes the stage's three channels, `grey_out_dev` their grey conversion.
/** enqueue the remap of `bgr_in_dev` (in_w x in_h pixels) on `stream`: out_w x out_h pixels */
void enqueueUndistortBgr(const dsopp_hip_undistorter *u, const uint8_t *bgr_in_dev, uint8_t *bgr_out_dev, uint8_t *grey_out_dev, hipStream_t stream);
/** enqueue the linear resize + crop of `bgr_in_dev` (in_w x in_h pixels) on `stream`: out_w x out_h pixels.  The identity is the plain
 *  conversion for the grey output and one device-to-device copy for the colour one (none when bgr_out_dev == bgr_in_dev). */
void enqueueTransformBgr(const dsopp_hip_transformer *t, const uint8_t *bgr_in_dev, uint8_t *bgr_out_dev, uint8_t *grey_out_dev, hipStream_t stream);
/** enqueue the conversion of `n` BGR pixels into `n` grey bytes on `stream` */
void enqueueBgrToGrey(const uint8_t *bgr_in_dev, uint8_t *grey_out_dev, size_t n, hipStream_t stream);
}  // namespace dsopp_hip
