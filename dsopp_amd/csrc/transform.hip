// Image transformers on the device: the resize and the crop every camera frame, class image, static mask and vignette go through behind
// the undistortion, and the dsopp_hip_transformer_* entry points.
//   CameraResizer::transformImage = cv::resize(img, img, Size((int)(cols * ratio), (int)(rows * ratio)), 0, 0, interpolation)
//                                                   src/sensors/camera_transformers/src/camera_resizer.cpp:7-16
//   ImageCropper::transformImage  = the top-left (cols >> 4 << 4) x (rows >> 4 << 4) pixels
//                                                   src/sensors/camera_transformers/src/image_cropper.cpp:7-16, camera_image_crop.hpp:15-20
//   the list: a resizer if configured, then always the cropper      src/sensors/camera_transformers/src/fabric.cpp:12-31
//   per frame (image: INTER_LINEAR, class image: INTER_NEAREST)     src/sensors/camera/src/camera.cpp:57-70
//   mask, vignette and calibration, once                            src/sensors_builder/src/camera_fabric.cpp:157-167
//
// The arithmetic is the fixed-point one of an 8-bit bilinear resize, all integer once the two axes are tabulated (DESIGN.md section 4 and
// include/dsopp_hip.h state it in full).  Both passes are separable and every tap index and weight is a constant of the sizes, so create()
// folds each axis into one 8-byte entry per output column and per output row — out_w + out_h entries, cropped columns and rows get none:
//   word 0   the first tap: its column (column entries) or its row * in_w (row entries)
//   word 1   weight of the second tap (bits 0-11) | weight of the first tap (bits 12-23) | the second tap is one pixel / one row on (bit 24)
// Bit 24 is clear where the first tap is the last pixel of its axis: the second tap then has weight 0 and reads the first one again.
// INTER_NEAREST and the pure crop are the same kernel over another table: weights (2048, 0) on both axes give
// ((2048 * ((2048 * p) >> 4)) >> 16 + 2) >> 2 = p.  The kernel sees the output as N = out_w * out_h bytes in a row, as the remap does
// (rows of a dense output are not word aligned when out_w is no multiple of 4): a thread finds the row and column of its first byte with one
// division, reads the few table entries it needs (the tables stay in cache: 16 KiB for 1024 x 1024), gathers its 16 taps as bytes and
// stores one 32-bit word.  The N mod 4 bytes that are left are stored one by one by the thread behind the last full word.
#include "transform.hpp"

#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "pyramid.hpp"

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxCropLevels = 8;

typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned transformPixel(GlobalPtr<const uint8_t> src, unsigned in_w, u32x2 col, u32x2 row) {
  const int a1 = col.y & kResizeWeightMask, a0 = (col.y >> kResizeFirstWeightShift) & kResizeWeightMask;
  const int b1 = row.y & kResizeWeightMask, b0 = (row.y >> kResizeFirstWeightShift) & kResizeWeightMask;
  const unsigned dx = (col.y & kResizeStep) ? 1u : 0u, dy = (row.y & kResizeStep) ? in_w : 0u;
  GlobalPtr<const uint8_t> p = src + (row.x + col.x);
  const int p00 = p[0], p01 = p[dx], p10 = p[dy], p11 = p[dx + dy];
  const int r0 = a0 * p00 + a1 * p01, r1 = a0 * p10 + a1 * p11;
  return static_cast<unsigned>((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
}

/** bytes [first, first + count) of the output, count <= 4, as one little-endian word */
__device__ __forceinline__ unsigned transformBytes(GlobalPtr<const u32x2> cols, GlobalPtr<const u32x2> rows, GlobalPtr<const uint8_t> src,
                                                   unsigned in_w, unsigned out_w, unsigned first, unsigned count) {
  unsigned y = first / out_w, x = first - y * out_w;
  u32x2 row = rows[y];
  unsigned word = 0;
  for (unsigned k = 0; k < count; ++k) {
    word |= transformPixel(src, in_w, cols[x], row) << (8 * k);
    if (++x == out_w && k + 1 < count) {  // (the next byte exists, so does its row)
      x = 0;
      row = rows[++y];
    }
  }
  return word;
}

// (the parameters are plain pointers — a kernel's name must be the same in the host and the device pass — and are typed as HBM inside)
__global__ void __launch_bounds__(kBlock) transformKernel(const unsigned *__restrict__ table_, const uint8_t *__restrict__ src_, unsigned in_w,
                                                          unsigned out_w, unsigned *__restrict__ out_, unsigned words, unsigned tail) {
  GlobalPtr<const u32x2> cols = reinterpret_cast<GlobalPtr<const u32x2>>(glb(table_)), rows = cols + out_w;
  GlobalPtr<const uint8_t> src = glb(src_);
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    glb(out_)[t] = transformBytes(cols, rows, src, in_w, out_w, 4 * t, 4);
  } else if (t == words) {
    for (unsigned i = 4 * words; i < 4 * words + tail; ++i)
      reinterpret_cast<GlobalPtr<uint8_t>>(glb(out_))[i] = static_cast<uint8_t>(transformBytes(cols, rows, src, in_w, out_w, i, 1));
  }
}

struct Sizes {
  int resized_w, resized_h, out_w, out_h;
};

/** CameraResizer's and ImageCropper's sizes; refuses what dsopp_hip_transformer_create refuses */
Sizes transformedSizes(int in_w, int in_h, double ratio, int crop_levels) {
  if (!std::isfinite(ratio) || !(ratio > 0)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the resize ratio is %g", ratio);
  if (in_w < 1 || in_h < 1) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the input image is %d x %d", in_w, in_h);
  if (crop_levels < 0 || crop_levels > kMaxCropLevels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d crop levels: 0 .. %d", crop_levels, kMaxCropLevels);
  const double w = static_cast<double>(in_w) * ratio, h = static_cast<double>(in_h) * ratio;
  if (static_cast<long long>(in_w) * in_h > INT_MAX || w * h > static_cast<double>(INT_MAX) || w > static_cast<double>(INT_MAX) ||
      h > static_cast<double>(INT_MAX))
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image too large");
  Sizes s;
  s.resized_w = static_cast<int>(w);  // camera_resizer.cpp:9-10: truncated
  s.resized_h = static_cast<int>(h);
  s.out_w = (s.resized_w >> crop_levels) << crop_levels;  // camera_image_crop.hpp:17-18
  s.out_h = (s.resized_h >> crop_levels) << crop_levels;
  if (s.out_w < 1 || s.out_h < 1)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d x %d at ratio %g and %d crop levels leaves %d x %d", in_w, in_h, ratio, crop_levels, s.out_w, s.out_h);
  return s;
}

uint32_t packWeights(int first, int second, bool step) {
  return static_cast<uint32_t>(second) | (static_cast<uint32_t>(first) << kResizeFirstWeightShift) | (step ? kResizeStep : 0u);
}

/** the entries of the first n_out of n_resized output indices of one axis; `stride` = 1 for columns, in_w for rows */
void axisTable(int n_in, int n_resized, int n_out, int interpolation, uint32_t stride, uint32_t *entries) {
#pragma clang fp contract(off)  // every product and sum below rounds on its own, as in cv::resize
  const double scale = 1.0 / (static_cast<double>(n_resized) / n_in);
  for (int d = 0; d < n_out; ++d) {
    int s, first = kResizeCoefOne, second = 0;
    if (interpolation == kTransformNearest) {
      s = static_cast<int>(std::min<double>(std::floor(d * scale), n_in - 1));
    } else {
      float f = static_cast<float>((d + 0.5) * scale - 0.5);
      const float whole = std::floor(f);
      s = static_cast<int>(whole);
      f -= whole;
      if (s < 0) s = 0, f = 0;
      if (s >= n_in - 1) s = n_in - 1, f = 0;
      second = static_cast<int>(std::lrintf(f * 2048.0f));  // cvRound: half to even
      first = static_cast<int>(std::lrintf((1.0f - f) * 2048.0f));
    }
    entries[2 * d] = static_cast<uint32_t>(s) * stride;
    entries[2 * d + 1] = packWeights(first, second, s + 1 < n_in);
  }
}

void checkHandle(const dsopp_hip_transformer *t) {
  if (!t) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null transformer");
}

void transformHost(dsopp_hip_transformer *t, const uint8_t *in_host, uint8_t *out_host, int interpolation) {
  checkHandle(t);
  if (!in_host || !out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  t->sr.use();
  const size_t n_in = static_cast<size_t>(t->in_w) * t->in_h, n_out = static_cast<size_t>(t->out_w) * t->out_h;
  if (!t->d_in) t->d_in.alloc(n_in);
  if (!t->d_out) t->d_out.alloc(n_out);
  HIP_CHECK(hipMemcpyAsync(t->d_in.get(), in_host, n_in, hipMemcpyHostToDevice, t->sr.stream));
  enqueueTransform(t, t->d_in.get(), t->d_out.get(), interpolation, t->sr.stream);
  HIP_CHECK(hipMemcpyAsync(out_host, t->d_out.get(), n_out, hipMemcpyDeviceToHost, t->sr.stream));
  t->sr.sync();
}

}  // namespace

void enqueueTransform(const dsopp_hip_transformer *t, const uint8_t *in_dev, uint8_t *out_dev, int interpolation, hipStream_t stream) {
  if (interpolation != kTransformLinear && interpolation != kTransformNearest)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "interpolation %d: 0 = linear, 1 = nearest", interpolation);
  if ((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device images must be 4-byte aligned");
  const size_t n = static_cast<size_t>(t->out_w) * t->out_h;
  if (t->identity()) {
    if (in_dev != out_dev) HIP_CHECK(hipMemcpyAsync(out_dev, in_dev, n, hipMemcpyDeviceToDevice, stream));
    return;
  }
  const unsigned words = static_cast<unsigned>(n / 4), tail = static_cast<unsigned>(n % 4);
  const unsigned threads = words + (tail ? 1u : 0u);
  transformKernel<<<(threads + kBlock - 1) / kBlock, kBlock, 0, stream>>>(t->table[interpolation].get(), in_dev, static_cast<unsigned>(t->in_w),
                                                                          static_cast<unsigned>(t->out_w), reinterpret_cast<unsigned *>(out_dev), words, tail);
  HIP_CHECK(hipGetLastError());
}

}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_transform_calibration(int in_w, int in_h, double resize_ratio, int crop_levels, const double intrinsics_in[4], double image_size_out[2],
                                    double intrinsics_out[4], int *out_w, int *out_h) {
  return guarded([&] {
    const Sizes s = transformedSizes(in_w, in_h, resize_ratio, crop_levels);
    // CameraCalibration::resize (camera_calibration.cpp:33-42), pinhole: the size (not truncated) and all four intrinsics scale
    const double size[2] = {in_w * resize_ratio, in_h * resize_ratio};
    for (int i = 0; i < 4 && intrinsics_in && intrinsics_out; ++i) intrinsics_out[i] = intrinsics_in[i] * resize_ratio;
    // CameraCalibration::crop (:44-46): the size alone, the origin stays at the top-left pixel
    for (int i = 0; i < 2 && image_size_out; ++i)
      image_size_out[i] = static_cast<double>((static_cast<size_t>(size[i]) >> crop_levels) << crop_levels);
    if (out_w) *out_w = s.out_w;
    if (out_h) *out_h = s.out_h;
  });
}

int dsopp_hip_transformer_create(int device, void *stream, int in_w, int in_h, double resize_ratio, int crop_levels, dsopp_hip_transformer **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    const Sizes s = transformedSizes(in_w, in_h, resize_ratio, crop_levels);
    auto t = std::make_unique<dsopp_hip_transformer>();
    t->sr.init(device, stream);
    t->in_w = in_w;
    t->in_h = in_h;
    t->resized_w = s.resized_w;
    t->resized_h = s.resized_h;
    t->out_w = s.out_w;
    t->out_h = s.out_h;
    if (s.out_w != in_w || s.out_h != in_h || s.resized_w != in_w || s.resized_h != in_h) {
      const size_t words = 2 * (static_cast<size_t>(s.out_w) + s.out_h);
      std::vector<uint32_t> table(words);
      for (int interpolation : {kTransformLinear, kTransformNearest}) {
        axisTable(in_w, s.resized_w, s.out_w, interpolation, 1u, table.data());
        axisTable(in_h, s.resized_h, s.out_h, interpolation, static_cast<uint32_t>(in_w), table.data() + 2 * static_cast<size_t>(s.out_w));
        t->table[interpolation].alloc(words * sizeof(uint32_t));
        HIP_CHECK(hipMemcpyAsync(t->table[interpolation].get(), table.data(), words * sizeof(uint32_t), hipMemcpyHostToDevice, t->sr.stream));
        t->sr.sync();  // (the host vector is filled again)
      }
    }
    *out = t.release();
  });
}

void dsopp_hip_transformer_destroy(dsopp_hip_transformer *t) {
  if (!t) return;
  (void)hipSetDevice(t->sr.device);
  if (t->sr.stream) (void)hipStreamSynchronize(t->sr.stream);
  delete t;
}

int dsopp_hip_transformer_sizes(const dsopp_hip_transformer *t, int *in_w, int *in_h, int *resized_w, int *resized_h, int *out_w, int *out_h) {
  return guarded([&] {
    checkHandle(t);
    if (in_w) *in_w = t->in_w;
    if (in_h) *in_h = t->in_h;
    if (resized_w) *resized_w = t->resized_w;
    if (resized_h) *resized_h = t->resized_h;
    if (out_w) *out_w = t->out_w;
    if (out_h) *out_h = t->out_h;
  });
}

int dsopp_hip_transformer_transform_image(dsopp_hip_transformer *t, const uint8_t *image_host, uint8_t *out_host) {
  return guarded([&] { transformHost(t, image_host, out_host, kTransformLinear); });
}

int dsopp_hip_transformer_transform_mask(dsopp_hip_transformer *t, const uint8_t *mask_host, uint8_t *out_host) {
  return guarded([&] { transformHost(t, mask_host, out_host, kTransformNearest); });
}

int dsopp_hip_transformer_transform_device(dsopp_hip_transformer *t, const void *in_dev, void *out_dev, int interpolation, void *stream) {
  return guarded([&] {
    checkHandle(t);
    if (!in_dev || !out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    t->sr.use();
    enqueueTransform(t, static_cast<const uint8_t *>(in_dev), static_cast<uint8_t *>(out_dev), interpolation,
                     stream ? static_cast<hipStream_t>(stream) : t->sr.stream);
  });
}

}  // extern "C"
