// Image undistortion on the device: the remap every camera frame, the static mask and the vignette go through before anything else sees
// them, and the dsopp_hip_undistorter_* entry points.
//   Undistorter::undistort = cv::remap(img, dst, remapX, remapY, INTER_LINEAR, BORDER_REFLECT_101)
//                                                   src/sensors/camera_calibration/src/undistorter.cpp:7-18
//   per frame                                       src/sensors/camera/src/camera.cpp:70
//   mask and vignette, once                         src/sensors_builder/src/camera_fabric.cpp:164-167
//   the two CV_32F maps (constructRemaps)           src/sensors/camera_calibration/include/sensors/camera_calibration/undistorter/undistorter.hpp:69-142
//
// The arithmetic is the fixed-point one of an 8-bit bilinear remap, all integer (DESIGN.md section 4 states it in full): coordinates
// rounded half to even to 1/32 pixel, each of the four taps reflected on its own, weights (32 - fx)(32 - fy) * 32 ... summing to 32768,
// out = (sum + 16384) >> 15.  Every tap index after reflection is a constant of the map, so create() folds the float maps once into one
// 8-byte entry per output pixel:
//   word 0   y0 * in_w + x0, the offset of the first tap
//   word 1   fx (bits 0-4) | fy (bits 8-12) | x1 < x0 (bit 16) | y1 < y0 (bit 17)
// x1 - x0 and y1 - y0 are +-1 for every image of at least 2 x 2 pixels, -1 exactly where the reflection turned the pair round.  The
// per-frame kernel then has no float arithmetic and no border branch.  It sees the output as N = out_w * out_h bytes in a row: a thread
// loads the 32 bytes of table of 4 consecutive pixels as two 16-byte words (a wave: 2 KiB contiguous), gathers its 16 taps as bytes
// (neighbouring lanes share lines: L2 serves them) and stores one 32-bit word (a wave: 256 contiguous bytes).  The N mod 4 bytes that
// are left are stored one by one by the thread behind the last full word.
#include "undistort.hpp"

#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "pyramid.hpp"
#include "remap_fold.hpp"

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr float kMaxCoordinate = 1048576.0f;  // 2^20: 32 * coordinate stays far inside int32

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ unsigned remapPixel(GlobalPtr<const uint8_t> src, int in_w, unsigned offset, unsigned bits) {
  const int fx = bits & (kRemapOne - 1), fy = (bits >> kRemapFyShift) & (kRemapOne - 1);
  const int dx = (bits & kRemapFlipX) ? -1 : 1;
  const int dy = (bits & kRemapFlipY) ? -in_w : in_w;
  GlobalPtr<const uint8_t> p = src + offset;
  const int p00 = p[0], p01 = p[dx], p10 = p[dy], p11 = p[dx + dy];
  const int gx = kRemapOne - fx, gy = kRemapOne - fy;
  const int sum = gx * gy * kRemapOne * p00 + fx * gy * kRemapOne * p01 + gx * fy * kRemapOne * p10 + fx * fy * kRemapOne * p11;
  return static_cast<unsigned>((sum + 16384) >> 15);
}

// (the parameters are plain pointers — a kernel's name must be the same in the host and the device pass — and are typed as HBM inside)
__global__ void __launch_bounds__(kBlock) undistortKernel(const unsigned *__restrict__ table_, const uint8_t *__restrict__ src_, int in_w,
                                                          unsigned *__restrict__ out_, unsigned words, unsigned tail) {
  GlobalPtr<const uint8_t> src = glb(src_);
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    GlobalPtr<const u32x4> e = reinterpret_cast<GlobalPtr<const u32x4>>(glb(table_)) + 2 * static_cast<size_t>(t);
    const u32x4 a = e[0], b = e[1];
    glb(out_)[t] = remapPixel(src, in_w, a.x, a.y) | (remapPixel(src, in_w, a.z, a.w) << 8) | (remapPixel(src, in_w, b.x, b.y) << 16) |
                   (remapPixel(src, in_w, b.z, b.w) << 24);
  } else if (t == words) {
    const size_t first = 4 * static_cast<size_t>(words);
    for (unsigned k = 0; k < tail; ++k) {
      const u32x2 e = reinterpret_cast<GlobalPtr<const u32x2>>(glb(table_))[first + k];
      reinterpret_cast<GlobalPtr<uint8_t>>(glb(out_))[first + k] = static_cast<uint8_t>(remapPixel(src, in_w, e.x, e.y));
    }
  }
}

bool usable(float c) { return std::isfinite(c) && std::fabs(c) <= kMaxCoordinate; }

void checkHandle(const dsopp_hip_undistorter *u) {
  if (!u) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null undistorter");
}

}  // namespace

void enqueueUndistort(const dsopp_hip_undistorter *u, const uint8_t *in_dev, uint8_t *out_dev, hipStream_t stream) {
  if ((reinterpret_cast<uintptr_t>(in_dev) | reinterpret_cast<uintptr_t>(out_dev)) & 3)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device images must be 4-byte aligned");
  const size_t n = static_cast<size_t>(u->out_w) * u->out_h;
  const unsigned words = static_cast<unsigned>(n / 4), tail = static_cast<unsigned>(n % 4);
  const unsigned threads = words + (tail ? 1u : 0u);
  undistortKernel<<<(threads + kBlock - 1) / kBlock, kBlock, 0, stream>>>(u->table.get(), in_dev, u->in_w, reinterpret_cast<unsigned *>(out_dev), words, tail);
  HIP_CHECK(hipGetLastError());
}

}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_undistorter_create(int device, void *stream, int in_w, int in_h, int out_w, int out_h, const float *map_x, const float *map_y,
                                 dsopp_hip_undistorter **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (in_w < 2 || in_h < 2) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the input image is %d x %d: reflection needs 2 x 2", in_w, in_h);
    if (out_w < 1 || out_h < 1) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the output image is %d x %d", out_w, out_h);
    if (static_cast<long long>(in_w) * in_h > INT_MAX || static_cast<long long>(out_w) * out_h > INT_MAX)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image too large");
    if (!map_x != !map_y) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "one map without the other");
    if (!map_x && (in_w != out_w || in_h != out_h))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the identity needs equal sizes, not %d x %d -> %d x %d", in_w, in_h, out_w, out_h);
    const size_t n = static_cast<size_t>(out_w) * out_h;
    std::vector<uint32_t> table(2 * n);
    for (size_t i = 0; i < n; ++i) {
      // no maps = Undistorter::Identity (undistorter.cpp:8-10,20-22): the image is cloned, every pixel maps to itself
      const float cx = map_x ? map_x[i] : static_cast<float>(i % out_w), cy = map_y ? map_y[i] : static_cast<float>(i / out_w);
      if (!usable(cx) || !usable(cy))
        fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "map entry %zu is (%g, %g): not finite or beyond 2^20", i, static_cast<double>(cx), static_cast<double>(cy));
      foldMapEntry(cx, cy, in_w, in_h, table[2 * i], table[2 * i + 1]);
    }
    auto u = std::make_unique<dsopp_hip_undistorter>();
    u->sr.init(device, stream);
    u->in_w = in_w;
    u->in_h = in_h;
    u->out_w = out_w;
    u->out_h = out_h;
    u->table.alloc(table.size() * sizeof(uint32_t));
    HIP_CHECK(hipMemcpyAsync(u->table.get(), table.data(), table.size() * sizeof(uint32_t), hipMemcpyHostToDevice, u->sr.stream));
    u->sr.sync();
    *out = u.release();
  });
}

void dsopp_hip_undistorter_destroy(dsopp_hip_undistorter *u) {
  if (!u) return;
  (void)hipSetDevice(u->sr.device);
  if (u->sr.stream) (void)hipStreamSynchronize(u->sr.stream);
  delete u;
}

int dsopp_hip_undistorter_sizes(const dsopp_hip_undistorter *u, int *in_w, int *in_h, int *out_w, int *out_h) {
  return guarded([&] {
    checkHandle(u);
    if (in_w) *in_w = u->in_w;
    if (in_h) *in_h = u->in_h;
    if (out_w) *out_w = u->out_w;
    if (out_h) *out_h = u->out_h;
  });
}

int dsopp_hip_undistorter_undistort(dsopp_hip_undistorter *u, const uint8_t *image_host, uint8_t *out_host) {
  return guarded([&] {
    checkHandle(u);
    if (!image_host || !out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    u->sr.use();
    const size_t n_in = static_cast<size_t>(u->in_w) * u->in_h, n_out = static_cast<size_t>(u->out_w) * u->out_h;
    if (!u->d_in) u->d_in.alloc(n_in);
    if (!u->d_out) u->d_out.alloc(n_out);
    HIP_CHECK(hipMemcpyAsync(u->d_in.get(), image_host, n_in, hipMemcpyHostToDevice, u->sr.stream));
    enqueueUndistort(u, u->d_in.get(), u->d_out.get(), u->sr.stream);
    HIP_CHECK(hipMemcpyAsync(out_host, u->d_out.get(), n_out, hipMemcpyDeviceToHost, u->sr.stream));
    u->sr.sync();
  });
}

int dsopp_hip_undistorter_undistort_device(dsopp_hip_undistorter *u, const void *image_dev, void *out_dev, void *stream) {
  return guarded([&] {
    checkHandle(u);
    if (!image_dev || !out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    u->sr.use();
    enqueueUndistort(u, static_cast<const uint8_t *>(image_dev), static_cast<uint8_t *>(out_dev),
                     stream ? static_cast<hipStream_t>(stream) : u->sr.stream);
  });
}

}  // extern "C"
