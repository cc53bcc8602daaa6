// Semantic segmentation on the device: the per-camera semantics object, the per-frame class image and camera masks of a pyramid, and
// the dsopp_hip_semantics_* / dsopp_hip_pyramid_{set_semantics, get_semantics, get_mask} entry points.
//   class image undistorted per frame              src/sensors/camera/src/camera.cpp:57-65
//   CameraMask::filterSemanticObjects              src/sensors/camera_calibration/src/camera_mask.cpp:31-39
//   the frame's mask pyramid                       src/features/src/camera_features.cpp:71-84
//   SemanticFilter::is_filtered_                   src/common/semantics/src/semantic_filter.cpp:5-14
//
// The class image takes the path of a camera image in dsopp_hip_pyramid_build_undistorted: pinned buffer, DMA, the undistorter's remap
// kernel on the pyramid's stream, and with a transformer (dsopp_hip_semantics_create_transformed) its nearest resize and crop behind
// that (runMaskTransformers, camera.cpp:62).  Then ONE launch writes the mask lane of the texels of every level and the level-0 mask bytes.  Every
// level is formed from level 0 directly (the reference resizes the finest mask to every size, it does not chain), so no level waits for
// another: a thread of level l >= 1 filters its own four level-0 pixels.  All integer: m_l = (sum of the 2 x 2 block around the sample
// point + 2) >> 2, which is cv::resize(INTER_LINEAR) at the ratio 2^-l — the sample point (x + 0.5) 2^l - 0.5 lies midway between two
// pixel centres, the two 11-bit weights per axis are equal (1024), and (1024 * 1024 * sum + 2^21) >> 22 = (sum + 2) >> 2.
#include <algorithm>
#include <memory>

#include "pyramid.hpp"
#include "transform.hpp"
#include "undistort.hpp"

struct dsopp_hip_semantics {
  dsopp_hip::StreamRef sr;
  int width = 0, height = 0, levels = 0;
  dsopp_hip::DeviceMem<uint8_t> static_mask;  // W x H bytes (all 255 without a static mask)
  dsopp_hip::DeviceMem<uint8_t> is_filtered;  // 256 bytes; null = filterBySemantic() is false
  const dsopp_hip_undistorter *undistorter = nullptr;  // borrowed; null = class images arrive undistorted
  const dsopp_hip_transformer *transformer = nullptr;  // borrowed; null = class images are neither resized nor cropped
};

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;

struct MaskArgs {
  const uint8_t *static_mask;
  const uint8_t *cls;          // undistorted class image, null = none
  const uint8_t *is_filtered;  // 256 bytes, null = no filter
  uint8_t *mask0;              // level-0 mask bytes
  int levels, width, height;
  unsigned first_block[DSOPP_HIP_MAX_LEVELS + 1];  // workgroups [first_block[l], first_block[l + 1]) write level l
  void *tex[DSOPP_HIP_MAX_LEVELS];
};

/** one level: thread `idx` of the level's range writes the mask lane of texel idx */
template <typename S, int L>
__device__ __forceinline__ void maskLevel(const MaskArgs &a, const uint8_t *filtered, unsigned idx) {
  const int W = a.width, wl = a.width >> L, hl = a.height >> L;
  if (idx >= static_cast<unsigned>(wl) * static_cast<unsigned>(hl)) return;
  GlobalPtr<const uint8_t> st = glb(a.static_mask), cls = glb(a.cls);
  auto m0 = [&](size_t i) -> unsigned { return (cls && filtered[cls[i]]) ? 0u : st[i]; };
  unsigned m;
  if (L == 0) {
    m = m0(idx);
    glb(a.mask0)[idx] = static_cast<uint8_t>(m);
  } else {
    const int y = static_cast<int>(idx / static_cast<unsigned>(wl)), x = static_cast<int>(idx - static_cast<unsigned>(y) * wl);
    // cx + 1 <= 2^L (wl - 1) + 2^(L-1) < W and alike for cy: inside the image because W and H are multiples of 2^L (checked at create)
    const int cx = (x << L) + (1 << (L - 1)) - 1, cy = (y << L) + (1 << (L - 1)) - 1;
    const size_t i = static_cast<size_t>(cy) * W + cx;
    m = (m0(i) + m0(i + 1) + m0(i + W) + m0(i + W + 1) + 2u) >> 2;
  }
  glb(static_cast<Texel<S> *>(a.tex[L]))[idx].mask = m ? S(1) : S(0);
}

template <typename S>
__global__ void __launch_bounds__(kBlock) semanticMasksKernel(MaskArgs a) {
  __shared__ uint8_t filtered[256];
  filtered[threadIdx.x] = a.is_filtered ? glb(a.is_filtered)[threadIdx.x] : uint8_t(0);
  __syncthreads();
  const unsigned b = blockIdx.x;
  if (b < a.first_block[1]) {
    maskLevel<S, 0>(a, filtered, b * kBlock + threadIdx.x);
  } else if (b < a.first_block[2]) {
    maskLevel<S, 1>(a, filtered, (b - a.first_block[1]) * kBlock + threadIdx.x);
  } else if (b < a.first_block[3]) {
    maskLevel<S, 2>(a, filtered, (b - a.first_block[2]) * kBlock + threadIdx.x);
  } else if (b < a.first_block[4]) {
    maskLevel<S, 3>(a, filtered, (b - a.first_block[3]) * kBlock + threadIdx.x);
  } else {
    maskLevel<S, 4>(a, filtered, (b - a.first_block[4]) * kBlock + threadIdx.x);
  }
}

template <typename S>
__global__ void __launch_bounds__(kBlock) getMaskKernel(const Texel<S> *__restrict__ tex, uint8_t *__restrict__ out, size_t n) {
  const size_t i = static_cast<size_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i < n) out[i] = glb(tex)[i].mask != S(0) ? 1 : 0;
}

/** the class image of n bytes through the pyramid's pinned semantics buffer into dst_dev, enqueued on the pyramid's stream */
void uploadClassImage(dsopp_hip_pyramid *p, uint8_t *dst_dev, const uint8_t *host, size_t n) {
  hipStream_t st = p->sr.stream;
  // the buffer's previous upload (last frame's: long done) — not the stream, on which this frame's build may still run
  if (p->semantics_uploaded) HIP_CHECK(hipEventSynchronize(p->semantics_uploaded.h));
  p->h_semantics.reserve(n);
  const size_t pieces = n >= (size_t(1) << 19) ? 4 : 1;  // as the camera image: the DMA of a piece runs while the host copies the next
  const size_t piece = ((n + pieces - 1) / pieces + 4095) & ~static_cast<size_t>(4095);
  for (size_t off = 0; off < n; off += piece) {
    const size_t len = std::min(piece, n - off);
    copyToPinned(p->h_semantics.get() + off, host + off, len);
    HIP_CHECK(hipMemcpyAsync(dst_dev + off, p->h_semantics.get() + off, len, hipMemcpyHostToDevice, st));
  }
  HIP_CHECK(hipEventRecord(p->semantics_uploaded.get(hipEventDisableTiming), st));
}

template <typename S>
void launchMasks(dsopp_hip_pyramid *p, const dsopp_hip_semantics *s, const uint8_t *cls_dev) {
  MaskArgs a;
  std::memset(&a, 0, sizeof(a));
  a.static_mask = s->static_mask.get();
  a.cls = s->is_filtered ? cls_dev : nullptr;  // without a filter the class image decides nothing
  a.is_filtered = s->is_filtered.get();
  a.mask0 = p->mask0_u8.get();
  a.levels = p->levels;
  a.width = p->width;
  a.height = p->height;
  unsigned blocks = 0;
  for (int l = 0; l <= DSOPP_HIP_MAX_LEVELS; ++l) {
    a.first_block[l] = blocks;
    if (l < p->levels) {
      a.tex[l] = p->texels[l].get();
      blocks += static_cast<unsigned>((static_cast<size_t>(p->w(l)) * p->h(l) + kBlock - 1) / kBlock);
    }
  }
  semanticMasksKernel<S><<<blocks, kBlock, 0, p->sr.stream>>>(a);
  HIP_CHECK(hipGetLastError());
}

/** what both creators share; the sizes of `undistorter` and `transformer` are the caller's to check */
void createSemantics(int device, void *stream, int width, int height, int levels, const uint8_t *static_mask_host, const uint8_t *is_filtered256,
                     const dsopp_hip_undistorter *undistorter, const dsopp_hip_transformer *transformer, dsopp_hip_semantics **out) {
  if (!out || width <= 0 || height <= 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "bad semantics dimensions");
  if (levels < 1 || levels > DSOPP_HIP_MAX_LEVELS) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d levels: 1 .. %d", levels, DSOPP_HIP_MAX_LEVELS);
  const int step = 1 << (levels - 1);
  if (width % step || height % step)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d x %d is not divisible by %d: the masks of %d levels would not have the sizes of the image levels", width,
         height, step, levels);
  if (undistorter && undistorter->sr.device != device)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the undistorter lives on device %d, not %d", undistorter->sr.device, device);
  auto s = std::make_unique<dsopp_hip_semantics>();
  s->sr.init(device, stream);
  s->width = width;
  s->height = height;
  s->levels = levels;
  s->undistorter = undistorter;
  s->transformer = transformer;
  const size_t n = static_cast<size_t>(width) * height;
  s->static_mask.alloc(n);
  if (static_mask_host)
    HIP_CHECK(hipMemcpyAsync(s->static_mask.get(), static_mask_host, n, hipMemcpyHostToDevice, s->sr.stream));
  else
    HIP_CHECK(hipMemsetAsync(s->static_mask.get(), 255, n, s->sr.stream));  // CameraMask(rows, cols)
  if (is_filtered256) {
    s->is_filtered.alloc(256);
    HIP_CHECK(hipMemcpyAsync(s->is_filtered.get(), is_filtered256, 256, hipMemcpyHostToDevice, s->sr.stream));
  }
  s->sr.sync();
  *out = s.release();
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_semantics_create(int device, void *stream, int width, int height, int levels, const uint8_t *static_mask_host,
                               const uint8_t *is_filtered256, const dsopp_hip_undistorter *undistorter, dsopp_hip_semantics **out) {
  return guarded([&] {
    if (undistorter && (undistorter->out_w != width || undistorter->out_h != height))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the undistorter writes %d x %d, the masks are %d x %d", undistorter->out_w, undistorter->out_h, width, height);
    createSemantics(device, stream, width, height, levels, static_mask_host, is_filtered256, undistorter, nullptr, out);
  });
}

int dsopp_hip_semantics_create_transformed(int device, void *stream, int levels, const uint8_t *static_mask_host, const uint8_t *is_filtered256,
                                           const dsopp_hip_undistorter *undistorter, const dsopp_hip_transformer *transformer,
                                           dsopp_hip_semantics **out) {
  return guarded([&] {
    if (!transformer) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null transformer");
    if (undistorter && (undistorter->out_w != transformer->in_w || undistorter->out_h != transformer->in_h))
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the undistorter writes %d x %d, the transformer reads %d x %d", undistorter->out_w, undistorter->out_h,
           transformer->in_w, transformer->in_h);
    if (transformer->sr.device != device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the transformer lives on device %d, not %d", transformer->sr.device, device);
    createSemantics(device, stream, transformer->out_w, transformer->out_h, levels, static_mask_host, is_filtered256, undistorter, transformer, out);
  });
}

void dsopp_hip_semantics_destroy(dsopp_hip_semantics *s) {
  if (!s) return;
  (void)hipSetDevice(s->sr.device);
  if (s->sr.stream) (void)hipStreamSynchronize(s->sr.stream);
  delete s;
}

int dsopp_hip_pyramid_set_semantics(dsopp_hip_pyramid *p, const dsopp_hip_semantics *s, const uint8_t *class_image_host) {
  return guarded([&] {
    if (!p || !s) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (s->sr.device != p->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the semantics object lives on device %d, the pyramid on %d", s->sr.device, p->sr.device);
    if (s->width != p->width || s->height != p->height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the semantics object is %d x %d, the pyramid %d x %d", s->width, s->height, p->width, p->height);
    if (p->levels > s->levels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid has %d levels, the semantics object was created for %d", p->levels, s->levels);
    p->sr.use();
    hipStream_t st = p->sr.stream;
    const size_t n = static_cast<size_t>(p->width) * p->height;
    if (!p->mask0_u8) p->mask0_u8.alloc(n);
    const uint8_t *cls_dev = nullptr;
    p->has_semantics = false;
    if (class_image_host) {
      if (!p->semantics_u8) p->semantics_u8.alloc(n);
      const dsopp_hip_undistorter *u = s->undistorter;
      const dsopp_hip_transformer *t = s->transformer && !s->transformer->identity() ? s->transformer : nullptr;
      // class image -> [remap] -> [nearest resize + crop] -> semantics_u8 (camera.cpp:57-65); a stage that is not there hands its buffer on
      uint8_t *untransformed_dev = p->semantics_u8.get();
      if (t)
        untransformed_dev = reserveImage(p->semantics_untransformed_u8, p->semantics_untransformed_bytes, static_cast<size_t>(t->in_w) * t->in_h, st);
      if (u) {
        const size_t n_in = static_cast<size_t>(u->in_w) * u->in_h;
        reserveImage(p->semantics_in_u8, p->semantics_in_bytes, n_in, st);
        uploadClassImage(p, p->semantics_in_u8.get(), class_image_host, n_in);
        enqueueUndistort(u, p->semantics_in_u8.get(), untransformed_dev, st);
      } else {
        uploadClassImage(p, untransformed_dev, class_image_host, t ? static_cast<size_t>(t->in_w) * t->in_h : n);
      }
      if (t) enqueueTransform(t, untransformed_dev, p->semantics_u8.get(), kTransformNearest, st);
      cls_dev = p->semantics_u8.get();
    }
    if (p->dtype == DSOPP_HIP_F64)
      launchMasks<double>(p, s, cls_dev);
    else
      launchMasks<float>(p, s, cls_dev);
    p->has_semantics = cls_dev != nullptr;
    p->has_mask0 = true;
    p->markReady();
  });
}

int dsopp_hip_pyramid_get_semantics(dsopp_hip_pyramid *p, uint8_t *out_host, int *present) {
  return guarded([&] {
    if (!p) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null pyramid");
    if (present) *present = p->has_semantics ? 1 : 0;
    if (!p->has_semantics || !out_host) return;
    p->sr.use();
    HIP_CHECK(hipMemcpyAsync(out_host, p->semantics_u8.get(), static_cast<size_t>(p->width) * p->height, hipMemcpyDeviceToHost, p->sr.stream));
    p->sr.sync();
  });
}

int dsopp_hip_pyramid_get_mask(dsopp_hip_pyramid *p, int level, uint8_t *out_host) {
  return guarded([&] {
    if (!p || !out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (level < 0 || level >= p->levels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "level %d out of range [0,%d)", level, p->levels);
    p->sr.use();
    const size_t n = static_cast<size_t>(p->w(level)) * p->h(level);
    DeviceMem<uint8_t> tmp;
    tmp.alloc(n);
    const unsigned grid = static_cast<unsigned>((n + kBlock - 1) / kBlock);
    if (p->dtype == DSOPP_HIP_F64)
      getMaskKernel<double><<<grid, kBlock, 0, p->sr.stream>>>(static_cast<const Texel<double> *>(p->texels[level].get()), tmp.get(), n);
    else
      getMaskKernel<float><<<grid, kBlock, 0, p->sr.stream>>>(static_cast<const Texel<float> *>(p->texels[level].get()), tmp.get(), n);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(out_host, tmp.get(), n, hipMemcpyDeviceToHost, p->sr.stream));
    p->sr.sync();
  });
}

}  // extern "C"
