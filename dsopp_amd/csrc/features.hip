// Tracking-feature extraction on the device: the reference's default extractor and what the tracker does with its result.
//   SobelTrackingFeaturesExtractor::extract     — src/features/src/sobel_tracking_features_extractor.cpp:75-134
//   CameraMask::getEroded (4, then 3)           — src/sensors/camera_calibration/src/camera_mask.cpp:20-29
//   buildFeatures + pushImmatureLandmarks       — src/tracker/tracker/internal/tracker/build_features.hpp:20-32,
//                                                 src/track/frames/src/active_keyframe.cpp:95-112
//
// Per call: the 8-bit image is uploaded, sobelKernel writes the int16 L1 gradient norm |Sx| + |Sy| (and on the first call a
// 2041-bin histogram of it, from which the quantile threshold is exact: the norm is an integer below 2041), windowFirstHitKernel
// gives every window its first pixel in raster order above the threshold and inside the eroded mask (one wave per window,
// 64 pixels per ballot), and a device select keeps the hits in window order.  The hit count and the list come back to the host,
// where the threshold update and std::shuffle run in the library's own C++ (libstdc++'s permutation, as in the reference).
// The final list stays on the device for dsopp_hip_immature_set_create_from_features.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <memory>
#include <numeric>
#include <random>
#include <vector>

#include "common.hpp"
#include "features.hpp"
#include "immature_set.hpp"
#include "pyramid.hpp"

namespace dsopp_hip {
namespace {

constexpr int kGradBins = 2041;   // |Sx| + |Sy| <= 4 * 255 + 4 * 255
constexpr int kErodeRadius = 7;   // getEroded(4) then getEroded(3): a 15 x 15 rectangle
constexpr int kBlock = 256;

// cv::Sobel(img, CV_16S, 1, 0) / (0, 1) with BORDER_REFLECT_101, then |Sx| + |Sy| (sobel_tracking_features_extractor.cpp:80-90).
// HIST: also counts the norms into bins (first call: the quantile threshold), LDS bins per workgroup, then global atomics.
template <bool HIST>
__global__ void __launch_bounds__(kBlock) sobelKernel(const uint8_t *__restrict__ img, int W, int H, int16_t *__restrict__ g,
                                                      unsigned *__restrict__ hist) {
  __shared__ unsigned bins[HIST ? kGradBins : 1];
  if (HIST) {
    for (int i = threadIdx.x; i < kGradBins; i += kBlock) bins[i] = 0;
    __syncthreads();
  }
  const int n = W * H;
  for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
    const int y = i / W, x = i - y * W;
    const int xm = x > 0 ? x - 1 : 1, xp = x < W - 1 ? x + 1 : W - 2;  // reflect 101: -1 -> 1, W -> W - 2
    const int ym = y > 0 ? y - 1 : 1, yp = y < H - 1 ? y + 1 : H - 2;
    const uint8_t *rm = img + ym * W, *r0 = img + y * W, *rp = img + yp * W;
    const int sx = (rm[xp] - rm[xm]) + 2 * (r0[xp] - r0[xm]) + (rp[xp] - rp[xm]);
    const int sy = (rp[xm] + 2 * rp[x] + rp[xp]) - (rm[xm] + 2 * rm[x] + rm[xp]);
    const int v = abs(sx) + abs(sy);
    g[i] = static_cast<int16_t>(v);
    if (HIST) atomicAdd(&bins[v], 1u);
  }
  if (HIST) {
    __syncthreads();
    for (int i = threadIdx.x; i < kGradBins; i += kBlock)
      if (bins[i]) atomicAdd(&hist[i], bins[i]);
  }
}

// Separable 15-tap erosion of the mask with the image edge never eroding (cv::erode's default border value is +max):
// pass 0 reads the caller's mask bytes along rows, pass 1 the row result along columns.  Output 1 = valid, 0 = masked.
template <bool ROWS>
__global__ void __launch_bounds__(kBlock) erodeKernel(const uint8_t *__restrict__ in, int W, int H, uint8_t *__restrict__ out) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= W * H) return;
  const int y = i / W, x = i - y * W;
  uint8_t v = 1;
  if (ROWS) {
    const int x0 = max(0, x - kErodeRadius), x1 = min(W - 1, x + kErodeRadius);
    for (int k = x0; k <= x1; ++k) v &= in[y * W + k] != 0;
  } else {
    const int y0 = max(0, y - kErodeRadius), y1 = min(H - 1, y + kErodeRadius);
    for (int k = y0; k <= y1; ++k) v &= in[k * W + x] != 0;
  }
  out[i] = v;
}

// findPointInWindow (sobel_tracking_features_extractor.cpp:55-67) for every window: one wave per window walks its ws x ws
// pixels in raster order, 64 per ballot; the lowest set bit is the first pixel with g > thr inside the eroded mask.
// hit[w] = y * W + x of that pixel, or -1.  Windows are numbered in the reference's raster order (nwx per row).
__global__ void __launch_bounds__(kBlock) windowFirstHitKernel(const int16_t *__restrict__ g, const uint8_t *__restrict__ valid, int W, int ws,
                                                               int nwx, int nwin, int thr, int *__restrict__ hit) {
  const int w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (w >= nwin) return;  // (wave-uniform)
  const int y0 = (w / nwx) * ws, x0 = (w % nwx) * ws;
  const int area = ws * ws;
  int result = -1;
  for (int base = 0; base < area; base += 64) {
    const int p = base + lane;
    bool ok = false;
    if (p < area) {
      const int idx = (y0 + p / ws) * W + x0 + p % ws;
      ok = g[idx] > thr && (!valid || valid[idx]);
    }
    const unsigned long long b = __ballot(ok);
    if (b) {
      const int first = base + __ffsll(b) - 1;
      result = (y0 + first / ws) * W + x0 + first % ws;
      break;
    }
  }
  if (lane == 0) hit[w] = result;
}

struct IsHit {
  __host__ __device__ bool operator()(int v) const { return v >= 0; }
};

// CameraModelBase::insideCameraROI (camera_model_base.hpp:52-60, border 4) of an integer pixel: what buildFeatures keeps
struct InsideRoi {
  int W, H;
  __host__ __device__ int operator()(int idx) const {
    const int y = idx / W, x = idx - y * W;
    return (x >= 4 && y >= 4 && x <= W - 5 && y <= H - 5) ? 1 : 0;
  }
};

// buildFeatures + pushImmatureLandmarks, one thread per extracted feature: the ROI drops are compacted in list order (pos = exclusive
// scan of InsideRoi), direction = ((x - cx) / fx, (y - cy) / fy, 1) with the inverse focal lengths precomputed (PinholeCamera::unproject),
// patch = level-0 intensity at the 8 pattern pixels, gradient = sum of their (dI/dx, dI/dy) from zero in pattern order in the image
// scalar (separatePixelPatch, active_keyframe.cpp:20-29).  Output: the set's input planes projection 2n | direction 3n | patch 8n | gradient 2n.
template <typename S>
__global__ void __launch_bounds__(kBlock) buildImmatureKernel(const int *__restrict__ list, const int *__restrict__ pos, int n_list, int W, int H,
                                                              const Texel<S> *__restrict__ tex, double cx, double cy, double ifx, double ify, int n,
                                                              double *__restrict__ in) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_list) return;
  const int idx = list[i];
  if (!InsideRoi{W, H}(idx)) return;
  const int j = pos[i];
  const int y = idx / W, x = idx - y * W;
  const double u = x, v = y;
  in[2 * j] = u;
  in[2 * j + 1] = v;
  double *dir = in + 2 * n + 3 * j;
  dir[0] = (u - cx) * ifx;
  dir[1] = (v - cy) * ify;
  dir[2] = 1.0;
  double *patch = in + 5 * n + 8 * j;
  S gx = S(0), gy = S(0);
  constexpr int kPx[8] = {0, -1, 1, -2, 0, 2, -1, 0}, kPy[8] = {2, 1, 1, 0, 0, 0, -1, -2};  // pattern.hpp:21-32
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const Texel<S> t = loadTexel(tex + (y + kPy[k]) * W + x + kPx[k]);
    patch[k] = static_cast<double>(t.I);
    gx += t.Ix;
    gy += t.Iy;
  }
  in[13 * n + 2 * j] = static_cast<double>(gx);
  in[13 * n + 2 * j + 1] = static_cast<double>(gy);
}

inline unsigned gridFor(long n) { return static_cast<unsigned>(std::max<long>(1, (n + kBlock - 1) / kBlock)); }

/** The threshold update of the reference (calculateThreshold, sobel_tracking_features_extractor.cpp:26-29), int / int
 *  divisions included.  Where the reference is undefined (a zero divisor: SIGFPE on x86; a non-finite or out-of-range quotient)
 *  the threshold is kept: the one deliberate deviation. */
int updatedThreshold(int num_pixels, int desired, int found, int thr) {
  if (found == 0 || desired == 0) return thr;
  const double t = thr * std::log(num_pixels / desired) / std::log(num_pixels / found);
  if (!std::isfinite(t) || t >= 2147483648.0 || t <= -2147483649.0) return thr;
  return static_cast<int>(t);
}

/** SobelTrackingFeaturesExtractor::extract over the 8-bit image img_dev, which the extractor's stream may read */
void sobelExtract(dsopp_hip_feature_extractor *ex, const uint8_t *img_dev, int32_t capacity, double *xy, int32_t *n) {
  hipStream_t st = ex->sr.stream;
  const int W = ex->width, H = ex->height, N = W * H;
  // everything below is computed into locals and committed at the end: a failed call leaves the state as it was
  bool initialized = ex->initialized;
  int thr = ex->threshold, ws = ex->window_size;
  double density = ex->density;
  if (!initialized) {
    HIP_CHECK(hipMemsetAsync(ex->d_hist.ptr, 0, kGradBins * sizeof(unsigned), st));
    sobelKernel<true><<<std::min(gridFor(N), 256u), kBlock, 0, st>>>(img_dev, W, H, ex->d_grad.ptr, ex->d_hist.ptr);
    HIP_CHECK(hipGetLastError());
    ex->h_hist.reserve(kGradBins * sizeof(unsigned));
    HIP_CHECK(hipMemcpyAsync(ex->h_hist.get(), ex->d_hist.ptr, kGradBins * sizeof(unsigned), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    // quantile(): nth_element at k = (long)(size * q) — the k-th smallest norm, read off the cumulative histogram
    const long k = static_cast<long>(static_cast<double>(N) * ex->quantile);
    const unsigned *h = ex->h_hist.get();
    long cum = 0;
    thr = kGradBins - 1;
    for (int b = 0; b < kGradBins; ++b) {
      cum += h[b];
      if (cum > k) {
        thr = b;
        break;
      }
    }
    double potential = std::sqrt(static_cast<double>(N) * (1.0 - ex->quantile) / density);
    if (potential < 1.0) {
      density *= potential * potential / (1.0 * 1.0);
      potential = 1.0;
    }
    ws = static_cast<int>(potential);
    initialized = true;
  } else {
    sobelKernel<false><<<std::min(gridFor(N), 2048u), kBlock, 0, st>>>(img_dev, W, H, ex->d_grad.ptr, nullptr);
    HIP_CHECK(hipGetLastError());
  }

  // windows at y = 0, ws, ... while y + ws < H, the same in x
  const int nwx = (W - 1) / ws, nwy = (H - 1) / ws, nwin = nwx * nwy;
  int found = 0;
  if (nwin > 0) {
    windowFirstHitKernel<<<static_cast<unsigned>((nwin + kBlock / 64 - 1) / (kBlock / 64)), kBlock, 0, st>>>(
        ex->d_grad.ptr, ex->has_mask ? ex->d_valid.ptr : nullptr, W, ws, nwx, nwin, thr, ex->d_hit.ptr);
    HIP_CHECK(hipGetLastError());
    size_t temp_bytes = 0;
    HIP_CHECK(hipcub::DeviceSelect::If(nullptr, temp_bytes, ex->d_hit.ptr, ex->d_list.ptr, ex->d_count.ptr, nwin, IsHit{}, st));
    ex->d_temp.reserve(std::max<size_t>(1, temp_bytes), 0, st);
    HIP_CHECK(hipcub::DeviceSelect::If(ex->d_temp.ptr, temp_bytes, ex->d_hit.ptr, ex->d_list.ptr, ex->d_count.ptr, nwin, IsHit{}, st));
    HIP_CHECK(hipMemcpyAsync(ex->h_count.get(), ex->d_count.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    found = *ex->h_count.get();
  }

  // truncation to (long)density after the shuffle (:128-131)
  const long needed = static_cast<double>(found) > density ? static_cast<long>(density) : found;
  *n = static_cast<int32_t>(needed);
  if (needed > capacity) fail(DSOPP_HIP_ERR_CAPACITY, "capacity %d < %ld features", capacity, needed);

  thr = updatedThreshold(N, static_cast<int>(density), found, thr);

  std::vector<int> perm(static_cast<size_t>(found));
  std::iota(perm.begin(), perm.end(), 0);
  std::shuffle(perm.begin(), perm.end(), std::default_random_engine{});
  std::vector<int> final_list(static_cast<size_t>(needed));
  if (needed > 0) {
    ex->h_list.reserve(static_cast<size_t>(found) * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(ex->h_list.get(), ex->d_list.ptr, static_cast<size_t>(found) * sizeof(int), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    const int *list = ex->h_list.get();
    for (long i = 0; i < needed; ++i) {
      const int idx = list[perm[static_cast<size_t>(i)]];
      final_list[static_cast<size_t>(i)] = idx;
      xy[2 * i] = static_cast<double>(idx % W);
      xy[2 * i + 1] = static_cast<double>(idx / W);
    }
    // the list stays on the device for the immature-landmark build (the stream is idle: the pinned buffer's last upload is done)
    ex->d_final.reserve(static_cast<size_t>(needed), 0, st);
    ex->h_final.reserve(static_cast<size_t>(needed) * sizeof(int));
    std::memcpy(ex->h_final.get(), final_list.data(), static_cast<size_t>(needed) * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(ex->d_final.ptr, ex->h_final.get(), static_cast<size_t>(needed) * sizeof(int), hipMemcpyHostToDevice, st));
  }
  HIP_CHECK(hipEventRecord(ex->final_ready.h, st));

  ex->initialized = initialized;
  ex->threshold = thr;
  ex->window_size = ws;
  ex->density = density;
  ex->found_last = found;
  ex->final_list = std::move(final_list);
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_features_shuffle_order(int32_t n, int32_t *perm) {
  return guarded([&] {
    if (n < 0 || (n > 0 && !perm)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    std::iota(perm, perm + n, 0);
    // std::shuffle(features, std::default_random_engine{}) — a fresh engine per call (sobel_tracking_features_extractor.cpp:92,127)
    std::shuffle(perm, perm + n, std::default_random_engine{});
  });
}

int dsopp_hip_feature_extractor_create(int device, void *stream, int width, int height, double point_density_for_detector,
                                       double quantile_level, dsopp_hip_feature_extractor **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (width < 16 || height < 16 || static_cast<long long>(width) * height > INT_MAX / 2)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image size %d x %d out of range", width, height);
    if (!(point_density_for_detector > 0)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "point_density_for_detector must be > 0");
    if (!(quantile_level > 0 && quantile_level < 1)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "quantile_level must lie in (0, 1)");
    auto ex = std::make_unique<dsopp_hip_feature_extractor>();
    ex->sr.init(device, stream);
    ex->width = width;
    ex->height = height;
    ex->density = point_density_for_detector;
    ex->quantile = quantile_level;
    hipStream_t st = ex->sr.stream;
    const size_t n = static_cast<size_t>(width) * height;
    ex->d_image.reserve(n, 0, st);
    ex->d_grad.reserve(n, 0, st);
    ex->d_hist.reserve(kGradBins, 0, st);
    ex->d_hit.reserve(n, 0, st);   // at most (W - 1) x (H - 1) windows (window size 1)
    ex->d_list.reserve(n, 0, st);
    ex->d_count.reserve(1, 0, st);
    ex->h_image.reserve(n);
    ex->h_count.reserve(sizeof(int));
    (void)ex->final_ready.get(hipEventDisableTiming);
    ex->sr.sync();
    *out = ex.release();
  });
}

void dsopp_hip_feature_extractor_destroy(dsopp_hip_feature_extractor *ex) {
  if (!ex) return;
  (void)hipSetDevice(ex->sr.device);
  if (ex->sr.stream) (void)hipStreamSynchronize(ex->sr.stream);
  delete ex;
}

int dsopp_hip_feature_extractor_set_mask(dsopp_hip_feature_extractor *ex, const uint8_t *mask_host) {
  return guarded([&] {
    if (!ex) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null extractor");
    ex->sr.use();
    if (!mask_host) {
      ex->has_mask = false;
      return;
    }
    hipStream_t st = ex->sr.stream;
    const int W = ex->width, H = ex->height;
    const size_t n = static_cast<size_t>(W) * H;
    ex->d_mask.reserve(n, 0, st);
    ex->d_valid.reserve(n, 0, st);
    ex->d_mask.upload(mask_host, n, 0, st);
    erodeKernel<true><<<gridFor(static_cast<long>(n)), kBlock, 0, st>>>(ex->d_mask.ptr, W, H, ex->d_valid.ptr);
    erodeKernel<false><<<gridFor(static_cast<long>(n)), kBlock, 0, st>>>(ex->d_valid.ptr, W, H, ex->d_mask.ptr);
    HIP_CHECK(hipGetLastError());
    std::swap(ex->d_mask, ex->d_valid);
    ex->has_mask = true;
    ex->sr.sync();
  });
}

int dsopp_hip_feature_extractor_set_mask_from_pyramid(dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *p) {
  return guarded([&] {
    if (!ex || !p) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->has_mask0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid keeps no level-0 mask: it never had dsopp_hip_pyramid_set_semantics");
    if (p->width != ex->width || p->height != ex->height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "pyramid is %d x %d, the extractor %d x %d", p->width, p->height, ex->width, ex->height);
    if (p->sr.device != ex->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "extractor / pyramid live on another device");
    ex->sr.use();
    hipStream_t st = ex->sr.stream;
    const int W = ex->width, H = ex->height;
    const size_t n = static_cast<size_t>(W) * H;
    ex->d_mask.reserve(n, 0, st);
    ex->d_valid.reserve(n, 0, st);
    p->waitReady(st);  // the masks are written in front of the event
    // rows from the pyramid's bytes, columns from the row result: the eroded mask lands in d_valid without a copy of the input
    erodeKernel<true><<<gridFor(static_cast<long>(n)), kBlock, 0, st>>>(p->mask0_u8.get(), W, H, ex->d_mask.ptr);
    erodeKernel<false><<<gridFor(static_cast<long>(n)), kBlock, 0, st>>>(ex->d_mask.ptr, W, H, ex->d_valid.ptr);
    HIP_CHECK(hipGetLastError());
    ex->has_mask = true;
  });
}

int dsopp_hip_feature_extractor_extract(dsopp_hip_feature_extractor *ex, const uint8_t *image_host, int32_t capacity, double *xy, int32_t *n) {
  return guarded([&] {
    if (!ex || !image_host || !n || capacity < 0 || (capacity > 0 && !xy)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (ex->kind == ExtractorKind::Eigen) return eigenExtract(ex, image_host, nullptr, capacity, xy, n);
    ex->sr.use();
    hipStream_t st = ex->sr.stream;
    const size_t N = static_cast<size_t>(ex->width) * ex->height;
    // the caller's image leaves from pinned memory (the stream is idle here: every call ends with a synchronisation)
    std::memcpy(ex->h_image.get(), image_host, N);
    HIP_CHECK(hipMemcpyAsync(ex->d_image.ptr, ex->h_image.get(), N, hipMemcpyHostToDevice, st));
    sobelExtract(ex, ex->d_image.ptr, capacity, xy, n);
  });
}

int dsopp_hip_feature_extractor_extract_from_pyramid(dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *p, int32_t capacity, double *xy, int32_t *n) {
  return guarded([&] {
    if (!ex || !p || !n || capacity < 0 || (capacity > 0 && !xy)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (!p->has_undistorted) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid keeps no 8-bit image: it was not built by dsopp_hip_pyramid_build_undistorted or _build_transformed");
    if (p->width != ex->width || p->height != ex->height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "pyramid is %d x %d, the extractor %d x %d", p->width, p->height, ex->width, ex->height);
    if (p->sr.device != ex->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "extractor / pyramid live on another device");
    ex->sr.use();
    p->waitReady(ex->sr.stream);  // the remap is enqueued in front of the build that the event follows
    if (ex->kind == ExtractorKind::Eigen) return eigenExtract(ex, nullptr, p->undistorted_u8.get(), capacity, xy, n);
    sobelExtract(ex, p->undistorted_u8.get(), capacity, xy, n);
  });
}

int dsopp_hip_feature_extractor_get_state(const dsopp_hip_feature_extractor *ex, int32_t *initialized, int32_t *grad_norm_threshold,
                                          int32_t *window_size, double *point_density, int32_t *found_last) {
  return guarded([&] {
    if (!ex) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null extractor");
    if (initialized) *initialized = ex->initialized ? 1 : 0;
    if (grad_norm_threshold) *grad_norm_threshold = ex->threshold;
    if (window_size) *window_size = ex->window_size;
    if (point_density) *point_density = ex->density;
    if (found_last) *found_last = ex->found_last;
  });
}

int dsopp_hip_immature_set_create_from_features(int device, void *stream, const dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *pyramid,
                                                const double intrinsics[4], dsopp_hip_immature_set **out, int32_t *n) {
  return guarded([&] {
    if (!ex || !pyramid || !intrinsics || !out || !n) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (pyramid->width != ex->width || pyramid->height != ex->height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "pyramid is %d x %d, the extractor %d x %d", pyramid->width, pyramid->height, ex->width, ex->height);
    if (pyramid->sr.device != device || ex->sr.device != device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "extractor / pyramid live on another device");
    const int W = ex->width, H = ex->height;
    const int n_list = static_cast<int>(ex->final_list.size());
    // the number kept is known on the host (the same predicate over the host copy of the list): the set is sized without a read-back
    int kept = 0;
    for (int idx : ex->final_list) kept += InsideRoi{W, H}(idx);
    ImmatureSetPtr s = newImmatureSet(device, stream, kept, nullptr, nullptr, nullptr, nullptr);
    hipStream_t st = s->sr.stream;
    if (kept > 0) {
      pyramid->waitReady(st);
      if (st != ex->sr.stream) HIP_CHECK(hipStreamWaitEvent(st, ex->final_ready.h, 0));
      DeviceBuffer<int> pos;
      DeviceBuffer<char> temp;
      pos.reserve(static_cast<size_t>(n_list), 0, st);
      hipcub::TransformInputIterator<int, InsideRoi, const int *> flags(ex->d_final.ptr, InsideRoi{W, H});
      size_t temp_bytes = 0;
      HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, temp_bytes, flags, pos.ptr, n_list, st));
      temp.reserve(std::max<size_t>(1, temp_bytes), 0, st);
      HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(temp.ptr, temp_bytes, flags, pos.ptr, n_list, st));
      const double cx = intrinsics[2], cy = intrinsics[3], ifx = 1.0 / intrinsics[0], ify = 1.0 / intrinsics[1];
      if (pyramid->dtype == DSOPP_HIP_F64)
        buildImmatureKernel<double><<<gridFor(n_list), kBlock, 0, st>>>(ex->d_final.ptr, pos.ptr, n_list, W, H,
                                                                        static_cast<const Texel<double> *>(pyramid->texels[0].get()), cx, cy, ifx, ify, kept,
                                                                        s->d_in.ptr);
      else
        buildImmatureKernel<float><<<gridFor(n_list), kBlock, 0, st>>>(ex->d_final.ptr, pos.ptr, n_list, W, H,
                                                                       static_cast<const Texel<float> *>(pyramid->texels[0].get()), cx, cy, ifx, ify, kept,
                                                                       s->d_in.ptr);
      HIP_CHECK(hipGetLastError());
      s->sr.sync();  // (the scratch above is freed on return)
    }
    *n = kept;
    *out = s.release();
  });
}

}  // extern "C"
