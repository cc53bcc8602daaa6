// Pyramidal Lucas-Kanade tracking on the device: the pixel step of the monocular initialiser, and the dsopp_hip_flow_tracker_* entry points.
//   MonocularInitializer::tick tracks the first frame's features into every new frame   src/feature_based_slam/tracker/src/monocular_initializer.cpp:36-102
//   features::OpticalFlowMatch = cv::calcOpticalFlowPyrLK(from, to, pts_from, pts_to, status, err, Size(15, 15), 3,
//                                                         TermCriteria(COUNT + EPS, 10, 0.01))   src/feature_based_slam/features/src/optical_flow.cpp:19-31
//
// The arithmetic is the one include/dsopp_hip.h states (a restatement of OpenCV 4's scalar path, lkpyramid.cpp; tests/optical_flow_model.py
// is its NumPy form): integer pyramids, Scharr planes and window samples, exact integer window sums, and a short chain of single IEEE
// binary32 steps between them.  This file is compiled without floating-point contraction (build.sh and the pragma below): no product and
// sum of that chain may fuse.  Division and square root are taken in binary64 and rounded once, which is the correctly rounded binary32
// result (53 >= 2 * 24 + 2).
//
// Layout.  A level's image is row-major bytes with a row stride rounded up to 4 (the pad bytes are 0), its Scharr plane one 32-bit word
// per pixel (dx in the low, dy in the high half) with the same stride in pixels: every row starts on a word of the image and on 16 bytes
// of the plane, so the two plane kernels store whole words whatever the width.  Level 0 is a strided copy of the caller's image.
//   pyrDownKernel   a thread owns 4 neighbouring pixels of one output row: the 11 x 5 source bytes under them, as 4 aligned words per row
//                   where no column reflects, and one word stored
//   scharrKernel    a thread owns 4 neighbouring pixels: 6 x 3 source bytes (3 aligned words per row away from the borders), 16 bytes stored
//   trackKernel     one launch for all points and levels, one wave per point: window pixel p = lane + 64 k (k < 4) is lane `lane`'s, its
//                   I, Ix, Iy stay in registers over the iterations; the window sums are 64-bit integer butterflies over the wave, exact and
//                   therefore order-free; every quantity behind a sum is read through readfirstlane, so every branch is a scalar one;
//                   lane 0 stores the results.  The 16 x 16 footprint of the target is read straight through the vector cache (it moves
//                   by less than a pixel between iterations).
#include "common.hpp"

#include <cfloat>
#include <climits>
#include <cmath>
#include <memory>

#include "pyramid.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kFlowMaxLevels = 6;  // max_level 0 .. 5
constexpr int kWeightBits = 14;    // W_BITS of lkpyramid.cpp: the bilinear weights sum to 1 << 14

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

/** BORDER_REFLECT_101 of any integer for an axis of n >= 2 pixels (one fold serves every index within n - 1 of the axis) */
__device__ __forceinline__ int reflect101(int i, int n) {
  int r = i < 0 ? -i : i;
  if (r >= n) r = 2 * (n - 1) - r;
  if (static_cast<unsigned>(r) >= static_cast<unsigned>(n)) {
    const int period = 2 * (n - 1);
    r = i % period;
    if (r < 0) r += period;
    if (r >= n) r = period - r;
  }
  return r;
}

__device__ __forceinline__ unsigned byteOf(const unsigned (&w)[4], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

// (the parameters are plain pointers — a kernel's name must be the same in the host and the device pass — and are typed as HBM inside)
__global__ void __launch_bounds__(kBlock) pyrDownKernel(const uint8_t *__restrict__ src_, int sw, int sh, int sstride, unsigned *__restrict__ dst_,
                                                        int dw, int dh, int dwords) {
  GlobalPtr<const uint8_t> src = glb(src_);
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= static_cast<unsigned>(dwords) * static_cast<unsigned>(dh)) return;
  const int y = static_cast<int>(idx / static_cast<unsigned>(dwords)), t = static_cast<int>(idx - static_cast<unsigned>(y) * dwords);
  // output columns 4 t .. 4 t + 3 read source columns 8 t - 2 .. 8 t + 8: bytes 2 .. 12 of the four words at column 8 t - 4
  const bool inside = t > 0 && 8 * t + 8 <= sw - 1;
  constexpr int kTap[5] = {1, 4, 6, 4, 1};
  unsigned acc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    GlobalPtr<const uint8_t> row = src + static_cast<size_t>(reflect101(2 * y - 2 + i, sh)) * sstride;
    unsigned b[11];
    if (inside) {
      GlobalPtr<const unsigned> w = reinterpret_cast<GlobalPtr<const unsigned>>(row + (8 * t - 4));
      const unsigned words[4] = {w[0], w[1], w[2], w[3]};
#pragma unroll
      for (int k = 0; k < 11; ++k) b[k] = byteOf(words, k + 2);
    } else {
#pragma unroll
      for (int k = 0; k < 11; ++k) b[k] = row[reflect101(8 * t - 2 + k, sw)];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) acc[c] += kTap[i] * (b[2 * c] + b[2 * c + 4] + 4 * (b[2 * c + 1] + b[2 * c + 3]) + 6 * b[2 * c + 2]);
  }
  unsigned word = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if (4 * t + c < dw) word |= ((acc[c] + 128) >> 8) << (8 * c);  // (the pad bytes of a row stay 0)
  glb(dst_)[idx] = word;
}

__global__ void __launch_bounds__(kBlock) scharrKernel(const uint8_t *__restrict__ src_, int w, int h, int stride, unsigned *__restrict__ deriv_) {
  GlobalPtr<const uint8_t> src = glb(src_);
  const int words = stride / 4;
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= static_cast<unsigned>(words) * static_cast<unsigned>(h)) return;
  const int y = static_cast<int>(idx / static_cast<unsigned>(words)), t = static_cast<int>(idx - static_cast<unsigned>(y) * words);
  // pixels 4 t .. 4 t + 3 read columns 4 t - 1 .. 4 t + 4: bytes 3 .. 8 of the three words at column 4 t - 4
  const bool inside = t > 0 && 4 * t + 4 <= w - 1;
  int b[3][6];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    GlobalPtr<const uint8_t> row = src + static_cast<size_t>(reflect101(y - 1 + i, h)) * stride;
    if (inside) {
      GlobalPtr<const unsigned> p = reinterpret_cast<GlobalPtr<const unsigned>>(row + (4 * t - 4));
      const unsigned wd[4] = {p[0], p[1], p[2], 0u};
#pragma unroll
      for (int k = 0; k < 6; ++k) b[i][k] = static_cast<int>(byteOf(wd, k + 3));
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) b[i][k] = row[reflect101(4 * t - 1 + k, w)];
    }
  }
  int t0[6], t1[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) {
    t0[k] = (b[0][k] + b[2][k]) * 3 + b[1][k] * 10;
    t1[k] = b[2][k] - b[0][k];
  }
  u32x4 out;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int dx = t0[c + 2] - t0[c], dy = (t1[c + 2] + t1[c]) * 3 + t1[c + 1] * 10;  // both within +-4080
    const unsigned pair = (static_cast<unsigned>(dx) & 0xffffu) | (static_cast<unsigned>(dy) << 16);
    out[c] = 4 * t + c < w ? pair : 0u;
  }
  reinterpret_cast<GlobalPtr<u32x4>>(glb(deriv_))[idx] = out;
}

struct FlowLevel {
  const uint8_t *reference;  // level image of the reference frame
  const unsigned *deriv;     // its Scharr plane
  const uint8_t *target;     // level image of the frame tracked into
  int w, h, stride, pad_;
};

struct FlowArgs {
  FlowLevel level[kFlowMaxLevels];
  int n_levels, win, max_count, n;
  double eps2, min_eig;
  const float *points_from;  // n x 2
  float *points_to;          // n x 2
  float *err;                // n
  int *iterations;           // n x n_levels
  uint8_t *status;           // n
};

/** floor as an integer; anything beyond +-1e9 and NaN become -1e9, which every range test refuses */
__device__ __forceinline__ int floorInt(float x) {
  const float f = floorf(x);
  return (f >= -1e9f && f <= 1e9f) ? static_cast<int>(f) : -1000000000;
}

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

/** the exact sum of v over the wave, the same scalar in every lane */
__device__ __forceinline__ long long waveSum(long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const unsigned lo = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(v)));
  const int hi = __builtin_amdgcn_readfirstlane(static_cast<int>(v >> 32));
  return (static_cast<long long>(hi) << 32) | lo;
}

/** an integer sum rounded once to binary32 (int64 -> binary64 is exact below 2^53) */
__device__ __forceinline__ float roundedSum(long long s) { return static_cast<float>(static_cast<double>(s)); }

__device__ __forceinline__ float divide(float a, float b) { return static_cast<float>(static_cast<double>(a) / static_cast<double>(b)); }

struct Weights {
  int w00, w01, w10, w11;
};

__device__ __forceinline__ Weights bilinearWeights(float a, float b) {
  const float ia = 1.0f - a, ib = 1.0f - b, one = static_cast<float>(1 << kWeightBits);
  Weights w;
  w.w00 = static_cast<int>(rintf(ia * ib * one));  // (rintf: half to even, as cvRound)
  w.w01 = static_cast<int>(rintf(a * ib * one));
  w.w10 = static_cast<int>(rintf(ia * b * one));
  w.w11 = (1 << kWeightBits) - w.w00 - w.w01 - w.w10;
  return w;
}

/** the weighted sum of the 2 x 2 pixels at (x, y) of an image plane, read through REFLECT_101 */
__device__ __forceinline__ int sampleImage(GlobalPtr<const uint8_t> img, int w, int h, int stride, int x, int y, const Weights &q) {
  const int x0 = reflect101(x, w), x1 = reflect101(x + 1, w);
  GlobalPtr<const uint8_t> r0 = img + static_cast<size_t>(reflect101(y, h)) * stride, r1 = img + static_cast<size_t>(reflect101(y + 1, h)) * stride;
  return r0[x0] * q.w00 + r0[x1] * q.w01 + r1[x0] * q.w10 + r1[x1] * q.w11;
}

/** the same of the Scharr plane, which reads 0 outside the level */
__device__ __forceinline__ void sampleDeriv(GlobalPtr<const unsigned> plane, int w, int h, int stride, int x, int y, const Weights &q, int &ix, int &iy) {
  const bool cx0 = static_cast<unsigned>(x) < static_cast<unsigned>(w), cx1 = static_cast<unsigned>(x + 1) < static_cast<unsigned>(w);
  const bool cy0 = static_cast<unsigned>(y) < static_cast<unsigned>(h), cy1 = static_cast<unsigned>(y + 1) < static_cast<unsigned>(h);
  GlobalPtr<const unsigned> r0 = plane + static_cast<long>(y) * stride, r1 = r0 + stride;
  const unsigned p00 = cx0 && cy0 ? r0[x] : 0u, p01 = cx1 && cy0 ? r0[x + 1] : 0u;
  const unsigned p10 = cx0 && cy1 ? r1[x] : 0u, p11 = cx1 && cy1 ? r1[x + 1] : 0u;
  auto dx = [](unsigned p) { return static_cast<int>(static_cast<short>(p & 0xffffu)); };
  auto dy = [](unsigned p) { return static_cast<int>(p) >> 16; };
  constexpr int kHalf = 1 << (kWeightBits - 1);
  ix = (dx(p00) * q.w00 + dx(p01) * q.w01 + dx(p10) * q.w10 + dx(p11) * q.w11 + kHalf) >> kWeightBits;
  iy = (dy(p00) * q.w00 + dy(p01) * q.w01 + dy(p10) * q.w10 + dy(p11) * q.w11 + kHalf) >> kWeightBits;
}

/** intensities carry 5 fraction bits: DESCALE(v, W_BITS - 5) */
__device__ __forceinline__ int descaleIntensity(int v) { return (v + (1 << (kWeightBits - 6))) >> (kWeightBits - 5); }

__device__ __forceinline__ bool outsideLevel(int x, int y, int win, int w, int h) { return x < -win || x >= w || y < -win || y >= h; }

__global__ void __launch_bounds__(kBlock) trackKernel(const FlowArgs a) {
  const int lane = threadIdx.x & 63;
  const int point = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
  if (point >= a.n) return;
  const int win = a.win, area = win * win;
  const float half = static_cast<float>(win - 1) * 0.5f, kScale = 1.0f / static_cast<float>(1 << 20);
  // window pixel lane + 64 k: column wx[k], row wy[k] (a slot past the window stays at pixel 0 and is never summed)
  int wx[4], wy[4];
  bool on[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int p = lane + 64 * k;
    on[k] = p < area;
    wy[k] = on[k] ? p / win : 0;
    wx[k] = on[k] ? p - wy[k] * win : 0;
  }
  GlobalPtr<const float> from = glb(a.points_from);
  const float ptx = uniform(from[2 * static_cast<size_t>(point)]), pty = uniform(from[2 * static_cast<size_t>(point) + 1]);
  float rx = 0.0f, ry = 0.0f, err = 0.0f;
  int status = 1;
  const int top = a.n_levels - 1;
  for (int level = top; level >= 0; --level) {
    const FlowLevel L = a.level[level];
    GlobalPtr<const uint8_t> ref = glb(L.reference), tgt = glb(L.target);
    GlobalPtr<const unsigned> deriv = glb(L.deriv);
    const float scale = __int_as_float((127 - level) << 23);  // 2^-level
    float px = ptx * scale, py = pty * scale;
    float nx = level == top ? px : rx * 2.0f, ny = level == top ? py : ry * 2.0f;
    rx = nx;
    ry = ny;
    int passes = 0;
    do {  // (left by `break` where the reference `continue`s with the next level)
      px -= half;
      py -= half;
      const int ipx = floorInt(px), ipy = floorInt(py);
      if (outsideLevel(ipx, ipy, win, L.w, L.h)) {
        if (level == 0) status = 0, err = 0.0f;
        break;
      }
      const Weights q = bilinearWeights(px - static_cast<float>(ipx), py - static_cast<float>(ipy));
      int I[4], Ix[4], Iy[4];
      long long s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        I[k] = Ix[k] = Iy[k] = 0;
        if (on[k]) {
          I[k] = descaleIntensity(sampleImage(ref, L.w, L.h, L.stride, ipx + wx[k], ipy + wy[k], q));
          sampleDeriv(deriv, L.w, L.h, L.stride, ipx + wx[k], ipy + wy[k], q, Ix[k], Iy[k]);
          s11 += Ix[k] * Ix[k];  // each product is below 2^25
          s12 += Ix[k] * Iy[k];
          s22 += Iy[k] * Iy[k];
        }
      }
      const float A11 = roundedSum(waveSum(s11)) * kScale, A12 = roundedSum(waveSum(s12)) * kScale, A22 = roundedSum(waveSum(s22)) * kScale;
      float D = A11 * A22 - A12 * A12;
      const float root = static_cast<float>(__builtin_sqrt(static_cast<double>((A11 - A22) * (A11 - A22) + 4.0f * A12 * A12)));
      const float min_eig = divide(A22 + A11 - root, static_cast<float>(2 * win * win));
      if (static_cast<double>(min_eig) < a.min_eig || D < FLT_EPSILON) {
        if (level == 0) status = 0;
        break;
      }
      D = divide(1.0f, D);
      nx -= half;
      ny -= half;
      float pdx = 0.0f, pdy = 0.0f;
      for (int j = 0; j < a.max_count; ++j) {
        const int inx = floorInt(nx), iny = floorInt(ny);
        if (outsideLevel(inx, iny, win, L.w, L.h)) {
          if (level == 0) status = 0;
          break;
        }
        passes = j + 1;
        const Weights qj = bilinearWeights(nx - static_cast<float>(inx), ny - static_cast<float>(iny));
        long long sb1 = 0, sb2 = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (on[k]) {
            const int diff = descaleIntensity(sampleImage(tgt, L.w, L.h, L.stride, inx + wx[k], iny + wy[k], qj)) - I[k];
            sb1 += diff * Ix[k];  // |diff| <= 8160, |Ix| <= 4080: below 2^25
            sb2 += diff * Iy[k];
          }
        const float b1 = roundedSum(waveSum(sb1)) * kScale, b2 = roundedSum(waveSum(sb2)) * kScale;
        const float dx = (A12 * b2 - A22 * b1) * D, dy = (A12 * b1 - A11 * b2) * D;
        nx += dx;
        ny += dy;
        rx = nx + half;
        ry = ny + half;
        if (static_cast<double>(dx) * static_cast<double>(dx) + static_cast<double>(dy) * static_cast<double>(dy) <= a.eps2) break;
        if (j > 0 && fabs(static_cast<double>(dx + pdx)) < 0.01 && fabs(static_cast<double>(dy + pdy)) < 0.01) {
          rx -= dx * 0.5f;
          ry -= dy * 0.5f;
          break;
        }
        pdx = dx;
        pdy = dy;
      }
      if (level == 0 && status == 1) {
        const float qx = rx - half, qy = ry - half;
        const int iqx = floorInt(qx), iqy = floorInt(qy);
        if (outsideLevel(iqx, iqy, win, L.w, L.h)) {
          status = 0;
        } else {
          const Weights qe = bilinearWeights(qx - static_cast<float>(iqx), qy - static_cast<float>(iqy));
          long long se = 0;
#pragma unroll
          for (int k = 0; k < 4; ++k)
            if (on[k]) {
              const int diff = descaleIntensity(sampleImage(tgt, L.w, L.h, L.stride, iqx + wx[k], iqy + wy[k], qe)) - I[k];
              se += diff < 0 ? -diff : diff;
            }
          err = divide(roundedSum(waveSum(se)), static_cast<float>(32 * win * win));
        }
      }
    } while (false);
    if (lane == 0) glb(a.iterations)[static_cast<size_t>(point) * a.n_levels + level] = passes;
  }
  if (lane == 0) {
    glb(a.points_to)[2 * static_cast<size_t>(point)] = rx;
    glb(a.points_to)[2 * static_cast<size_t>(point) + 1] = ry;
    glb(a.err)[point] = err;
    glb(a.status)[point] = static_cast<uint8_t>(status);
  }
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_flow_tracker {
  dsopp_hip::StreamRef sr;
  int width = 0, height = 0, win = 15, max_level = 3, max_count = 10, n_levels = 1;
  double eps2 = 1e-4, min_eig = 1e-4;
  int w[dsopp_hip::kFlowMaxLevels] = {0}, h[dsopp_hip::kFlowMaxLevels] = {0}, stride[dsopp_hip::kFlowMaxLevels] = {0};
  dsopp_hip::DeviceMem<uint8_t> image[2][dsopp_hip::kFlowMaxLevels];  // [0] the reference's levels, [1] the last target's
  dsopp_hip::DeviceMem<unsigned> deriv[dsopp_hip::kFlowMaxLevels];    // the reference's Scharr planes
  bool has[2] = {false, false};
  // a host image leaves from this pinned copy (rows at stride[0]); image_uploaded guards its reuse
  dsopp_hip::PinnedMem<uint8_t> h_image;
  dsopp_hip::Event image_uploaded, image_read;
  bool upload_pending = false;
  // the points and the results of a track(): one device block and its pinned mirror, laid out by trackLayout; both grow geometrically
  dsopp_hip::DeviceBuffer<uint8_t> d_io;
  dsopp_hip::PinnedMem<uint8_t> h_io;
  size_t h_io_capacity = 0;
};

namespace dsopp_hip {
namespace {

/** offsets in the block of one track() of n points: points_from | points_to | err | iterations | status */
struct TrackLayout {
  size_t from, to, err, iterations, status, bytes;
  TrackLayout(size_t n, size_t levels) {
    from = 0;
    to = from + 8 * n;
    err = to + 8 * n;
    iterations = err + 4 * n;
    status = iterations + 4 * n * levels;
    bytes = status + n;
  }
};

void checkHandle(const dsopp_hip_flow_tracker *t) {
  if (!t) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null flow tracker");
}

/** levels 1 .. n - 1 of image[which] from its level 0, and the Scharr planes of the reference */
void enqueueLevels(dsopp_hip_flow_tracker *t, int which) {
  const hipStream_t st = t->sr.stream;
  for (int l = 0; l < t->n_levels; ++l) {
    if (l > 0) {
      const int words = t->stride[l] / 4;
      const unsigned threads = static_cast<unsigned>(words) * static_cast<unsigned>(t->h[l]);
      pyrDownKernel<<<(threads + kBlock - 1) / kBlock, kBlock, 0, st>>>(t->image[which][l - 1].get(), t->w[l - 1], t->h[l - 1], t->stride[l - 1],
                                                                        reinterpret_cast<unsigned *>(t->image[which][l].get()), t->w[l], t->h[l], words);
      HIP_CHECK(hipGetLastError());
    }
    if (which == 0) {
      const unsigned threads = static_cast<unsigned>(t->stride[l] / 4) * static_cast<unsigned>(t->h[l]);
      scharrKernel<<<(threads + kBlock - 1) / kBlock, kBlock, 0, st>>>(t->image[0][l].get(), t->w[l], t->h[l], t->stride[l], t->deriv[l].get());
      HIP_CHECK(hipGetLastError());
    }
  }
  t->has[which] = true;
}

void setImageHost(dsopp_hip_flow_tracker *t, int which, const uint8_t *image_host, size_t stride) {
  checkHandle(t);
  if (!image_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (stride < static_cast<size_t>(t->width)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a row stride of %zu bytes for %d pixels", stride, t->width);
  t->sr.use();
  if (t->upload_pending) HIP_CHECK(hipEventSynchronize(t->image_uploaded.h));  // (the pinned copy's last upload)
  const size_t pitch = static_cast<size_t>(t->stride[0]);
  for (int y = 0; y < t->height; ++y) copyToPinned(t->h_image.get() + y * pitch, image_host + y * stride, static_cast<size_t>(t->width));
  HIP_CHECK(hipMemcpyAsync(t->image[which][0].get(), t->h_image.get(), pitch * t->height, hipMemcpyHostToDevice, t->sr.stream));
  HIP_CHECK(hipEventRecord(t->image_uploaded.get(hipEventDisableTiming), t->sr.stream));
  t->upload_pending = true;
  enqueueLevels(t, which);
}

/** level 0 from an image in HBM: a strided copy on the tracker's stream, which the call waits for (the levels are built behind it) */
void setImageDevice(dsopp_hip_flow_tracker *t, int which, const void *image_dev, size_t stride) {
  HIP_CHECK(hipMemcpy2DAsync(t->image[which][0].get(), static_cast<size_t>(t->stride[0]), image_dev, stride, static_cast<size_t>(t->width),
                             static_cast<size_t>(t->height), hipMemcpyDeviceToDevice, t->sr.stream));
  HIP_CHECK(hipEventRecord(t->image_read.get(hipEventDisableTiming), t->sr.stream));
  enqueueLevels(t, which);
  HIP_CHECK(hipEventSynchronize(t->image_read.h));
}

void setImageDevicePointer(dsopp_hip_flow_tracker *t, int which, const void *image_dev, size_t stride) {
  checkHandle(t);
  if (!image_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (stride < static_cast<size_t>(t->width)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a row stride of %zu bytes for %d pixels", stride, t->width);
  t->sr.use();
  setImageDevice(t, which, image_dev, stride);
}

void setImagePyramid(dsopp_hip_flow_tracker *t, int which, const dsopp_hip_pyramid *p) {
  checkHandle(t);
  if (!p) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null pyramid");
  if (p->sr.device != t->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid lives on device %d, the flow tracker on %d", p->sr.device, t->sr.device);
  if (p->width != t->width || p->height != t->height)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid is %d x %d, the flow tracker %d x %d", p->width, p->height, t->width, t->height);
  if (!p->has_undistorted) fail(DSOPP_HIP_ERR_STATE, "the pyramid keeps no 8-bit image (its last build was none of build_undistorted, build_transformed, build_colour)");
  t->sr.use();
  p->waitReady(t->sr.stream);
  setImageDevice(t, which, p->undistorted_u8.get(), static_cast<size_t>(p->width));
}

/** the tracking launch behind the target's levels, and the one wait of a track() */
void trackPoints(dsopp_hip_flow_tracker *t, int n, const float *points_from, float *points_to, uint8_t *status, float *err, int32_t *iterations) {
  const hipStream_t st = t->sr.stream;
  if (n == 0) {
    t->sr.sync();
    return;
  }
  const size_t count = static_cast<size_t>(n);
  const TrackLayout lay(count, static_cast<size_t>(t->n_levels));
  t->d_io.reserve(lay.bytes, 0, st);
  if (t->h_io_capacity < lay.bytes) {
    size_t cap = t->h_io_capacity ? t->h_io_capacity : 4096;
    while (cap < lay.bytes) cap *= 2;
    t->h_io.reserve(cap);
    t->h_io_capacity = cap;
  }
  uint8_t *h = t->h_io.get(), *d = t->d_io.ptr;
  std::memcpy(h + lay.from, points_from, 8 * count);
  HIP_CHECK(hipMemcpyAsync(d + lay.from, h + lay.from, 8 * count, hipMemcpyHostToDevice, st));
  FlowArgs a;
  std::memset(&a, 0, sizeof(a));
  for (int l = 0; l < t->n_levels; ++l) {
    a.level[l].reference = t->image[0][l].get();
    a.level[l].deriv = t->deriv[l].get();
    a.level[l].target = t->image[1][l].get();
    a.level[l].w = t->w[l];
    a.level[l].h = t->h[l];
    a.level[l].stride = t->stride[l];
  }
  a.n_levels = t->n_levels;
  a.win = t->win;
  a.max_count = t->max_count;
  a.n = n;
  a.eps2 = t->eps2;
  a.min_eig = t->min_eig;
  a.points_from = reinterpret_cast<const float *>(d + lay.from);
  a.points_to = reinterpret_cast<float *>(d + lay.to);
  a.err = reinterpret_cast<float *>(d + lay.err);
  a.iterations = reinterpret_cast<int *>(d + lay.iterations);
  a.status = d + lay.status;
  const unsigned per_block = kBlock / 64;
  trackKernel<<<(static_cast<unsigned>(n) + per_block - 1) / per_block, kBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(h + lay.to, d + lay.to, lay.bytes - lay.to, hipMemcpyDeviceToHost, st));
  t->sr.sync();
  std::memcpy(points_to, h + lay.to, 8 * count);
  std::memcpy(err, h + lay.err, 4 * count);
  if (iterations) std::memcpy(iterations, h + lay.iterations, 4 * count * t->n_levels);
  std::memcpy(status, h + lay.status, count);
}

void checkTrack(const dsopp_hip_flow_tracker *t, int n, const float *points_from, const float *points_to, const uint8_t *status, const float *err) {
  checkHandle(t);
  if (n < 0 || n > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d points", n);
  if (n > 0 && (!points_from || !points_to || !status || !err)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!t->has[0]) fail(DSOPP_HIP_ERR_STATE, "track before set_reference");
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_flow_tracker_create(int width, int height, int window, int max_level, int max_iterations, double epsilon, double min_eig_threshold,
                                  int device, void *stream, dsopp_hip_flow_tracker **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (window < 3 || window > 15 || window % 2 == 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a window of %d: odd, 3 .. 15", window);
    if (width < 2 || height < 2) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an image of %d x %d", width, height);
    if (static_cast<long long>(width) * height > INT_MAX / 8) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image too large");
    if (max_level < 0 || max_level >= kFlowMaxLevels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "max_level %d: 0 .. %d", max_level, kFlowMaxLevels - 1);
    if (!(epsilon == epsilon) || !(min_eig_threshold == min_eig_threshold)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a threshold is not a number");
    auto t = std::make_unique<dsopp_hip_flow_tracker>();
    t->sr.init(device, stream);
    t->width = width;
    t->height = height;
    t->win = window;
    t->max_level = max_level;
    t->max_count = max_iterations < 0 ? 0 : (max_iterations > 100 ? 100 : max_iterations);  // calcOpticalFlowPyrLK clamps both criteria
    const double eps = epsilon < 0 ? 0.0 : (epsilon > 10 ? 10.0 : epsilon);
    t->eps2 = eps * eps;
    t->min_eig = min_eig_threshold;
    // buildOpticalFlowPyramid's stop rule: after level l the size is halved, and a halved width or height <= window ends the pyramid
    int w = width, h = height;
    t->n_levels = 0;
    for (int l = 0; l <= max_level; ++l) {
      t->w[l] = w;
      t->h[l] = h;
      t->stride[l] = (w + 3) / 4 * 4;
      t->n_levels = l + 1;
      w = (w + 1) / 2;
      h = (h + 1) / 2;
      if (w <= window || h <= window) break;
    }
    for (int l = 0; l < t->n_levels; ++l) {
      const size_t bytes = static_cast<size_t>(t->stride[l]) * t->h[l];
      for (int which = 0; which < 2; ++which) t->image[which][l].alloc(bytes);
      t->deriv[l].alloc(bytes * sizeof(unsigned));
    }
    t->h_image.reserve(static_cast<size_t>(t->stride[0]) * height);
    std::memset(t->h_image.get(), 0, static_cast<size_t>(t->stride[0]) * height);  // (the pad bytes of level 0 stay 0)
    for (int which = 0; which < 2; ++which)
      HIP_CHECK(hipMemsetAsync(t->image[which][0].get(), 0, static_cast<size_t>(t->stride[0]) * height, t->sr.stream));
    t->sr.sync();
    *out = t.release();
  });
}

void dsopp_hip_flow_tracker_destroy(dsopp_hip_flow_tracker *t) {
  if (!t) return;
  (void)hipSetDevice(t->sr.device);
  if (t->sr.stream) (void)hipStreamSynchronize(t->sr.stream);
  delete t;
}

int dsopp_hip_flow_tracker_num_levels(const dsopp_hip_flow_tracker *t, int *n) {
  return guarded([&] {
    checkHandle(t);
    if (!n) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    *n = t->n_levels;
  });
}

int dsopp_hip_flow_tracker_set_reference(dsopp_hip_flow_tracker *t, const uint8_t *image_host, size_t stride) {
  return guarded([&] { setImageHost(t, 0, image_host, stride); });
}

int dsopp_hip_flow_tracker_set_reference_device(dsopp_hip_flow_tracker *t, const void *image_dev, size_t stride) {
  return guarded([&] { setImageDevicePointer(t, 0, image_dev, stride); });
}

int dsopp_hip_flow_tracker_set_reference_from_pyramid(dsopp_hip_flow_tracker *t, const dsopp_hip_pyramid *pyramid) {
  return guarded([&] { setImagePyramid(t, 0, pyramid); });
}

int dsopp_hip_flow_tracker_track(dsopp_hip_flow_tracker *t, const uint8_t *image_host, size_t stride, int n, const float *points_from, float *points_to,
                                 uint8_t *status, float *err, int32_t *iterations) {
  return guarded([&] {
    checkTrack(t, n, points_from, points_to, status, err);
    setImageHost(t, 1, image_host, stride);
    trackPoints(t, n, points_from, points_to, status, err, iterations);
  });
}

int dsopp_hip_flow_tracker_track_device(dsopp_hip_flow_tracker *t, const void *image_dev, size_t stride, int n, const float *points_from, float *points_to,
                                        uint8_t *status, float *err, int32_t *iterations) {
  return guarded([&] {
    checkTrack(t, n, points_from, points_to, status, err);
    setImageDevicePointer(t, 1, image_dev, stride);
    trackPoints(t, n, points_from, points_to, status, err, iterations);
  });
}

int dsopp_hip_flow_tracker_track_from_pyramid(dsopp_hip_flow_tracker *t, const dsopp_hip_pyramid *pyramid, int n, const float *points_from,
                                              float *points_to, uint8_t *status, float *err, int32_t *iterations) {
  return guarded([&] {
    checkTrack(t, n, points_from, points_to, status, err);
    setImagePyramid(t, 1, pyramid);
    trackPoints(t, n, points_from, points_to, status, err, iterations);
  });
}

int dsopp_hip_flow_tracker_get_level(dsopp_hip_flow_tracker *t, int which, int level, uint8_t *image_out, int16_t *deriv_out) {
  return guarded([&] {
    checkHandle(t);
    if (which != 0 && which != 1) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "which = %d: 0 = the reference, 1 = the last target", which);
    if (level < 0 || level >= t->n_levels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "level %d of %d", level, t->n_levels);
    if (which == 1 && deriv_out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "only the reference has derivative planes");
    if (!t->has[which]) fail(DSOPP_HIP_ERR_STATE, which == 0 ? "no reference was set" : "no frame was tracked");
    t->sr.use();
    const size_t w = static_cast<size_t>(t->w[level]), h = static_cast<size_t>(t->h[level]), pitch = static_cast<size_t>(t->stride[level]);
    if (image_out) HIP_CHECK(hipMemcpy2DAsync(image_out, w, t->image[which][level].get(), pitch, w, h, hipMemcpyDeviceToHost, t->sr.stream));
    if (deriv_out) HIP_CHECK(hipMemcpy2DAsync(deriv_out, 4 * w, t->deriv[level].get(), 4 * pitch, 4 * w, h, hipMemcpyDeviceToHost, t->sr.stream));
    t->sr.sync();
  });
}

}  // extern "C"
