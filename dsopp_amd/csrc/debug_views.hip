// The tracker's two debug views on the device: the images MonocularTracker::tick pushes to its camera_output_interface_ (the viewer).
//   debugCurrentFrame(features), every frame                                       src/tracker/tracker/src/monocular_tracker.cpp:323-333, 485-487
//   debugCurrentKeyframe(features, depth_map[0], maximum_visualized_idepth_)       src/tracker/tracker/src/monocular_tracker.cpp:335-374, 511-514
// Both read what is in HBM already (the 8-bit grey image the pyramid keeps, the level-0 mask lane of its texels, the level-0 planes of the
// reference depth maps) and write one interleaved 8-bit BGR image.  include/dsopp_hip.h states the arithmetic; tests/debug_views_model.py
// is its NumPy statement, and the kernels are held to it byte for byte and, for the state M, bit for bit (-ffp-contract=off: every
// binary64 step below is a single IEEE operation).
//
// Frame view: ONE launch (debugViewsFrameKernel), a thread owns 4 consecutive pixels of the image in row-major order and stores their 12
// bytes as three words, as colour.hip's threads do; the N mod 4 pixels of the image's tail are stored byte by byte.
//
// Keyframe view: TWO launches on one stream, no host wait between them.
//  1 debugViewsAverageKernel: sum and count of q = idepth / weight over the cells with idepth > 0, in this FIXED order (i = y * W + x, a
//    cell without idepth > 0 adds 0.0):
//      workgroup b, thread t (256 threads):  s = 0; for k = 0 .. 15: s += q[4096 b + 256 k + t]
//      a wave's 64 lanes:                    for off = 32, 16, 8, 4, 2, 1: s[l] += s[l + off]     (lane 0 holds the wave's sum)
//      the workgroup's partial:              ((wave 0 + wave 1) + wave 2) + wave 3
//    The workgroup that takes the last ticket then adds the partials the same way — thread j: partials j, j + 256, j + 512, ... in that
//    order, then the lanes and the waves as above — updates M in device memory and writes {M, cells} into pinned host memory.  The count is
//    an integer.  No floating-point atomics; the result does not depend on the order in which workgroups run.
//  2 debugViewsKeyframeKernel: a GATHER.  A workgroup of 256 threads owns a tile of 64 x 16 pixels; it turns the cells of the tile plus a
//    halo of 3 (and 3 more columns to the right, see below) into levels ONCE, into LDS (16-bit entries, kEmptyLevel = no circle).  Every
//    output pixel p then scans the set taps of the stencil, c = p - offset, in ascending (dy, dx) — that is DESCENDING (c.y, c.x) — and
//    takes the first occupied one: the circle the reference's raster-order painting would have drawn last.  No scatter, no atomics: the
//    output is a pure function of the inputs.  A tile without any occupied cell in reach skips the scan.
//    Stores: as in the frame view a thread owns one GROUP of 4 consecutive pixels in row-major order over the whole image (so that the 12
//    bytes are three aligned words whatever the width) — the group whose first pixel lies in the thread's 4 columns of its row.  When the
//    width is no multiple of 4 a group may reach up to 3 pixels to the right of the tile (hence the 3 extra LDS columns) or wrap into the
//    first pixels of the next row: those few pixels (at most one group per row) compute their taps from the planes in HBM instead of LDS.
#include "common.hpp"
#include "depth_maps.hpp"
#include "pyramid.hpp"

#include <climits>
#include <cmath>
#include <memory>

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kSumItems = 16, kSumChunk = kSumItems * kBlock;  // cells per thread and per workgroup of the average launch
constexpr int kStencil = 7, kRadius = 3;
constexpr int kTileW = 64, kTileH = 16;  // pixels per workgroup of the render launch: 16 x 16 threads of 4 pixels
constexpr int kLdsW = kTileW + 2 * kRadius + 3, kLdsH = kTileH + 2 * kRadius;
constexpr unsigned kEmptyLevel = 0x100;
enum MaskKind : int { kMaskNone = 0, kMaskBytes = 1, kMaskTexelF64 = 2, kMaskTexelF32 = 3 };

/** what the average launch leaves for the host (pinned memory) */
struct ViewResult {
  double maximum_idepth;
  long long cells;
};

/** pixels 4 t .. 4 t + 3 as three words of BGR */
__device__ __forceinline__ void storeWord(GlobalPtr<unsigned> out, size_t t, const unsigned (&c)[4][3]) {
  GlobalPtr<unsigned> o = out + 3 * t;
  o[0] = c[0][0] | (c[0][1] << 8) | (c[0][2] << 16) | (c[1][0] << 24);
  o[1] = c[1][1] | (c[1][2] << 8) | (c[2][0] << 16) | (c[2][1] << 24);
  o[2] = c[2][2] | (c[3][0] << 8) | (c[3][1] << 16) | (c[3][2] << 24);
}

/** the single pixel i of a tail, byte by byte (volatile: three byte stores stay three byte stores, as in colour.hip) */
__device__ __forceinline__ void storePixel(GlobalPtr<unsigned> out, size_t i, const unsigned (&c)[3]) {
  for (int ch = 0; ch < 3; ++ch) reinterpret_cast<GlobalPtr<volatile uint8_t>>(out)[3 * i + ch] = static_cast<uint8_t>(c[ch]);
}

__device__ __forceinline__ bool maskedAt(const void *mask, int kind, size_t i) {
  if (kind == kMaskBytes) return glb(static_cast<const uint8_t *>(mask))[i] == 0;
  if (kind == kMaskTexelF64) return glb(static_cast<const double *>(mask))[4 * i + 1] == 0.0;
  if (kind == kMaskTexelF32) return glb(static_cast<const float *>(mask))[4 * i + 1] == 0.0f;
  return false;
}

/** debug - ((mask == 0) - Scalar(0, 0, 255)) / 2 in saturating 8-bit arithmetic: B and G lose 128 where the pixel is masked */
__device__ __forceinline__ void framePixel(unsigned g, bool masked, unsigned (&c)[3]) {
  const unsigned dark = g > 128u ? g - 128u : 0u;
  c[0] = c[1] = masked ? dark : g;
  c[2] = g;
}

__global__ void __launch_bounds__(kBlock) debugViewsFrameKernel(const uint8_t *__restrict__ grey_, const void *__restrict__ mask, int mask_kind,
                                                               unsigned *__restrict__ out_, unsigned words, unsigned tail) {
  GlobalPtr<const uint8_t> grey = glb(grey_);
  GlobalPtr<unsigned> out = glb(out_);
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    const size_t first = 4 * static_cast<size_t>(t);
    unsigned c[4][3];
#pragma unroll
    for (int k = 0; k < 4; ++k) framePixel(grey[first + k], maskedAt(mask, mask_kind, first + k), c[k]);
    storeWord(out, t, c);
  } else if (t == words) {
    for (size_t i = 4 * static_cast<size_t>(words); i < 4 * static_cast<size_t>(words) + tail; ++i) {
      unsigned c[3];
      framePixel(grey[i], maskedAt(mask, mask_kind, i), c);
      storePixel(out, i, c);
    }
  }
}

/** lane 0 of every wave gets the wave's sum in the stated order */
__device__ __forceinline__ double waveSum(double s) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off);
  return s;
}
__device__ __forceinline__ unsigned long long waveCount(unsigned long long c) {
  for (int off = 32; off > 0; off >>= 1) c += __shfl_down(c, off);
  return c;
}

__global__ void __launch_bounds__(kBlock) debugViewsAverageKernel(const double *__restrict__ idepth_sum_, const double *__restrict__ weight_, unsigned n,
                                                                 double *partial_sum, unsigned long long *partial_count, unsigned *ticket,
                                                                 double *state, ViewResult *result) {
  GlobalPtr<const double> ids = glb(idepth_sum_), wgt = glb(weight_);
  __shared__ double lds_s[kBlock / 64];
  __shared__ unsigned long long lds_c[kBlock / 64];
  __shared__ unsigned s_last;
  const unsigned tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double s = 0;
  unsigned long long c = 0;
  // (all loads of the thread leave before the first is used: the launch is bound by their latency, not by their bytes)
  double id[kSumItems], w[kSumItems];
#pragma unroll
  for (int k = 0; k < kSumItems; ++k) {
    const size_t i = static_cast<size_t>(blockIdx.x) * kSumChunk + k * kBlock + tid;
    id[k] = i < n ? ids[i] : 0.0;
    w[k] = i < n ? wgt[i] : 1.0;
  }
#pragma unroll
  for (int k = 0; k < kSumItems; ++k) {
    double q = 0;
    if (id[k] > 0) {
      q = id[k] / w[k];
      c += 1;
    }
    s += q;
  }
  s = waveSum(s);
  c = waveCount(c);
  if (lane == 0) {
    lds_s[wave] = s;
    lds_c[wave] = c;
  }
  __syncthreads();
  if (tid == 0) {
    const double ps = ((lds_s[0] + lds_s[1]) + lds_s[2]) + lds_s[3];
    const unsigned long long pc = lds_c[0] + lds_c[1] + lds_c[2] + lds_c[3];
    __hip_atomic_store(&partial_sum[blockIdx.x], ps, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(&partial_count[blockIdx.x], pc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __atomic_thread_fence(__ATOMIC_RELEASE);  // (device scope: the partial above is visible before the ticket)
    s_last = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1 ? 1u : 0u;
  }
  __syncthreads();
  if (!s_last) return;
  // the last workgroup: all partials are in memory; thread j adds workgroups j, j + 256, ... in order, then lanes and waves as above
  s = 0;
  c = 0;
  for (unsigned b = tid; b < gridDim.x; b += kBlock) {
    s += __hip_atomic_load(&partial_sum[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    c += __hip_atomic_load(&partial_count[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  s = waveSum(s);
  c = waveCount(c);
  if (lane == 0) {  // (the first round's values were read before the barrier above)
    lds_s[wave] = s;
    lds_c[wave] = c;
  }
  __syncthreads();
  if (tid == 0) {
    const double total = ((lds_s[0] + lds_s[1]) + lds_s[2]) + lds_s[3];
    const unsigned long long cells = lds_c[0] + lds_c[1] + lds_c[2] + lds_c[3];
    double M = state[0];
    if (cells > 0) {  // (no cell: the reference divides 0 by 0 and M is NaN for good; here M stays)
      const double avg = total / static_cast<double>(cells);
      const double twice = 2.0 * avg;
      if (M == 0) M = twice;
      const double kept = 0.9 * M, fresh = 0.1 * twice;
      M = kept + fresh;
      state[0] = M;
    }
    result->maximum_idepth = M;
    result->cells = static_cast<long long>(cells);
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // armed for the next launch
  }
}

/** rint(clamp((255 q) / M, 0, 255)), a NaN gives 0 */
__device__ __forceinline__ unsigned levelOf(double idepth, double weight, double M) {
  const double q = idepth / weight;
  const double scaled = 255.0 * q;
  double v = scaled / M;
  if (!(v >= 0.0)) v = 0.0;  // below 0, and NaN
  if (v > 255.0) v = 255.0;
  return static_cast<unsigned>(static_cast<int>(rint(v)));  // half to even
}

__global__ void __launch_bounds__(kBlock) debugViewsKeyframeKernel(const uint8_t *__restrict__ grey_, const double *__restrict__ idepth_sum_,
                                                                  const double *__restrict__ weight_, const double *__restrict__ state,
                                                                  const unsigned *__restrict__ colormap_, unsigned long long stencil, int W, int H,
                                                                  unsigned *__restrict__ out_) {
  GlobalPtr<const uint8_t> grey = glb(grey_);
  GlobalPtr<const double> ids = glb(idepth_sum_), wgt = glb(weight_);
  GlobalPtr<const unsigned> colormap = glb(colormap_);
  GlobalPtr<unsigned> out = glb(out_);
  __shared__ unsigned short levels[kLdsH][kLdsW + 1];
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const double M = glb(state)[0];
  int any = 0;
  constexpr int kRounds = (kLdsH * kLdsW + kBlock - 1) / kBlock;
  double id[kRounds];  // (all loads of the thread leave before the first is used; the weight is read only where a cell is occupied)
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int e = tid + r * kBlock, ly = e / kLdsW, lx = e - ly * kLdsW;
    const int cx = x0 - kRadius + lx, cy = y0 - kRadius + ly;
    id[r] = e < kLdsH * kLdsW && cx >= 0 && cx < W && cy >= 0 && cy < H ? ids[static_cast<size_t>(cy) * W + cx] : 0.0;
  }
#pragma unroll
  for (int r = 0; r < kRounds; ++r) {
    const int e = tid + r * kBlock, ly = e / kLdsW, lx = e - ly * kLdsW;
    if (e >= kLdsH * kLdsW) break;
    unsigned level = kEmptyLevel;
    if (id[r] > 0) {
      level = levelOf(id[r], wgt[static_cast<size_t>(y0 - kRadius + ly) * W + (x0 - kRadius + lx)], M);
      any = 1;
    }
    levels[ly][lx] = static_cast<unsigned short>(level);
  }
  const int occupied = __syncthreads_or(any);
  // the group of this thread: the one whose first pixel (a multiple of 4 in row-major order) lies in its 4 columns of its row
  const int tx = tid & 15, ty = tid >> 4;
  const int y = y0 + ty, xa = x0 + 4 * tx;
  if (y >= H || xa >= W) return;
  const unsigned n = static_cast<unsigned>(W) * static_cast<unsigned>(H), row = static_cast<unsigned>(y) * static_cast<unsigned>(W);
  const unsigned first = (row + static_cast<unsigned>(xa) + 3u) & ~3u;
  const unsigned end = row + static_cast<unsigned>(xa + 4 < W ? xa + 4 : W);
  if (first >= end) return;
  const unsigned count = n - first < 4u ? n - first : 4u;
  unsigned c[4][3];
  // (the group's grey bytes as one word where the image is aligned: `first` is a multiple of 4)
  const bool grey_word = count == 4 && (reinterpret_cast<uintptr_t>(grey_) & 3) == 0;
  const unsigned grey4 = grey_word ? *reinterpret_cast<GlobalPtr<const unsigned>>(grey + first) : 0u;
  for (unsigned k = 0; k < count; ++k) {
    const unsigned p = first + k;
    const unsigned g = grey_word ? (grey4 >> (8 * k)) & 255u : grey[p];
    unsigned level = kEmptyLevel;
    const unsigned px = p - row;
    if (px < static_cast<unsigned>(W)) {  // in the thread's own row: all taps are in LDS
      if (occupied) {
        const int bx = static_cast<int>(px) - x0 + 2 * kRadius, by = ty + 2 * kRadius;
        for (unsigned long long m = stencil; m;) {
          const int bit = __ffsll(static_cast<long long>(m)) - 1;
          m &= m - 1;
          const int sy = bit / kStencil, sx = bit - sy * kStencil;  // the tap (dy, dx) = (sy - 3, sx - 3): the cell p - (dx, dy)
          const unsigned l = levels[by - sy][bx - sx];
          if (l != kEmptyLevel) {
            level = l;
            break;
          }
        }
      }
    } else {  // wrapped into a later row (the width is no multiple of 4): the taps from the planes
      const int qy = static_cast<int>(p / static_cast<unsigned>(W)), qx = static_cast<int>(p - static_cast<unsigned>(qy) * static_cast<unsigned>(W));
      for (unsigned long long m = stencil; m;) {
        const int bit = __ffsll(static_cast<long long>(m)) - 1;
        m &= m - 1;
        const int sy = bit / kStencil, sx = bit - sy * kStencil;
        const int cx = qx - (sx - kRadius), cy = qy - (sy - kRadius);
        if (cx < 0 || cx >= W || cy < 0 || cy >= H) continue;
        const size_t i = static_cast<size_t>(cy) * W + cx;
        const double id = ids[i];
        if (id > 0) {
          level = levelOf(id, wgt[i], M);
          break;
        }
      }
    }
    if (level != kEmptyLevel) {
      const unsigned bgr = colormap[level];
      c[k][0] = bgr & 255u, c[k][1] = (bgr >> 8) & 255u, c[k][2] = (bgr >> 16) & 255u;
    } else {
      c[k][0] = c[k][1] = c[k][2] = g;
    }
  }
  if (count == 4) {
    storeWord(out, first / 4, c);
  } else {
    for (unsigned k = 0; k < count; ++k) storePixel(out, static_cast<size_t>(first) + k, c[k]);
  }
}

/** the library's jet: x = v / 255, channel = rint(255 clamp(1.5 - |4 x - centre|, 0, 1)), centres 3 (R), 2 (G), 1 (B) */
unsigned jetChannel(int v, double centre) {
  const double x = v / 255.0;
  double c = 1.5 - std::fabs(4.0 * x - centre);
  c = c < 0.0 ? 0.0 : c > 1.0 ? 1.0 : c;
  return static_cast<unsigned>(std::nearbyint(255.0 * c));  // (the default rounding mode: half to even)
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

struct dsopp_hip_debug_views {
  StreamRef sr;
  int width = 0, height = 0;
  size_t n = 0;
  unsigned sum_blocks = 0;
  unsigned long long stencil = 0;   // bit (dy + 3) * 7 + dx + 3
  DeviceMem<unsigned> colormap;     // 256 x {B, G << 8, R << 16}
  DeviceMem<uint8_t> grey, bgr;     // the host forms' input and output images
  DeviceMem<double> partial_sum, state;  // state[0] = M
  DeviceMem<unsigned long long> partial_count;
  DeviceMem<unsigned> ticket;
  PinnedMem<ViewResult> h_result;
  DeviceMem<double> planes;  // the host-planes form's two planes, allocated by its first call
  Event pyramid_done, maps_done, done;
  bool pending = false;  // a keyframe view was enqueued since the last wait for `done`, on last_stream
  hipStream_t last_stream = nullptr;

  /** everything enqueued on `consumer` after this call runs behind what `producer` holds now */
  static void orderBehind(Event &e, hipStream_t producer, hipStream_t consumer) {
    if (producer == consumer) return;
    HIP_CHECK(hipEventRecord(e.get(hipEventDisableTiming), producer));
    HIP_CHECK(hipStreamWaitEvent(consumer, e.h, 0));
  }
  void waitDone() {
    if (pending) HIP_CHECK(hipEventSynchronize(done.h));
    pending = false;
  }
  void checkPyramid(const dsopp_hip_pyramid *p, bool needs_image) const {
    if (!p) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null pyramid");
    if (p->sr.device != sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid lives on device %d, the views on %d", p->sr.device, sr.device);
    if (p->width != width || p->height != height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid is %d x %d, the views are %d x %d", p->width, p->height, width, height);
    if (needs_image && !p->has_undistorted) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid keeps no 8-bit grey image and none was given");
  }
  void checkMaps(const dsopp_hip_depth_maps *m) const {
    if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null depth maps");
    if (m->sr.device != sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the depth maps live on device %d, the views on %d", m->sr.device, sr.device);
    if (m->levels < 1 || m->width[0] != width || m->height[0] != height)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "level 0 of the depth maps is %d x %d, the views are %d x %d", m->levels ? m->width[0] : 0,
           m->levels ? m->height[0] : 0, width, height);
  }
  /** the image to read: the caller's, uploaded on the views' stream, or the one the pyramid keeps */
  const uint8_t *greyImage(const dsopp_hip_pyramid *p, const uint8_t *grey_host) {
    if (!grey_host) return p->undistorted_u8.get();
    HIP_CHECK(hipMemcpyAsync(grey.get(), grey_host, n, hipMemcpyHostToDevice, sr.stream));
    return grey.get();
  }
  void enqueueFrame(const uint8_t *grey_dev, const void *mask, int kind, uint8_t *out_dev, hipStream_t st) const {
    const unsigned words = static_cast<unsigned>(n / 4), tail = static_cast<unsigned>(n % 4);
    const unsigned blocks = (words + (tail ? 1u : 0u) + kBlock - 1) / kBlock;
    debugViewsFrameKernel<<<blocks, kBlock, 0, st>>>(grey_dev, mask, kind, reinterpret_cast<unsigned *>(out_dev), words, tail);
    HIP_CHECK(hipGetLastError());
  }
  void enqueueKeyframe(const uint8_t *grey_dev, const double *ids, const double *wgt, uint8_t *out_dev, hipStream_t st) {
    // (one keyframe view of an object at a time: they share M, the partials and the ticket — one on another stream runs behind the last)
    if (pending && st != last_stream) HIP_CHECK(hipStreamWaitEvent(st, done.h, 0));
    debugViewsAverageKernel<<<sum_blocks, kBlock, 0, st>>>(ids, wgt, static_cast<unsigned>(n), partial_sum.get(), partial_count.get(), ticket.get(),
                                                           state.get(), h_result.get());
    HIP_CHECK(hipGetLastError());
    const dim3 grid(static_cast<unsigned>((width + kTileW - 1) / kTileW), static_cast<unsigned>((height + kTileH - 1) / kTileH));
    debugViewsKeyframeKernel<<<grid, kBlock, 0, st>>>(grey_dev, ids, wgt, state.get(), colormap.get(), stencil, width, height,
                                                      reinterpret_cast<unsigned *>(out_dev));
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(done.get(hipEventDisableTiming), st));
    pending = true;
    last_stream = st;
  }
  /** the blocking forms' end: the image to the caller, then {M, cells} as the average launch left them */
  void finish(uint8_t *bgr_out_host, double *maximum_idepth, int64_t *cells) {
    HIP_CHECK(hipMemcpyAsync(bgr_out_host, bgr.get(), 3 * n, hipMemcpyDeviceToHost, sr.stream));
    sr.sync();
    pending = false;
    if (maximum_idepth) *maximum_idepth = h_result.get()->maximum_idepth;
    if (cells) *cells = h_result.get()->cells;
  }
};

extern "C" {

int dsopp_hip_debug_views_create(int device, void *stream, int width, int height, const uint8_t *colormap_bgr, const uint8_t *stencil,
                                 dsopp_hip_debug_views **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null output");
    if (width <= 0 || height <= 0 || static_cast<size_t>(width) * static_cast<size_t>(height) > static_cast<size_t>(INT_MAX) ||
        (height + kTileH - 1) / kTileH > 65535)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an image of %d x %d", width, height);
    if (stencil && !stencil[kRadius * kStencil + kRadius]) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the stencil's centre byte is 0");
    auto v = std::make_unique<dsopp_hip_debug_views>();
    v->sr.init(device, stream);
    v->width = width;
    v->height = height;
    v->n = static_cast<size_t>(width) * static_cast<size_t>(height);
    v->sum_blocks = static_cast<unsigned>((v->n + kSumChunk - 1) / kSumChunk);
    for (int dy = -kRadius; dy <= kRadius; ++dy)
      for (int dx = -kRadius; dx <= kRadius; ++dx) {
        const int bit = (dy + kRadius) * kStencil + dx + kRadius;
        if (stencil ? stencil[bit] != 0 : dx * dx + dy * dy <= kRadius * kRadius) v->stencil |= 1ull << bit;
      }
    unsigned table[256];
    for (int i = 0; i < 256; ++i) {
      if (colormap_bgr)
        table[i] = colormap_bgr[3 * i] | (static_cast<unsigned>(colormap_bgr[3 * i + 1]) << 8) | (static_cast<unsigned>(colormap_bgr[3 * i + 2]) << 16);
      else
        table[i] = jetChannel(i, 1.0) | (jetChannel(i, 2.0) << 8) | (jetChannel(i, 3.0) << 16);
    }
    hipStream_t st = v->sr.stream;
    v->colormap.alloc(sizeof(table));
    v->grey.alloc(v->n);
    v->bgr.alloc(3 * v->n);
    v->partial_sum.alloc(v->sum_blocks * sizeof(double));
    v->partial_count.alloc(v->sum_blocks * sizeof(unsigned long long));
    v->state.alloc(sizeof(double));
    v->ticket.alloc(sizeof(unsigned));
    v->h_result.reserve(sizeof(ViewResult));
    *v->h_result.get() = ViewResult{0.0, 0};
    HIP_CHECK(hipMemcpyAsync(v->colormap.get(), table, sizeof(table), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemsetAsync(v->state.get(), 0, sizeof(double), st));
    HIP_CHECK(hipMemsetAsync(v->ticket.get(), 0, sizeof(unsigned), st));
    v->sr.sync();  // (`table` leaves scope)
    *out = v.release();
  });
}

void dsopp_hip_debug_views_destroy(dsopp_hip_debug_views *v) {
  if (!v) return;
  (void)hipSetDevice(v->sr.device);
  if (v->pending) (void)hipEventSynchronize(v->done.h);
  (void)hipStreamSynchronize(v->sr.stream);
  delete v;
}

int dsopp_hip_debug_views_frame(dsopp_hip_debug_views *v, const dsopp_hip_pyramid *pyramid, const uint8_t *grey_host, uint8_t *bgr_out_host) {
  return guarded([&] {
    if (!v || !bgr_out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    v->checkPyramid(pyramid, !grey_host);
    v->sr.use();
    hipStream_t st = v->sr.stream;
    const uint8_t *grey_dev = v->greyImage(pyramid, grey_host);
    dsopp_hip_debug_views::orderBehind(v->pyramid_done, pyramid->sr.stream, st);
    v->enqueueFrame(grey_dev, pyramid->texels[0].get(), pyramid->dtype == DSOPP_HIP_F64 ? kMaskTexelF64 : kMaskTexelF32, v->bgr.get(), st);
    HIP_CHECK(hipMemcpyAsync(bgr_out_host, v->bgr.get(), 3 * v->n, hipMemcpyDeviceToHost, st));
    v->sr.sync();
  });
}

int dsopp_hip_debug_views_frame_device(dsopp_hip_debug_views *v, const void *grey_dev, const void *mask_dev, void *bgr_out_dev, void *stream) {
  return guarded([&] {
    if (!v || !grey_dev || !bgr_out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (reinterpret_cast<uintptr_t>(bgr_out_dev) & 3) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device output images must be 4-byte aligned");
    v->sr.use();
    v->enqueueFrame(static_cast<const uint8_t *>(grey_dev), mask_dev, mask_dev ? kMaskBytes : kMaskNone, static_cast<uint8_t *>(bgr_out_dev),
                    stream ? static_cast<hipStream_t>(stream) : v->sr.stream);
  });
}

int dsopp_hip_debug_views_keyframe(dsopp_hip_debug_views *v, const dsopp_hip_pyramid *pyramid, const uint8_t *grey_host,
                                   const dsopp_hip_depth_maps *maps, uint8_t *bgr_out_host, double *maximum_idepth, int64_t *cells) {
  return guarded([&] {
    if (!v || !bgr_out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    v->checkPyramid(pyramid, !grey_host);
    v->checkMaps(maps);
    v->sr.use();
    hipStream_t st = v->sr.stream;
    const uint8_t *grey_dev = v->greyImage(pyramid, grey_host);
    if (!grey_host) dsopp_hip_debug_views::orderBehind(v->pyramid_done, pyramid->sr.stream, st);
    dsopp_hip_debug_views::orderBehind(v->maps_done, maps->sr.stream, st);
    v->enqueueKeyframe(grey_dev, maps->idepth_sum[0].ptr, maps->weight[0].ptr, v->bgr.get(), st);
    v->finish(bgr_out_host, maximum_idepth, cells);
  });
}

int dsopp_hip_debug_views_keyframe_device(dsopp_hip_debug_views *v, const void *grey_dev, const dsopp_hip_depth_maps *maps, void *bgr_out_dev,
                                          void *stream) {
  return guarded([&] {
    if (!v || !grey_dev || !bgr_out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (reinterpret_cast<uintptr_t>(bgr_out_dev) & 3) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device output images must be 4-byte aligned");
    v->checkMaps(maps);
    v->sr.use();
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : v->sr.stream;
    dsopp_hip_debug_views::orderBehind(v->maps_done, maps->sr.stream, st);
    v->enqueueKeyframe(static_cast<const uint8_t *>(grey_dev), maps->idepth_sum[0].ptr, maps->weight[0].ptr, static_cast<uint8_t *>(bgr_out_dev), st);
  });
}

int dsopp_hip_debug_views_keyframe_planes(dsopp_hip_debug_views *v, const uint8_t *grey_host, const double *idepth_sum_host, const double *weight_host,
                                          uint8_t *bgr_out_host, double *maximum_idepth, int64_t *cells) {
  return guarded([&] {
    if (!v || !grey_host || !idepth_sum_host || !weight_host || !bgr_out_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    v->sr.use();
    hipStream_t st = v->sr.stream;
    if (!v->planes) v->planes.alloc(2 * v->n * sizeof(double));
    double *ids = v->planes.get(), *wgt = ids + v->n;
    HIP_CHECK(hipMemcpyAsync(ids, idepth_sum_host, v->n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(wgt, weight_host, v->n * sizeof(double), hipMemcpyHostToDevice, st));
    HIP_CHECK(hipMemcpyAsync(v->grey.get(), grey_host, v->n, hipMemcpyHostToDevice, st));
    v->enqueueKeyframe(v->grey.get(), ids, wgt, v->bgr.get(), st);
    v->finish(bgr_out_host, maximum_idepth, cells);
  });
}

int dsopp_hip_debug_views_get_maximum_idepth(dsopp_hip_debug_views *v, double *maximum_idepth) {
  return guarded([&] {
    if (!v || !maximum_idepth) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    v->sr.use();
    v->waitDone();
    *maximum_idepth = v->h_result.get()->maximum_idepth;
  });
}

int dsopp_hip_debug_views_set_maximum_idepth(dsopp_hip_debug_views *v, double maximum_idepth) {
  return guarded([&] {
    if (!v) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null views");
    v->sr.use();
    v->waitDone();
    v->h_result.get()->maximum_idepth = maximum_idepth;
    HIP_CHECK(hipMemcpyAsync(v->state.get(), &v->h_result.get()->maximum_idepth, sizeof(double), hipMemcpyHostToDevice, v->sr.stream));
    v->sr.sync();
  });
}

}  // extern "C"
