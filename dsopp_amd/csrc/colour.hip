// Colour camera frames on the device: the remap and the resize + crop of an 8-bit BGR image, the grey conversion behind them, and the
// dsopp_hip_*_bgr_device entry points.
//   the image provider reads colour (read_grayscale = false)        src/sensors/sensors_builder/src/camera_fabric.cpp:35
//   per frame: undistort, then the transformer list, on the BGR Mat  src/sensors/camera/src/camera.cpp:70
//   cv::cvtColor(raw_image_, frame_data_, cv::COLOR_BGR2GRAY), last  src/features/src/camera_features.cpp:32
//   the colour image stays with the frame (CameraFeatures::image())  src/features/src/camera_features.cpp:49
//
// cv::remap and cv::resize of a CV_8UC3 image share coordinates, reflection and weights between the channels, so both stages are the
// single-channel integer statements of undistort.hip and transform.hip applied to B, G and R on their own, over the SAME device tables:
// tap o of channel c is byte 3 * o + c, the +-1 / +-in_w steps of the table's flip and step bits become +-3 / +-3 * in_w bytes.  The
// conversion runs on the 8-bit result of the last stage (DESIGN.md section 4 and include/dsopp_hip.h state it):
//   grey = (3735 * B + 19235 * G + 9798 * R + 16384) >> 15
// A thread owns 4 consecutive output pixels, as the grey kernels' threads do: it computes their 12 channel bytes in registers and stores
// one word of grey (a wave: 256 contiguous bytes), three words of BGR at byte 12 * t (a wave: 768 contiguous bytes), or both — the
// conversion is the stage kernels' epilogue, never a pass of its own behind a stage.  The N mod 4 pixels that are left are stored byte by
// byte by the thread behind the last full word.  The BGR input has no alignment (a tap is 3 bytes at 3 * o), and the six bytes of a horizontal
// tap pair are neighbours: a stage reads them as the two or three ALIGNED words they lie in and funnel-shifts them into place (loadBytes)
// — half the load instructions of byte loads, and measurably faster.  The plain conversion reads the 12 bytes of a
// thread the same way.  No load of the image is narrower than a word or starts at an address that is no multiple of 4; where two or three
// such words are neighbours hipcc merges them into one global_load_dwordx2 / _dwordx3 at that 4-byte aligned address (an 8- or 12-byte
// access at 4-byte alignment, which gfx950 serves as it stands; every word of it holds bytes the thread needs).
#include "colour.hpp"

#include <climits>

#include "pyramid.hpp"

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr unsigned kGreyB = 3735, kGreyG = 19235, kGreyR = 9798, kGreyHalf = 16384, kGreyShift = 15;  // the weights sum to 1 << 15

/** the grey level of one pixel's {B, G, R} */
__device__ __forceinline__ unsigned greyOf(const unsigned (&c)[3]) { return (kGreyB * c[0] + kGreyG * c[1] + kGreyR * c[2] + kGreyHalf) >> kGreyShift; }

/** the common epilogue: pixels 4 t .. 4 t + 3 as one word of grey and / or three words of BGR */
__device__ __forceinline__ void storeWord(GlobalPtr<unsigned> bgr_out, GlobalPtr<unsigned> grey_out, unsigned t, const unsigned (&c)[4][3]) {
  if (grey_out) grey_out[t] = greyOf(c[0]) | (greyOf(c[1]) << 8) | (greyOf(c[2]) << 16) | (greyOf(c[3]) << 24);
  if (bgr_out) {
    GlobalPtr<unsigned> o = bgr_out + 3 * static_cast<size_t>(t);
    o[0] = c[0][0] | (c[0][1] << 8) | (c[0][2] << 16) | (c[1][0] << 24);
    o[1] = c[1][1] | (c[1][2] << 8) | (c[2][0] << 16) | (c[2][1] << 24);
    o[2] = c[2][2] | (c[3][0] << 8) | (c[3][1] << 16) | (c[3][2] << 24);
  }
}

/** the same for the single pixel i of the tail, byte by byte */
__device__ __forceinline__ void storePixel(GlobalPtr<unsigned> bgr_out, GlobalPtr<unsigned> grey_out, size_t i, const unsigned (&c)[3]) {
  if (grey_out) reinterpret_cast<GlobalPtr<uint8_t>>(grey_out)[i] = static_cast<uint8_t>(greyOf(c));
  if (bgr_out)  // (volatile: three byte stores stay three byte stores — merged into a short, that store would start at the odd address 3 i)
    for (int ch = 0; ch < 3; ++ch) reinterpret_cast<GlobalPtr<volatile uint8_t>>(bgr_out)[3 * i + ch] = static_cast<uint8_t>(c[ch]);
}

/** the `count` <= 6 bytes at p, of any alignment, as {bytes 0-3, bytes 4-5}: aligned words funnel-shifted into place.  Every word that is
 *  read holds at least one of those bytes, so none lies in another page than they do.  (w[0] and w[1] become one global_load_dwordx2 at the
 *  4-byte aligned address where count makes the second word certain: see the head of this file.) */
__device__ __forceinline__ void loadBytes(GlobalPtr<const uint8_t> p, unsigned count, unsigned &lo, unsigned &hi) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  const unsigned s = static_cast<unsigned>(a & 3), last = s + count - 1;
  GlobalPtr<const unsigned> w = reinterpret_cast<GlobalPtr<const unsigned>>(a - s);
  const unsigned i1 = last >= 4 ? 1u : 0u, i2 = last >= 8 ? 2u : i1;
  const unsigned d0 = w[0], d1 = w[i1], d2 = w[i2];
  lo = __builtin_amdgcn_alignbyte(d1, d0, s);
  hi = __builtin_amdgcn_alignbyte(d2, d1, s);
}
/** channel ch of the first (second = false) or second pixel of such a pair */
__device__ __forceinline__ int pairByte(unsigned lo, unsigned hi, bool second, int ch) {
  const int k = (second ? 3 : 0) + ch;
  return static_cast<int>(((k < 4 ? lo : hi) >> (8 * (k & 3))) & 255u);
}

/** undistort.hip's remapPixel for the three channels of one table entry; row_bytes = 3 * in_w */
__device__ __forceinline__ void remapBgr(GlobalPtr<const uint8_t> src, long row_bytes, unsigned offset, unsigned bits, unsigned (&c)[3]) {
  const int fx = bits & (kRemapOne - 1), fy = (bits >> kRemapFyShift) & (kRemapOne - 1);
  const bool flip = bits & kRemapFlipX;
  const long dy = (bits & kRemapFlipY) ? -row_bytes : row_bytes;
  GlobalPtr<const uint8_t> p = src + 3 * static_cast<size_t>(offset);
  const int gx = kRemapOne - fx, gy = kRemapOne - fy;
  const int w00 = gx * gy * kRemapOne, w01 = fx * gy * kRemapOne, w10 = gx * fy * kRemapOne, w11 = fx * fy * kRemapOne;
  // (the two taps of a row are neighbours, the second one in front of the first where the reflection turned the pair round)
  unsigned lo0, hi0, lo1, hi1;
  loadBytes(p + (flip ? -3 : 0), 6, lo0, hi0);
  loadBytes(p + dy + (flip ? -3 : 0), 6, lo1, hi1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int p00 = flip ? pairByte(lo0, hi0, true, ch) : pairByte(lo0, hi0, false, ch);
    const int p01 = flip ? pairByte(lo0, hi0, false, ch) : pairByte(lo0, hi0, true, ch);
    const int p10 = flip ? pairByte(lo1, hi1, true, ch) : pairByte(lo1, hi1, false, ch);
    const int p11 = flip ? pairByte(lo1, hi1, false, ch) : pairByte(lo1, hi1, true, ch);
    c[ch] = static_cast<unsigned>((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 16384) >> 15);
  }
}

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));

// (the parameters are plain pointers — a kernel's name must be the same in the host and the device pass — and are typed as HBM inside)
__global__ void __launch_bounds__(kBlock) undistortBgrKernel(const unsigned *__restrict__ table_, const uint8_t *__restrict__ src_, int in_w,
                                                             unsigned *__restrict__ bgr_out_, unsigned *__restrict__ grey_out_, unsigned words,
                                                             unsigned tail) {
  GlobalPtr<const uint8_t> src = glb(src_);
  GlobalPtr<unsigned> bgr_out = glb(bgr_out_), grey_out = glb(grey_out_);
  const long row_bytes = 3L * in_w;
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    GlobalPtr<const u32x4> e = reinterpret_cast<GlobalPtr<const u32x4>>(glb(table_)) + 2 * static_cast<size_t>(t);
    const u32x4 a = e[0], b = e[1];
    unsigned c[4][3];
    remapBgr(src, row_bytes, a.x, a.y, c[0]);
    remapBgr(src, row_bytes, a.z, a.w, c[1]);
    remapBgr(src, row_bytes, b.x, b.y, c[2]);
    remapBgr(src, row_bytes, b.z, b.w, c[3]);
    storeWord(bgr_out, grey_out, t, c);
  } else if (t == words) {
    const size_t first = 4 * static_cast<size_t>(words);
    for (unsigned k = 0; k < tail; ++k) {
      const u32x2 e = reinterpret_cast<GlobalPtr<const u32x2>>(glb(table_))[first + k];
      unsigned c[3];
      remapBgr(src, row_bytes, e.x, e.y, c);
      storePixel(bgr_out, grey_out, first + k, c);
    }
  }
}

/** transform.hip's transformPixel for the three channels of one column and row entry; row_bytes = 3 * in_w */
__device__ __forceinline__ void transformBgr(GlobalPtr<const uint8_t> src, size_t row_bytes, u32x2 col, u32x2 row, unsigned (&c)[3]) {
  const int a1 = col.y & kResizeWeightMask, a0 = (col.y >> kResizeFirstWeightShift) & kResizeWeightMask;
  const int b1 = row.y & kResizeWeightMask, b0 = (row.y >> kResizeFirstWeightShift) & kResizeWeightMask;
  const size_t dx = (col.y & kResizeStep) ? 3u : 0u, dy = (row.y & kResizeStep) ? row_bytes : 0u;
  GlobalPtr<const uint8_t> p = src + 3 * static_cast<size_t>(row.x + col.x);
  // (without the step the second tap is the first one again, with weight 0: only its three bytes are read)
  unsigned lo0, hi0, lo1, hi1;
  loadBytes(p, dx ? 6 : 3, lo0, hi0);
  loadBytes(p + dy, dx ? 6 : 3, lo1, hi1);
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int p00 = pairByte(lo0, hi0, false, ch), p01 = dx ? pairByte(lo0, hi0, true, ch) : p00;
    const int p10 = pairByte(lo1, hi1, false, ch), p11 = dx ? pairByte(lo1, hi1, true, ch) : p10;
    const int r0 = a0 * p00 + a1 * p01, r1 = a0 * p10 + a1 * p11;
    c[ch] = static_cast<unsigned>((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2);
  }
}

/** pixels [first, first + count) of the output, count <= 4 */
__device__ __forceinline__ void transformPixels(GlobalPtr<const u32x2> cols, GlobalPtr<const u32x2> rows, GlobalPtr<const uint8_t> src,
                                                size_t row_bytes, unsigned out_w, unsigned first, unsigned count, unsigned (*c)[3]) {
  unsigned y = first / out_w, x = first - y * out_w;
  u32x2 row = rows[y];
  for (unsigned k = 0; k < count; ++k) {
    transformBgr(src, row_bytes, cols[x], row, c[k]);
    if (++x == out_w && k + 1 < count) {  // (the next pixel exists, so does its row)
      x = 0;
      row = rows[++y];
    }
  }
}

__global__ void __launch_bounds__(kBlock) transformBgrKernel(const unsigned *__restrict__ table_, const uint8_t *__restrict__ src_, unsigned in_w,
                                                             unsigned out_w, unsigned *__restrict__ bgr_out_, unsigned *__restrict__ grey_out_,
                                                             unsigned words, unsigned tail) {
  GlobalPtr<const u32x2> cols = reinterpret_cast<GlobalPtr<const u32x2>>(glb(table_)), rows = cols + out_w;
  GlobalPtr<const uint8_t> src = glb(src_);
  GlobalPtr<unsigned> bgr_out = glb(bgr_out_), grey_out = glb(grey_out_);
  const size_t row_bytes = 3 * static_cast<size_t>(in_w);
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    unsigned c[4][3];
    transformPixels(cols, rows, src, row_bytes, out_w, 4 * t, 4, c);
    storeWord(bgr_out, grey_out, t, c);
  } else if (t == words) {
    for (unsigned i = 4 * words; i < 4 * words + tail; ++i) {
      unsigned c[1][3];
      transformPixels(cols, rows, src, row_bytes, out_w, i, 1, c);
      storePixel(bgr_out, grey_out, i, c[0]);
    }
  }
}

/** the plain conversion.  The 12 bytes of a thread start `s` = src & 3 bytes (the same for every thread) behind an aligned word: they are
 *  read as the three aligned words they lie in, or four when s != 0, and funnel-shifted into place; the pixels of the tail as in loadBytes */
__global__ void __launch_bounds__(kBlock) bgrToGreyKernel(const uint8_t *__restrict__ src_, unsigned *__restrict__ grey_out_, unsigned words, unsigned tail) {
  GlobalPtr<const uint8_t> src = glb(src_);
  GlobalPtr<unsigned> grey_out = glb(grey_out_);
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t < words) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) + 12 * static_cast<size_t>(t);
    const unsigned s = static_cast<unsigned>(a & 3);
    GlobalPtr<const unsigned> w = reinterpret_cast<GlobalPtr<const unsigned>>(a - s);
    const unsigned d0 = w[0], d1 = w[1], d2 = w[2], d3 = w[s ? 3 : 2];  // (the fourth word holds bytes of the thread only when s != 0)
    const unsigned w0 = __builtin_amdgcn_alignbyte(d1, d0, s), w1 = __builtin_amdgcn_alignbyte(d2, d1, s), w2 = __builtin_amdgcn_alignbyte(d3, d2, s);
    unsigned c[4][3];
    c[0][0] = w0 & 255, c[0][1] = (w0 >> 8) & 255, c[0][2] = (w0 >> 16) & 255, c[1][0] = w0 >> 24;
    c[1][1] = w1 & 255, c[1][2] = (w1 >> 8) & 255, c[2][0] = (w1 >> 16) & 255, c[2][1] = w1 >> 24;
    c[2][2] = w2 & 255, c[3][0] = (w2 >> 8) & 255, c[3][1] = (w2 >> 16) & 255, c[3][2] = w2 >> 24;
    storeWord(nullptr, grey_out, t, c);
  } else if (t == words) {
    for (size_t i = 4 * static_cast<size_t>(words); i < 4 * static_cast<size_t>(words) + tail; ++i) {
      unsigned lo, hi;
      loadBytes(src + 3 * i, 3, lo, hi);
      const unsigned c[3] = {lo & 255, (lo >> 8) & 255, (lo >> 16) & 255};
      storePixel(nullptr, grey_out, i, c);
    }
  }
}

void checkOutputs(const uint8_t *bgr_in_dev, const uint8_t *bgr_out_dev, const uint8_t *grey_out_dev) {
  if (!bgr_in_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (!bgr_out_dev && !grey_out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "neither a colour nor a grey output");
  if ((reinterpret_cast<uintptr_t>(bgr_out_dev) | reinterpret_cast<uintptr_t>(grey_out_dev)) & 3)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device output images must be 4-byte aligned");
}

struct Launch {
  unsigned words, tail, blocks;
  explicit Launch(size_t n) : words(static_cast<unsigned>(n / 4)), tail(static_cast<unsigned>(n % 4)) {
    const unsigned threads = words + (tail ? 1u : 0u);
    blocks = (threads + kBlock - 1) / kBlock;
  }
};

}  // namespace

void enqueueUndistortBgr(const dsopp_hip_undistorter *u, const uint8_t *bgr_in_dev, uint8_t *bgr_out_dev, uint8_t *grey_out_dev, hipStream_t stream) {
  checkOutputs(bgr_in_dev, bgr_out_dev, grey_out_dev);
  const Launch l(static_cast<size_t>(u->out_w) * u->out_h);
  undistortBgrKernel<<<l.blocks, kBlock, 0, stream>>>(u->table.get(), bgr_in_dev, u->in_w, reinterpret_cast<unsigned *>(bgr_out_dev),
                                                      reinterpret_cast<unsigned *>(grey_out_dev), l.words, l.tail);
  HIP_CHECK(hipGetLastError());
}

void enqueueBgrToGrey(const uint8_t *bgr_in_dev, uint8_t *grey_out_dev, size_t n, hipStream_t stream) {
  if (!bgr_in_dev || !grey_out_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (reinterpret_cast<uintptr_t>(grey_out_dev) & 3) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "device output images must be 4-byte aligned");
  if (n == 0 || n > static_cast<size_t>(INT_MAX)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an image of %zu pixels", n);
  const Launch l(n);
  bgrToGreyKernel<<<l.blocks, kBlock, 0, stream>>>(bgr_in_dev, reinterpret_cast<unsigned *>(grey_out_dev), l.words, l.tail);
  HIP_CHECK(hipGetLastError());
}

void enqueueTransformBgr(const dsopp_hip_transformer *t, const uint8_t *bgr_in_dev, uint8_t *bgr_out_dev, uint8_t *grey_out_dev, hipStream_t stream) {
  checkOutputs(bgr_in_dev, bgr_out_dev, grey_out_dev);
  const size_t n = static_cast<size_t>(t->out_w) * t->out_h;
  if (t->identity()) {
    if (grey_out_dev) enqueueBgrToGrey(bgr_in_dev, grey_out_dev, n, stream);
    if (bgr_out_dev && bgr_out_dev != bgr_in_dev) HIP_CHECK(hipMemcpyAsync(bgr_out_dev, bgr_in_dev, 3 * n, hipMemcpyDeviceToDevice, stream));
    return;
  }
  const Launch l(n);
  transformBgrKernel<<<l.blocks, kBlock, 0, stream>>>(t->table[kTransformLinear].get(), bgr_in_dev, static_cast<unsigned>(t->in_w),
                                                      static_cast<unsigned>(t->out_w), reinterpret_cast<unsigned *>(bgr_out_dev),
                                                      reinterpret_cast<unsigned *>(grey_out_dev), l.words, l.tail);
  HIP_CHECK(hipGetLastError());
}

}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_undistorter_undistort_bgr_device(dsopp_hip_undistorter *u, const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream) {
  return guarded([&] {
    if (!u) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null undistorter");
    u->sr.use();
    enqueueUndistortBgr(u, static_cast<const uint8_t *>(bgr_in_dev), static_cast<uint8_t *>(bgr_out_dev), static_cast<uint8_t *>(grey_out_dev),
                        stream ? static_cast<hipStream_t>(stream) : u->sr.stream);
  });
}

int dsopp_hip_transformer_transform_bgr_device(dsopp_hip_transformer *t, const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream) {
  return guarded([&] {
    if (!t) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null transformer");
    t->sr.use();
    enqueueTransformBgr(t, static_cast<const uint8_t *>(bgr_in_dev), static_cast<uint8_t *>(bgr_out_dev), static_cast<uint8_t *>(grey_out_dev),
                        stream ? static_cast<hipStream_t>(stream) : t->sr.stream);
  });
}

}  // extern "C"
