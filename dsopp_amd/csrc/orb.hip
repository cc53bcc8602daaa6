// ORB keypoint detection on the device: the feature refill of the bootstrap, and the dsopp_hip_orb_detector_* entry points.
//   DistinctFeaturesExtractorORB = cv::ORB::create(nfeatures, 2.0f, 5)->detect   src/feature_based_slam/features/src/distinct_features_extractor_orb.cpp:11-38
//   features::OpticalFlowMatch detects on every new frame and refills lost features   src/feature_based_slam/features/src/optical_flow.cpp:44-53
//   the first frame's features                                                        src/feature_based_slam/features/src/correspondences_finder.cpp:12-15
//
// The arithmetic is the one include/dsopp_hip.h states (a restatement of OpenCV 4's orb.cpp, fast.cpp and keypoint.cpp for keypoint
// positions; tests/orb_model.py is its NumPy form): integer level images, masks, FAST scores and Harris sums, and a short chain of single
// IEEE binary32 steps for the Harris response.  This file is compiled without floating-point contraction (build.sh and the pragma below).
//
// Layout.  Every plane of a level (image, mask, FAST score, survivor score) is dense row-major bytes.  The launches of a detect():
//   resizeKernel    one per level above 0: a thread owns an output pixel, the taps and 11-bit weights of its column and row come from
//                   tables the host computed at create (the float steps of cv::resize's index arithmetic are taken there, once).  The
//                   arithmetic is the image transformer's (transform.hip), whose handle cannot state these sizes: it resizes to
//                   (int)(n * ratio) and crops, a level is cvRound(n / 2^l) (163 -> 82, not 81)
//   fastKernel      all levels: a workgroup owns a 32 x 8 tile, the ring is read from an LDS tile with a 3-pixel halo
//   nmsKernel       all levels: a thread owns a pixel; the survivors of the 3 x 3 suppression, the mask and the border keep their score in
//                   the survivor plane and count into a 256-bin histogram per level (integer atomics: order-free)
//   rowCountKernel  all levels: a wave owns a row and counts its survivors at or above the level's first cut, which every wave reads off
//                   the histogram from the top
//   harrisKernel    all levels: a wave owns a row; its offset is the sum of the rows above, its survivors are compacted by ballot in
//                   ascending x and get their Harris response: the list of a level is in raster order whatever the scheduling
//   selectKernel    one workgroup: per level a radix select of the n-th largest response over the list (LDS histograms of integer
//                   counts), then an ordered compaction of the responses at or above it into the output records
// No step depends on the order in which atomics land.
#include "common.hpp"

#include <climits>
#include <cmath>
#include <memory>

#include "pyramid.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kOrbMaxLevels = 8;
constexpr int kTileW = 32, kTileH = 8, kHalo = 3;  // fastKernel's tile: kTileW * kTileH == kBlock
constexpr int kSelectBlock = 1024;
constexpr int kHarrisBlock = 7;

struct OrbLevel {
  const uint8_t *image;
  const uint8_t *mask;  // null = no mask
  uint8_t *score;       // FAST score, 0 where there is no corner
  uint8_t *nms;         // the score of a survivor of suppression, mask and border, else 0
  int w, h;
  int n;                        // n_l: the features this level may return
  int list_offset, row_offset;  // of this level in the candidate lists / in the row counts
  int tiles_x;
  unsigned first_tile, first_pixel_block, first_row;  // the first workgroup / wave of this level in fastKernel / nmsKernel / the row kernels
};

struct OrbArgs {
  OrbLevel level[kOrbMaxLevels];
  int n_levels, edge, threshold;
  unsigned tiles, pixel_blocks, rows;  // totals over the levels
  unsigned *histogram;                 // n_levels x 256
  int *row_count;                      // one per row of every level
  unsigned *cand_xy;                   // x | y << 16, a level's list in raster order
  float *cand_response;
  int *header;       // [0] = n, [1 + l] = the detections of level l
  float *records;    // n x {x, y, level (int bits), response}
};

/** one axis entry of the resize: taps x0, x1 and their 11-bit weights */
struct AxisEntry {
  int i0, i1, w0, w1;
};

__device__ __forceinline__ AxisEntry loadEntry(const AxisEntry *p) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  const i32x4 q = *reinterpret_cast<GlobalPtr<const i32x4>>(glb(p));
  return AxisEntry{q.x, q.y, q.z, q.w};
}

__global__ void __launch_bounds__(kBlock) resizeKernel(const uint8_t *__restrict__ src_, int sw, uint8_t *__restrict__ dst_, int dw, int dh,
                                                       const AxisEntry *__restrict__ xtab_, const AxisEntry *__restrict__ ytab_, int to_zero_below) {
  GlobalPtr<const uint8_t> src = glb(src_);
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= static_cast<unsigned>(dw) * static_cast<unsigned>(dh)) return;
  const int y = static_cast<int>(idx / static_cast<unsigned>(dw)), x = static_cast<int>(idx - static_cast<unsigned>(y) * dw);
  const AxisEntry ex = loadEntry(xtab_ + x), ey = loadEntry(ytab_ + y);
  GlobalPtr<const uint8_t> r0 = src + static_cast<size_t>(ey.i0) * sw, r1 = src + static_cast<size_t>(ey.i1) * sw;
  const int h0 = ex.w0 * r0[ex.i0] + ex.w1 * r0[ex.i1], h1 = ex.w0 * r1[ex.i0] + ex.w1 * r1[ex.i1];
  int v = (((ey.w0 * (h0 >> 4)) >> 16) + ((ey.w1 * (h1 >> 4)) >> 16) + 2) >> 2;
  if (v < to_zero_below) v = 0;  // threshold(254, THRESH_TOZERO) of a mask level: to_zero_below = 255; an image level: 0
  glb(dst_)[idx] = static_cast<uint8_t>(v);
}

/** level 0 of a mask from a pyramid's validity bytes: 255 / 0 */
__global__ void __launch_bounds__(kBlock) validityKernel(const uint8_t *__restrict__ src_, uint8_t *__restrict__ dst_, unsigned n) {
  const unsigned idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx < n) glb(dst_)[idx] = glb(src_)[idx] ? 255 : 0;
}

/** the level a workgroup or wave index belongs to, by the levels' first indices (ascending) */
template <typename First>
__device__ __forceinline__ int levelOf(const OrbArgs &a, unsigned index, First first) {
  int l = 0;
  for (int k = 1; k < a.n_levels; ++k)
    if (index >= first(a.level[k])) l = k;
  return l;
}

__global__ void __launch_bounds__(kBlock) fastKernel(const OrbArgs a) {
  __shared__ uint8_t tile[kTileH + 2 * kHalo][kTileW + 2 * kHalo + 2];
  const int l = levelOf(a, blockIdx.x, [](const OrbLevel &L) { return L.first_tile; });
  const OrbLevel L = a.level[l];
  const unsigned t = blockIdx.x - L.first_tile;
  const int ty = static_cast<int>(t / static_cast<unsigned>(L.tiles_x)), tx = static_cast<int>(t - static_cast<unsigned>(ty) * L.tiles_x);
  const int x0 = tx * kTileW, y0 = ty * kTileH;
  GlobalPtr<const uint8_t> img = glb(L.image);
  constexpr int kRows = kTileH + 2 * kHalo, kCols = kTileW + 2 * kHalo;
  for (int i = threadIdx.x; i < kRows * kCols; i += kBlock) {
    const int r = i / kCols, c = i - r * kCols;
    const int gx = x0 - kHalo + c, gy = y0 - kHalo + r;
    const bool inside = gx >= 0 && gx < L.w && gy >= 0 && gy < L.h;
    tile[r][c] = inside ? img[static_cast<size_t>(gy) * L.w + gx] : 0;
  }
  __syncthreads();
  const int lx = threadIdx.x % kTileW, ly = threadIdx.x / kTileW;
  const int x = x0 + lx, y = y0 + ly;
  if (x >= L.w || y >= L.h) return;
  int score = 0;
  if (x >= 3 && x < L.w - 3 && y >= 3 && y < L.h - 3) {
    constexpr int kRingX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int kRingY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    const int v = tile[ly + kHalo][lx + kHalo];
    int d[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = static_cast<int>(tile[ly + kHalo + kRingY[k]][lx + kHalo + kRingX[k]]) - v;
    // the minimum (bright) and the maximum (dark) of every circular arc of 9, by doubling: 2, 4, 8, then the ninth
    int lo[16], hi[16], lo2[16], hi2[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) lo[k] = min(d[k], d[(k + 1) & 15]), hi[k] = max(d[k], d[(k + 1) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) lo2[k] = min(lo[k], lo[(k + 2) & 15]), hi2[k] = max(hi[k], hi[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; ++k) lo[k] = min(lo2[k], lo2[(k + 4) & 15]), hi[k] = max(hi2[k], hi2[(k + 4) & 15]);
    int m = -255;
#pragma unroll
    for (int k = 0; k < 16; ++k) m = max(m, max(min(lo[k], d[(k + 8) & 15]), -max(hi[k], d[(k + 8) & 15])));
    if (m > a.threshold) score = m - 1;
  }
  glb(L.score)[static_cast<size_t>(y) * L.w + x] = static_cast<uint8_t>(score);
}

__global__ void __launch_bounds__(kBlock) nmsKernel(const OrbArgs a) {
  const int l = levelOf(a, blockIdx.x, [](const OrbLevel &L) { return L.first_pixel_block; });
  const OrbLevel L = a.level[l];
  const unsigned idx = (blockIdx.x - L.first_pixel_block) * kBlock + threadIdx.x;
  if (idx >= static_cast<unsigned>(L.w) * static_cast<unsigned>(L.h)) return;
  const int y = static_cast<int>(idx / static_cast<unsigned>(L.w)), x = static_cast<int>(idx - static_cast<unsigned>(y) * L.w);
  const int e = a.edge;  // >= 4: the 8 neighbours lie inside the level
  int keep = 0;
  if (x >= e && x < L.w - e && y >= e && y < L.h - e) {
    GlobalPtr<const uint8_t> s = glb(L.score) + static_cast<size_t>(y) * L.w + x;
    const int v = s[0];
    if (v > 0) {
      GlobalPtr<const uint8_t> up = s - L.w, down = s + L.w;
      const int around = max(max(max(up[-1], up[0]), max(up[1], s[-1])), max(max(s[1], down[-1]), max(down[0], down[1])));
      const bool valid = !L.mask || glb(L.mask)[idx] != 0;
      if (v > around && valid) keep = v;
    }
  }
  glb(L.nms)[idx] = static_cast<uint8_t>(keep);
  if (keep) atomicAdd(a.histogram + l * 256 + keep, 1u);
}

__device__ __forceinline__ int waveSumInt(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return __builtin_amdgcn_readfirstlane(v);
}

__device__ __forceinline__ int waveMaxInt(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
  return __builtin_amdgcn_readfirstlane(v);
}

/** retainBest(2 n) over a level's survivors, read off its histogram by one wave: the least score that stays.  At most 2 n survivors:
 *  all stay (1); else n = 0 keeps none (256); else every score at or above the 2 n-th largest, ties included. */
__device__ __forceinline__ int firstCut(const OrbArgs &a, int l, int lane) {
  GlobalPtr<const unsigned> hist = glb(a.histogram) + l * 256;
  const int want = 2 * a.level[l].n;
  int bin[4], own = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) bin[k] = static_cast<int>(hist[4 * lane + k]), own += bin[k];
  // above = the survivors in the bins of the lanes above this one
  int suffix = own;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int other = __shfl_down(suffix, o, 64);
    if (lane + o < 64) suffix += other;
  }
  const int total = __builtin_amdgcn_readfirstlane(__shfl(suffix, 0, 64));
  int running = suffix - own, best = 0;
#pragma unroll
  for (int k = 3; k >= 0; --k) {
    running += bin[k];
    if (best == 0 && running >= want) best = 4 * lane + k;
  }
  const int cut = waveMaxInt(best);
  if (total <= want) return 1;
  if (want == 0) return 256;
  return cut;
}

/** the (level, row) of a wave of the row kernels; false past the last row */
__device__ __forceinline__ bool rowOfWave(const OrbArgs &a, int &l, int &y) {
  const unsigned wave = __builtin_amdgcn_readfirstlane(static_cast<int>(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
  if (wave >= a.rows) return false;
  l = levelOf(a, wave, [](const OrbLevel &L) { return L.first_row; });
  y = static_cast<int>(wave - a.level[l].first_row);
  return true;
}

__global__ void __launch_bounds__(kBlock) rowCountKernel(const OrbArgs a) {
  int l, y;
  if (!rowOfWave(a, l, y)) return;
  const int lane = threadIdx.x & 63;
  const OrbLevel L = a.level[l];
  const int cut = firstCut(a, l, lane);
  GlobalPtr<const uint8_t> row = glb(L.nms) + static_cast<size_t>(y) * L.w;
  int count = 0;
  for (int x = lane; x < L.w; x += 64) {
    const int v = row[x];
    count += (v != 0 && v >= cut) ? 1 : 0;
  }
  count = waveSumInt(count);
  if (lane == 0) glb(a.row_count)[L.row_offset + y] = count;
}

/** HarrisResponses of orb.cpp at (x, y), block 7: the caller keeps 4 pixels of border */
__device__ __forceinline__ float harris(GlobalPtr<const uint8_t> img, int w, int x, int y) {
  int sa = 0, sb = 0, sc = 0;
  for (int dy = -3; dy <= 3; ++dy) {
    GlobalPtr<const uint8_t> r0 = img + static_cast<size_t>(y + dy - 1) * w + x, r1 = r0 + w, r2 = r1 + w;
#pragma unroll
    for (int dx = -3; dx <= 3; ++dx) {
      const int ix = 2 * (r1[dx + 1] - r1[dx - 1]) + (r0[dx + 1] - r0[dx - 1]) + (r2[dx + 1] - r2[dx - 1]);
      const int iy = 2 * (r2[dx] - r0[dx]) + (r2[dx - 1] - r0[dx - 1]) + (r2[dx + 1] - r0[dx + 1]);
      sa += ix * ix;  // |ix| <= 1020: 49 squares stay below 2^26
      sb += iy * iy;
      sc += ix * iy;
    }
  }
  const float scale = 1.0f / (4 * kHarrisBlock * 255.0f);
  const float s4 = scale * scale * scale * scale;
  const float fa = static_cast<float>(sa), fb = static_cast<float>(sb), fc = static_cast<float>(sc);
  const float trace = fa + fb;
  return ((fa * fb - fc * fc) - (0.04f * trace) * trace) * s4;
}

__global__ void __launch_bounds__(kBlock) harrisKernel(const OrbArgs a) {
  int l, y;
  if (!rowOfWave(a, l, y)) return;
  const int lane = threadIdx.x & 63;
  const OrbLevel L = a.level[l];
  GlobalPtr<const int> counts = glb(a.row_count) + L.row_offset;
  if (__builtin_amdgcn_readfirstlane(counts[y]) == 0) return;
  const int cut = firstCut(a, l, lane);
  int above = 0;
  for (int r = lane; r < y; r += 64) above += counts[r];
  int at = L.list_offset + waveSumInt(above);
  GlobalPtr<const uint8_t> row = glb(L.nms) + static_cast<size_t>(y) * L.w;
  for (int x0 = 0; x0 < L.w; x0 += 64) {
    const int x = x0 + lane;
    const int v = x < L.w ? row[x] : 0;
    const bool kept = v != 0 && v >= cut;
    const unsigned long long ballot = __ballot(kept);
    if (kept) {
      const int slot = at + __popcll(ballot & ((1ull << lane) - 1ull));
      glb(a.cand_xy)[slot] = static_cast<unsigned>(x) | (static_cast<unsigned>(y) << 16);
      glb(a.cand_response)[slot] = harris(glb(L.image), L.w, x, y);
    }
    at += __popcll(ballot);
  }
}

/** a float as an unsigned key of the same order; -0 counts as +0 */
__device__ __forceinline__ unsigned orderedKey(float r) {
  const unsigned bits = __float_as_uint(r + 0.0f);
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

__global__ void __launch_bounds__(kSelectBlock) selectKernel(const OrbArgs a) {
  __shared__ unsigned hist[256];
  __shared__ int wave_total[kSelectBlock / 64];
  __shared__ unsigned s_prefix;
  __shared__ int s_rank;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;  // the records written so far (the same in every thread)
  for (int l = 0; l < a.n_levels; ++l) {
    const OrbLevel L = a.level[l];
    // K = the length of the level's list
    int part = 0;
    for (int r = tid; r < L.h; r += kSelectBlock) part += glb(a.row_count)[L.row_offset + r];
    part = waveSumInt(part);
    __syncthreads();  // (the shared words of the level before are read no more)
    if (lane == 0) wave_total[wave] = part;
    __syncthreads();
    int K = 0;
    for (int k = 0; k < kSelectBlock / 64; ++k) K += wave_total[k];
    GlobalPtr<const float> resp = glb(a.cand_response) + L.list_offset;
    GlobalPtr<const unsigned> cxy = glb(a.cand_xy) + L.list_offset;
    // retainBest(n): at most n stay as they are; else n = 0 keeps none; else the keys at or above the n-th largest
    unsigned least = 0;
    bool none = false;
    if (K > L.n) {
      if (L.n == 0) {
        none = true;
      } else {
        unsigned prefix = 0, known = 0;
        int rank = L.n;  // the rank of the wanted key among those that share `prefix` in the bits `known`
        for (int shift = 24; shift >= 0; shift -= 8) {
          __syncthreads();
          if (tid < 256) hist[tid] = 0;
          __syncthreads();
          for (int i = tid; i < K; i += kSelectBlock) {
            const unsigned key = orderedKey(resp[i]);
            if ((key & known) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
          }
          __syncthreads();
          if (tid == 0) {
            int seen = 0, digit = 255;
            for (; digit > 0; --digit) {
              if (seen + static_cast<int>(hist[digit]) >= rank) break;
              seen += static_cast<int>(hist[digit]);
            }
            s_prefix = prefix | (static_cast<unsigned>(digit) << shift);
            s_rank = rank - seen;
          }
          __syncthreads();
          prefix = s_prefix;
          rank = s_rank;
          known |= 255u << shift;
        }
        least = prefix;
      }
    }
    // the ordered compaction of the list into the records
    int level_count = 0;
    if (!none) {
      const float up = static_cast<float>(1 << l);
      for (int i0 = 0; i0 < K; i0 += kSelectBlock) {
        const int i = i0 + tid;
        float r = 0.0f;
        bool kept = false;
        if (i < K) {
          r = resp[i];
          kept = orderedKey(r) >= least;
        }
        const unsigned long long ballot = __ballot(kept);
        __syncthreads();
        if (lane == 0) wave_total[wave] = __popcll(ballot);
        __syncthreads();
        int before = 0, all = 0;
        for (int k = 0; k < kSelectBlock / 64; ++k) {
          before += k < wave ? wave_total[k] : 0;
          all += wave_total[k];
        }
        if (kept) {
          const int slot = base + level_count + before + __popcll(ballot & ((1ull << lane) - 1ull));
          const unsigned p = cxy[i];
          GlobalPtr<float> rec = glb(a.records) + 4 * static_cast<size_t>(slot);
          rec[0] = static_cast<float>(p & 0xffffu) * up;
          rec[1] = static_cast<float>(p >> 16) * up;
          rec[2] = __int_as_float(l);
          rec[3] = r;
        }
        level_count += all;
      }
    }
    if (tid == 0) glb(a.header)[1 + l] = level_count;
    base += level_count;
  }
  if (tid == 0) glb(a.header)[0] = base;
}

/** cvRound of n / 2^l: to nearest, ties to even */
int halvedSize(int n, int l) {
  const int q = n >> l, rem = n - (q << l), half = l > 0 ? 1 << (l - 1) : 0;
  if (l == 0 || rem < half) return q;
  if (rem > half) return q + 1;
  return q + (q & 1);
}

/** the taps and weights of cv::resize(INTER_LINEAR) along an axis of n_in pixels resized to n_out (tests/transform_model.py: linear_axis) */
void linearAxis(int n_in, int n_out, AxisEntry *out) {
  const double scale = 1.0 / (static_cast<double>(n_out) / static_cast<double>(n_in));
  for (int d = 0; d < n_out; ++d) {
    float f = static_cast<float>((static_cast<double>(d) + 0.5) * scale - 0.5);
    const float whole = std::floor(f);
    int s = static_cast<int>(whole);
    f = f - whole;
    const bool low = s < 0, high = s >= n_in - 1;
    if (low) s = 0;
    if (high) s = n_in - 1;
    if (low || high) f = 0.0f;
    out[d].i0 = s;
    out[d].i1 = s + 1 < n_in ? s + 1 : n_in - 1;
    out[d].w1 = static_cast<int>(std::rint(f * 2048.0f));
    out[d].w0 = static_cast<int>(std::rint((1.0f - f) * 2048.0f));
  }
}

void featuresPerLevel(int nfeatures, int nlevels, int32_t *out) {
  const float factor = 0.5f;
  float nd = static_cast<float>(nfeatures) * (1.0f - factor) / (1.0f - static_cast<float>(std::pow(static_cast<double>(factor), static_cast<double>(nlevels))));
  int sum = 0;
  for (int l = 0; l < nlevels - 1; ++l) {
    out[l] = static_cast<int32_t>(std::lrint(nd));
    sum += out[l];
    nd *= factor;
  }
  out[nlevels - 1] = nfeatures - sum > 0 ? nfeatures - sum : 0;
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_orb_detector {
  dsopp_hip::StreamRef sr;
  int width = 0, height = 0, nfeatures = 0, n_levels = 1, edge = 31, threshold = 20;
  int w[dsopp_hip::kOrbMaxLevels] = {0}, h[dsopp_hip::kOrbMaxLevels] = {0}, n[dsopp_hip::kOrbMaxLevels] = {0};
  dsopp_hip::DeviceMem<uint8_t> image[dsopp_hip::kOrbMaxLevels], mask[dsopp_hip::kOrbMaxLevels], score[dsopp_hip::kOrbMaxLevels],
      nms[dsopp_hip::kOrbMaxLevels];
  dsopp_hip::DeviceMem<dsopp_hip::AxisEntry> xtab[dsopp_hip::kOrbMaxLevels], ytab[dsopp_hip::kOrbMaxLevels];  // of the resize INTO level l
  dsopp_hip::DeviceMem<unsigned> histogram, cand_xy;
  dsopp_hip::DeviceMem<int> row_count;
  dsopp_hip::DeviceMem<float> cand_response;
  dsopp_hip::DeviceMem<uint8_t> d_out;  // header (kHeaderBytes) | records
  dsopp_hip::OrbArgs args;
  size_t bound = 0;       // the most detections any input can give: the sum of ceil(w / 2) ceil(h / 2) over the levels
  size_t first_copy = 0;  // the records that come back with the header; more (boundary ties only) cost a second copy
  bool has_mask = false, detected = false;
  // a host image or mask leaves from this pinned copy; uploaded guards its reuse
  dsopp_hip::PinnedMem<uint8_t> h_image, h_out;
  dsopp_hip::Event uploaded, image_read;
  bool upload_pending = false;
};

namespace dsopp_hip {
namespace {

constexpr size_t kHeaderBytes = 64;  // 1 + kOrbMaxLevels counts, and the records start on a 64-byte line

void checkHandle(const dsopp_hip_orb_detector *d) {
  if (!d) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null ORB detector");
}

unsigned blocksFor(size_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

/** levels 1 .. of `plane` from its level 0 (masks: with the threshold) */
void enqueueResizes(dsopp_hip_orb_detector *d, dsopp_hip::DeviceMem<uint8_t> *plane, bool is_mask) {
  for (int l = 1; l < d->n_levels; ++l) {
    resizeKernel<<<blocksFor(static_cast<size_t>(d->w[l]) * d->h[l]), kBlock, 0, d->sr.stream>>>(
        plane[l - 1].get(), d->w[l - 1], plane[l].get(), d->w[l], d->h[l], d->xtab[l].get(), d->ytab[l].get(), is_mask ? 255 : 0);
    HIP_CHECK(hipGetLastError());
  }
}

/** rows of a host plane (stride >= width) through the pinned copy into `dst` (dense) */
void uploadPlane(dsopp_hip_orb_detector *d, uint8_t *dst, const uint8_t *host, size_t stride) {
  if (d->upload_pending) HIP_CHECK(hipEventSynchronize(d->uploaded.h));
  const size_t W = static_cast<size_t>(d->width);
  for (int y = 0; y < d->height; ++y) copyToPinned(d->h_image.get() + y * W, host + y * stride, W);
  HIP_CHECK(hipMemcpyAsync(dst, d->h_image.get(), W * d->height, hipMemcpyHostToDevice, d->sr.stream));
  HIP_CHECK(hipEventRecord(d->uploaded.get(hipEventDisableTiming), d->sr.stream));
  d->upload_pending = true;
}

void checkDetect(const dsopp_hip_orb_detector *d, int32_t capacity, const float *xy, const int32_t *level, const float *response, const int32_t *n) {
  checkHandle(d);
  if (!n || capacity < 0 || (capacity > 0 && (!xy || !level || !response))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
}

void imageFromHost(dsopp_hip_orb_detector *d, const uint8_t *image_host, size_t stride) {
  if (!image_host) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (stride < static_cast<size_t>(d->width)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a row stride of %zu bytes for %d pixels", stride, d->width);
  d->sr.use();
  uploadPlane(d, d->image[0].get(), image_host, stride);
}

/** level 0 from an image in HBM: a strided copy on the detector's stream (every detect ends with a wait, behind which the image has been read) */
void imageFromDevice(dsopp_hip_orb_detector *d, const void *image_dev, size_t stride) {
  HIP_CHECK(hipMemcpy2DAsync(d->image[0].get(), static_cast<size_t>(d->width), image_dev, stride, static_cast<size_t>(d->width),
                             static_cast<size_t>(d->height), hipMemcpyDeviceToDevice, d->sr.stream));
}

void imageFromDevicePointer(dsopp_hip_orb_detector *d, const void *image_dev, size_t stride) {
  if (!image_dev) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null image");
  if (stride < static_cast<size_t>(d->width)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a row stride of %zu bytes for %d pixels", stride, d->width);
  d->sr.use();
  imageFromDevice(d, image_dev, stride);
}

void checkPyramid(const dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *p) {
  if (!p) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null pyramid");
  if (p->sr.device != d->sr.device) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid lives on device %d, the ORB detector on %d", p->sr.device, d->sr.device);
  if (p->width != d->width || p->height != d->height)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid is %d x %d, the ORB detector %d x %d", p->width, p->height, d->width, d->height);
}

void imageFromPyramid(dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *p) {
  checkPyramid(d, p);
  if (!p->has_undistorted) fail(DSOPP_HIP_ERR_STATE, "the pyramid keeps no 8-bit image (its last build was none of build_undistorted, build_transformed, build_colour)");
  d->sr.use();
  p->waitReady(d->sr.stream);
  imageFromDevice(d, p->undistorted_u8.get(), static_cast<size_t>(p->width));
}

/** everything behind level 0 of the image, and the one wait of a detect() */
void detect(dsopp_hip_orb_detector *d, int32_t capacity, float *xy, int32_t *level, float *response, int32_t *n) {
  const hipStream_t st = d->sr.stream;
  enqueueResizes(d, d->image, false);
  OrbArgs &a = d->args;
  for (int l = 0; l < d->n_levels; ++l) a.level[l].mask = d->has_mask ? d->mask[l].get() : nullptr;
  HIP_CHECK(hipMemsetAsync(d->histogram.get(), 0, sizeof(unsigned) * 256 * d->n_levels, st));
  fastKernel<<<a.tiles, kBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  nmsKernel<<<a.pixel_blocks, kBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  const unsigned row_blocks = (a.rows + kBlock / 64 - 1) / (kBlock / 64);
  rowCountKernel<<<row_blocks, kBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  harrisKernel<<<row_blocks, kBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  selectKernel<<<1, kSelectBlock, 0, st>>>(a);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(d->h_out.get(), d->d_out.get(), kHeaderBytes + 16 * d->first_copy, hipMemcpyDeviceToHost, st));
  d->sr.sync();
  d->detected = true;
  const int count = reinterpret_cast<const int *>(d->h_out.get())[0];
  *n = count;
  if (count > capacity) fail(DSOPP_HIP_ERR_CAPACITY, "%d detections for a capacity of %d", count, capacity);
  if (static_cast<size_t>(count) > d->first_copy) {  // boundary ties kept more than the features asked for and the slack: fetch the rest
    const size_t need = kHeaderBytes + 16 * static_cast<size_t>(count);
    if (d->h_out.bytes < need) {
      d->h_out.reserve(need);
      HIP_CHECK(hipMemcpyAsync(d->h_out.get(), d->d_out.get(), need, hipMemcpyDeviceToHost, st));
    } else {
      const size_t done = kHeaderBytes + 16 * d->first_copy;
      HIP_CHECK(hipMemcpyAsync(d->h_out.get() + done, d->d_out.get() + done, need - done, hipMemcpyDeviceToHost, st));
    }
    d->sr.sync();
  }
  const float *rec = reinterpret_cast<const float *>(d->h_out.get() + kHeaderBytes);
  for (int i = 0; i < count; ++i) {
    xy[2 * i] = rec[4 * i];
    xy[2 * i + 1] = rec[4 * i + 1];
    std::memcpy(&level[i], &rec[4 * i + 2], sizeof(int32_t));
    response[i] = rec[4 * i + 3];
  }
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_orb_features_per_level(int nfeatures, int nlevels, int32_t *out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nfeatures < 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d features", nfeatures);
    if (nlevels < 1 || nlevels > kOrbMaxLevels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d levels: 1 .. %d", nlevels, kOrbMaxLevels);
    featuresPerLevel(nfeatures, nlevels, out);
  });
}

int dsopp_hip_orb_detector_create(int width, int height, int nfeatures, int nlevels, int edge_threshold, int fast_threshold, int device, void *stream,
                                  dsopp_hip_orb_detector **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (nlevels < 1 || nlevels > kOrbMaxLevels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d levels: 1 .. %d", nlevels, kOrbMaxLevels);
    if (edge_threshold < 4) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an edge threshold of %d: the Harris block needs 4 pixels of border", edge_threshold);
    if (fast_threshold < 0 || fast_threshold > 255) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a FAST threshold of %d: 0 .. 255", fast_threshold);
    if (nfeatures < 0 || nfeatures > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d features", nfeatures);
    if (width < 1 || height < 1 || width > 65535 || height > 65535) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an image of %d x %d", width, height);
    if (static_cast<long long>(width) * height > INT_MAX / 8) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image too large");
    if (halvedSize(width, nlevels - 1) < 1 || halvedSize(height, nlevels - 1) < 1)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "level %d of an image of %d x %d is empty", nlevels - 1, width, height);
    auto d = std::make_unique<dsopp_hip_orb_detector>();
    d->sr.init(device, stream);
    d->width = width;
    d->height = height;
    d->nfeatures = nfeatures;
    d->n_levels = nlevels;
    d->edge = edge_threshold;
    d->threshold = fast_threshold;
    featuresPerLevel(nfeatures, nlevels, d->n);
    const hipStream_t st = d->sr.stream;
    OrbArgs &a = d->args;
    std::memset(&a, 0, sizeof(a));
    size_t lists = 0, rows = 0, tiles = 0, pixel_blocks = 0;
    std::vector<AxisEntry> axis;
    for (int l = 0; l < nlevels; ++l) {
      const int w = halvedSize(width, l), h = halvedSize(height, l);
      d->w[l] = w;
      d->h[l] = h;
      const size_t bytes = static_cast<size_t>(w) * h;
      d->image[l].alloc(bytes);
      d->mask[l].alloc(bytes);
      d->score[l].alloc(bytes);
      d->nms[l].alloc(bytes);
      if (l > 0) {
        axis.resize(static_cast<size_t>(w > h ? w : h));
        d->xtab[l].alloc(sizeof(AxisEntry) * w);
        d->ytab[l].alloc(sizeof(AxisEntry) * h);
        linearAxis(d->w[l - 1], w, axis.data());
        HIP_CHECK(hipMemcpy(d->xtab[l].get(), axis.data(), sizeof(AxisEntry) * w, hipMemcpyHostToDevice));
        linearAxis(d->h[l - 1], h, axis.data());
        HIP_CHECK(hipMemcpy(d->ytab[l].get(), axis.data(), sizeof(AxisEntry) * h, hipMemcpyHostToDevice));
      }
      OrbLevel &L = a.level[l];
      L.image = d->image[l].get();
      L.score = d->score[l].get();
      L.nms = d->nms[l].get();
      L.w = w;
      L.h = h;
      L.n = d->n[l];
      L.list_offset = static_cast<int>(lists);
      L.row_offset = static_cast<int>(rows);
      L.tiles_x = (w + kTileW - 1) / kTileW;
      L.first_tile = static_cast<unsigned>(tiles);
      L.first_pixel_block = static_cast<unsigned>(pixel_blocks);
      L.first_row = static_cast<unsigned>(rows);
      // no two survivors of the 3 x 3 suppression share a 2 x 2 cell: no input fills a level's list beyond this
      lists += static_cast<size_t>((w + 1) / 2) * ((h + 1) / 2);
      rows += static_cast<size_t>(h);
      tiles += static_cast<size_t>(L.tiles_x) * ((h + kTileH - 1) / kTileH);
      pixel_blocks += blocksFor(bytes);
    }
    d->bound = lists;
    const size_t slack = static_cast<size_t>(nfeatures) + 256;
    d->first_copy = lists < slack ? lists : slack;
    d->histogram.alloc(sizeof(unsigned) * 256 * nlevels);
    d->row_count.alloc(sizeof(int) * rows);
    d->cand_xy.alloc(sizeof(unsigned) * lists);
    d->cand_response.alloc(sizeof(float) * lists);
    d->d_out.alloc(kHeaderBytes + 16 * lists);
    d->h_out.reserve(kHeaderBytes + 16 * d->first_copy);
    d->h_image.reserve(static_cast<size_t>(width) * height);
    a.n_levels = nlevels;
    a.edge = edge_threshold;
    a.threshold = fast_threshold;
    a.tiles = static_cast<unsigned>(tiles);
    a.pixel_blocks = static_cast<unsigned>(pixel_blocks);
    a.rows = static_cast<unsigned>(rows);
    a.histogram = d->histogram.get();
    a.row_count = d->row_count.get();
    a.cand_xy = d->cand_xy.get();
    a.cand_response = d->cand_response.get();
    a.header = reinterpret_cast<int *>(d->d_out.get());
    a.records = reinterpret_cast<float *>(d->d_out.get() + kHeaderBytes);
    HIP_CHECK(hipMemsetAsync(d->d_out.get(), 0, kHeaderBytes, st));
    d->sr.sync();
    *out = d.release();
  });
}

void dsopp_hip_orb_detector_destroy(dsopp_hip_orb_detector *d) {
  if (!d) return;
  (void)hipSetDevice(d->sr.device);
  if (d->sr.stream) (void)hipStreamSynchronize(d->sr.stream);
  delete d;
}

int dsopp_hip_orb_detector_set_mask(dsopp_hip_orb_detector *d, const uint8_t *mask_host) {
  return guarded([&] {
    checkHandle(d);
    d->sr.use();
    if (!mask_host) {
      d->has_mask = false;
      return;
    }
    uploadPlane(d, d->mask[0].get(), mask_host, static_cast<size_t>(d->width));
    enqueueResizes(d, d->mask, true);
    d->has_mask = true;
  });
}

int dsopp_hip_orb_detector_set_mask_from_pyramid(dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *pyramid) {
  return guarded([&] {
    checkHandle(d);
    checkPyramid(d, pyramid);
    if (!pyramid->has_mask0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the pyramid keeps no level-0 mask: it never had dsopp_hip_pyramid_set_semantics");
    d->sr.use();
    pyramid->waitReady(d->sr.stream);
    const size_t n = static_cast<size_t>(d->width) * d->height;
    validityKernel<<<blocksFor(n), kBlock, 0, d->sr.stream>>>(pyramid->mask0_u8.get(), d->mask[0].get(), static_cast<unsigned>(n));
    HIP_CHECK(hipGetLastError());
    enqueueResizes(d, d->mask, true);
    d->has_mask = true;
  });
}

int dsopp_hip_orb_detector_detect(dsopp_hip_orb_detector *d, const uint8_t *image_host, size_t stride, int32_t capacity, float *xy, int32_t *level,
                                  float *response, int32_t *n) {
  return guarded([&] {
    checkDetect(d, capacity, xy, level, response, n);
    imageFromHost(d, image_host, stride);
    detect(d, capacity, xy, level, response, n);
  });
}

int dsopp_hip_orb_detector_detect_device(dsopp_hip_orb_detector *d, const void *image_dev, size_t stride, int32_t capacity, float *xy, int32_t *level,
                                         float *response, int32_t *n) {
  return guarded([&] {
    checkDetect(d, capacity, xy, level, response, n);
    imageFromDevicePointer(d, image_dev, stride);
    detect(d, capacity, xy, level, response, n);
  });
}

int dsopp_hip_orb_detector_detect_from_pyramid(dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *pyramid, int32_t capacity, float *xy, int32_t *level,
                                               float *response, int32_t *n) {
  return guarded([&] {
    checkDetect(d, capacity, xy, level, response, n);
    imageFromPyramid(d, pyramid);
    detect(d, capacity, xy, level, response, n);
  });
}

int dsopp_hip_orb_detector_get_level(dsopp_hip_orb_detector *d, int level, uint8_t *image_out, uint8_t *mask_out, uint8_t *score_out, int *w, int *h) {
  return guarded([&] {
    checkHandle(d);
    if (level < 0 || level >= d->n_levels) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "level %d of %d", level, d->n_levels);
    if (w) *w = d->w[level];
    if (h) *h = d->h[level];
    if (!image_out && !mask_out && !score_out) return;
    if ((image_out || score_out) && !d->detected) fail(DSOPP_HIP_ERR_STATE, "no image was detected on");
    d->sr.use();
    const size_t bytes = static_cast<size_t>(d->w[level]) * d->h[level];
    if (image_out) HIP_CHECK(hipMemcpyAsync(image_out, d->image[level].get(), bytes, hipMemcpyDeviceToHost, d->sr.stream));
    if (score_out) HIP_CHECK(hipMemcpyAsync(score_out, d->score[level].get(), bytes, hipMemcpyDeviceToHost, d->sr.stream));
    if (mask_out && d->has_mask) HIP_CHECK(hipMemcpyAsync(mask_out, d->mask[level].get(), bytes, hipMemcpyDeviceToHost, d->sr.stream));
    d->sr.sync();
    if (mask_out && !d->has_mask) std::memset(mask_out, 255, bytes);  // without a mask every pixel is valid
  });
}

}  // extern "C"
