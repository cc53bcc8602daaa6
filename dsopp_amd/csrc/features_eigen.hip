// The reference's `eigen` tracking-feature extractor (DSO's pixel selector) on the device:
//   EigenTrackingFeaturesExtractor::extract — src/features/src/eigen_tracking_features_extractor.cpp:432-469
//
// Per call: the extractor's own raw pyramid (5 levels, identity LUT, no vignette: the library's pyramid build), the threshold map
// (eigenCellKernel: one workgroup per 32 x 32-ish cell histograms (int)min(|g|, 49) and takes its median bin + 7; eigenMapKernel:
// the square of the clipped 3 x 3 mean), and eigenPixelKernel: per level-0 pixel and level the direction-free part of
// findBestCandidate (border, map cell, g^2 > threshold) and whether any of the 16 directions gives an exactly zero projection.
//
// The walk of findFeaturesInWindow is serial in the reference: the direction a window uses is pattern[n], n = the features emitted so
// far.  It is split by what does not depend on n.  Inside a level-L window, "some level below L accepted a candidate" holds exactly
// when some visited pixel has a level l < L that passes the direction-free test with a non-zero projection (the first such pair in
// traversal order is accepted: nothing can block it), and the window emits exactly when that is false and some visited pixel passes
// level L with a non-zero projection.  A projection is zero only for directions in the pixel's zero set, so each of these facts is
// certain, impossible or undetermined.  eigenWindowBitsKernel ORs the pixel bits per level-0 window, eigenCountKernel reduces them up
// the 4-ary window tree of every top (level-4) window into its emission count and an undetermined flag, eigenChainKernel (one wave)
// scans the counts into start offsets and walks the undetermined top windows in order as their starts become known, and
// eigenEmitKernel walks every other top window from its start: the candidate records of levels >= 1 carry across its level-0 windows,
// and each level-0 window's pixels are resolved 64 per ballot.  A record only decides its own level's emission and blocks nothing
// below it, so when no level-3 or level-4 window of a determined top window can emit, its 16 level-2 windows are walked by 16 waves
// from their own start counts; otherwise one wave walks the whole top window.  The emission count of the pass comes back to the
// host, which decides on a second pass (calculatePotential) and runs the final reduction as a stable device select.
//
// Arithmetic: g^2 = dx^2 + dy^2 of dyadic values with few bits is exact; the projection |cos dx + sin dy| rounds each product and the
// sum, as the reference's scalar code (this file is compiled without contraction).  A reference built with FMA contraction may fuse
// that sum; that cannot be pinned.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cmath>
#include <climits>
#include <cstring>
#include <memory>
#include <vector>

#include "common.hpp"
#include "features.hpp"
#include "pyramid.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {

constexpr int kLevels = 5;        // kMaxPyramidDepth of the extractor's pyramid
constexpr int kBorder = 4;        // kBorderSize
constexpr int kMapShift = 5;      // the threshold-map cell of a pixel is (x >> 5, y >> 5)
constexpr int kBins = 50;         // kMaxGradientLength
constexpr double kMinGradient = 7;
constexpr int kWindowsPerTop = 256;  // 4^4 level-0 windows in a level-4 window
constexpr int kBlock = 256;
constexpr int kBatch = 4;            // pixel chunks of a level-0 window whose loads the walk issues together (resolved by hand below)
constexpr int kInitialPotential = 15;
constexpr unsigned kRandomSeed = 3141592;
constexpr uint16_t kVisitedBit = 1u << 15;

struct Levels {
  const Texel<double> *tex[kLevels];
  int w[kLevels], h[kLevels];
};

// pow(0.75, l) as the reference's loop computes it (exact: 3^4 / 4^4)
__host__ __device__ constexpr double levelFactor(int l) { return l == 0 ? 1.0 : l == 1 ? 0.75 : l == 2 ? 0.5625 : l == 3 ? 0.421875 : 0.31640625; }

__device__ __forceinline__ bool cornerValid(const uint8_t *__restrict__ valid, int W, int H, int x, int y) {
  return x >= 0 && y >= 0 && x < W && y < H && (!valid || valid[y * W + x]);
}

__device__ __forceinline__ double2 gradientAt(const Levels &L, int l, int x, int y) {
  const int xl = min(x >> l, L.w[l] - 1), yl = min(y >> l, L.h[l] - 1);
  const double *t = reinterpret_cast<const double *>(L.tex[l] + yl * L.w[l] + xl);
  return *reinterpret_cast<const double2 *>(t + 2);  // {Ix, Iy}
}

// fillGradientThresholdMap, one workgroup per cell: the histogram of (int)min(sqrt(g^2), 49) over the valid pixels of
// [max(cw i, 1), min(cw (i + 1), W - 2)) x [max(ch j, 1), min(ch (j + 1), H - 2)), then computeMedian + 7.  The bin is the largest
// b <= 49 with b^2 <= g^2, which is (int)sqrt(g^2) for a correctly rounded sqrt.
__global__ void __launch_bounds__(kBlock) eigenCellKernel(const Texel<double> *__restrict__ lv0, int W, int H, const uint8_t *__restrict__ valid,
                                                          int mw, int cw, int ch, double *__restrict__ raw) {
  __shared__ unsigned bins[kBins];
  const int cell = blockIdx.x, i = cell % mw, j = cell / mw;
  for (int b = threadIdx.x; b < kBins; b += kBlock) bins[b] = 0;
  __syncthreads();
  const int x0 = max(cw * i, 1), x1 = min(cw * (i + 1), W - 2);
  const int y0 = max(ch * j, 1), y1 = min(ch * (j + 1), H - 2);
  const int nx = x1 - x0, ny = y1 - y0;
  if (nx > 0 && ny > 0) {
    for (int k = threadIdx.x; k < nx * ny; k += kBlock) {
      const int x = x0 + k % nx, y = y0 + k / nx;
      if (valid && !valid[y * W + x]) continue;
      const double2 g = *reinterpret_cast<const double2 *>(reinterpret_cast<const double *>(lv0 + y * W + x) + 2);  // {Ix, Iy}
      const double g2 = g.x * g.x + g.y * g.y;
      int b = 0;
      while (b + 1 < kBins && static_cast<double>((b + 1) * (b + 1)) <= g2) ++b;
      atomicAdd(&bins[b], 1u);
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    unsigned total = 0;
    for (int b = 0; b < kBins; ++b) total += bins[b];
    long thr = static_cast<long>(round(static_cast<double>(total) * 0.5));
    int median = 0;
    for (int b = 0; b < kBins; ++b) {
      thr -= bins[b];
      if (thr < 0) {
        median = b;
        break;
      }
    }
    raw[cell] = static_cast<double>(median) + kMinGradient;
  }
}

// medianFilter: the square of the mean over the 3 x 3 neighbourhood clipped to the map (summed x-offset outer, y-offset inner)
__global__ void __launch_bounds__(kBlock) eigenMapKernel(const double *__restrict__ raw, int mw, int mh, double *__restrict__ map) {
  const int cell = blockIdx.x * kBlock + threadIdx.x;
  if (cell >= mw * mh) return;
  const int i = cell % mw, j = cell / mw;
  double sum = 0, num = 0;
  for (int a = -1; a <= 1; ++a)
    for (int b = -1; b <= 1; ++b) {
      const int xi = i + a, yj = j + b;
      if (xi < 0 || xi > mw - 1 || yj < 0 || yj > mh - 1) continue;
      num += 1;
      sum += raw[yj * mw + xi];
    }
  map[cell] = (sum / num) * (sum / num);
}

// findBestCandidate without the directions, per level-0 pixel: bit l = the pixel is valid in the eroded mask and level l passes the
// border, map-cell and g^2 > threshold tests (the threshold cumulative, a failed border ending the pixel); bit 5 + l = in addition
// no direction of the 16 gives an exactly zero projection at level l.
__global__ void __launch_bounds__(kBlock) eigenPixelKernel(Levels L, int W, int H, const uint8_t *__restrict__ valid, const double *__restrict__ map,
                                                           int mw, int mh, const double *__restrict__ dirs, uint16_t *__restrict__ bits) {
  const int idx = blockIdx.x * kBlock + threadIdx.x;
  if (idx >= W * H) return;
  const int y = idx / W, x = idx - y * W;
  unsigned out = 0;
  const bool inside = x >= kBorder && x < W - 1 - kBorder && y >= kBorder && y <= H - 1 - kBorder;
  if ((!valid || valid[idx]) && inside && (x >> kMapShift) < mw && (y >> kMapShift) < mh) {
    double thr = map[(y >> kMapShift) * mw + (x >> kMapShift)];
    for (int l = 0; l < kLevels; ++l) {
      thr = thr * levelFactor(l);
      const int xl = x >> l, yl = y >> l;
      if (xl < kBorder || xl >= W - 1 - kBorder || yl < kBorder || yl > H - 1 - kBorder) break;
      const double2 g = gradientAt(L, l, x, y);
      const double g2 = g.x * g.x + g.y * g.y;
      if (!(g2 > thr)) continue;
      out |= 1u << l;
      bool nonzero = true;
      for (int d = 0; d < 16; ++d) {
        const double pr = dirs[2 * d] * g.x + dirs[2 * d + 1] * g.y;
        nonzero = nonzero && pr != 0.0;
      }
      if (nonzero) out |= 1u << (kLevels + l);
    }
  }
  bits[idx] = static_cast<uint16_t>(out);
}

struct TopGrid {
  int p, ntx, nt;
  __device__ void corner(int T, int &x, int &y) const {
    x = (T % ntx) * 16 * p;
    y = (T / ntx) * 16 * p;
  }
};

// the corner of child c (row-major 2 x 2) of a level-L window at (x, y): step 2^(L-1) p
__device__ __forceinline__ void child(int L, int p, int c, int &x, int &y) {
  const int step = (1 << (L - 1)) * p;
  x += (c & 1) * step;
  y += (c >> 1) * step;
}

__device__ __forceinline__ unsigned waveOr(unsigned v) {
  for (int o = 32; o > 0; o >>= 1) v |= __shfl_xor(v, o);
  return v;
}

// one wave per level-0 window t of top window T (t's base-4 digits, most significant first, are the child indices at levels 3..0):
// whether every corner on its path passes the eroded mask, and the OR of its pixels' bits
__global__ void __launch_bounds__(kBlock) eigenWindowBitsKernel(const uint16_t *__restrict__ bits, const uint8_t *__restrict__ valid, int W, int H,
                                                                TopGrid g, uint16_t *__restrict__ wbits) {
  const int gw = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  const int T = gw / kWindowsPerTop, t = gw % kWindowsPerTop;
  if (T >= g.nt) return;  // (wave-uniform)
  int x, y;
  g.corner(T, x, y);
  bool visited = true;
  for (int L = 4; L >= 1 && visited; --L) {
    child(L, g.p, (t >> (2 * (L - 1))) & 3, x, y);
    visited = cornerValid(valid, W, H, x, y);
  }
  unsigned acc = 0;
  if (visited) {
    const int np = g.p * g.p;
    for (int k = lane; k < np; k += 64) {
      const int px = x + k % g.p, py = y + k / g.p;
      if (px < W && py < H) acc |= bits[py * W + px];
    }
    acc = waveOr(acc);
  }
  if (lane == 0) wbits[gw] = static_cast<uint16_t>(acc | (visited ? kVisitedBit : 0u));
}

// the emission decision of a window from the OR of its visited pixels' bits: (certain emission, undetermined)
__device__ __forceinline__ void decide(unsigned b, int L, int &E, int &und) {
  const unsigned poss = b & 31u, cert = (b >> kLevels) & 31u, low = (1u << L) - 1u;
  const bool emit_cert = !(poss & low) && ((cert >> L) & 1u);
  const bool emit_poss = !(cert & low) && ((poss >> L) & 1u);
  E += emit_cert;
  und |= emit_poss && !emit_cert;
}

// per top window: the number of emissions and whether every emission decision in it is determined, reduced up the window tree; the
// emissions of each level-2 window, and split = determined with no level-3 or level-4 window that may emit: then the records of levels
// 3 and 4 cannot matter, and the 16 level-2 windows can be walked independently from their own start counts
__global__ void __launch_bounds__(kWindowsPerTop) eigenCountKernel(const uint16_t *__restrict__ wbits, int *__restrict__ count, int *__restrict__ undet,
                                                                   int *__restrict__ count2, int *__restrict__ split) {
  __shared__ unsigned sb[kWindowsPerTop];
  __shared__ int se[kWindowsPerTop], su[kWindowsPerTop], sh[kWindowsPerTop];
  const int T = blockIdx.x, t = threadIdx.x;
  const unsigned b = wbits[T * kWindowsPerTop + t] & 0x3ffu;
  int E = 0, und = 0;
  decide(b, 0, E, und);
  sb[t] = b;
  se[t] = E;
  su[t] = und;
  sh[t] = 0;
  for (int L = 1; L < kLevels; ++L) {
    __syncthreads();
    const int n = kWindowsPerTop >> (2 * L);
    unsigned cb = 0;
    int ce = 0, cu = 0, ch = 0;
    if (t < n) {
      for (int c = 0; c < 4; ++c) {
        cb |= sb[4 * t + c];
        ce += se[4 * t + c];
        cu |= su[4 * t + c];
        ch |= sh[4 * t + c];
      }
      int own = 0, own_und = 0;
      decide(cb, L, own, own_und);
      ce += own;
      cu |= own_und;
      if (L >= 3) ch |= own | own_und;
    }
    __syncthreads();
    if (t < n) {
      sb[t] = cb;
      se[t] = ce;
      su[t] = cu;
      sh[t] = ch;
      if (L == 2) count2[T * 16 + t] = ce;
    }
  }
  if (t == 0) {
    count[T] = se[0];
    undet[T] = su[0];
    split[T] = !su[0] && !sh[0];
  }
}

struct WalkArgs {
  Levels L;
  const uint16_t *bits, *wbits;
  const uint8_t *valid;
  const uint8_t *pattern;
  const double *dirs;
  int W, H, npattern;
  TopGrid g;
  int *out;
  int cap;
};

// findFeaturesInWindow over one top window, started with n features emitted, by one wave (every value below is wave-uniform except
// the per-lane pixel data); writes its emissions at out[n...] when `write`.  Returns n after the window.  sub >= 0 walks only the
// level-2 window sub = 4 c3 + c2 of a split top window and emits nothing on levels 3 and 4 (which emit nothing there).
__device__ int walkTop(const WalkArgs &a, int T, int n, bool write, int sub) {
  const int lane = threadIdx.x & 63;
  const int p = a.g.p;
  int cand[kLevels];  // -1: none, -2: blocked by a lower level, else the pixel index y * W + x
  double weight[kLevels], dc[kLevels], ds[kLevels];
#pragma unroll
  for (int l = 0; l < kLevels; ++l) {
    cand[l] = -1;
    weight[l] = 0;
    dc[l] = 0;
    ds[l] = 0;
  }
  auto setDir = [&](int level) {
    const int d = a.pattern[min(n, a.npattern - 1)] & 15;
    const double c = a.dirs[2 * d], s = a.dirs[2 * d + 1];
#pragma unroll
    for (int l = 0; l < kLevels; ++l)
      if (l == level) {
        dc[l] = c;
        ds[l] = s;
      }
  };
  auto emit = [&](int level) {
    int c = -1;
#pragma unroll
    for (int l = 0; l < kLevels; ++l)
      if (l == level) c = cand[l];
    if (c >= 0) {  // (x >= 4 > 0 for every accepted pixel)
      if (write && lane == 0 && n < a.cap) a.out[n] = c;
      ++n;
#pragma unroll
      for (int l = 1; l < kLevels; ++l)
        if (l == level + 1) weight[l] = 1e10;
    }
  };
  auto startWindow = [&](int level) {
#pragma unroll
    for (int l = 0; l < kLevels; ++l)
      if (l == level) {
        cand[l] = -1;
        weight[l] = 0;
      }
  };
  // one chunk of 64 pixels of the current level-0 window: a pixel acts at the lowest level that is not blocked, passes the
  // direction-free test and projects above the level's weight; the first acting pixel is applied, then the rest are re-tested
  auto resolveChunk = [&](unsigned b, const double2 *gr, int pidx) {
    double g2[kLevels], pr[kLevels];
    for (int l = 0; l < kLevels; ++l) {
      g2[l] = gr[l].x * gr[l].x + gr[l].y * gr[l].y;
      pr[l] = fabs(dc[l] * gr[l].x + ds[l] * gr[l].y);
    }
    int done = -1;  // lanes <= done are resolved
    for (;;) {
      int al = -1;
      double ag2 = 0;
      for (int l = kLevels - 1; l >= 0; --l)
        if (((b >> l) & 1u) && cand[l] != -2 && pr[l] > weight[l]) {
          al = l;
          ag2 = g2[l];
        }
      const unsigned long long m = __ballot(lane > done && al >= 0);
      if (!m) break;
      const int f = __ffsll(m) - 1;
      const int lf = __shfl(al, f);
      const double wf = __shfl(ag2, f);
      const int idx = __shfl(pidx, f);
      for (int l = 0; l < kLevels; ++l) {
        if (l == lf) {
          weight[l] = wf;
          cand[l] = idx;
        } else if (l > lf) {
          cand[l] = -2;
        }
      }
      done = f;
    }
  };
  const int np = p * p, nchunks = (np + 63) / 64;
  // the possible bits of the top window's 256 level-0 windows, four per lane (eigenWindowBitsKernel)
  const uint16_t *wt = a.wbits + static_cast<size_t>(T) * kWindowsPerTop + 4 * lane;
  const unsigned long long wpack = static_cast<unsigned long long>(wt[0]) | static_cast<unsigned long long>(wt[1]) << 16 |
                                   static_cast<unsigned long long>(wt[2]) << 32 | static_cast<unsigned long long>(wt[3]) << 48;
  int x4, y4;
  a.g.corner(T, x4, y4);
  startWindow(4);
  for (int c3 = 0; c3 < 4; ++c3) {
    if (sub >= 0 && c3 != (sub >> 2)) continue;
    int x3 = x4, y3 = y4;
    child(4, p, c3, x3, y3);
    if (!cornerValid(a.valid, a.W, a.H, x3, y3)) continue;
    setDir(4);
    startWindow(3);
    for (int c2 = 0; c2 < 4; ++c2) {
      if (sub >= 0 && c2 != (sub & 3)) continue;
      int x2 = x3, y2 = y3;
      child(3, p, c2, x2, y2);
      if (!cornerValid(a.valid, a.W, a.H, x2, y2)) continue;
      setDir(3);
      startWindow(2);
      for (int c1 = 0; c1 < 4; ++c1) {
        int x1 = x2, y1 = y2;
        child(2, p, c1, x1, y1);
        if (!cornerValid(a.valid, a.W, a.H, x1, y1)) continue;
        setDir(2);
        startWindow(1);
        for (int c0 = 0; c0 < 4; ++c0) {
          int x0 = x1, y0 = y1;
          child(1, p, c0, x0, y0);
          if (!cornerValid(a.valid, a.W, a.H, x0, y0)) continue;
          setDir(1);
          startWindow(0);
          const int t = c3 * 64 + c2 * 16 + c1 * 4 + c0;
          setDir(0);  // n is constant inside a level-0 window: every visited pixel gets this direction
          const unsigned wb = static_cast<unsigned>(__shfl(wpack, t >> 2) >> (16 * (t & 3))) & 31u;
          // the window's p x p pixels in raster order, 64 per chunk; the loads of kBatch chunks are issued together.  A window none of
          // whose pixels passes a direction-free test (wb == 0) cannot change any record.
          for (int c = 0; wb && c < nchunks; c += kBatch) {
            unsigned b[kBatch];
            int pidx[kBatch];
            double2 gr[kBatch][kLevels];
#pragma unroll
            for (int j = 0; j < kBatch; ++j) {
              const int k = (c + j) * 64 + lane;
              const int px = x0 + k % p, py = y0 + k / p;
              const bool in = c + j < nchunks && k < np && px < a.W && py < a.H;
              b[j] = in ? a.bits[py * a.W + px] : 0u;
              pidx[j] = py * a.W + px;
#pragma unroll
              for (int l = 0; l < kLevels; ++l) gr[j][l] = in ? gradientAt(a.L, l, px, py) : make_double2(0, 0);
            }
            // (written out: the loop around the convergent resolve is not unrolled by the compiler, and gr must stay in registers)
            resolveChunk(b[0] & 31u, gr[0], pidx[0]);
            if (c + 1 < nchunks) resolveChunk(b[1] & 31u, gr[1], pidx[1]);
            if (c + 2 < nchunks) resolveChunk(b[2] & 31u, gr[2], pidx[2]);
            if (c + 3 < nchunks) resolveChunk(b[3] & 31u, gr[3], pidx[3]);
          }
          emit(0);
        }
        emit(1);
      }
      emit(2);
    }
    if (sub < 0) emit(3);
  }
  if (sub < 0) emit(4);
  return n;
}

// one wave: start offsets by a scan over the determined top windows; an undetermined window is walked (and written) once its start
// is known.  result = {found, chained windows}.
__global__ void __launch_bounds__(64) eigenChainKernel(WalkArgs a, const int *__restrict__ count, const int *__restrict__ undet, int *__restrict__ start,
                                                       int *__restrict__ result) {
  const int lane = threadIdx.x;
  int n = 0, chained = 0, base = 0;
  const int nt = a.g.nt;
  while (base < nt) {
    const int k = base + lane;
    const bool in = k < nt;
    const unsigned long long um = __ballot(in && undet[k]);
    const int lim = um ? __ffsll(um) - 1 : 64;  // lanes below lim are determined
    const int e = (in && lane < lim) ? count[k] : 0;
    int incl = e;
    for (int o = 1; o < 64; o <<= 1) {
      const int v = __shfl_up(incl, o);
      if (lane >= o) incl += v;
    }
    if (in && lane < lim) start[k] = n + incl - e;
    n += __shfl(incl, 63);
    if (um) {
      const int tu = base + lim;
      if (lane == 0) start[tu] = n;
      n = walkTop(a, tu, n, true, -1);
      ++chained;
      base = tu + 1;
    } else {
      base += 64;
    }
  }
  if (lane == 0) {
    result[0] = n;
    result[1] = chained;
  }
}

// the exact walk of every determined top window from its start offset: one wave per level-2 window of a split top window (its start
// = the top window's plus the counts of the level-2 windows before it), else one wave for the whole top window
__global__ void __launch_bounds__(kBlock) eigenEmitKernel(WalkArgs a, const int *__restrict__ undet, const int *__restrict__ start,
                                                          const int *__restrict__ count2, const int *__restrict__ split) {
  const int w = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
  const int T = w >> 4, sub = w & 15;
  if (T >= a.g.nt || undet[T]) return;  // (wave-uniform)
  if (split[T]) {
    int n = start[T];
    for (int k = 0; k < sub; ++k) n += count2[T * 16 + k];
    (void)walkTop(a, T, n, true, sub);
  } else if (sub == 0) {
    (void)walkTop(a, T, start[T], true, -1);
  }
}

struct KeepByPattern {
  const uint8_t *pattern;
  int thr;
  __host__ __device__ bool operator()(int idx) const { return static_cast<int>(pattern[idx]) <= thr; }
};

inline unsigned gridFor(long n) { return static_cast<unsigned>(std::max<long>(1, (n + kBlock - 1) / kBlock)); }

/** srand(seed) then (uint8_t)rand() n times: glibc's TYPE_3 additive feedback generator (31 words, separation 3, 310 outputs
 *  discarded by the seeding), written out so that no process-global libc state is touched */
void glibcRandomBytes(unsigned seed, size_t n, uint8_t *out) {
  int32_t r[31];
  r[0] = static_cast<int32_t>(seed == 0 ? 1 : seed);
  for (int i = 1; i < 31; ++i) {
    const long hi = r[i - 1] / 127773, lo = r[i - 1] % 127773;
    long word = 16807 * lo - 2836 * hi;
    if (word < 0) word += 2147483647;
    r[i] = static_cast<int32_t>(word);
  }
  int f = 3, b = 0;
  auto next = [&]() {
    const uint32_t v = static_cast<uint32_t>(r[f]) + static_cast<uint32_t>(r[b]);
    r[f] = static_cast<int32_t>(v);
    f = f == 30 ? 0 : f + 1;
    b = b == 30 ? 0 : b + 1;
    return v >> 1;
  };
  for (int i = 0; i < 310; ++i) (void)next();
  for (size_t i = 0; i < n; ++i) out[i] = static_cast<uint8_t>(next());
}

/** RandomDirections<16> (eigen_tracking_features_extractor.cpp:27-45): the Taylor polynomials evaluated as written, left to right */
void randomDirections(double out[32]) {
  const double pi = 3.14159265358979323846;
  for (int i = 0; i < 16; ++i) {
    const double a = -pi / 2 + (pi / 16) * static_cast<double>(i);
    out[2 * i] = 1 - a * a / (1 * 2) + a * a * a * a / (1 * 2 * 3 * 4) - a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6) +
                 a * a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7 * 8);
    out[2 * i + 1] = a - a * a * a / (1 * 2 * 3) + a * a * a * a * a / (1 * 2 * 3 * 4 * 5) - a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7) +
                     a * a * a * a * a * a * a * a * a / (1 * 2 * 3 * 4 * 5 * 6 * 7 * 8 * 9);
  }
}

/** calculatePotential (:143-149) */
int idealPotential(double ratio, int potential) {
  const int ideal = static_cast<int>(std::sqrt(1.0 / ratio) * (potential + 1) - 1);
  return ideal < 1 ? 1 : ideal;
}

}  // namespace

void eigenExtract(dsopp_hip_feature_extractor *ex, const uint8_t *image_host, const uint8_t *image_dev, int32_t capacity, double *xy, int32_t *n) {
  EigenExtractorState &es = *ex->eigen;
  ex->sr.use();
  hipStream_t st = ex->sr.stream;
  const int W = ex->width, H = ex->height, N = W * H;
  const int rc = image_host ? dsopp_hip_pyramid_build(es.pyramid.get(), image_host, nullptr, nullptr)
                            : dsopp_hip_pyramid_build_device(es.pyramid.get(), image_dev, nullptr, nullptr, 0.0);
  if (rc != DSOPP_HIP_OK) throw Error(rc, lastError());
  const dsopp_hip_pyramid &pyr = *es.pyramid;
  Levels L;
  for (int l = 0; l < kLevels; ++l) {
    L.tex[l] = static_cast<const Texel<double> *>(pyr.texels[l].get());
    L.w[l] = pyr.w(l);
    L.h[l] = pyr.h(l);
  }
  const uint8_t *valid = ex->has_mask ? ex->d_valid.ptr : nullptr;
  const int mw = W >> kMapShift, mh = H >> kMapShift;
  eigenCellKernel<<<mw * mh, kBlock, 0, st>>>(L.tex[0], W, H, valid, mw, W / mw, H / mh, es.d_raw.ptr);
  eigenMapKernel<<<gridFor(mw * mh), kBlock, 0, st>>>(es.d_raw.ptr, mw, mh, es.d_map.ptr);
  eigenPixelKernel<<<gridFor(N), kBlock, 0, st>>>(L, W, H, valid, es.d_map.ptr, mw, mh, es.d_dirs.ptr, es.d_bits.ptr);
  HIP_CHECK(hipGetLastError());

  // everything below is computed into locals and committed at the end: a failed call leaves the state as it was
  int potential = ex->window_size;
  int passes = 0, potentials[2] = {0, 0}, found_pass[2] = {0, 0}, chained = 0, found = 0;
  double ratio = 0;
  for (int pass = 0; pass < 2; ++pass) {
    TopGrid g;
    g.p = potential;
    const long top = 16L * potential;
    g.ntx = static_cast<int>((W + top - 1) / top);
    g.nt = g.ntx * static_cast<int>((H + top - 1) / top);
    const size_t nwin = static_cast<size_t>(g.nt) * kWindowsPerTop;  // also the most emissions a pass can have (one per level-0 window)
    es.d_wbits.reserve(nwin, 0, st);
    ex->d_list.reserve(nwin, 0, st);
    es.d_count.reserve(g.nt, 0, st);
    es.d_undet.reserve(g.nt, 0, st);
    es.d_start.reserve(g.nt, 0, st);
    es.d_split.reserve(g.nt, 0, st);
    es.d_count2.reserve(static_cast<size_t>(g.nt) * 16, 0, st);
    WalkArgs a{L, es.d_bits.ptr, es.d_wbits.ptr, valid, es.d_pattern.ptr, es.d_dirs.ptr, W, H, N, g, ex->d_list.ptr, static_cast<int>(nwin)};
    eigenWindowBitsKernel<<<static_cast<unsigned>((nwin + kBlock / 64 - 1) / (kBlock / 64)), kBlock, 0, st>>>(es.d_bits.ptr, valid, W, H, g, es.d_wbits.ptr);
    eigenCountKernel<<<g.nt, kWindowsPerTop, 0, st>>>(es.d_wbits.ptr, es.d_count.ptr, es.d_undet.ptr, es.d_count2.ptr, es.d_split.ptr);
    eigenChainKernel<<<1, 64, 0, st>>>(a, es.d_count.ptr, es.d_undet.ptr, es.d_start.ptr, es.d_result.ptr);
    eigenEmitKernel<<<static_cast<unsigned>(g.nt) * 16 / (kBlock / 64), kBlock, 0, st>>>(a, es.d_undet.ptr, es.d_start.ptr, es.d_count2.ptr,
                                                                                          es.d_split.ptr);
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipMemcpyAsync(es.h_result.get(), es.d_result.ptr, 2 * sizeof(int), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    found = es.h_result.get()[0];
    chained += es.h_result.get()[1];
    if (found < 0 || static_cast<size_t>(found) > nwin) fail(DSOPP_HIP_ERR_HIP, "eigen extractor: %d emissions exceed the %zu level-0 windows", found, nwin);
    potentials[pass] = potential;
    found_pass[pass] = found;
    passes = pass + 1;
    // fillFeatureCoordinates (:352-389): at most one re-sampling
    ratio = found > 0 ? ex->density / static_cast<double>(found) : HUGE_VAL;
    const int ideal = idealPotential(ratio, potential);
    if (pass == 0 && ratio > 1.25 && potential > 1) {
      potential = std::min(ideal, potential - 1);
    } else if (pass == 0 && ratio < 0.25) {
      potential = std::max(ideal, potential + 1);
    } else {
      break;
    }
  }

  // reduceTheNumberOfPoints: a stable select of the features whose pattern byte is <= (int)(255 ratio), into the scratch list (d_final
  // is replaced only once the capacity check has passed)
  int kept = found;
  const int *kept_list = ex->d_list.ptr;
  if (found > 0 && ratio < 0.95) {
    ex->d_hit.reserve(static_cast<size_t>(found), 0, st);
    const KeepByPattern keep{es.d_pattern.ptr, static_cast<int>(255. * ratio)};
    size_t temp_bytes = 0;
    HIP_CHECK(hipcub::DeviceSelect::If(nullptr, temp_bytes, ex->d_list.ptr, ex->d_hit.ptr, ex->d_count.ptr, found, keep, st));
    ex->d_temp.reserve(std::max<size_t>(1, temp_bytes), 0, st);
    HIP_CHECK(hipcub::DeviceSelect::If(ex->d_temp.ptr, temp_bytes, ex->d_list.ptr, ex->d_hit.ptr, ex->d_count.ptr, found, keep, st));
    HIP_CHECK(hipMemcpyAsync(ex->h_count.get(), ex->d_count.ptr, sizeof(int), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    kept = *ex->h_count.get();
    kept_list = ex->d_hit.ptr;
  }
  *n = kept;
  if (kept > capacity) fail(DSOPP_HIP_ERR_CAPACITY, "capacity %d < %d features", capacity, kept);

  std::vector<int> final_list(static_cast<size_t>(kept));
  if (kept > 0) {
    ex->d_final.reserve(static_cast<size_t>(kept), 0, st);
    HIP_CHECK(hipMemcpyAsync(ex->d_final.ptr, kept_list, static_cast<size_t>(kept) * sizeof(int), hipMemcpyDeviceToDevice, st));
    ex->h_list.reserve(static_cast<size_t>(kept) * sizeof(int));
    HIP_CHECK(hipMemcpyAsync(ex->h_list.get(), kept_list, static_cast<size_t>(kept) * sizeof(int), hipMemcpyDeviceToHost, st));
    ex->sr.sync();
    const int *list = ex->h_list.get();
    for (int i = 0; i < kept; ++i) {
      final_list[static_cast<size_t>(i)] = list[i];
      xy[2 * i] = static_cast<double>(list[i] % W);
      xy[2 * i + 1] = static_cast<double>(list[i] / W);
    }
  }
  HIP_CHECK(hipEventRecord(ex->final_ready.h, st));

  ex->initialized = true;
  ex->window_size = potential;
  ex->found_last = found;
  ex->final_list = std::move(final_list);
  es.passes = passes;
  es.potentials[0] = potentials[0];
  es.potentials[1] = potentials[1];
  es.found[0] = found_pass[0];
  es.found[1] = found_pass[1];
  es.chained = chained;
}

}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_eigen_random_pattern(int width, int height, uint8_t *out) {
  return guarded([&] {
    if (!out || width <= 0 || height <= 0 || static_cast<long long>(width) * height > INT_MAX)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "bad pattern size %d x %d", width, height);
    glibcRandomBytes(kRandomSeed, static_cast<size_t>(width) * height, out);
  });
}

int dsopp_hip_feature_extractor_create_eigen(int device, void *stream, int width, int height, double point_density_for_detector,
                                             dsopp_hip_feature_extractor **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    if (width < 32 || height < 32 || static_cast<long long>(width) * height > INT_MAX / 2)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image size %d x %d out of range (the threshold map needs 32 x 32)", width, height);
    if (!(point_density_for_detector > 0)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "point_density_for_detector must be > 0");
    auto ex = std::make_unique<dsopp_hip_feature_extractor>();
    ex->sr.init(device, stream);
    ex->kind = ExtractorKind::Eigen;
    ex->width = width;
    ex->height = height;
    ex->density = point_density_for_detector;
    ex->window_size = kInitialPotential;
    ex->eigen = std::make_unique<EigenExtractorState>();
    EigenExtractorState &es = *ex->eigen;
    hipStream_t st = ex->sr.stream;
    dsopp_hip_pyramid *pyr = nullptr;
    const int rc = dsopp_hip_pyramid_create(device, st, width, height, kLevels, DSOPP_HIP_F64, &pyr);
    if (rc != DSOPP_HIP_OK) throw Error(rc, lastError());
    es.pyramid.reset(pyr);
    const size_t n = static_cast<size_t>(width) * height;
    std::vector<uint8_t> pattern(n);
    glibcRandomBytes(kRandomSeed, n, pattern.data());
    double dirs[32];
    randomDirections(dirs);
    es.d_pattern.reserve(n, 0, st);
    es.d_pattern.upload(pattern.data(), n, 0, st);
    es.d_dirs.reserve(32, 0, st);
    es.d_dirs.upload(dirs, 32, 0, st);
    const size_t cells = static_cast<size_t>(width >> kMapShift) * (height >> kMapShift);
    es.d_raw.reserve(cells, 0, st);
    es.d_map.reserve(cells, 0, st);
    es.d_bits.reserve(n, 0, st);
    es.d_result.reserve(2, 0, st);
    es.h_result.reserve(2 * sizeof(int));
    ex->d_count.reserve(1, 0, st);
    ex->h_count.reserve(sizeof(int));
    (void)ex->final_ready.get(hipEventDisableTiming);
    ex->sr.sync();
    *out = ex.release();
  });
}

int dsopp_hip_feature_extractor_get_eigen_stats(const dsopp_hip_feature_extractor *ex, int32_t *passes, int32_t potentials[2], int32_t found[2],
                                                int32_t *chained_windows) {
  return guarded([&] {
    if (!ex) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null extractor");
    if (ex->kind != ExtractorKind::Eigen) fail(DSOPP_HIP_ERR_STATE, "not an eigen extractor");
    const EigenExtractorState &es = *ex->eigen;
    if (passes) *passes = es.passes;
    for (int k = 0; k < 2; ++k) {
      if (potentials) potentials[k] = es.potentials[k];
      if (found) found[k] = es.found[k];
    }
    if (chained_windows) *chained_windows = es.chained;
  });
}

}  // extern "C"
