// The pure-rotation RANSAC of the bootstrap's standstill test on the device, and the dsopp_hip_rotation_ransac_* entry points.
//   estimateSO3inlierCount<3>            src/feature_based_slam/tracker/src/estimate_so3_inlier_count.cpp:17-48
//   ransac::ransac                       src/ransac/include/ransac/ransac.hpp:27-56
//   PureRorationSolver::solve, findBest  src/energy/n_point_solvers/src/pure_rotation_estimator.cpp:14-67
//
// The arithmetic is the one include/dsopp_hip.h states (tests/rotation_ransac_model.py is its NumPy form), all of it binary64.  The
// reference's loop is serial only through its stopping rule: every hypothesis is a function of its own sample triple (and, when that
// triple is invalid, of the triples before it), so all of them are scored at once and the loop's meaning is applied to the counts after.
//
// One launch.  A wave owns one hypothesis, four waves a workgroup.  Every lane of the wave computes the 3 x 3 decomposition redundantly
// (it is a few hundred scalar-like operations; no lane waits for another), then the lanes stride over the points and the wave counts by
// ballot and population count.  The points are read straight through the vector cache: the waves of a workgroup walk the same 32 n bytes
// side by side.  A wave whose triple is invalid looks for its nearest valid predecessor itself (the triples' validity is six comparisons
// each) and solves and scores that one, or the identity: no wave reads what another wave wrote.
//   The workgroup that takes the last ticket of a counter closes the call (lastWorkgroup, ransac_device.hpp): the selection walk over the
// counts (a prefix maximum over the wave), then the winner's inlier list in ascending order (ballots again).
//
// The polar factor: a one-sided (Hestenes) Jacobi SVD of H — rotations of column pairs of G = H V until the columns are orthogonal to
// rounding, G = U S — which is backward stable and needs no inverse, so a singular H is no special case up to here.  U is then rebuilt as
// an orthonormal frame: u0 from the longest column, u1 from the second, re-orthogonalised, u2 = +-(u0 x u1) with the sign of the shortest
// column.  For a well-conditioned H that changes U by rounding; for a vanishing smallest singular value it still yields a rotation.
#include "ransac_device.hpp"
#include "staged_call.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {
using namespace ransac;

constexpr int kMaxSweeps = 30;  // a 3 x 3 one-sided Jacobi converges in 4 .. 7 sweeps; the cap only bounds the loop for NaN input

struct RansacParams : PinholeRoi {
  double threshold, tolerance;
  int n, iterations;
};

/** all six points of triple i inside the ROI */
__device__ __forceinline__ bool sampleValid(const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ samples, int i,
                                            const RansacParams &p) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int s = samples[3 * static_cast<size_t>(i) + k];
    ok = ok && insideRoi(A[2 * static_cast<size_t>(s)], A[2 * static_cast<size_t>(s) + 1], p) &&
         insideRoi(B[2 * static_cast<size_t>(s)], B[2 * static_cast<size_t>(s) + 1], p);
  }
  return ok;
}

__device__ __forceinline__ void swapColumns(double *ga, double *gb, double *va, double *vb, double &na, double &nb) {
  if (na < nb) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const double tg = ga[r], tv = va[r];
      ga[r] = gb[r];
      gb[r] = tg;
      va[r] = vb[r];
      vb[r] = tv;
    }
    const double t = na;
    na = nb;
    nb = t;
  }
}

/** R = det(Q) Q with Q = V U^T of H = U S V^T (H row-major) */
__device__ void rotationOf(const double *H, double *R) {
  double g[3][3], v[3][3];  // columns: g[c][r] = (H V)(r, c)
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      g[c][r] = H[3 * r + c];
      v[c][r] = r == c ? 1.0 : 0.0;
    }
  for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pair = 0; pair < 3; ++pair) {
      const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2;
      const double alpha = dot3(g[p], g[p]), beta = dot3(g[q], g[q]), gamma = dot3(g[p], g[q]);
      if (fabs(gamma) > DBL_EPSILON * sqrt(alpha * beta)) {
        rotated = true;
        const double zeta = (beta - alpha) / (2.0 * gamma);
        const double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
        const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const double gp = g[p][r], gq = g[q][r], vp = v[p][r], vq = v[q][r];
          g[p][r] = c * gp - s * gq;
          g[q][r] = s * gp + c * gq;
          v[p][r] = c * vp - s * vq;
          v[q][r] = s * vp + c * vq;
        }
      }
    }
    if (!rotated) break;
  }
  double norm[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) norm[c] = sqrt(dot3(g[c], g[c]));
  swapColumns(g[0], g[1], v[0], v[1], norm[0], norm[1]);  // the longest column first, the shortest last (Q does not depend on the order)
  swapColumns(g[1], g[2], v[1], v[2], norm[1], norm[2]);
  swapColumns(g[0], g[1], v[0], v[1], norm[0], norm[1]);
  double u[3][3];
#pragma unroll
  for (int r = 0; r < 3; ++r) u[0][r] = g[0][r] / norm[0];
  double w[3];
  const double along = dot3(g[1], u[0]);
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] = g[1][r] - along * u[0][r];
  double nw = sqrt(dot3(w, w));
  if (!(nw > 1e-14 * norm[0])) {
    // rank one to rounding: any unit vector across u0, from the axis u0 leans on least
    const double a0 = fabs(u[0][0]), a1 = fabs(u[0][1]), a2 = fabs(u[0][2]);
    const int axis = a0 <= a1 && a0 <= a2 ? 0 : (a1 <= a2 ? 1 : 2);
#pragma unroll
    for (int r = 0; r < 3; ++r) w[r] = (r == axis ? 1.0 : 0.0) - u[0][axis] * u[0][r];
    nw = sqrt(dot3(w, w));
  }
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] /= nw;
  const double again = dot3(w, u[0]);
#pragma unroll
  for (int r = 0; r < 3; ++r) w[r] -= again * u[0][r];
  nw = sqrt(dot3(w, w));
#pragma unroll
  for (int r = 0; r < 3; ++r) u[1][r] = w[r] / nw;
  u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
  u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
  u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
  if (dot3(g[2], u[2]) < 0.0) {
#pragma unroll
    for (int r = 0; r < 3; ++r) u[2][r] = -u[2][r];
  }
  double Q[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[3 * r + c] = v[0][r] * u[0][c] + v[1][r] * u[1][c] + v[2][r] * u[2][c];
  const double det = Q[0] * (Q[4] * Q[8] - Q[5] * Q[7]) - Q[1] * (Q[3] * Q[8] - Q[5] * Q[6]) + Q[2] * (Q[3] * Q[7] - Q[4] * Q[6]);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = det * Q[k];
}

/** PureRorationSolver::solve of triple i, which is valid */
__device__ void solveSample(const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ samples, int i, const RansacParams &p,
                            double *R) {
  double H[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const size_t s = static_cast<size_t>(samples[3 * static_cast<size_t>(i) + k]);
    double a[3] = {(A[2 * s] - p.cx) / p.fx, (A[2 * s + 1] - p.cy) / p.fy, 1.0};
    double b[3] = {(B[2 * s] - p.cx) / p.fx, (B[2 * s + 1] - p.cy) / p.fy, 1.0};
    const double na = sqrt(dot3(a, a)), nb = sqrt(dot3(b, b));
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      a[r] /= na;
      b[r] /= nb;
    }
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) H[3 * r + c] += a[r] * b[c];
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) H[k] /= 9.0;
  rotationOf(H, R);
}

/** findBest's test of one pair */
__device__ __forceinline__ bool isInlier(const double *R, double ax, double ay, double bx, double by, const RansacParams &p) {
  if (!insideRoi(ax, ay, p)) return false;
  const double ux = (ax - p.cx) / p.fx, uy = (ay - p.cy) / p.fy;
  const double x = R[0] * ux + R[1] * uy + R[2], y = R[3] * ux + R[4] * uy + R[5], z = R[6] * ux + R[7] * uy + R[8];
  const double dx = p.fx * x / z + p.cx - bx, dy = p.fy * y / z + p.cy - by;
  return sqrt(dx * dx + dy * dy) < p.threshold;  // (false for a NaN)
}

__global__ void __launch_bounds__(kBlock) rotationRansacKernel(const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ samples,
                                                               unsigned *ticket, int *hyp_counts, double *hyp_rotations, uint8_t *hyp_valid,
                                                               dsopp_hip_rotation_ransac_result *result, int *__restrict__ inliers,
                                                               const RansacParams p) {
  __shared__ unsigned s_last;
  __shared__ int s_run, s_best_iteration;
  __shared__ int s_wave_count[kWavesPerBlock];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hyp = static_cast<int>(blockIdx.x) * kWavesPerBlock + wave;
  if (hyp < p.iterations) {
    const bool valid = sampleValid(A, B, samples, hyp, p);
    int source = valid ? hyp : -1;
    if (!valid) {
      // the nearest valid predecessor: 64 triples per step, the lowest lane holds the nearest
      for (int base = hyp - 1; base >= 0 && source < 0; base -= 64) {
        const int j = base - lane;
        const bool ok = j >= 0 && sampleValid(A, B, samples, j, p);
        const unsigned long long mask = __ballot(ok);
        if (mask) source = base - __builtin_ctzll(mask);
      }
    }
    double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    if (source >= 0) solveSample(A, B, samples, source, p, R);
    int count = 0;
    for (int base = 0; base < p.n; base += 64) {
      const int j = base + lane;
      bool in = false;
      if (j < p.n) in = isInlier(R, A[2 * static_cast<size_t>(j)], A[2 * static_cast<size_t>(j) + 1], B[2 * static_cast<size_t>(j)], B[2 * static_cast<size_t>(j) + 1], p);
      count += __builtin_popcountll(__ballot(in));
    }
    if (lane == 0) {
      hyp_counts[hyp] = count;
      hyp_valid[hyp] = valid ? 1 : 0;
#pragma unroll
      for (int k = 0; k < 9; ++k) hyp_rotations[9 * static_cast<size_t>(hyp) + k] = R[k];
    }
  }
  if (!lastWorkgroup(ticket, s_last)) return;

  // the selection walk, by wave 0: before[i] = the greatest count ahead of i; the walk stops before the first i with before[i] / n >= tolerance
  if (wave == 0) {
    int carry = 0, run = p.iterations;
    for (int base = 0; base < p.iterations; base += 64) {
      const int i = base + lane;
      int v = i < p.iterations ? freshLoad(hyp_counts + i) : 0;
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        const int t = __shfl_up(v, o, 64);
        if (lane >= o) v = v > t ? v : t;
      }
      const int shifted = __shfl_up(v, 1, 64);
      const int before = lane == 0 ? carry : (shifted > carry ? shifted : carry);
      const bool stop = i < p.iterations && static_cast<double>(before) / static_cast<double>(p.n) >= p.tolerance;
      const unsigned long long mask = __ballot(stop);
      if (mask) {
        const int first = __builtin_ctzll(mask);
        run = base + first;
        carry = __shfl(before, first, 64);
        break;
      }
      const int last = __shfl(v, 63, 64);
      carry = last > carry ? last : carry;
    }
    // the winner is the first hypothesis of the walk that reached the final best (a later equal count is not strictly greater)
    int best_iteration = -1;
    if (carry > 0) {
      for (int base = 0; base < run && best_iteration < 0; base += 64) {
        const int i = base + lane;
        const bool hit = i < run && freshLoad(hyp_counts + i) == carry;
        const unsigned long long mask = __ballot(hit);
        if (mask) best_iteration = base + __builtin_ctzll(mask);
      }
    }
    if (lane == 0) {
      s_run = run;
      s_best_iteration = best_iteration;
    }
  }
  __syncthreads();
  const int best_iteration = s_best_iteration;
  double R[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  int total = 0;
  if (best_iteration >= 0) {
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = freshLoad(hyp_rotations + 9 * static_cast<size_t>(best_iteration) + k);
    const auto inlier = [&](int j) {
      return isInlier(R, A[2 * static_cast<size_t>(j)], A[2 * static_cast<size_t>(j) + 1], B[2 * static_cast<size_t>(j)], B[2 * static_cast<size_t>(j) + 1], p);
    };
    total = listInliers(p.n, inlier, s_wave_count, tid, inliers);
  }
  if (tid == 0) {
    result->iterations_run = s_run;
    result->best_iteration = best_iteration;
    result->inlier_count = total;
    result->matches = p.n;
#pragma unroll
    for (int k = 0; k < 9; ++k) result->rotation[k] = R[k];
  }
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_rotation_ransac : dsopp_hip::StagedCall {};

namespace dsopp_hip {
namespace {

/** in:  ticket (16 bytes) | A | B | samples;   out: result (96 bytes) | hyp_rotations | inliers | hyp_counts | hyp_valid */
struct RansacLayout {
  size_t a, b, samples, in_bytes;
  size_t rotations, inliers, counts, valid, out_bytes;
  RansacLayout(size_t n, size_t iterations) {
    a = 16;
    b = a + 16 * n;
    samples = b + 16 * n;
    in_bytes = samples + 12 * iterations;
    static_assert(sizeof(dsopp_hip_rotation_ransac_result) <= 96, "the result's slot");
    rotations = 96;
    inliers = rotations + 72 * iterations;
    counts = inliers + 4 * n;
    valid = counts + 4 * iterations;
    out_bytes = valid + iterations;
  }
};

void estimate(dsopp_hip_rotation_ransac *h, double fx, double fy, double cx, double cy, int width, int height, int n, const double *points_a,
              const double *points_b, int iterations, const int32_t *samples, double threshold, double inliers_tolerance,
              dsopp_hip_rotation_ransac_result *result, int32_t *inlier_indices, int32_t *hyp_counts, double *hyp_rotations, uint8_t *hyp_valid) {
  if (!h) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null rotation ransac");
  if (!result) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 0 || n > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d points", n);
  if (iterations < 0 || iterations > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d iterations", iterations);
  if (!(threshold == threshold) || !(inliers_tolerance == inliers_tolerance)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a threshold is not a number");
  if (n > 0 && (!points_a || !points_b || !inlier_indices)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  result->iterations_run = 0;
  result->best_iteration = -1;
  result->inlier_count = 0;
  result->matches = n;
  for (int k = 0; k < 9; ++k) result->rotation[k] = k % 4 == 0 ? 1.0 : 0.0;
  // n = 0: 0 / 0 < tolerance is false and the reference's loop runs no iteration, whatever the triples are
  if (n == 0 || iterations == 0) return;
  if (n < 3) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d points: a triple of distinct indices needs 3", n);
  checkSamples<3, true>(samples, iterations, n, "points");
  h->sr.use();
  const hipStream_t st = h->sr.stream;
  const size_t count = static_cast<size_t>(n), hyps = static_cast<size_t>(iterations);
  const RansacLayout lay(count, hyps);
  h->ensure(lay.in_bytes, lay.out_bytes);
  uint8_t *hi = h->h_in.get(), *di = h->d_in.get(), *ho = h->h_out.get(), *dout = h->d_out.get();
  std::memset(hi, 0, 16);  // (the ticket is armed by the upload)
  std::memcpy(hi + lay.a, points_a, 16 * count);
  std::memcpy(hi + lay.b, points_b, 16 * count);
  std::memcpy(hi + lay.samples, samples, 12 * hyps);
  HIP_CHECK(hipMemcpyAsync(di, hi, lay.in_bytes, hipMemcpyHostToDevice, st));
  RansacParams p;
  p.fx = fx;
  p.fy = fy;
  p.cx = cx;
  p.cy = cy;
  p.xmax = static_cast<double>(width) - 5.0;
  p.ymax = static_cast<double>(height) - 5.0;
  p.threshold = threshold;
  p.tolerance = inliers_tolerance;
  p.n = n;
  p.iterations = iterations;
  const unsigned blocks = (static_cast<unsigned>(iterations) + kWavesPerBlock - 1) / kWavesPerBlock;
  rotationRansacKernel<<<blocks, kBlock, 0, st>>>(reinterpret_cast<const double *>(di + lay.a), reinterpret_cast<const double *>(di + lay.b),
                                                  reinterpret_cast<const int *>(di + lay.samples), reinterpret_cast<unsigned *>(di),
                                                  reinterpret_cast<int *>(dout + lay.counts), reinterpret_cast<double *>(dout + lay.rotations),
                                                  dout + lay.valid, reinterpret_cast<dsopp_hip_rotation_ransac_result *>(dout),
                                                  reinterpret_cast<int *>(dout + lay.inliers), p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(ho, dout, lay.out_bytes, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipEventRecord(h->done.get(hipEventDisableTiming), st));
  HIP_CHECK(hipEventSynchronize(h->done.h));  // the one wait of the call
  std::memcpy(result, ho, sizeof(*result));
  if (result->inlier_count < 0 || result->inlier_count > n) fail(DSOPP_HIP_ERR_HIP, "the device returned %d inliers of %d points", result->inlier_count, n);
  std::memcpy(inlier_indices, ho + lay.inliers, 4 * static_cast<size_t>(result->inlier_count));
  if (hyp_counts) std::memcpy(hyp_counts, ho + lay.counts, 4 * hyps);
  if (hyp_rotations) std::memcpy(hyp_rotations, ho + lay.rotations, 72 * hyps);
  if (hyp_valid) std::memcpy(hyp_valid, ho + lay.valid, hyps);
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_rotation_ransac_create(int device, void *stream, dsopp_hip_rotation_ransac **out) { return createHandle(device, stream, out); }

void dsopp_hip_rotation_ransac_destroy(dsopp_hip_rotation_ransac *r) { destroyHandle(r); }

int dsopp_hip_rotation_ransac_estimate(dsopp_hip_rotation_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                       const double *points_a, const double *points_b, int iterations, const int32_t *samples, double threshold,
                                       double inliers_tolerance, dsopp_hip_rotation_ransac_result *result, int32_t *inlier_indices,
                                       int32_t *hyp_counts, double *hyp_rotations, uint8_t *hyp_valid) {
  return guarded([&] {
    estimate(r, fx, fy, cx, cy, width, height, n, points_a, points_b, iterations, samples, threshold, inliers_tolerance, result, inlier_indices,
             hyp_counts, hyp_rotations, hyp_valid);
  });
}

}  // extern "C"
