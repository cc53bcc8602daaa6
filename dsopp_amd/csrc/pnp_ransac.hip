// The PnP RANSAC of a bootstrap frame on the device, and the dsopp_hip_pnp_ransac_* entry points.
//   estimateSE3PnP                       src/feature_based_slam/tracker/src/estimate_se3_pnp.cpp:23-77
//   its callers                          src/feature_based_slam/tracker/src/monocular_tracker.cpp:54-56, initialize_poses.cpp:47-73
// The reference hands the matches to OpenGV (EPnP inside its RANSAC, then optimizeModelCoefficients and selectWithinDistance); OpenGV is
// not part of the reference tree, so the solver here is the library's own: a three-point pose by Grunert's elimination per hypothesis,
// and an LM refinement of the winner over its inliers.  What is mirrored is everything around the solver (include/dsopp_hip.h).
//
// The arithmetic is the one include/dsopp_hip.h states (tests/pnp_ransac_model.py is its NumPy form), all of it binary64.
//
// One launch.  A wave owns one hypothesis, four waves a workgroup.  Every lane of the wave solves the three-point problem redundantly
// (no lane waits for another), then the lanes stride over the points with up to four poses in registers and the wave counts by ballot
// and population count.  The solutions live in statically indexed slots throughout, so nothing of them goes to scratch.
//   The workgroup that takes the last ticket of a counter closes the call (lastWorkgroup, ransac_device.hpp): the selection (wave 0),
// then with all four waves the LM refinement over the winner's inliers — thread-strided partial sums, a butterfly over the wave, the
// four waves' sums added in wave order, so the same input gives the same bits — and the final inlier list in ascending order.
//
// The quartic's real roots: no closed form.  The positive roots of a polynomial lie one in each interval between its positive critical
// points where its sign changes, so the second derivative's roots (a quadratic, closed form) bracket the derivative's, and those bracket
// the quartic's; within a bracket a safeguarded Newton iteration (bracketedRoot, ransac_device.hpp) runs to its fixed point.  Whether a
// pair of roots exists is then decided by the polynomial's sign at a critical point, which an error of the critical point moves in
// second order only.
#include "ransac_device.hpp"
#include "se3_math.hpp"
#include "staged_call.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {
using namespace ransac;

constexpr double kMinDepth = 0.001;

struct PnpParams : PinholeRoi {
  double t_ang;
  double lambda_0, function_tolerance, parameter_tolerance, decrease_factor, increase_factor;
  int n, iterations, max_iterations;
};

// ---- polynomials of degree <= 4, c[0] + c[1] x + ... + c[4] x^4

__device__ __forceinline__ double evalPoly(const double (&c)[5], double x) { return (((c[4] * x + c[3]) * x + c[2]) * x + c[1]) * x + c[0]; }
__device__ __forceinline__ double evalDerivative(const double (&c)[5], double x) {
  return ((4.0 * c[4] * x + 3.0 * c[3]) * x + 2.0 * c[2]) * x + c[1];
}

/** the positive roots of c, one slot per interval between its positive critical points `crit` (ascending, NaN = none): a NaN slot holds
 *  no root; the filled slots ascend */
template <int K>
__device__ __forceinline__ void positiveRoots(const double (&c)[5], const double (&crit)[K], double (&root)[K + 1]) {
  const double top = c[4] != 0.0 ? c[4] : (c[3] != 0.0 ? c[3] : (c[2] != 0.0 ? c[2] : c[1]));  // the leading coefficient
  const double big = fmax(fmax(fmax(fabs(c[0]), fabs(c[1])), fmax(fabs(c[2]), fabs(c[3]))), fabs(c[4]));
  const double bound = 1.0 + big / fabs(top);  // Cauchy's: no root lies beyond
  const auto eval = [&](double x) { return evalPoly(c, x); };
  const auto derivative = [&](double x) { return evalDerivative(c, x); };
  double lo = 0.0, flo = c[0];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    root[k] = NAN;
    const double hi = crit[k];
    if (hi > lo && hi < bound) {
      const double fhi = evalPoly(c, hi);
      if (fhi == 0.0) {
        root[k] = hi;
      } else if (flo != 0.0 && (flo > 0.0) != (fhi > 0.0)) {
        root[k] = bracketedRoot<true>(eval, derivative, lo, hi, flo);
      }
      lo = hi;
      flo = fhi;
    }
  }
  root[K] = NAN;
  if (top != 0.0 && bound < DBL_MAX && flo != 0.0 && (flo > 0.0) != (top > 0.0)) root[K] = bracketedRoot<true>(eval, derivative, lo, bound, flo);
}

/** the positive real roots of the quartic c, ascending in the filled slots */
__device__ void quarticPositiveRoots(const double (&c)[5], double (&root)[4]) {
  const double d1[5] = {c[1], 2.0 * c[2], 3.0 * c[3], 4.0 * c[4], 0.0};
  const double d2[5] = {2.0 * c[2], 6.0 * c[3], 12.0 * c[4], 0.0, 0.0};
  // the second derivative's roots in closed form
  double crit2[2] = {NAN, NAN};
  const double qa = d2[2], qb = d2[1], qc = d2[0];
  if (qa == 0.0) {
    if (qb != 0.0) crit2[0] = -qc / qb;
  } else {
    const double disc = qb * qb - 4.0 * qa * qc;
    if (disc >= 0.0) {
      const double q = -0.5 * (qb + copysign(sqrt(disc), qb));
      const double r0 = q / qa, r1 = q != 0.0 ? qc / q : 0.0;
      crit2[0] = fmin(r0, r1);
      crit2[1] = fmax(r0, r1);
    }
  }
  double crit3[3];
  positiveRoots<2>(d1, crit2, crit3);
  positiveRoots<3>(c, crit3, root);
}

// ---- the three-point pose

/** E = [e1 e2 e3] of the triangle P0 P1 P2, as e[k][r] */
__device__ __forceinline__ void triangleFrame(const double *P0, const double *P1, const double *P2, double (&e)[3][3]) {
  double d[3], g[3], c[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    d[r] = P1[r] - P0[r];
    g[r] = P2[r] - P0[r];
  }
  const double nd = sqrt(dot3(d, d));
#pragma unroll
  for (int r = 0; r < 3; ++r) e[0][r] = d[r] / nd;
  cross3(e[0], g, c);
  const double nc = sqrt(dot3(c, c));
#pragma unroll
  for (int r = 0; r < 3; ++r) e[2][r] = c[r] / nc;
  cross3(e[2], e[0], e[1]);
}

/** the solutions of one triple, ascending in v, into the first slots of `pose` (12 doubles each: R row-major, t); returns their number */
__device__ __forceinline__ int solveP3P(const double (&X)[3][3], const double (&f)[3][3], double (&pose)[4][12]) {
  double d12[3], d13[3], d23[3], cr[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    d12[r] = X[1][r] - X[0][r];
    d13[r] = X[2][r] - X[0][r];
    d23[r] = X[1][r] - X[2][r];
  }
  const double a2 = dot3(d23, d23), b2 = dot3(d13, d13), c2 = dot3(d12, d12);
  cross3(d12, d13, cr);
  if (b2 == 0.0 || !(dot3(cr, cr) > 1e-12 * c2 * b2)) return 0;
  const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
  const double K = (a2 - c2) / b2, m = c2 / b2;
  const double n2 = K - 1.0, n1 = -2.0 * K * cb, n0 = 1.0 + K;
  const double d1 = -2.0 * ca, d0 = 2.0 * cg;
  const double q1 = -2.0 * cb;
  double c[5];
  c[4] = n2 * n2 - m * d1 * d1;
  c[3] = 2.0 * n2 * n1 - 2.0 * cg * n2 * d1 - m * (2.0 * d0 * d1 + q1 * d1 * d1);
  c[2] = d1 * d1 + n1 * n1 + 2.0 * n2 * n0 - 2.0 * cg * (n2 * d0 + n1 * d1) - m * (d0 * d0 + 2.0 * q1 * d0 * d1 + d1 * d1);
  c[1] = 2.0 * d0 * d1 + 2.0 * n1 * n0 - 2.0 * cg * (n1 * d0 + n0 * d1) - m * (q1 * d0 * d0 + 2.0 * d0 * d1);
  c[0] = d0 * d0 + n0 * n0 - 2.0 * cg * n0 * d0 - m * d0 * d0;
  bool finite = true;
#pragma unroll
  for (int k = 0; k < 5; ++k) finite = finite && fabs(c[k]) <= DBL_MAX;
  if (!finite) return 0;
  double root[4];
  quarticPositiveRoots(c, root);
  double ew[3][3];
  triangleFrame(X[0], X[1], X[2], ew);
  int count = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const double v = root[k];
    const double u = ((n2 * v + n1) * v + n0) / (d1 * v + d0);
    const double Q = (v + q1) * v + 1.0;
    if (v > 0.0 && u > 0.0 && Q > 0.0) {
      const double s1 = sqrt(b2 / Q), s2 = u * s1, s3 = v * s1;
      double Y[3][3], ec[3][3], T[12];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        Y[0][r] = s1 * f[0][r];
        Y[1][r] = s2 * f[1][r];
        Y[2][r] = s3 * f[2][r];
      }
      triangleFrame(Y[0], Y[1], Y[2], ec);
      bool ok = true;
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) T[3 * r + cc] = ec[0][r] * ew[0][cc] + ec[1][r] * ew[1][cc] + ec[2][r] * ew[2][cc];
#pragma unroll
      for (int r = 0; r < 3; ++r) T[9 + r] = Y[0][r] - (T[3 * r] * X[0][0] + T[3 * r + 1] * X[0][1] + T[3 * r + 2] * X[0][2]);
#pragma unroll
      for (int e = 0; e < 12; ++e) ok = ok && fabs(T[e]) <= DBL_MAX;
      // (selects, not a store behind an index: the slots stay in registers)
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        const bool here = ok && s == count;
#pragma unroll
        for (int e = 0; e < 12; ++e) pose[s][e] = here ? T[e] : pose[s][e];
      }
      if (ok) ++count;
    }
  }
  return count;
}

/** d = 1 - f . p / |p|, p = R X + t */
__device__ __forceinline__ double angularDistance(const double *T, const double *X, const double *f) {
  const double px = T[0] * X[0] + T[1] * X[1] + T[2] * X[2] + T[9];
  const double py = T[3] * X[0] + T[4] * X[1] + T[5] * X[2] + T[10];
  const double pz = T[6] * X[0] + T[7] * X[1] + T[8] * X[2] + T[11];
  const double norm = sqrt(px * px + py * py + pz * pz);
  return 1.0 - (f[0] * px + f[1] * py + f[2] * pz) / norm;
}

/** the inlier test of point j against pose T (strict; false for a NaN and for an observation outside the ROI) */
__device__ __forceinline__ bool isInlier(const double *T, const double *__restrict__ X, const double *__restrict__ obs, int j, const PnpParams &p) {
  const double x = obs[2 * static_cast<size_t>(j)], y = obs[2 * static_cast<size_t>(j) + 1];
  if (!insideRoi(x, y, p)) return false;
  double f[3];
  bearing(x, y, p, f);
  const double Xj[3] = {X[3 * static_cast<size_t>(j)], X[3 * static_cast<size_t>(j) + 1], X[3 * static_cast<size_t>(j) + 2]};
  return angularDistance(T, Xj, f) < p.t_ang;
}

// ---- the refinement: what refinePose (ransac_device.hpp) minimises

/** the pixel residual of point j at pose T: false when the point does not count (p_z < 0.001) */
__device__ __forceinline__ bool pixelResidual(const double *T, const double *__restrict__ X, const double *__restrict__ obs, int j, const PnpParams &p,
                                              double *Xj, double *pc, double *r) {
#pragma unroll
  for (int k = 0; k < 3; ++k) Xj[k] = X[3 * static_cast<size_t>(j) + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) pc[k] = T[3 * k] * Xj[0] + T[3 * k + 1] * Xj[1] + T[3 * k + 2] * Xj[2] + T[9 + k];
  if (!(pc[2] >= kMinDepth)) return false;
  r[0] = obs[2 * static_cast<size_t>(j)] - (p.fx * pc[0] / pc[2] + p.cx);
  r[1] = obs[2 * static_cast<size_t>(j) + 1] - (p.fy * pc[1] / pc[2] + p.cy);
  return true;
}

/** the reprojection error over the six degrees of freedom of the pose; s_sum: kWavesPerBlock x 27 doubles */
struct PnpRefinement {
  static constexpr int kUnknowns = 6;
  const double *X, *obs;
  const PnpParams &p;
  double *s_sum;
  int tid;

  /** sum |r|^2 and the number of counting points over the inliers of `Tsel`, at pose T: (cost, count) on every thread */
  __device__ __forceinline__ void cost(const double *T, const double *Tsel, double &value, double &count) const {
    double v[2] = {0.0, 0.0};
    for (int j = tid; j < p.n; j += kBlock) {
      if (!isInlier(Tsel, X, obs, j, p)) continue;
      double Xj[3], pc[3], r[2];
      if (!pixelResidual(T, X, obs, j, p, Xj, pc, r)) continue;
      v[0] += r[0] * r[0] + r[1] * r[1];
      v[1] += 1.0;
    }
    blockSum<2>(v, s_sum, tid & 63, tid >> 6);
    value = 0.5 * v[0];
    count = v[1];
  }

  /** H (upper triangle, row by row: 21) and b (6) over the inliers of `Tsel`, at pose T */
  __device__ __forceinline__ void linearise(const double *T, const double *Tsel, double (&Hb)[27]) const {
#pragma unroll
    for (int k = 0; k < 27; ++k) Hb[k] = 0.0;
    for (int j = tid; j < p.n; j += kBlock) {
      if (!isInlier(Tsel, X, obs, j, p)) continue;
      double Xj[3], pc[3], r[2];
      if (!pixelResidual(T, X, obs, j, p, Xj, pc, r)) continue;
      const double z = pc[2];
      const double g00 = p.fx / z, g02 = -p.fx * pc[0] / (z * z), g11 = p.fy / z, g12 = -p.fy * pc[1] / (z * z);
      double J[2][6];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        J[0][c] = -(g00 * T[c] + g02 * T[6 + c]);
        J[1][c] = -(g11 * T[3 + c] + g12 * T[6 + c]);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        J[k][3] = J[k][2] * Xj[1] - J[k][1] * Xj[2];
        J[k][4] = J[k][0] * Xj[2] - J[k][2] * Xj[0];
        J[k][5] = J[k][1] * Xj[0] - J[k][0] * Xj[1];
      }
      int at = 0;
#pragma unroll
      for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int b = a; b < 6; ++b) Hb[at++] += J[0][a] * J[0][b] + J[1][a] * J[1][b];
#pragma unroll
      for (int a = 0; a < 6; ++a) Hb[21 + a] += J[0][a] * r[0] + J[1][a] * r[1];
    }
    blockSum<27>(Hb, s_sum, tid & 63, tid >> 6);
  }

  /** T Exp(delta) */
  __device__ __forceinline__ void retract(const double *T, const double (&delta)[6], double *C) const {
    Rigid current;
#pragma unroll
    for (int e = 0; e < 9; ++e) current.R[e] = T[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) current.t[e] = T[9 + e];
    const Rigid candidate = rigidMul(current, rigidExp(delta));
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = candidate.R[e];
#pragma unroll
    for (int e = 0; e < 3; ++e) C[9 + e] = candidate.t[e];
  }
};

__global__ void __launch_bounds__(kBlock) pnpRansacKernel(const double *__restrict__ X, const double *__restrict__ obs, const int *__restrict__ samples,
                                                          unsigned *ticket, int *hyp_num_solutions, double *hyp_poses, int *hyp_counts,
                                                          dsopp_hip_pnp_ransac_result *result, int *__restrict__ inliers, const PnpParams p) {
  __shared__ unsigned s_last;
  __shared__ int s_best_iteration, s_best_solution, s_best_count;
  __shared__ int s_wave_count[kWavesPerBlock];
  __shared__ double s_sum[kWavesPerBlock * 27];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hyp = static_cast<int>(blockIdx.x) * kWavesPerBlock + wave;
  if (hyp < p.iterations) {
    double Xs[3][3], fs[3][3];
    bool valid = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t s = static_cast<size_t>(samples[3 * static_cast<size_t>(hyp) + k]);
      const double x = obs[2 * s], y = obs[2 * s + 1];
      valid = valid && insideRoi(x, y, p);
      bearing(x, y, p, fs[k]);
#pragma unroll
      for (int r = 0; r < 3; ++r) Xs[k][r] = X[3 * s + r];
    }
    double pose[4][12];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int e = 0; e < 12; ++e) pose[s][e] = 0.0;
    int solutions = 0;
    if (valid) solutions = solveP3P(Xs, fs, pose);
    int count[4] = {0, 0, 0, 0};
    if (solutions > 0) {
      for (int base = 0; base < p.n; base += 64) {
        const int j = base + lane;
        bool match = false;
        double f[3] = {0.0, 0.0, 1.0}, Xj[3] = {0.0, 0.0, 0.0};
        if (j < p.n) {
          const double x = obs[2 * static_cast<size_t>(j)], y = obs[2 * static_cast<size_t>(j) + 1];
          match = insideRoi(x, y, p);
          bearing(x, y, p, f);
#pragma unroll
          for (int r = 0; r < 3; ++r) Xj[r] = X[3 * static_cast<size_t>(j) + r];
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          const bool in = match && s < solutions && angularDistance(pose[s], Xj, f) < p.t_ang;
          count[s] += __builtin_popcountll(__ballot(in));
        }
      }
    }
    if (lane == 0) {
      hyp_num_solutions[hyp] = solutions;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        hyp_counts[4 * static_cast<size_t>(hyp) + s] = count[s];
#pragma unroll
        for (int e = 0; e < 12; ++e) hyp_poses[48 * static_cast<size_t>(hyp) + 12 * s + e] = pose[s][e];
      }
    }
  }
  if (!lastWorkgroup(ticket, s_last)) return;

  if (wave == 0) selectBest<4>(hyp_counts, p.iterations, lane, s_best_iteration, s_best_solution, s_best_count);
  __syncthreads();
  const int best_iteration = s_best_iteration, best_solution = s_best_solution;
  double T0[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, T[12];
  if (best_iteration >= 0) {
#pragma unroll
    for (int e = 0; e < 12; ++e) T0[e] = freshLoad(hyp_poses + 48 * static_cast<size_t>(best_iteration) + 12 * best_solution + e);
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) T[e] = T0[e];
  int iterations = 0, flags = 0, total = 0;
  double cost_initial = 0.0, cost = 0.0;
  if (best_iteration >= 0) {
    refinePose(PnpRefinement{X, obs, p, s_sum, tid}, T, T0, iterations, flags, cost_initial, cost);
    total = listInliers(p.n, [&](int j) { return isInlier(T, X, obs, j, p); }, s_wave_count, tid, inliers);
  }
  if (tid == 0) {
    result->matches = 0;  // (the host counts them)
    result->best_iteration = best_iteration;
    result->best_solution = best_solution;
    result->ransac_inlier_count = s_best_count;
    result->refined_inlier_count = total;
    result->refine_iterations = iterations;
    result->refine_flags = flags;
    result->reserved = 0;
    result->cost_initial = cost_initial;
    result->cost_final = cost;
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      result->pose_ransac[e] = T0[e];
      result->pose[e] = T[e];
    }
  }
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_pnp_ransac : dsopp_hip::StagedCall {};

namespace dsopp_hip {
namespace {

/** in:  ticket (16 bytes) | X | obs | samples;   out: result (256 bytes) | inliers | hyp_poses | hyp_counts | hyp_num_solutions.
 *  The per-hypothesis outputs come last, so a call that does not ask for them copies the head only */
struct PnpLayout {
  size_t x, obs, samples, in_bytes;
  size_t inliers, poses, counts, solutions, head_bytes, out_bytes;
  PnpLayout(size_t n, size_t iterations) {
    x = 16;
    obs = x + 24 * n;
    samples = obs + 16 * n;
    in_bytes = samples + 12 * iterations;
    static_assert(sizeof(dsopp_hip_pnp_ransac_result) <= 256, "the result's slot");
    inliers = 256;
    head_bytes = inliers + 4 * n;
    poses = (head_bytes + 7) / 8 * 8;
    counts = poses + 384 * iterations;
    solutions = counts + 16 * iterations;
    out_bytes = solutions + 4 * iterations;
  }
};

void defaultOptions(dsopp_hip_pnp_ransac_options *o) {
  o->lambda_0 = 1e-4;
  o->function_tolerance = 1e-10;
  o->parameter_tolerance = 1e-10;
  o->decrease_factor = 2.0;
  o->increase_factor = 10.0;
  o->max_iterations = 10;
  o->reserved = 0;
}

void estimate(dsopp_hip_pnp_ransac *h, double fx, double fy, double cx, double cy, int width, int height, int n, const double *positions,
              const double *observations, int iterations, const int32_t *samples, double threshold_px, const dsopp_hip_pnp_ransac_options *options,
              dsopp_hip_pnp_ransac_result *result, int32_t *inlier_indices, int32_t *hyp_num_solutions, double *hyp_poses, int32_t *hyp_counts) {
  if (!h) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null pnp ransac");
  if (!result) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (n < 0 || n > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d points", n);
  if (iterations < 0 || iterations > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d iterations", iterations);
  if (!finite(fx) || !finite(fy) || !finite(cx) || !finite(cy)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an intrinsic is not finite");
  if (!finite(threshold_px)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the threshold is not finite");
  if (n > 0 && (!positions || !observations || !inlier_indices)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  dsopp_hip_pnp_ransac_options o;
  defaultOptions(&o);
  if (options) o = *options;
  if (!finite(o.lambda_0) || !finite(o.function_tolerance) || !finite(o.parameter_tolerance) || !finite(o.decrease_factor) ||
      !finite(o.increase_factor) || o.lambda_0 < 0.0 || !(o.decrease_factor > 0.0) || !(o.increase_factor > 0.0) || o.max_iterations < 0)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a refinement option is out of range");
  const size_t count = static_cast<size_t>(n), hyps = static_cast<size_t>(iterations);
  const double xmax = static_cast<double>(width) - 5.0, ymax = static_cast<double>(height) - 5.0;
  int matches = 0;
  for (size_t j = 0; j < count; ++j) {
    for (size_t k = 0; k < 3; ++k)
      if (!finite(positions[3 * j + k])) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "position %zu is not finite", j);
    const double x = observations[2 * j], y = observations[2 * j + 1];
    if (!finite(x) || !finite(y)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "observation %zu is not finite", j);
    if (x >= 4.0 && x <= xmax && y >= 4.0 && y <= ymax) ++matches;
  }
  if (n > 0 && iterations > 0) {
    if (n < 3) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d points: a triple of distinct indices needs 3", n);
    checkSamples<3, true>(samples, iterations, n, "points");
  }
  std::memset(result, 0, sizeof(*result));
  result->matches = matches;
  result->best_iteration = -1;
  result->best_solution = -1;
  for (int k = 0; k < 9; ++k) result->pose_ransac[k] = result->pose[k] = k % 4 == 0 ? 1.0 : 0.0;
  if (n == 0 || iterations == 0) return;  // no hypothesis: the identity, no inliers, no refinement
  h->sr.use();
  const hipStream_t st = h->sr.stream;
  const PnpLayout lay(count, hyps);
  h->ensure(lay.in_bytes, lay.out_bytes);
  uint8_t *hi = h->h_in.get(), *di = h->d_in.get(), *ho = h->h_out.get(), *dout = h->d_out.get();
  std::memset(hi, 0, 16);  // (the ticket is armed by the upload)
  std::memcpy(hi + lay.x, positions, 24 * count);
  std::memcpy(hi + lay.obs, observations, 16 * count);
  std::memcpy(hi + lay.samples, samples, 12 * hyps);
  HIP_CHECK(hipMemcpyAsync(di, hi, lay.in_bytes, hipMemcpyHostToDevice, st));
  PnpParams p;
  p.fx = fx;
  p.fy = fy;
  p.cx = cx;
  p.cy = cy;
  p.xmax = xmax;
  p.ymax = ymax;
  p.t_ang = 1.0 - std::cos(std::atan(threshold_px / fx));
  p.lambda_0 = o.lambda_0;
  p.function_tolerance = o.function_tolerance;
  p.parameter_tolerance = o.parameter_tolerance;
  p.decrease_factor = o.decrease_factor;
  p.increase_factor = o.increase_factor;
  p.n = n;
  p.iterations = iterations;
  p.max_iterations = o.max_iterations;
  const unsigned blocks = (static_cast<unsigned>(iterations) + kWavesPerBlock - 1) / kWavesPerBlock;
  pnpRansacKernel<<<blocks, kBlock, 0, st>>>(reinterpret_cast<const double *>(di + lay.x), reinterpret_cast<const double *>(di + lay.obs),
                                             reinterpret_cast<const int *>(di + lay.samples), reinterpret_cast<unsigned *>(di),
                                             reinterpret_cast<int *>(dout + lay.solutions), reinterpret_cast<double *>(dout + lay.poses),
                                             reinterpret_cast<int *>(dout + lay.counts), reinterpret_cast<dsopp_hip_pnp_ransac_result *>(dout),
                                             reinterpret_cast<int *>(dout + lay.inliers), p);
  HIP_CHECK(hipGetLastError());
  const bool with_hypotheses = hyp_num_solutions || hyp_poses || hyp_counts;
  HIP_CHECK(hipMemcpyAsync(ho, dout, with_hypotheses ? lay.out_bytes : lay.head_bytes, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipEventRecord(h->done.get(hipEventDisableTiming), st));
  HIP_CHECK(hipEventSynchronize(h->done.h));  // the one wait of the call
  std::memcpy(result, ho, sizeof(*result));
  result->matches = matches;
  if (result->refined_inlier_count < 0 || result->refined_inlier_count > n)
    fail(DSOPP_HIP_ERR_HIP, "the device returned %d inliers of %d points", result->refined_inlier_count, n);
  std::memcpy(inlier_indices, ho + lay.inliers, 4 * static_cast<size_t>(result->refined_inlier_count));
  if (hyp_num_solutions) std::memcpy(hyp_num_solutions, ho + lay.solutions, 4 * hyps);
  if (hyp_poses) std::memcpy(hyp_poses, ho + lay.poses, 384 * hyps);
  if (hyp_counts) std::memcpy(hyp_counts, ho + lay.counts, 16 * hyps);
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_pnp_ransac_default_iterations(void) { return 256; }

void dsopp_hip_pnp_ransac_default_options(dsopp_hip_pnp_ransac_options *options) {
  if (options) defaultOptions(options);
}

int dsopp_hip_pnp_ransac_create(int device, void *stream, dsopp_hip_pnp_ransac **out) { return createHandle(device, stream, out); }

void dsopp_hip_pnp_ransac_destroy(dsopp_hip_pnp_ransac *r) { destroyHandle(r); }

int dsopp_hip_pnp_ransac_estimate(dsopp_hip_pnp_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                  const double *positions, const double *observations, int iterations, const int32_t *samples, double threshold_px,
                                  const dsopp_hip_pnp_ransac_options *options, dsopp_hip_pnp_ransac_result *result, int32_t *inlier_indices,
                                  int32_t *hyp_num_solutions, double *hyp_poses, int32_t *hyp_counts) {
  return guarded([&] {
    estimate(r, fx, fy, cx, cy, width, height, n, positions, observations, iterations, samples, threshold_px, options, result, inlier_indices,
             hyp_num_solutions, hyp_poses, hyp_counts);
  });
}

}  // extern "C"
