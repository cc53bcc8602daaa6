// The bootstrap's geometric (reprojection-error) bundle adjustment on the device, with the triangulation and the pruning around it, and the
// dsopp_hip_geometric_ba_* entry points.
//   optimizeTransformations              src/feature_based_slam/tracker/src/refine_track.cpp:16-83
//   CeresGeometricBundleAdjustmentSolver src/energy/problems/src/geometric_bundle_adjustment/ceres_geometric_bundle_adjustment_solver.cpp:33-108
//   the cost functor, the camera          bundle_adjustment_geometric_cost_functor.hpp:41-60, pinhole_camera.hpp:78-90
//   the LM driver                        src/energy/problems/include/energy/levenberg_marquardt_algorithm/levenberg_marquardt_algorithm.hpp:77-128
//   triangulation, removeOutliers        triangulate_points.cpp:47-71, triangulation.hpp:52-64, remove_outliers.cpp:15-47
//
// The arithmetic is the one include/dsopp_hip.h states (tests/geometric_ba_model.py is its NumPy form), all of it binary64.
//
// The problem is small (thousands of observations, at most 89 pose unknowns): what costs is the number of dependent launches.  An LM
// iteration is five launches on the object's stream, each of which leaves at once when the state record says the solve is over:
//   linearise  a thread per landmark walks its (at most 16) observations in list order: residual, Huber weight, C = w Jx^T Jx and
//              c = w Jx^T r per observation to global memory, their sums H_ll and b_l per landmark.  Every pose-side block is a function of
//              C, c and the landmark's position (J_p = J_x [I | -hat(X)]), so nothing larger than nine doubles per observation is stored.
//              It runs only after an accepted step: after a reject the blocks are kept.
//   reduce     a workgroup per pair (f, g), f <= g, of free frames: sum over the landmarks of Y_f^T Y_g with Y_f = L^-1 W_f^T and
//              L L^T = H_ll + lambda diag(H_ll); the diagonal pairs also sum H_pp, b_p and the Schur part of the right-hand side.
//              A thread's landmarks in index order, then every sum down its wave's butterfly and the four waves in order.
//   solve      one workgroup: assembles the reduced system (frame 0 dropped, frame 1 through its 6 x 5 tangent basis, the damping on the
//              mapped diagonal), Cholesky of the system bordered by its right-hand side and the back-substitution in LDS, the candidate poses.
//   update     a thread per landmark: back-substitution, candidate point, candidate residuals and cost.
//   decide     one workgroup: the fixed-order sums of the candidate cost and the norms, the LM driver's decision, the accepted state.
// No workgroup waits for another, no floating-point atomics: two calls with the same inputs return the same bytes.  The host enqueues
// the iterations in groups and reads the state record between groups.
//
// The camera block (dsopp_hip_geometric_ba_evaluate_camera / _solve_camera: optimizeTransformations<Model, OPTIMIZE_CAMERA>, the intrinsics
// of a pinhole or simple-radial camera as a third parameter block, ParameterParameterization's five fix flags) is the CAM instance of
// the same five kernels; what the entry points without a camera launch is the instance without it, whose arithmetic is untouched.
//   linearise  also stores per observation dr/dc (2 x 5) and w J_x^T J_c (3 x 5), over all five parameter slots: which of them are free
//              is decided where the system is assembled.
//   reduce     behind the frame pairs a workgroup per free frame (H_pc and S_fc = sum_l Y_f^T Y_c) and one for the camera (H_cc, b_c,
//              S_cc, s_c), each with its own 60 or 40 accumulators in place of the pairs' 84: the roles are uniform per workgroup.
//              Without a free intrinsic nothing reads their sums and, with free poses, they are not launched.
//   solve      up to 89 + 5 unknowns, the free intrinsics' rows last; the candidate camera, its max_valid_radius
//              (simple_radial_radius.hpp, on one thread) and the rule that fails the step.
//   update     adds W_lc delta_c and evaluates with the candidate camera; decide accepts it with the state.
#include "common.hpp"
#include "se3_math.hpp"
#include "simple_radial_radius.hpp"

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <memory>

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxFrames = 16;
constexpr int kMaxUnknowns = 6 * (kMaxFrames - 1) - 1;  // 89
constexpr int kCam = 5;                                 // the intrinsics of the widest camera model
constexpr int kFixPoses = DSOPP_HIP_GEOMETRIC_BA_FIX_POSES, kFixLandmarks = DSOPP_HIP_GEOMETRIC_BA_FIX_LANDMARKS;
constexpr int kJacobiSweeps = 30;                       // a 4 x 4 Jacobi converges in 5 .. 8 sweeps; the cap bounds the loop for NaN input
constexpr int kDefaultGroup = 8;

struct GbaState {
  double cost, cand_cost, lambda, step_sq, state_sq, system_lambda, initial_cost, pad0;
  int nvalid, cand_nvalid, it, accepted, relin, done, reason, solve_failed;
};
static_assert(sizeof(GbaState) == 96, "the state record");

struct GbaParams {
  double fx, fy, cx, cy, xmax, ymax;
  double a, ftol, ptol, dec, inc, norm1;  // norm1 = |t_1| on entry
  int F, L, M, max_it;
  double *poses, *cand_poses, *X, *candX;
  const int *off, *ofr;
  const double *oxy;
  double *C, *res, *wgt;
  uint8_t *valid;
  double *Hll, *bl, *lm;  // lm: L x 4 = cost, candidate cost, |delta_l|^2, |X|^2
  int *lmn;               // L x 2 = valid, candidate valid
  double *Spair, *Hpp, *bp, *rs, *delta6, *sysH, *sysb, *sysx;
  GbaState *st;
  dsopp_hip_geometric_ba_trace *trace;
  // the camera block (the *_camera entry points; the kernels' CAM instances): the model, the fixed bits, the pose unknowns (0 with fixed
  // poses), the free intrinsics in parameter order
  int model, fixed, npose, ncam, cidx[kCam];
  double width, height;
  double *camrec;  // intrinsics[5], max_valid_radius, 2 unused; the candidate's likewise
  double *Jc, *Wc;  // per observation dr/dc (2 x 5) and w J_x^T J_c (3 x 5)
  double *Hpc, *Sfc, *camsum, *deltac;  // F x (6 x 5) twice; H_cc (15, packed lower), b_c (5), S_cc (15), s_c (5); the step over all five
};

/** a camera as the kernels read it */
struct Camera {
  int model;
  double c[kCam], radius;
};

__device__ __forceinline__ Camera loadCamera(const GbaParams &p, bool candidate) {
  Camera cam;
  cam.model = p.model;
  const double *rec = p.camrec + (candidate ? 8 : 0);
#pragma unroll
  for (int k = 0; k < kCam; ++k) cam.c[k] = rec[k];
  cam.radius = rec[5];
  return cam;
}

__device__ __forceinline__ bool insideRoi(double x, double y, const GbaParams &p) { return x >= 4.0 && x <= p.xmax && y >= 4.0 && y <= p.ymax; }

/** pc = R X + t, the projection q; false when p_z < 0.001 or q leaves the ROI (or anything is NaN) */
__device__ __forceinline__ bool project(const double *T, const double *X, const GbaParams &p, double *pc, double *q) {
#pragma unroll
  for (int r = 0; r < 3; ++r) pc[r] = T[3 * r] * X[0] + T[3 * r + 1] * X[1] + T[3 * r + 2] * X[2] + T[9 + r];
  q[0] = q[1] = 0.0;
  if (!(pc[2] >= 0.001)) return false;
  q[0] = p.fx * pc[0] / pc[2] + p.cx;
  q[1] = p.fy * pc[1] / pc[2] + p.cy;
  return insideRoi(q[0], q[1], p);
}

/** the same for a camera of the camera block.  Pinhole: as above.  Simple radial (simple_radial.hpp:133-160): u = p_x / p_z, v = p_y / p_z,
 *  rho2 = u u + v v, d = (1 + k1 rho2) + (k2 rho2) rho2, q = f (d (u, v)) + (cx, cy); false when sqrt(rho2) > max_valid_radius or q leaves
 *  the ROI; no test on p_z */
__device__ __forceinline__ bool projectCamera(const double *T, const double *X, const GbaParams &p, const Camera &cam, double *pc, double *q) {
#pragma unroll
  for (int r = 0; r < 3; ++r) pc[r] = T[3 * r] * X[0] + T[3 * r + 1] * X[1] + T[3 * r + 2] * X[2] + T[9 + r];
  q[0] = q[1] = 0.0;
  if (cam.model == DSOPP_HIP_GEOMETRIC_BA_PINHOLE) {
    if (!(pc[2] >= 0.001)) return false;
    q[0] = cam.c[0] * pc[0] / pc[2] + cam.c[2];
    q[1] = cam.c[1] * pc[1] / pc[2] + cam.c[3];
    return insideRoi(q[0], q[1], p);
  }
  const double u = pc[0] / pc[2], v = pc[1] / pc[2], rho2 = u * u + v * v;
  const double d = (1.0 + cam.c[3] * rho2) + (cam.c[4] * rho2) * rho2;
  q[0] = cam.c[0] * (d * u) + cam.c[1];
  q[1] = cam.c[0] * (d * v) + cam.c[2];
  return sqrt(rho2) <= cam.radius && insideRoi(q[0], q[1], p);
}

/** Huber: the weight rho'(s) and rho(s) */
__device__ __forceinline__ void huber(double s, double a, double &w, double &rho) {
  if (s <= a * a) {
    w = 1.0;
    rho = s;
  } else {
    const double n = sqrt(s);
    w = a / n;
    rho = 2.0 * a * n - a * a;
  }
}

/** the residual of one observation: valid, r (0 when invalid) */
template <bool CAM>
__device__ __forceinline__ bool residualOf(const double *T, const double *X, const double *obs, const GbaParams &p, const Camera &cam, double *r,
                                           double *pc) {
  double q[2];
  bool ok;
  if constexpr (CAM) {
    ok = projectCamera(T, X, p, cam, pc, q);
  } else {
    ok = project(T, X, p, pc, q);
  }
  r[0] = ok ? obs[0] - q[0] : 0.0;
  r[1] = ok ? obs[1] - q[1] : 0.0;
  return ok;
}

/** L^-1 (lower, packed l00 l10 l11 l20 l21 l22) of H_ll + lambda diag(H_ll); false when a pivot is <= 0 or not finite */
__device__ __forceinline__ bool landmarkFactor(const double *H, double lambda, double *Li) {
  const double a00 = H[0] + lambda * H[0], a10 = H[1], a20 = H[2], a11 = H[3] + lambda * H[3], a21 = H[4], a22 = H[5] + lambda * H[5];
#pragma unroll
  for (int k = 0; k < 6; ++k) Li[k] = 0.0;
  if (!(a00 > 0.0) || !(a00 <= DBL_MAX)) return false;
  const double l00 = sqrt(a00), l10 = a10 / l00, l20 = a20 / l00;
  const double d1 = a11 - l10 * l10;
  if (!(d1 > 0.0) || !(d1 <= DBL_MAX)) return false;
  const double l11 = sqrt(d1), l21 = (a21 - l20 * l10) / l11;
  const double d2 = a22 - l20 * l20 - l21 * l21;
  if (!(d2 > 0.0) || !(d2 <= DBL_MAX)) return false;
  const double l22 = sqrt(d2);
  Li[0] = 1.0 / l00;
  Li[2] = 1.0 / l11;
  Li[5] = 1.0 / l22;
  Li[1] = -l10 * Li[0] / l11;
  Li[4] = -l21 * Li[2] / l22;
  Li[3] = -(l20 * Li[0] + l21 * Li[1]) / l22;
  return true;
}

/** y = L^-1 v */
__device__ __forceinline__ void lowerApply(const double *Li, const double *v, double *y) {
  y[0] = Li[0] * v[0];
  y[1] = Li[1] * v[0] + Li[2] * v[1];
  y[2] = Li[3] * v[0] + Li[4] * v[1] + Li[5] * v[2];
}

/** A = [I | -hat(X)], 3 x 6: d(R X + t) = R A (upsilon, omega) for the right increment T exp(delta) */
__device__ __forceinline__ void poseMap(const double *X, double A[3][6]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) A[r][c] = r == c ? 1.0 : 0.0;
  A[0][4] = X[2];
  A[0][5] = -X[1];
  A[1][3] = -X[2];
  A[1][5] = X[0];
  A[2][3] = X[1];
  A[2][4] = -X[0];
}

__device__ __forceinline__ void loadSym(const double *c, double S[3][3]) {
  S[0][0] = c[0];
  S[0][1] = S[1][0] = c[1];
  S[0][2] = S[2][0] = c[2];
  S[1][1] = c[3];
  S[1][2] = S[2][1] = c[4];
  S[2][2] = c[5];
}

/** the tangent basis of the sphere at direction d: k = the first axis d leans on least, b1 = normalize(d x e_k), b2 = d x b1 */
__device__ __forceinline__ void sphereBasis(const double *d, double *b1, double *b2) {
  const double a0 = fabs(d[0]), a1 = fabs(d[1]), a2 = fabs(d[2]);
  const int k = a0 <= a1 && a0 <= a2 ? 0 : (a1 <= a2 ? 1 : 2);
  const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
  double c[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
  const double n = sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) b1[r] = c[r] / n;
  b2[0] = d[1] * b1[2] - d[2] * b1[1];
  b2[1] = d[2] * b1[0] - d[0] * b1[2];
  b2[2] = d[0] * b1[1] - d[1] * b1[0];
}

/** the sum of v over the wave, in every lane: a butterfly */
__device__ __forceinline__ double waveSum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

/** the sum of v over the workgroup, in every thread: the wave's butterfly, then the waves in order */
__device__ __forceinline__ double blockSum(double v, double *s_wave) {
  v = waveSum(v);
  __syncthreads();  // (s_wave may still be read from the previous sum)
  if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kBlock / 64; ++w) s += s_wave[w];
  return s;
}

// ---------------------------------------------------------------------------------------------------------------- linearise

/** the camera block of one valid observation: J_x = -G R (2 x 3) and J_c = dr / dc (2 x 5; a pinhole's fifth column is zero) */
__device__ __forceinline__ void cameraJacobians(const double *T, const double *pc, const Camera &cam, double J[2][3], double Jc[2][kCam]) {
  if (cam.model == DSOPP_HIP_GEOMETRIC_BA_PINHOLE) {
    // J_x exactly as the instance without a camera block has it
    const double fx = cam.c[0], fy = cam.c[1];
    const double iz = 1.0 / pc[2];
    const double g00 = fx * iz, g02 = -fx * pc[0] * iz * iz, g11 = fy * iz, g12 = -fy * pc[1] * iz * iz;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      J[0][k] = -(g00 * T[k] + g02 * T[6 + k]);
      J[1][k] = -(g11 * T[3 + k] + g12 * T[6 + k]);
    }
    const double u = pc[0] / pc[2], v = pc[1] / pc[2];
    Jc[0][0] = -u;
    Jc[0][1] = 0.0;
    Jc[0][2] = -1.0;
    Jc[0][3] = 0.0;
    Jc[0][4] = 0.0;
    Jc[1][0] = 0.0;
    Jc[1][1] = -v;
    Jc[1][2] = 0.0;
    Jc[1][3] = -1.0;
    Jc[1][4] = 0.0;
    return;
  }
  // simple radial: G as simple_radial.hpp:190-199 writes it
  const double f = cam.c[0], k1 = cam.c[3], k2 = cam.c[4];
  const double x = pc[0], y = pc[1], z = pc[2];
  const double u = x / z, v = y / z, rho2 = u * u + v * v;
  const double d = (1.0 + k1 * rho2) + (k2 * rho2) * rho2;
  const double common = (2.0 * k1 + 4.0 * k2 * rho2) / z / z;
  const double last = -3.0 * k1 * rho2 - 5.0 * k2 * rho2 * rho2 - 1.0;
  double G[2][3];
  G[0][0] = f * (x * x * common + d) / z;
  G[0][1] = f * x * y * common / z;
  G[1][0] = G[0][1];
  G[1][1] = f * (y * y * common + d) / z;
  G[0][2] = f * x / z / z * last;
  G[1][2] = f * y / z / z * last;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    J[0][k] = -(G[0][0] * T[k] + G[0][1] * T[3 + k] + G[0][2] * T[6 + k]);
    J[1][k] = -(G[1][0] * T[k] + G[1][1] * T[3 + k] + G[1][2] * T[6 + k]);
  }
  const double f2 = f * rho2, f4 = f * (rho2 * rho2);
  Jc[0][0] = -(d * u);
  Jc[0][1] = -1.0;
  Jc[0][2] = 0.0;
  Jc[0][3] = -(f2 * u);
  Jc[0][4] = -(f4 * u);
  Jc[1][0] = -(d * v);
  Jc[1][1] = 0.0;
  Jc[1][2] = -1.0;
  Jc[1][3] = -(f2 * v);
  Jc[1][4] = -(f4 * v);
}

template <bool CAM>
__global__ void __launch_bounds__(kBlock) gbaLinearise(const GbaParams p) {
  if (p.st->done || !p.st->relin) return;
  const int l = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (l >= p.L) return;
  Camera cam;
  if constexpr (CAM) cam = loadCamera(p, false);
  const double X[3] = {p.X[3 * static_cast<size_t>(l)], p.X[3 * static_cast<size_t>(l) + 1], p.X[3 * static_cast<size_t>(l) + 2]};
  double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, cost = 0.0;
  int nv = 0;
  for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
    const double *T = p.poses + 12 * static_cast<size_t>(p.ofr[o]);
    const double obs[2] = {p.oxy[2 * static_cast<size_t>(o)], p.oxy[2 * static_cast<size_t>(o) + 1]};
    double r[2], pc[3], w = 0.0, C[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
    const bool ok = residualOf<CAM>(T, X, obs, p, cam, r, pc);
    if constexpr (CAM) {
      // the camera's columns: zero for an observation that is not valid
      double *Jo = p.Jc + 2 * kCam * static_cast<size_t>(o), *Wo = p.Wc + 3 * kCam * static_cast<size_t>(o);
#pragma unroll
      for (int k = 0; k < 2 * kCam; ++k) Jo[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3 * kCam; ++k) Wo[k] = 0.0;
    }
    if (ok) {
      double rho;
      huber(r[0] * r[0] + r[1] * r[1], p.a, w, rho);
      cost += rho;
      ++nv;
      // J_x = -G R, G = dq / dp
      double J[2][3];
      if constexpr (CAM) {
        double Jc[2][kCam];
        cameraJacobians(T, pc, cam, J, Jc);
        double *Jo = p.Jc + 2 * kCam * static_cast<size_t>(o), *Wo = p.Wc + 3 * kCam * static_cast<size_t>(o);
#pragma unroll
        for (int a = 0; a < kCam; ++a) {
          Jo[a] = Jc[0][a];
          Jo[kCam + a] = Jc[1][a];
#pragma unroll
          for (int k = 0; k < 3; ++k) Wo[kCam * k + a] = w * (J[0][k] * Jc[0][a] + J[1][k] * Jc[1][a]);
        }
      } else {
        const double iz = 1.0 / pc[2];
        const double g00 = p.fx * iz, g02 = -p.fx * pc[0] * iz * iz, g11 = p.fy * iz, g12 = -p.fy * pc[1] * iz * iz;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          J[0][k] = -(g00 * T[k] + g02 * T[6 + k]);
          J[1][k] = -(g11 * T[3 + k] + g12 * T[6 + k]);
        }
      }
      C[0] = w * (J[0][0] * J[0][0] + J[1][0] * J[1][0]);
      C[1] = w * (J[0][0] * J[0][1] + J[1][0] * J[1][1]);
      C[2] = w * (J[0][0] * J[0][2] + J[1][0] * J[1][2]);
      C[3] = w * (J[0][1] * J[0][1] + J[1][1] * J[1][1]);
      C[4] = w * (J[0][1] * J[0][2] + J[1][1] * J[1][2]);
      C[5] = w * (J[0][2] * J[0][2] + J[1][2] * J[1][2]);
#pragma unroll
      for (int k = 0; k < 3; ++k) c[k] = w * (J[0][k] * r[0] + J[1][k] * r[1]);
    }
    double *Co = p.C + 9 * static_cast<size_t>(o);
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      Co[k] = C[k];
      H[k] += C[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      Co[6 + k] = c[k];
      b[k] += c[k];
    }
    p.res[2 * static_cast<size_t>(o)] = r[0];
    p.res[2 * static_cast<size_t>(o) + 1] = r[1];
    p.wgt[o] = w;
    p.valid[o] = ok ? 1 : 0;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) p.Hll[6 * static_cast<size_t>(l) + k] = H[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) p.bl[3 * static_cast<size_t>(l) + k] = b[k];
  p.lm[4 * static_cast<size_t>(l)] = cost;
  p.lmn[2 * static_cast<size_t>(l)] = nv;
}

/** the cost of the first linearisation: cost = 1/2 sum rho; closes the solve at once when nothing is valid or no iteration is asked for */
__global__ void __launch_bounds__(kBlock) gbaInitialCost(const GbaParams p) {
  __shared__ double s_wave[kBlock / 64];
  double cost = 0.0, nv = 0.0;
  for (int l = threadIdx.x; l < p.L; l += kBlock) {
    cost += p.lm[4 * static_cast<size_t>(l)];
    nv += static_cast<double>(p.lmn[2 * static_cast<size_t>(l)]);
  }
  cost = blockSum(cost, s_wave);
  nv = blockSum(nv, s_wave);
  if (threadIdx.x == 0) {
    GbaState &s = *p.st;
    s.cost = s.initial_cost = 0.5 * cost;
    s.nvalid = static_cast<int>(nv);
    s.relin = 0;
    if (s.nvalid == 0) {
      s.done = 1;
      s.reason = DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL;
    } else if (p.max_it <= 0) {
      s.done = 1;
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------- reduce

/** the observation of landmark l in frame f, -1 when there is none */
__device__ __forceinline__ int observationIn(const GbaParams &p, int l, int f) {
  int found = -1;
  for (int o = p.off[l]; o < p.off[l + 1]; ++o)
    if (p.ofr[o] == f) found = o;
  return found;
}

/** Y = L^-1 C A, 3 x 6 */
__device__ __forceinline__ void schurFactor(const double *Li, const double *Cpacked, const double A[3][6], double Y[3][6]) {
  double C[3][3], CA[3][6];
  loadSym(Cpacked, C);
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = 0; c < 6; ++c) CA[r][c] = C[r][0] * A[0][c] + C[r][1] * A[1][c] + C[r][2] * A[2][c];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double v[3] = {CA[0][c], CA[1][c], CA[2][c]};
    double y[3];
    lowerApply(Li, v, y);
    Y[0][c] = y[0];
    Y[1][c] = y[1];
    Y[2][c] = y[2];
  }
}

__device__ __forceinline__ int pairIndex(int F, int fa, int fb) {  // 1 <= fa <= fb <= F - 1
  const int a = fa - 1, n = F - 1;
  return a * n - a * (a - 1) / 2 + (fb - fa);
}

/** W_lc = sum over the landmark's observations, in list order, of w J_x^T J_c (3 x 5) */
__device__ __forceinline__ void landmarkCameraBlock(const GbaParams &p, int l, double W[3][kCam]) {
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int a = 0; a < kCam; ++a) W[r][a] = 0.0;
  for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
    const double *Wo = p.Wc + 3 * kCam * static_cast<size_t>(o);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int a = 0; a < kCam; ++a) W[r][a] += Wo[kCam * r + a];
  }
}

/** Y_c = L^-1 W_lc, 3 x 5 */
__device__ __forceinline__ void cameraSchurFactor(const double *Li, const double W[3][kCam], double Y[3][kCam]) {
#pragma unroll
  for (int a = 0; a < kCam; ++a) {
    const double v[3] = {W[0][a], W[1][a], W[2][a]};
    double y[3];
    lowerApply(Li, v, y);
    Y[0][a] = y[0];
    Y[1][a] = y[1];
    Y[2][a] = y[2];
  }
}

/** the workgroup's sums of `count` values a thread: every value down its wave's butterfly, one barrier, then the waves in order into out */
template <int kCount>
__device__ __forceinline__ void blockSums(const double *v, double (*s_part)[84], double *out) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < kCount; ++k) {
    const double s = waveSum(v[k]);
    if (lane == 0) s_part[wave][k] = s;
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < kCount) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += s_part[w][k];
    out[k] = s;
  }
}

/** the (frame f, camera) workgroup: H_pc = sum A^T (w J_x^T J_c) over the frame's observations and S_fc = sum_l Y_f^T Y_c */
__device__ __forceinline__ void reduceFrameCamera(const GbaParams &p, int f, double lambda, double (*s_part)[84]) {
  double acc[2 * 6 * kCam];  // H_pc, then S_fc
#pragma unroll
  for (int k = 0; k < 2 * 6 * kCam; ++k) acc[k] = 0.0;
  const bool eliminate = !(p.fixed & kFixLandmarks);
  for (int l = threadIdx.x; l < p.L; l += kBlock) {
    const int oa = observationIn(p, l, f);
    if (oa < 0) continue;
    const double X[3] = {p.X[3 * static_cast<size_t>(l)], p.X[3 * static_cast<size_t>(l) + 1], p.X[3 * static_cast<size_t>(l) + 2]};
    double A[3][6];
    poseMap(X, A);
    const double *Wo = p.Wc + 3 * kCam * static_cast<size_t>(oa);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int a = 0; a < kCam; ++a) acc[kCam * r + a] += A[0][r] * Wo[a] + A[1][r] * Wo[kCam + a] + A[2][r] * Wo[2 * kCam + a];
    double Li[6];
    if (!eliminate || !landmarkFactor(p.Hll + 6 * static_cast<size_t>(l), lambda, Li)) continue;
    double Ya[3][6], W[3][kCam], Yc[3][kCam];
    schurFactor(Li, p.C + 9 * static_cast<size_t>(oa), A, Ya);
    landmarkCameraBlock(p, l, W);
    cameraSchurFactor(Li, W, Yc);
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int a = 0; a < kCam; ++a) acc[6 * kCam + kCam * r + a] += Ya[0][r] * Yc[0][a] + Ya[1][r] * Yc[1][a] + Ya[2][r] * Yc[2][a];
  }
  // Hpc and Sfc lie one behind the other, F x 30 each
  blockSums<6 * kCam>(acc, s_part, p.Hpc + 6 * kCam * static_cast<size_t>(f));
  __syncthreads();
  blockSums<6 * kCam>(acc + 6 * kCam, s_part, p.Sfc + 6 * kCam * static_cast<size_t>(f));
}

/** the (camera, camera) workgroup: H_cc = sum w J_c^T J_c, b_c = sum w J_c^T r, S_cc = sum_l Y_c^T Y_c, s_c = sum_l Y_c^T L^-1 b_l */
__device__ __forceinline__ void reduceCameraCamera(const GbaParams &p, double lambda, double (*s_part)[84]) {
  double acc[40];  // H_cc (15, packed lower), b_c (5), S_cc (15), s_c (5)
#pragma unroll
  for (int k = 0; k < 40; ++k) acc[k] = 0.0;
  const bool eliminate = !(p.fixed & kFixLandmarks);
  for (int l = threadIdx.x; l < p.L; l += kBlock) {
    for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
      const double *Jo = p.Jc + 2 * kCam * static_cast<size_t>(o);
      const double w = p.wgt[o], r0 = p.res[2 * static_cast<size_t>(o)], r1 = p.res[2 * static_cast<size_t>(o) + 1];
#pragma unroll
      for (int a = 0; a < kCam; ++a) {
#pragma unroll
        for (int b = 0; b <= a; ++b) acc[a * (a + 1) / 2 + b] += w * (Jo[a] * Jo[b] + Jo[kCam + a] * Jo[kCam + b]);
        acc[15 + a] += w * (Jo[a] * r0 + Jo[kCam + a] * r1);
      }
    }
    double Li[6];
    if (!eliminate || !landmarkFactor(p.Hll + 6 * static_cast<size_t>(l), lambda, Li)) continue;
    double W[3][kCam], Yc[3][kCam], z[3];
    landmarkCameraBlock(p, l, W);
    cameraSchurFactor(Li, W, Yc);
    lowerApply(Li, p.bl + 3 * static_cast<size_t>(l), z);
#pragma unroll
    for (int a = 0; a < kCam; ++a) {
#pragma unroll
      for (int b = 0; b <= a; ++b) acc[20 + a * (a + 1) / 2 + b] += Yc[0][a] * Yc[0][b] + Yc[1][a] * Yc[1][b] + Yc[2][a] * Yc[2][b];
      acc[35 + a] += Yc[0][a] * z[0] + Yc[1][a] * z[1] + Yc[2][a] * z[2];
    }
  }
  blockSums<40>(acc, s_part, p.camsum);
}

/** The workgroups of the instance with a camera block: the frame pairs first (none with fixed poses), then a (frame, camera) workgroup
 *  per free frame, then the (camera, camera) workgroup (the host leaves the last two out when no intrinsic is free). */
template <bool CAM>
__global__ void __launch_bounds__(kBlock) gbaReduce(const GbaParams p) {
  __shared__ double s_part[kBlock / 64][84];
  if (p.st->done) return;
  if constexpr (CAM) {
    const int pairs = p.npose > 0 ? (p.F - 1) * p.F / 2 : 0, frames = p.npose > 0 ? p.F - 1 : 0;
    const int role = static_cast<int>(blockIdx.x) - pairs;
    if (role >= frames) {
      reduceCameraCamera(p, p.st->lambda, s_part);
      return;
    }
    if (role >= 0) {
      reduceFrameCamera(p, 1 + role, p.st->lambda, s_part);
      return;
    }
  }
  int fa = 1, rest = static_cast<int>(blockIdx.x);
  while (rest >= p.F - fa) {
    rest -= p.F - fa;
    ++fa;
  }
  const int fb = fa + rest;
  const bool diag = fa == fb;
  const double lambda = p.st->lambda;
  double acc[36], hpp[36], bpv[6], rsv[6];
#pragma unroll
  for (int k = 0; k < 36; ++k) acc[k] = hpp[k] = 0.0;
#pragma unroll
  for (int k = 0; k < 6; ++k) bpv[k] = rsv[k] = 0.0;
  for (int l = threadIdx.x; l < p.L; l += kBlock) {
    const int oa = observationIn(p, l, fa);
    const int ob = diag ? oa : observationIn(p, l, fb);
    if (oa < 0 || ob < 0) continue;
    const double X[3] = {p.X[3 * static_cast<size_t>(l)], p.X[3 * static_cast<size_t>(l) + 1], p.X[3 * static_cast<size_t>(l) + 2]};
    double A[3][6];
    poseMap(X, A);
    const double *Ca = p.C + 9 * static_cast<size_t>(oa);
    if (diag) {
      // H_pp += A^T C A, b_p += A^T c
      double C[3][3], CA[3][6];
      loadSym(Ca, C);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) CA[r][c] = C[r][0] * A[0][c] + C[r][1] * A[1][c] + C[r][2] * A[2][c];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
#pragma unroll
        for (int c = 0; c < 6; ++c) hpp[6 * r + c] += A[0][r] * CA[0][c] + A[1][r] * CA[1][c] + A[2][r] * CA[2][c];
        bpv[r] += A[0][r] * Ca[6] + A[1][r] * Ca[7] + A[2][r] * Ca[8];
      }
    }
    if constexpr (CAM) {
      if (p.fixed & kFixLandmarks) continue;  // no elimination: S = 0
    }
    double Li[6];
    if (!landmarkFactor(p.Hll + 6 * static_cast<size_t>(l), lambda, Li)) continue;
    double Ya[3][6], Yb[3][6];
    schurFactor(Li, Ca, A, Ya);
    if (diag) {
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) Yb[r][c] = Ya[r][c];
      double z[3];
      lowerApply(Li, p.bl + 3 * static_cast<size_t>(l), z);
#pragma unroll
      for (int r = 0; r < 6; ++r) rsv[r] += Ya[0][r] * z[0] + Ya[1][r] * z[1] + Ya[2][r] * z[2];
    } else {
      schurFactor(Li, p.C + 9 * static_cast<size_t>(ob), A, Yb);
    }
#pragma unroll
    for (int r = 0; r < 6; ++r)
#pragma unroll
      for (int c = 0; c < 6; ++c) acc[6 * r + c] += Ya[0][r] * Yb[0][c] + Ya[1][r] * Yb[1][c] + Ya[2][r] * Yb[2][c];
  }
  // the workgroup's sums: every value down its wave's butterfly (independent chains), one barrier, then the four waves in order
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < 36; ++k) {
    const double s = waveSum(acc[k]);
    if (lane == 0) s_part[wave][k] = s;
  }
  if (diag) {
#pragma unroll
    for (int k = 0; k < 36; ++k) {
      const double s = waveSum(hpp[k]);
      if (lane == 0) s_part[wave][36 + k] = s;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      const double s = waveSum(bpv[k]), t = waveSum(rsv[k]);
      if (lane == 0) {
        s_part[wave][72 + k] = s;
        s_part[wave][78 + k] = t;
      }
    }
  }
  __syncthreads();
  const int k = threadIdx.x;
  if (k < (diag ? 84 : 36)) {
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) s += s_part[w][k];
    if (k < 36)
      p.Spair[36 * static_cast<size_t>(blockIdx.x) + k] = s;
    else if (k < 72)
      p.Hpp[36 * static_cast<size_t>(fa) + (k - 36)] = s;
    else if (k < 78)
      p.bp[6 * static_cast<size_t>(fa) + (k - 72)] = s;
    else
      p.rs[6 * static_cast<size_t>(fa) + (k - 78)] = s;
  }
}

// ---------------------------------------------------------------------------------------------------------------- solve

/** unknown i of the reduced system: its frame, and its coefficients over that frame's six tangent components */
struct Unknown {
  int frame, first, count;
  double coef[3];
};

__device__ __forceinline__ Unknown unknownOf(int i, const double Bt[3][2]) {
  Unknown u;
  if (i < 2) {
    u.frame = 1;
    u.first = 0;
    u.count = 3;
    u.coef[0] = Bt[0][i];
    u.coef[1] = Bt[1][i];
    u.coef[2] = Bt[2][i];
  } else {
    u.frame = i < 5 ? 1 : 2 + (i - 5) / 6;
    u.first = i < 5 ? i + 1 : (i - 5) % 6;
    u.count = 1;
    u.coef[0] = 1.0;
    u.coef[1] = u.coef[2] = 0.0;
  }
  return u;
}

__device__ __forceinline__ int packed(int i, int j) { return i * (i + 1) / 2 + j; }  // j <= i

/** entry (a, b) of a camera sum's packed lower triangle */
__device__ __forceinline__ double packedSym(const double *v, int a, int b) { return a >= b ? v[packed(a, b)] : v[packed(b, a)]; }

template <bool CAM>
__global__ void __launch_bounds__(kBlock) gbaSolve(const GbaParams p) {
  constexpr int kUnknowns = kMaxUnknowns + (CAM ? kCam : 0);       // 89, or 94 with the camera's rows behind the poses'
  __shared__ double s_L[(kUnknowns + 1) * (kUnknowns + 2) / 2];  // the lower triangle, packed; row n is the right-hand side
  __shared__ double s_x[kUnknowns];
  __shared__ double s_Bt[3][2], s_basis[6];
  __shared__ int s_fail;
  if (p.st->done) return;
  const int tid = threadIdx.x;
  const int npose = CAM ? p.npose : 6 * (p.F - 1) - 1, n = CAM ? p.npose + p.ncam : npose;
  const double lambda = p.st->lambda;
  const double *T1 = p.poses + 12;
  if (tid == 0) s_fail = 0;
  if (tid == 0 && npose > 0) {
    // frame 1: t = |t_1| d; the tangent directions b1, b2 at d; upsilon = R^T |t_1| (alpha b1 + beta b2)
    const double tn = sqrt(T1[9] * T1[9] + T1[10] * T1[10] + T1[11] * T1[11]);
    const double d[3] = {T1[9] / tn, T1[10] / tn, T1[11] / tn};
    double b1[3], b2[3];
    sphereBasis(d, b1, b2);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      s_Bt[r][0] = p.norm1 * (T1[r] * b1[0] + T1[3 + r] * b1[1] + T1[6 + r] * b1[2]);
      s_Bt[r][1] = p.norm1 * (T1[r] * b2[0] + T1[3 + r] * b2[1] + T1[6 + r] * b2[2]);
      s_basis[r] = b1[r];
      s_basis[3 + r] = b2[r];
    }
  }
  __syncthreads();
  double Bt[3][2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    Bt[r][0] = s_Bt[r][0];
    Bt[r][1] = s_Bt[r][1];
  }
  // the reduced system: B^T (H_pp - S) B + lambda diag(B^T H_pp B), g = -B^T (b_p - s)
  for (int e = tid; e < n * (n + 1) / 2; e += kBlock) {
    int i = static_cast<int>((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
    while (packed(i, 0) > e) --i;
    while (packed(i + 1, 0) <= e) ++i;
    const int j = e - packed(i, 0);
    if constexpr (CAM) {
      if (i >= npose) {
        // a camera row: H_pc - S_fc through the frame's basis, then H_cc - S_cc with the damping on its own diagonal
        const int a = p.cidx[i - npose];
        double v;
        if (j < npose) {
          const Unknown uj = unknownOf(j, Bt);
          const double *H = p.Hpc + 6 * kCam * static_cast<size_t>(uj.frame), *S = p.Sfc + 6 * kCam * static_cast<size_t>(uj.frame);
          double hp = 0.0, sc = 0.0;
          for (int b = 0; b < uj.count; ++b) {
            hp += uj.coef[b] * H[kCam * (uj.first + b) + a];
            sc += uj.coef[b] * S[kCam * (uj.first + b) + a];
          }
          v = hp - sc;
        } else {
          const int b = p.cidx[j - npose];
          const double hp = packedSym(p.camsum, a, b), sc = packedSym(p.camsum + 20, a, b);
          v = (hp - sc) + (i == j ? lambda * hp : 0.0);
        }
        s_L[e] = v;
        p.sysH[static_cast<size_t>(i) * n + j] = v;
        p.sysH[static_cast<size_t>(j) * n + i] = v;
        continue;
      }
    }
    const Unknown ui = unknownOf(i, Bt), uj = unknownOf(j, Bt);  // uj.frame <= ui.frame
    const double *S = p.Spair + 36 * static_cast<size_t>(pairIndex(p.F, uj.frame, ui.frame));
    const double *H = p.Hpp + 36 * static_cast<size_t>(ui.frame);
    double hp = 0.0, sc = 0.0;
    for (int a = 0; a < ui.count; ++a)
      for (int b = 0; b < uj.count; ++b) {
        const double w = ui.coef[a] * uj.coef[b];
        sc += w * S[6 * (uj.first + b) + (ui.first + a)];
        if (ui.frame == uj.frame) hp += w * H[6 * (ui.first + a) + (uj.first + b)];
      }
    const double v = (hp - sc) + (i == j ? lambda * hp : 0.0);
    s_L[e] = v;
    p.sysH[static_cast<size_t>(i) * n + j] = v;
    p.sysH[static_cast<size_t>(j) * n + i] = v;
  }
  for (int i = tid; i < n; i += kBlock) {
    if constexpr (CAM) {
      if (i >= npose) {
        const int a = p.cidx[i - npose];
        const double g = p.camsum[15 + a] - p.camsum[35 + a];
        s_L[packed(n, i)] = -g;
        p.sysb[i] = -g;
        continue;
      }
    }
    const Unknown u = unknownOf(i, Bt);
    double g = 0.0;
    for (int a = 0; a < u.count; ++a) g += u.coef[a] * (p.bp[6 * u.frame + u.first + a] - p.rs[6 * u.frame + u.first + a]);
    s_L[packed(n, i)] = -g;
    p.sysb[i] = -g;
  }
  __syncthreads();
  // Cholesky of the system bordered by its right-hand side (row n leaves as y of L y = g), column by column: a pivot that is <= 0 or not
  // finite fails the step.  The diagonal stays as it is and its root goes to s_x, so a column needs two barriers.
  for (int k = 0; k < n; ++k) {
    const double d = s_L[packed(k, k)];
    if (!(d > 0.0) || !(d <= DBL_MAX)) {
      if (tid == 0) s_fail = 1;
      break;  // (uniform: every thread reads the same pivot)
    }
    const double root = sqrt(d);
    if (tid == 0) s_x[k] = root;
    for (int i = k + 1 + tid; i <= n; i += kBlock) s_L[packed(i, k)] = s_L[packed(i, k)] / root;
    __syncthreads();
    // the trailing update on a 16 x 16 grid of threads: rows i, columns j <= i (row n stops at column n - 1)
    for (int i = k + 1 + (tid >> 4); i <= n; i += 16) {
      const double lik = s_L[packed(i, k)];
      const int last = i < n ? i : n - 1;
      for (int j = k + 1 + (tid & 15); j <= last; j += 16) s_L[packed(i, j)] -= lik * s_L[packed(j, k)];
    }
    __syncthreads();
  }
  __syncthreads();
  const bool failed = s_fail != 0;
  if (!failed) {
    for (int k = n - 1; k >= 0; --k) {  // L^T x = y, y in row n; s_x[k] turns from the pivot's root into x_k
      const double x = s_L[packed(n, k)] / s_x[k];
      __syncthreads();
      for (int i = tid; i <= k; i += kBlock) {
        if (i == k)
          s_x[k] = x;
        else
          s_L[packed(n, i)] -= s_L[packed(k, i)] * x;
      }
      __syncthreads();
    }
  } else {
    __syncthreads();
    for (int i = tid; i < n; i += kBlock) s_x[i] = 0.0;
    __syncthreads();
  }
  for (int i = tid; i < n; i += kBlock) p.sysx[i] = s_x[i];
  // the six-component steps and the candidate poses, a thread per frame
  if (tid < p.F) {
    const int f = tid;
    const double *T = p.poses + 12 * static_cast<size_t>(f);
    double *Tc = p.cand_poses + 12 * static_cast<size_t>(f);
    double d6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (f == 0 || failed || npose == 0) {
#pragma unroll
      for (int k = 0; k < 12; ++k) Tc[k] = T[k];
    } else if (f == 1) {
      const double al = s_x[0], be = s_x[1];
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        d6[r] = Bt[r][0] * al + Bt[r][1] * be;
        d6[3 + r] = s_x[2 + r];
      }
      const double w6[6] = {0.0, 0.0, 0.0, d6[3], d6[4], d6[5]};
      const Rigid E = rigidExp(w6);
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) Tc[3 * r + c] = T[3 * r] * E.R[c] + T[3 * r + 1] * E.R[3 + c] + T[3 * r + 2] * E.R[6 + c];
      // the retraction: t' = |t_1| normalize(d + alpha b1 + beta b2)
      const double tn = sqrt(T[9] * T[9] + T[10] * T[10] + T[11] * T[11]);
      double v[3];
#pragma unroll
      for (int r = 0; r < 3; ++r) v[r] = T[9 + r] / tn + al * s_basis[r] + be * s_basis[3 + r];
      const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
      for (int r = 0; r < 3; ++r) Tc[9 + r] = p.norm1 * (v[r] / vn);
    } else {
#pragma unroll
      for (int k = 0; k < 6; ++k) d6[k] = s_x[5 + 6 * (f - 2) + k];
      const Rigid E = rigidExp(d6);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
#pragma unroll
        for (int c = 0; c < 3; ++c) Tc[3 * r + c] = T[3 * r] * E.R[c] + T[3 * r + 1] * E.R[3 + c] + T[3 * r + 2] * E.R[6 + c];
        Tc[9 + r] = T[3 * r] * E.t[0] + T[3 * r + 1] * E.t[1] + T[3 * r + 2] * E.t[2] + T[9 + r];
      }
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) p.delta6[6 * static_cast<size_t>(f) + k] = d6[k];
  }
  if (tid == 0) {
    double step = 0.0, state = 0.0;
    for (int i = 0; i < n; ++i) step += s_x[i] * s_x[i];  // (the camera's step is among them)
    for (int f = 1; f < p.F && npose > 0; ++f) {
      const double *t = p.poses + 12 * static_cast<size_t>(f) + 9;
      state += t[0] * t[0] + t[1] * t[1] + t[2] * t[2] + 1.0;
    }
    bool camera_failed = false;
    if constexpr (CAM) {
      // the candidate camera c + delta_c, its radius, and the rule that fails the step
      double dc[kCam] = {0.0, 0.0, 0.0, 0.0, 0.0}, c[kCam];
      for (int k = 0; k < p.ncam; ++k) {
        dc[p.cidx[k]] = s_x[npose + k];
        state += p.camrec[p.cidx[k]] * p.camrec[p.cidx[k]];
      }
      for (int k = 0; k < kCam; ++k) {
        c[k] = p.camrec[k] + dc[k];
        p.deltac[k] = dc[k];
        p.camrec[8 + k] = c[k];
        if (!(fabs(c[k]) <= DBL_MAX)) camera_failed = true;
      }
      double radius = 0.0;
      if (p.model == DSOPP_HIP_GEOMETRIC_BA_PINHOLE) {
        if (!(c[0] > 0.0) || !(c[1] > 0.0)) camera_failed = true;
      } else {
        if (!(c[0] > 0.0)) camera_failed = true;
        radius = radial::maxValidRadius(p.width, p.height, c[0], c[1], c[2], c[3], c[4]);
        if (!(radius > 0.0) || !(radius <= DBL_MAX)) camera_failed = true;
      }
      p.camrec[13] = radius;
    }
    GbaState &s = *p.st;
    s.step_sq = step;
    s.state_sq = state;
    s.system_lambda = lambda;
    s.solve_failed = failed || camera_failed ? 1 : 0;
  }
}

// ---------------------------------------------------------------------------------------------------------------- update

template <bool CAM>
__global__ void __launch_bounds__(kBlock) gbaUpdate(const GbaParams p) {
  if (p.st->done) return;
  const int l = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (l >= p.L) return;
  const double lambda = p.st->lambda;
  const double X[3] = {p.X[3 * static_cast<size_t>(l)], p.X[3 * static_cast<size_t>(l) + 1], p.X[3 * static_cast<size_t>(l) + 2]};
  double Li[6], d[3] = {0.0, 0.0, 0.0};
  Camera cam;
  bool moves = true;  // fixed landmarks take no step
  if constexpr (CAM) {
    cam = loadCamera(p, true);
    moves = !(p.fixed & kFixLandmarks);
  }
  if (moves && landmarkFactor(p.Hll + 6 * static_cast<size_t>(l), lambda, Li)) {
    // delta_l = -(H_ll + lambda D)^-1 (b_l + sum_f W_f^T delta_f), W_f^T delta_f = C (upsilon + omega x X)
    double v[3] = {p.bl[3 * static_cast<size_t>(l)], p.bl[3 * static_cast<size_t>(l) + 1], p.bl[3 * static_cast<size_t>(l) + 2]};
    for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
      const double *d6 = p.delta6 + 6 * static_cast<size_t>(p.ofr[o]);
      const double u[3] = {d6[0] + (d6[4] * X[2] - d6[5] * X[1]), d6[1] + (d6[5] * X[0] - d6[3] * X[2]), d6[2] + (d6[3] * X[1] - d6[4] * X[0])};
      double C[3][3];
      loadSym(p.C + 9 * static_cast<size_t>(o), C);
#pragma unroll
      for (int r = 0; r < 3; ++r) v[r] += C[r][0] * u[0] + C[r][1] * u[1] + C[r][2] * u[2];
    }
    if (CAM && p.ncam > 0) {
      // + W_lc delta_c, W_lc the landmark's sum as the reducers take it
      double W[3][kCam];
      landmarkCameraBlock(p, l, W);
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double t = 0.0;
#pragma unroll
        for (int a = 0; a < kCam; ++a) t += W[r][a] * p.deltac[a];
        v[r] += t;
      }
    }
    double y[3];
    lowerApply(Li, v, y);
    d[0] = -(Li[0] * y[0] + Li[1] * y[1] + Li[3] * y[2]);
    d[1] = -(Li[2] * y[1] + Li[4] * y[2]);
    d[2] = -(Li[5] * y[2]);
  }
  const double Xc[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
  double cost = 0.0;
  int nv = 0;
  for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
    const double obs[2] = {p.oxy[2 * static_cast<size_t>(o)], p.oxy[2 * static_cast<size_t>(o) + 1]};
    double r[2], pc[3];
    if (residualOf<CAM>(p.cand_poses + 12 * static_cast<size_t>(p.ofr[o]), Xc, obs, p, cam, r, pc)) {
      double w, rho;
      huber(r[0] * r[0] + r[1] * r[1], p.a, w, rho);
      cost += rho;
      ++nv;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) p.candX[3 * static_cast<size_t>(l) + k] = Xc[k];
  p.lm[4 * static_cast<size_t>(l) + 1] = cost;
  p.lm[4 * static_cast<size_t>(l) + 2] = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
  p.lm[4 * static_cast<size_t>(l) + 3] = moves ? X[0] * X[0] + X[1] * X[1] + X[2] * X[2] : 0.0;  // fixed landmarks: no part in the state norm
  p.lmn[2 * static_cast<size_t>(l) + 1] = nv;
}

// ---------------------------------------------------------------------------------------------------------------- decide

template <bool CAM>
__global__ void __launch_bounds__(kBlock) gbaDecide(const GbaParams p) {
  __shared__ double s_wave[kBlock / 64];
  __shared__ int s_accept;
  if (p.st->done) return;
  double cost = 0.0, step = 0.0, state = 0.0, nv = 0.0;
  for (int l = threadIdx.x; l < p.L; l += kBlock) {
    cost += p.lm[4 * static_cast<size_t>(l) + 1];
    step += p.lm[4 * static_cast<size_t>(l) + 2];
    state += p.lm[4 * static_cast<size_t>(l) + 3];
    nv += static_cast<double>(p.lmn[2 * static_cast<size_t>(l) + 1]);
  }
  cost = blockSum(cost, s_wave);
  step = blockSum(step, s_wave);
  state = blockSum(state, s_wave);
  nv = blockSum(nv, s_wave);
  if (threadIdx.x == 0) {
    GbaState &s = *p.st;
    const double E = s.cost, En = s.solve_failed ? HUGE_VAL : 0.5 * cost;
    const int nvn = s.solve_failed ? s.nvalid : static_cast<int>(nv);
    int accept = 0;
    dsopp_hip_geometric_ba_trace &tr = p.trace[s.it];
    tr.cost_before = E;
    tr.cost_candidate = En;
    tr.lambda = s.lambda;
    s.cand_cost = En;
    s.cand_nvalid = nvn;
    if (nvn == 0) {
      s.done = 1;
      s.reason = DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL;
    } else {
      int reason = 0;
      if (!s.solve_failed && fabs(E - En) / E < p.ftol) reason |= DSOPP_HIP_GEOMETRIC_BA_FUNCTION_TOLERANCE;
      if (En < E) {
        accept = 1;
        if (s.step_sq + step < p.ptol * (s.state_sq + state + p.ptol)) reason |= DSOPP_HIP_GEOMETRIC_BA_PARAMETER_TOLERANCE;
        s.cost = En;
        s.nvalid = nvn;
        s.lambda = s.lambda / p.dec;
        s.relin = 1;
        ++s.accepted;
      } else {
        s.lambda = s.lambda * p.inc;
        s.relin = 0;
      }
      if (reason) {
        s.reason = reason;
        s.done = 1;
      }
    }
    tr.accepted = accept;
    tr.reserved = 0;
    ++s.it;
    if (s.it >= p.max_it) s.done = 1;
    s_accept = accept;
  }
  __syncthreads();
  if (!s_accept) return;
  for (int k = threadIdx.x; k < 3 * p.L; k += kBlock) p.X[k] = p.candX[k];
  for (int k = threadIdx.x; k < 12 * p.F; k += kBlock) p.poses[k] = p.cand_poses[k];
  if constexpr (CAM) {
    if (threadIdx.x < 6) p.camrec[threadIdx.x] = p.camrec[8 + threadIdx.x];  // the intrinsics and their radius
  }
}

// ---------------------------------------------------------------------------------------------------------------- pruning, triangulation

__global__ void __launch_bounds__(kBlock) gbaFlagOutliers(const GbaParams p, double threshold, uint8_t *flags) {
  const int l = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (l >= p.L) return;
  const double X[3] = {p.X[3 * static_cast<size_t>(l)], p.X[3 * static_cast<size_t>(l) + 1], p.X[3 * static_cast<size_t>(l) + 2]};
  for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
    const double obs[2] = {p.oxy[2 * static_cast<size_t>(o)], p.oxy[2 * static_cast<size_t>(o) + 1]};
    double r[2], pc[3];
    const bool ok = residualOf<false>(p.poses + 12 * static_cast<size_t>(p.ofr[o]), X, obs, p, Camera(), r, pc);
    flags[o] = (!ok || sqrt(r[0] * r[0] + r[1] * r[1]) > threshold) ? 1 : 0;
  }
}

__global__ void __launch_bounds__(kBlock) gbaTriangulate(const GbaParams p, const uint8_t *has_position, int min_projections, int retriangulation,
                                                         uint8_t *triangulated) {
  const int l = static_cast<int>(blockIdx.x) * kBlock + threadIdx.x;
  if (l >= p.L) return;
  const int count = p.off[l + 1] - p.off[l];
  const bool run = (retriangulation || !has_position[l]) && count > min_projections;
  triangulated[l] = run ? 1 : 0;
  if (!run) return;
  double A[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) A[r][c] = 0.0;
  for (int o = p.off[l]; o < p.off[l + 1]; ++o) {
    const double *T = p.poses + 12 * static_cast<size_t>(p.ofr[o]);
    double v[3] = {(p.oxy[2 * static_cast<size_t>(o)] - p.cx) / p.fx, (p.oxy[2 * static_cast<size_t>(o) + 1] - p.cy) / p.fy, 1.0};
    const double vn = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] /= vn;
    double P[3][4], u[4], Ai[3][4];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      P[r][0] = T[3 * r];
      P[r][1] = T[3 * r + 1];
      P[r][2] = T[3 * r + 2];
      P[r][3] = T[9 + r];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) u[c] = v[0] * P[0][c] + v[1] * P[1][c] + v[2] * P[2][c];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) Ai[r][c] = P[r][c] - v[r] * u[c];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int c = 0; c < 4; ++c) A[r][c] += Ai[0][r] * Ai[0][c] + Ai[1][r] * Ai[1][c] + Ai[2][r] * Ai[2][c];
  }
  // cyclic Jacobi on the symmetric 4 x 4: A <- G^T A G, V <- V G
  double V[4][4], frob = 0.0;
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      V[r][c] = r == c ? 1.0 : 0.0;
      frob += A[r][c] * A[r][c];
    }
  const double tiny = 1e-18 * sqrt(frob);
  for (int sweep = 0; sweep < kJacobiSweeps; ++sweep) {
    bool rotated = false;
#pragma unroll
    for (int pi = 0; pi < 3; ++pi)
#pragma unroll
      for (int qi = pi + 1; qi < 4; ++qi) {
        const double apq = A[pi][qi];
        if (fabs(apq) > tiny) {
          rotated = true;
          const double theta = (A[qi][qi] - A[pi][pi]) / (2.0 * apq);
          const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
          const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
          A[pi][pi] -= t * apq;
          A[qi][qi] += t * apq;
          A[pi][qi] = A[qi][pi] = 0.0;
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            if (k != pi && k != qi) {
              const double akp = A[k][pi], akq = A[k][qi];
              A[k][pi] = A[pi][k] = c * akp - s * akq;
              A[k][qi] = A[qi][k] = s * akp + c * akq;
            }
            const double vkp = V[k][pi], vkq = V[k][qi];
            V[k][pi] = c * vkp - s * vkq;
            V[k][qi] = s * vkp + c * vkq;
          }
        }
      }
    if (!rotated) break;
  }
  int best = 0;
  double least = A[0][0];
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (A[k][k] < least) {
      least = A[k][k];
      best = k;
    }
  double e[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
  for (int k = 1; k < 4; ++k)
    if (best == k) {
      e[0] = V[0][k];
      e[1] = V[1][k];
      e[2] = V[2][k];
      e[3] = V[3][k];
    }
#pragma unroll
  for (int k = 0; k < 3; ++k) p.candX[3 * static_cast<size_t>(l) + k] = e[k] / e[3];
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_geometric_ba {
  dsopp_hip::StreamRef sr;
  dsopp_hip::Event done;
  // one device block and one pinned mirror, laid out by GbaLayout; they grow geometrically
  dsopp_hip::DeviceMem<uint8_t> d_buf;
  dsopp_hip::PinnedMem<uint8_t> h_buf;
  size_t capacity = 0;
};

namespace dsopp_hip {
namespace {

size_t aligned(size_t bytes) { return (bytes + 255) & ~static_cast<size_t>(255); }

/** the device block; the host uploads [0, upload_end) and reads back what a call hands out, at the same offsets of the pinned mirror */
struct GbaLayout {
  size_t state, poses, X, oxy, off, ofr, has, upload_end;
  size_t cand_poses, candX, C, res, wgt, valid, Hll, bl, lm, lmn, Spair, Hpp, bp, rs, delta6, sysH, sysb, sysx, trace, flags, bytes;
  size_t camrec, Jc, Wc, Hpc, Sfc, camsum, deltac;  // the camera block: sized only for the *_camera calls
  GbaLayout(size_t F, size_t L, size_t M, size_t max_it, bool camera = false) {
    size_t at = 0;
    auto take = [&](size_t bytes) {
      const size_t here = at;
      at += aligned(bytes);
      return here;
    };
    const size_t n = 6 * (F > 1 ? F - 1 : 1) + (camera ? kCam : 0), pairs = F * (F + 1) / 2;
    state = take(sizeof(GbaState));
    poses = take(96 * F);
    X = take(24 * L);
    oxy = take(16 * M);
    off = take(4 * (L + 1));
    ofr = take(4 * M);
    has = take(L);
    camrec = take(camera ? 8 * 16 : 0);
    upload_end = at;
    cand_poses = take(96 * F);
    candX = take(24 * L);
    C = take(72 * M);
    res = take(16 * M);
    wgt = take(8 * M);
    valid = take(M);
    Hll = take(48 * L);
    bl = take(24 * L);
    lm = take(32 * L);
    lmn = take(8 * L);
    Spair = take(288 * pairs);
    Hpp = take(288 * F);
    bp = take(48 * F);
    rs = take(48 * F);
    delta6 = take(48 * F);
    sysH = take(8 * n * n);
    sysb = take(8 * n);
    sysx = take(8 * n);
    trace = take(sizeof(dsopp_hip_geometric_ba_trace) * (max_it > 0 ? max_it : 1));
    flags = take(M > L ? M : L);
    Jc = take(camera ? 8 * 2 * kCam * M : 0);
    Wc = take(camera ? 8 * 3 * kCam * M : 0);
    Hpc = take(camera ? 8 * 6 * kCam * F : 0);
    Sfc = take(camera ? 8 * 6 * kCam * F : 0);
    camsum = take(camera ? 8 * 40 : 0);
    deltac = take(camera ? 8 * kCam : 0);
    bytes = at;
  }
};

bool finiteAll(const double *v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(v[i])) return false;
  return true;
}

/** the checks every call shares; positions are checked by the calls that read them */
void validate(const dsopp_hip_geometric_ba *h, const dsopp_hip_geometric_ba_problem *pr, int min_frames, bool own_camera = true) {
  if (!h) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null geometric ba");
  if (!pr) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (pr->num_frames > kMaxFrames) fail(DSOPP_HIP_ERR_CAPACITY, "%d frames: the object takes %d", pr->num_frames, kMaxFrames);
  if (pr->num_frames < min_frames) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d frames: the call needs %d", pr->num_frames, min_frames);
  if (pr->num_landmarks < 0 || pr->num_landmarks > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d landmarks", pr->num_landmarks);
  if (pr->num_observations < 0 || pr->num_observations > (1 << 26)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d observations", pr->num_observations);
  if (pr->width < 9 || pr->height < 9) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a %d x %d image has no region of interest", pr->width, pr->height);
  const double cam[4] = {pr->fx, pr->fy, pr->cx, pr->cy};
  if (own_camera && (!finiteAll(cam, 4) || pr->fx == 0.0 || pr->fy == 0.0)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the camera is not finite or has a zero focal length");
  if (!pr->poses || !pr->landmark_offsets) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const int L = pr->num_landmarks, M = pr->num_observations, F = pr->num_frames;
  if ((L > 0 && !pr->positions) || (M > 0 && (!pr->obs_frame || !pr->obs_xy))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!finiteAll(pr->poses, 12 * static_cast<size_t>(F))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a pose is not finite");
  if (M > 0 && !finiteAll(pr->obs_xy, 2 * static_cast<size_t>(M))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an observation is not finite");
  if (pr->landmark_offsets[0] != 0 || pr->landmark_offsets[L] != M) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the offsets do not span the observations");
  for (int l = 0; l < L; ++l) {
    const int from = pr->landmark_offsets[l], to = pr->landmark_offsets[l + 1];
    if (to < from || to > M) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the offsets of landmark %d descend", l);
    unsigned seen = 0;
    for (int o = from; o < to; ++o) {
      const int f = pr->obs_frame[o];
      if (f < 0 || f >= F) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "observation %d names frame %d of %d", o, f, F);
      if (seen & (1u << f)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "landmark %d is observed twice in frame %d", l, f);
      seen |= 1u << f;
    }
  }
}

struct Call {
  dsopp_hip_geometric_ba *h;
  GbaLayout lay;
  GbaParams p;
  uint8_t *host, *dev;
  hipStream_t st;
  size_t F, L, M;
};

/** grows the block, fills the pinned mirror's upload region and enqueues the upload */
Call begin(dsopp_hip_geometric_ba *h, const dsopp_hip_geometric_ba_problem *pr, int max_it, const uint8_t *has_position, bool camera = false) {
  h->sr.use();
  const size_t F = static_cast<size_t>(pr->num_frames), L = static_cast<size_t>(pr->num_landmarks), M = static_cast<size_t>(pr->num_observations);
  Call c{h, GbaLayout(F, L, M, static_cast<size_t>(max_it > 0 ? max_it : 0), camera), GbaParams(), nullptr, nullptr, h->sr.stream, F, L, M};
  const GbaLayout &lay = c.lay;
  if (h->capacity < lay.bytes) {
    size_t cap = h->capacity ? h->capacity : 65536;
    while (cap < lay.bytes) cap *= 2;
    h->capacity = 0;
    h->d_buf.alloc(cap);
    h->h_buf.reserve(cap);
    h->capacity = cap;
  }
  c.host = h->h_buf.get();
  c.dev = h->d_buf.get();
  std::memset(c.host, 0, lay.upload_end);
  std::memcpy(c.host + lay.poses, pr->poses, 96 * F);
  if (L) std::memcpy(c.host + lay.X, pr->positions, 24 * L);
  if (M) std::memcpy(c.host + lay.oxy, pr->obs_xy, 16 * M);
  std::memcpy(c.host + lay.off, pr->landmark_offsets, 4 * (L + 1));
  if (M) std::memcpy(c.host + lay.ofr, pr->obs_frame, 4 * M);
  if (has_position && L) std::memcpy(c.host + lay.has, has_position, L);
  GbaParams &p = c.p;
  p.fx = pr->fx;
  p.fy = pr->fy;
  p.cx = pr->cx;
  p.cy = pr->cy;
  p.xmax = static_cast<double>(pr->width) - 5.0;
  p.ymax = static_cast<double>(pr->height) - 5.0;
  p.a = 1.5;
  p.ftol = p.ptol = 0.0;
  p.dec = p.inc = 1.0;
  p.norm1 = 1.0;
  p.F = pr->num_frames;
  p.L = pr->num_landmarks;
  p.M = pr->num_observations;
  p.max_it = max_it;
  uint8_t *d = c.dev;
  p.st = reinterpret_cast<GbaState *>(d + lay.state);
  p.poses = reinterpret_cast<double *>(d + lay.poses);
  p.X = reinterpret_cast<double *>(d + lay.X);
  p.oxy = reinterpret_cast<const double *>(d + lay.oxy);
  p.off = reinterpret_cast<const int *>(d + lay.off);
  p.ofr = reinterpret_cast<const int *>(d + lay.ofr);
  p.cand_poses = reinterpret_cast<double *>(d + lay.cand_poses);
  p.candX = reinterpret_cast<double *>(d + lay.candX);
  p.C = reinterpret_cast<double *>(d + lay.C);
  p.res = reinterpret_cast<double *>(d + lay.res);
  p.wgt = reinterpret_cast<double *>(d + lay.wgt);
  p.valid = d + lay.valid;
  p.Hll = reinterpret_cast<double *>(d + lay.Hll);
  p.bl = reinterpret_cast<double *>(d + lay.bl);
  p.lm = reinterpret_cast<double *>(d + lay.lm);
  p.lmn = reinterpret_cast<int *>(d + lay.lmn);
  p.Spair = reinterpret_cast<double *>(d + lay.Spair);
  p.Hpp = reinterpret_cast<double *>(d + lay.Hpp);
  p.bp = reinterpret_cast<double *>(d + lay.bp);
  p.rs = reinterpret_cast<double *>(d + lay.rs);
  p.delta6 = reinterpret_cast<double *>(d + lay.delta6);
  p.sysH = reinterpret_cast<double *>(d + lay.sysH);
  p.sysb = reinterpret_cast<double *>(d + lay.sysb);
  p.sysx = reinterpret_cast<double *>(d + lay.sysx);
  p.trace = reinterpret_cast<dsopp_hip_geometric_ba_trace *>(d + lay.trace);
  p.model = p.fixed = p.npose = p.ncam = 0;
  for (int &i : p.cidx) i = 0;
  p.width = static_cast<double>(pr->width);
  p.height = static_cast<double>(pr->height);
  p.camrec = reinterpret_cast<double *>(d + lay.camrec);
  p.Jc = reinterpret_cast<double *>(d + lay.Jc);
  p.Wc = reinterpret_cast<double *>(d + lay.Wc);
  p.Hpc = reinterpret_cast<double *>(d + lay.Hpc);
  p.Sfc = reinterpret_cast<double *>(d + lay.Sfc);
  p.camsum = reinterpret_cast<double *>(d + lay.camsum);
  p.deltac = reinterpret_cast<double *>(d + lay.deltac);
  return c;
}

void upload(Call &c) { HIP_CHECK(hipMemcpyAsync(c.dev, c.host, c.lay.upload_end, hipMemcpyHostToDevice, c.st)); }

void fetch(Call &c, size_t offset, size_t bytes) {
  if (bytes) HIP_CHECK(hipMemcpyAsync(c.host + offset, c.dev + offset, bytes, hipMemcpyDeviceToHost, c.st));
}

void wait(Call &c) {
  HIP_CHECK(hipEventRecord(c.h->done.get(hipEventDisableTiming), c.st));
  HIP_CHECK(hipEventSynchronize(c.h->done.h));
}

unsigned blocksFor(size_t n) { return static_cast<unsigned>((n + kBlock - 1) / kBlock); }

void requireFinitePositions(const dsopp_hip_geometric_ba_problem *pr) {
  if (pr->num_landmarks > 0 && !finiteAll(pr->positions, 3 * static_cast<size_t>(pr->num_landmarks)))
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a landmark position is not finite");
}

/** the camera of a *_camera call after its checks: what the device record and the kernels' parameters take */
struct CameraSetup {
  int model, fixed, ncam, cidx[kCam];
  double c[kCam], radius;
};

CameraSetup checkCamera(const dsopp_hip_geometric_ba_problem *pr, const dsopp_hip_geometric_ba_camera *cam) {
  if (!cam) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null camera");
  if (cam->model != DSOPP_HIP_GEOMETRIC_BA_PINHOLE && cam->model != DSOPP_HIP_GEOMETRIC_BA_SIMPLE_RADIAL)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "unknown camera model %d", cam->model);
  const int known = DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL | DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER | DSOPP_HIP_GEOMETRIC_BA_FIX_MODEL_SPECIFIC | kFixPoses | kFixLandmarks;
  if (cam->fixed & ~known) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "unknown fixed bits %d", cam->fixed);
  const bool radial = cam->model == DSOPP_HIP_GEOMETRIC_BA_SIMPLE_RADIAL;
  const int count = radial ? 5 : 4;
  CameraSetup cs{};
  cs.model = cam->model;
  cs.fixed = cam->fixed;
  for (int k = 0; k < count; ++k) cs.c[k] = cam->intrinsics[k];
  if (!finiteAll(cs.c, static_cast<size_t>(count))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an intrinsic is not finite");
  if (!(cs.c[0] > 0.0) || (!radial && !(cs.c[1] > 0.0))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a focal length is not positive");
  if (radial) {
    cs.radius = radial::maxValidRadius(static_cast<double>(pr->width), static_cast<double>(pr->height), cs.c[0], cs.c[1], cs.c[2], cs.c[3], cs.c[4]);
    if (!(cs.radius > 0.0) || !std::isfinite(cs.radius)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the camera's max_valid_radius is %g", cs.radius);
  }
  // constantParameterSet: focal, centre, model-specific
  const int group_pinhole[4] = {DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL, DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL, DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER,
                                DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER};
  const int group_radial[5] = {DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL, DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER, DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER,
                               DSOPP_HIP_GEOMETRIC_BA_FIX_MODEL_SPECIFIC, DSOPP_HIP_GEOMETRIC_BA_FIX_MODEL_SPECIFIC};
  for (int k = 0; k < count; ++k)
    if (!(cam->fixed & (radial ? group_radial[k] : group_pinhole[k]))) cs.cidx[cs.ncam++] = k;
  return cs;
}

void installCamera(Call &c, const CameraSetup &cs) {
  GbaParams &p = c.p;
  p.model = cs.model;
  p.fixed = cs.fixed;
  p.npose = (cs.fixed & kFixPoses) ? 0 : 6 * (p.F - 1) - 1;
  p.ncam = cs.ncam;
  for (int k = 0; k < kCam; ++k) p.cidx[k] = cs.cidx[k];
  double *rec = reinterpret_cast<double *>(c.host + c.lay.camrec);
  for (int half = 0; half < 2; ++half) {
    for (int k = 0; k < kCam; ++k) rec[8 * half + k] = cs.c[k];
    rec[8 * half + 5] = cs.radius;
  }
}

template <bool CAM>
void evaluate(dsopp_hip_geometric_ba *h, const dsopp_hip_geometric_ba_problem *pr, dsopp_hip_geometric_ba_camera *camera, double a, double *cost,
              int32_t *valid_residuals, uint8_t *obs_valid, double *obs_residual, double *obs_weight) {
  validate(h, pr, 1, !CAM);
  requireFinitePositions(pr);
  CameraSetup cs{};
  if constexpr (CAM) {
    cs = checkCamera(pr, camera);
    camera->max_valid_radius = cs.radius;
  }
  if (!cost || !valid_residuals) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (!(a > 0.0) || !std::isfinite(a)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the Huber width must be positive and finite");
  *cost = 0.0;
  *valid_residuals = 0;
  if (pr->num_observations == 0) return;
  Call c = begin(h, pr, 0, nullptr, CAM);
  c.p.a = a;
  if constexpr (CAM) installCamera(c, cs);
  reinterpret_cast<GbaState *>(c.host + c.lay.state)->relin = 1;
  upload(c);
  gbaLinearise<CAM><<<blocksFor(c.L), kBlock, 0, c.st>>>(c.p);
  HIP_CHECK(hipGetLastError());
  gbaInitialCost<<<1, kBlock, 0, c.st>>>(c.p);
  HIP_CHECK(hipGetLastError());
  fetch(c, c.lay.state, sizeof(GbaState));
  if (obs_valid) fetch(c, c.lay.valid, c.M);
  if (obs_residual) fetch(c, c.lay.res, 16 * c.M);
  if (obs_weight) fetch(c, c.lay.wgt, 8 * c.M);
  wait(c);
  const GbaState *s = reinterpret_cast<const GbaState *>(c.host + c.lay.state);
  *cost = s->cost;
  *valid_residuals = s->nvalid;
  if (obs_valid) std::memcpy(obs_valid, c.host + c.lay.valid, c.M);
  if (obs_residual) std::memcpy(obs_residual, c.host + c.lay.res, 16 * c.M);
  if (obs_weight) std::memcpy(obs_weight, c.host + c.lay.wgt, 8 * c.M);
}

template <bool CAM>
void solve(dsopp_hip_geometric_ba *h, dsopp_hip_geometric_ba_problem *pr, dsopp_hip_geometric_ba_camera *camera,
           const dsopp_hip_geometric_ba_options *opt, dsopp_hip_geometric_ba_result *result, const dsopp_hip_geometric_ba_debug *dbg,
           const dsopp_hip_geometric_ba_camera_debug *cdbg) {
  validate(h, pr, 2, !CAM);
  requireFinitePositions(pr);
  CameraSetup cs{};
  bool poses_free = true;
  if constexpr (CAM) {
    cs = checkCamera(pr, camera);
    poses_free = !(cs.fixed & kFixPoses);
    if (!poses_free && (cs.fixed & kFixLandmarks) && cs.ncam == 0)
      fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "nothing is free: poses, landmarks and every intrinsic are fixed");
    camera->max_valid_radius = cs.radius;
  }
  if (!opt || !result) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const double o[6] = {opt->a, opt->lambda_0, opt->function_tolerance, opt->parameter_tolerance, opt->decrease_factor, opt->increase_factor};
  if (!finiteAll(o, 6) || !(opt->a > 0.0) || !(opt->lambda_0 >= 0.0) || !(opt->decrease_factor > 0.0) || !(opt->increase_factor > 0.0))
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an option is not finite or not positive");
  if (opt->max_iterations < 0 || opt->max_iterations > (1 << 16)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d iterations", opt->max_iterations);
  if (opt->iteration_group < 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an iteration group of %d", opt->iteration_group);
  const double *t1 = pr->poses + 12 + 9;
  const double norm1 = std::sqrt(t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]);
  if (poses_free && (!(norm1 > 0.0) || !std::isfinite(norm1))) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "frame 1 has no translation: its direction is not defined");
  std::memset(result, 0, sizeof(*result));
  result->final_lambda = opt->lambda_0;
  const int n = (poses_free ? 6 * (pr->num_frames - 1) - 1 : 0) + cs.ncam;
  if (pr->num_observations == 0) {
    // nothing is valid: the driver's loop does not start
    result->reason = DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL;
    return;
  }
  Call c = begin(h, pr, opt->max_iterations, nullptr, CAM);
  GbaParams &p = c.p;
  if constexpr (CAM) installCamera(c, cs);
  p.a = opt->a;
  p.ftol = opt->function_tolerance;
  p.ptol = opt->parameter_tolerance;
  p.dec = opt->decrease_factor;
  p.inc = opt->increase_factor;
  p.norm1 = norm1;
  GbaState *s = reinterpret_cast<GbaState *>(c.host + c.lay.state);
  s->lambda = s->system_lambda = opt->lambda_0;
  s->relin = 1;
  upload(c);
  gbaLinearise<CAM><<<blocksFor(c.L), kBlock, 0, c.st>>>(p);
  HIP_CHECK(hipGetLastError());
  gbaInitialCost<<<1, kBlock, 0, c.st>>>(p);
  HIP_CHECK(hipGetLastError());
  const int group = opt->iteration_group > 0 ? opt->iteration_group : kDefaultGroup;
  // the reducers: a workgroup per pair of free frames; with a camera block one per free frame and one for the camera behind them
  const unsigned frame_pairs = static_cast<unsigned>((pr->num_frames - 1) * pr->num_frames / 2);
  // (no free intrinsic: the camera's sums are not read, and with free poses its reducers are not launched)
  const unsigned camera_reducers = cs.ncam > 0 ? static_cast<unsigned>(pr->num_frames - 1) + 1u : 0u;
  const unsigned pairs = !CAM ? frame_pairs : poses_free ? frame_pairs + camera_reducers : 1u;
  for (int launched = 0; launched < opt->max_iterations;) {
    const int now = std::min(group, opt->max_iterations - launched);
    for (int k = 0; k < now; ++k) {
      gbaLinearise<CAM><<<blocksFor(c.L), kBlock, 0, c.st>>>(p);
      gbaReduce<CAM><<<pairs, kBlock, 0, c.st>>>(p);
      gbaSolve<CAM><<<1, kBlock, 0, c.st>>>(p);
      gbaUpdate<CAM><<<blocksFor(c.L), kBlock, 0, c.st>>>(p);
      gbaDecide<CAM><<<1, kBlock, 0, c.st>>>(p);
    }
    HIP_CHECK(hipGetLastError());
    launched += now;
    if (launched >= opt->max_iterations) break;  // (the closing read-back below covers the state)
    fetch(c, c.lay.state, sizeof(GbaState));
    wait(c);
    if (s->done) break;
  }
  const GbaLayout &lay = c.lay;
  fetch(c, lay.state, lay.oxy - lay.state);  // the state, the poses, the positions
  if (dbg) {
    if (dbg->obs_valid) fetch(c, lay.valid, c.M);
    if (dbg->obs_residual) fetch(c, lay.res, 16 * c.M);
    if (dbg->obs_weight) fetch(c, lay.wgt, 8 * c.M);
    if (dbg->landmark_H) fetch(c, lay.Hll, 48 * c.L);
    if (dbg->landmark_b) fetch(c, lay.bl, 24 * c.L);
    if (dbg->reduced_H) fetch(c, lay.sysH, 8 * static_cast<size_t>(n) * n);
    if (dbg->reduced_b) fetch(c, lay.sysb, 8 * static_cast<size_t>(n));
    if (dbg->pose_step) fetch(c, lay.sysx, 8 * static_cast<size_t>(n));
    if (dbg->candidate_poses) fetch(c, lay.cand_poses, 96 * c.F);
    if (dbg->candidate_positions) fetch(c, lay.candX, 24 * c.L);
    if (dbg->trace && opt->max_iterations > 0) fetch(c, lay.trace, sizeof(dsopp_hip_geometric_ba_trace) * static_cast<size_t>(opt->max_iterations));
  }
  if constexpr (CAM) {
    fetch(c, lay.camrec, 8 * 16);
    if (cdbg && cdbg->obs_camera_jacobian) fetch(c, lay.Jc, 8 * 2 * kCam * c.M);
  }
  wait(c);
  if (s->it < 0 || s->it > opt->max_iterations) fail(DSOPP_HIP_ERR_HIP, "the device returned %d iterations of %d", s->it, opt->max_iterations);
  result->initial_cost = s->initial_cost;
  result->final_cost = s->cost;
  result->final_lambda = s->lambda;
  result->valid_residuals = s->nvalid;
  result->iterations = s->it;
  result->accepted_steps = s->accepted;
  result->reason = s->reason;
  result->converged = (s->reason & (DSOPP_HIP_GEOMETRIC_BA_FUNCTION_TOLERANCE | DSOPP_HIP_GEOMETRIC_BA_PARAMETER_TOLERANCE)) ? 1 : 0;
  std::memcpy(pr->poses, c.host + lay.poses, 96 * c.F);
  if (c.L) std::memcpy(pr->positions, c.host + lay.X, 24 * c.L);
  if (dbg) {
    const bool ran = s->it > 0;  // the system, the step and the candidate exist once an iteration ran
    if (dbg->obs_valid) std::memcpy(dbg->obs_valid, c.host + lay.valid, c.M);
    if (dbg->obs_residual) std::memcpy(dbg->obs_residual, c.host + lay.res, 16 * c.M);
    if (dbg->obs_weight) std::memcpy(dbg->obs_weight, c.host + lay.wgt, 8 * c.M);
    if (dbg->landmark_H) std::memcpy(dbg->landmark_H, c.host + lay.Hll, 48 * c.L);
    if (dbg->landmark_b) std::memcpy(dbg->landmark_b, c.host + lay.bl, 24 * c.L);
    if (dbg->system_lambda) *dbg->system_lambda = s->system_lambda;
    if (dbg->reduced_H) ran ? std::memcpy(dbg->reduced_H, c.host + lay.sysH, 8 * static_cast<size_t>(n) * n) : std::memset(dbg->reduced_H, 0, 8 * static_cast<size_t>(n) * n);
    if (dbg->reduced_b) ran ? std::memcpy(dbg->reduced_b, c.host + lay.sysb, 8 * static_cast<size_t>(n)) : std::memset(dbg->reduced_b, 0, 8 * static_cast<size_t>(n));
    if (dbg->pose_step) ran ? std::memcpy(dbg->pose_step, c.host + lay.sysx, 8 * static_cast<size_t>(n)) : std::memset(dbg->pose_step, 0, 8 * static_cast<size_t>(n));
    if (dbg->candidate_poses) std::memcpy(dbg->candidate_poses, c.host + (ran ? lay.cand_poses : lay.poses), 96 * c.F);
    if (dbg->candidate_positions && c.L) std::memcpy(dbg->candidate_positions, c.host + (ran ? lay.candX : lay.X), 24 * c.L);
    if (dbg->trace && s->it > 0) std::memcpy(dbg->trace, c.host + lay.trace, sizeof(dsopp_hip_geometric_ba_trace) * static_cast<size_t>(s->it));
  }
  if constexpr (CAM) {
    const double *rec = reinterpret_cast<const double *>(c.host + lay.camrec);
    std::memcpy(camera->intrinsics, rec, 8 * static_cast<size_t>(cs.model == DSOPP_HIP_GEOMETRIC_BA_SIMPLE_RADIAL ? 5 : 4));
    camera->max_valid_radius = rec[5];
    if (cdbg) {
      const bool ran = s->it > 0;  // without an iteration the candidate is the state
      if (cdbg->obs_camera_jacobian) std::memcpy(cdbg->obs_camera_jacobian, c.host + lay.Jc, 8 * 2 * kCam * c.M);
      if (cdbg->candidate_intrinsics) std::memcpy(cdbg->candidate_intrinsics, rec + (ran ? 8 : 0), 8 * kCam);
      if (cdbg->candidate_max_valid_radius) *cdbg->candidate_max_valid_radius = rec[(ran ? 8 : 0) + 5];
    }
  }
}

void triangulate(dsopp_hip_geometric_ba *h, dsopp_hip_geometric_ba_problem *pr, const uint8_t *has_position, int min_projections, int retriangulation,
                 uint8_t *triangulated) {
  validate(h, pr, 1);
  if (pr->num_landmarks > 0 && (!has_position || !triangulated)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (min_projections < 2) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "min_number_of_projections %d: the reference requires 2", min_projections);
  if (pr->num_landmarks == 0) return;
  Call c = begin(h, pr, 0, has_position);
  upload(c);
  uint8_t *flags = c.dev + c.lay.flags;
  gbaTriangulate<<<blocksFor(c.L), kBlock, 0, c.st>>>(c.p, c.dev + c.lay.has, min_projections, retriangulation, flags);
  HIP_CHECK(hipGetLastError());
  fetch(c, c.lay.flags, c.L);
  fetch(c, c.lay.candX, 24 * c.L);
  wait(c);
  std::memcpy(triangulated, c.host + c.lay.flags, c.L);
  const double *X = reinterpret_cast<const double *>(c.host + c.lay.candX);
  for (size_t l = 0; l < c.L; ++l)
    if (triangulated[l]) std::memcpy(pr->positions + 3 * l, X + 3 * l, 24);
}

void flagOutliers(dsopp_hip_geometric_ba *h, const dsopp_hip_geometric_ba_problem *pr, double threshold, uint8_t *flags, int32_t *count) {
  validate(h, pr, 1);
  requireFinitePositions(pr);
  if (threshold != threshold) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the threshold is not a number");
  if (pr->num_observations > 0 && !flags) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (count) *count = 0;
  if (pr->num_observations == 0) return;
  Call c = begin(h, pr, 0, nullptr);
  upload(c);
  gbaFlagOutliers<<<blocksFor(c.L), kBlock, 0, c.st>>>(c.p, threshold, c.dev + c.lay.flags);
  HIP_CHECK(hipGetLastError());
  fetch(c, c.lay.flags, c.M);
  wait(c);
  std::memcpy(flags, c.host + c.lay.flags, c.M);
  if (count) {
    int32_t total = 0;
    for (size_t o = 0; o < c.M; ++o) total += flags[o] ? 1 : 0;
    *count = total;
  }
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

void dsopp_hip_geometric_ba_default_options(dsopp_hip_geometric_ba_options *options) {
  if (!options) return;
  options->a = 1.5;
  options->lambda_0 = 1e-4;
  options->function_tolerance = 1e-10;
  options->parameter_tolerance = 1e-10;
  options->decrease_factor = 2.0;
  options->increase_factor = 10.0;
  options->max_iterations = 50;
  options->iteration_group = 0;
}

int dsopp_hip_geometric_ba_create(int device, void *stream, dsopp_hip_geometric_ba **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    auto b = std::make_unique<dsopp_hip_geometric_ba>();
    b->sr.init(device, stream);
    *out = b.release();
  });
}

void dsopp_hip_geometric_ba_destroy(dsopp_hip_geometric_ba *b) {
  if (!b) return;
  (void)hipSetDevice(b->sr.device);
  if (b->sr.stream) (void)hipStreamSynchronize(b->sr.stream);
  delete b;
}

int dsopp_hip_geometric_ba_evaluate(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem, double a, double *cost,
                                    int32_t *valid_residuals, uint8_t *obs_valid, double *obs_residual, double *obs_weight) {
  return guarded([&] { evaluate<false>(b, problem, nullptr, a, cost, valid_residuals, obs_valid, obs_residual, obs_weight); });
}

int dsopp_hip_geometric_ba_evaluate_camera(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem, dsopp_hip_geometric_ba_camera *camera,
                                           double a, double *cost, int32_t *valid_residuals, uint8_t *obs_valid, double *obs_residual,
                                           double *obs_weight) {
  return guarded([&] { evaluate<true>(b, problem, camera, a, cost, valid_residuals, obs_valid, obs_residual, obs_weight); });
}

int dsopp_hip_geometric_ba_solve(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, const dsopp_hip_geometric_ba_options *options,
                                 dsopp_hip_geometric_ba_result *result, const dsopp_hip_geometric_ba_debug *debug) {
  return guarded([&] { solve<false>(b, problem, nullptr, options, result, debug, nullptr); });
}

int dsopp_hip_geometric_ba_solve_camera(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, dsopp_hip_geometric_ba_camera *camera,
                                        const dsopp_hip_geometric_ba_options *options, dsopp_hip_geometric_ba_result *result,
                                        const dsopp_hip_geometric_ba_camera_debug *debug) {
  return guarded([&] { solve<true>(b, problem, camera, options, result, debug ? &debug->base : nullptr, debug); });
}

int dsopp_hip_geometric_ba_triangulate(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, const uint8_t *has_position,
                                       int min_number_of_projections, int retriangulation, uint8_t *triangulated) {
  return guarded([&] { triangulate(b, problem, has_position, min_number_of_projections, retriangulation, triangulated); });
}

int dsopp_hip_geometric_ba_flag_outliers(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem, double outlier_threshold,
                                         uint8_t *flags, int32_t *flagged) {
  return guarded([&] { flagOutliers(b, problem, outlier_threshold, flags, flagged); });
}

}  // extern "C"
