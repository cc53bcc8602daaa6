// The two-view pose of the bootstrap's initialisation on the device, and the dsopp_hip_two_view_ransac_* entry points.
//   estimateSO3xS2                       src/feature_based_slam/tracker/src/estimate_so3xs2.cpp:23-110
//   refineSO3xS2, sampsonDistance        src/energy/problems/src/so3xs2_refinement.cpp:13-50, cost_functors/sampson_distance_cost.hpp:17-66
//   triangulatePoints (two views)        src/feature_based_slam/tracker/src/triangulate_points.cpp:18-45, epipolar_geometry/triangulation.hpp:26-42
//   their caller                         src/feature_based_slam/tracker/src/initialize_poses.cpp:29-45
// The reference hands the matches to OpenGV (Stewenius' five-point solver inside its RANSAC, then optimizeModelCoefficients and
// selectWithinDistance) and refines with Ceres; neither is part of the reference tree, so the solver here is the library's own: the
// five-point essential matrices per hypothesis and an LM refinement of the Sampson error.  What is mirrored is everything around the
// solver (include/dsopp_hip.h).
//
// The arithmetic is the one include/dsopp_hip.h states (tests/two_view_ransac_model.py is its NumPy form), all of it binary64.
//
// One launch.  A wave owns one hypothesis, four waves a workgroup.  The five-point solve is too large for one lane's registers (its
// 10 x 20 matrix alone is 400 of them), so the wave shares it through its own slice of LDS:
//   the null space of the 5 x 9 constraints   a fully pivoted elimination, a lane per entry, then Gram-Schmidt over lanes 0..8 and a
//                                             Hadamard mix, so that the hidden variable is a generic direction of the null space;
//   the ten cubics                            lane (a, b, c) of 64 evaluates the ten polarised constraints at (E_a, E_b, E_c); the
//                                             coefficient of a monomial is the sum over the lanes that are its permutations;
//   Gauss-Jordan on the 10 x 20 matrix        row pivoting, the lanes own the entries;
//   the hidden-variable form                  det B(z), a lane per coefficient: a polynomial of degree 10 in z;
//   its real roots                            bracketed through the chain of its derivatives, from the linear one upwards: at every level
//                                             lane b owns the interval between the critical points b - 1 and b and runs the safeguarded
//                                             Newton iteration (bracketedRoot) in it; a ballot compacts the roots for the next level;
//   per root, one lane                        (x, y) from the null vector of B(z), Gauss-Newton on the ten cubics until the point stops
//                                             moving, the pose of E in closed form (R = Cof(E) -+ hat(t) E, t the unit normal of E's
//                                             columns), the four candidates tried against the five pairs.
// The poses are ranked by their trace into LDS slots and read from there with a uniform index; the lanes then stride over the points and
// the wave counts by ballot.  Nothing is indexed dynamically in registers.
//   The workgroup that takes the last ticket closes the call with the tools of ransac_device.hpp, as pnp_ransac.hip does: selection, the
// refinement over the winner's inliers, the re-selection, the refinement over its inliers, the ascending inlier list.
#include "ransac_device.hpp"
#include "se3_math.hpp"
#include "staged_call.hpp"

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace {
using namespace ransac;

constexpr int kMaxSolutions = 10;
constexpr int kPolishSteps = 12;
constexpr double kConstraintTolerance = 1e-9;

struct TwoViewParams : PinholeRoi {
  double t_ang;
  double a, lambda_0, function_tolerance, parameter_tolerance, decrease_factor, increase_factor;
  int n, iterations, max_iterations;
};

/** what a wave shares while it solves its sample */
struct WaveShared {
  double basis[4][9];    // the null space: E = x basis[0] + y basis[1] + z basis[2] + basis[3]
  double trio[10][64];   // the ten polarised constraints at (E_a, E_b, E_c), lane 16 a + 4 b + c
  double A[10][20];      // the ten cubics, columns x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
  double B[3][3][5];     // B(z): entries as polynomials in z, lowest power first
  double der[11][11];    // der[l][k]: coefficient k of the l-th derivative of det B(z)
  double crit[2][12];    // the real roots of a level, ascending: the next level's brackets
  double pose[kMaxSolutions][12];
  double fa[5][3], fb[5][3];
  double Q[5][9];
  int perm[9];
};

// the monomials of the columns above as sorted triples over (x, y, z, 1) = (0, 1, 2, 3), packed 16 a + 4 b + c
__constant__ unsigned char kMonomial[20] = {0, 21, 1, 5, 2, 3, 22, 23, 6, 7, 10, 11, 15, 26, 27, 31, 42, 43, 47, 63};

__device__ __forceinline__ void waveSync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the ten constraints

/** out[0] = det(row 0 of Ea, row 1 of Eb, row 2 of Ec); out[1 + 3 i + j] = (2 Ea Eb^T Ec - tr(Ea Eb^T) Ec)_ij */
__device__ __forceinline__ void trilinear(const double *Ea, const double *Eb, const double *Ec, double *out) {
  double c[3];
  cross3(Eb + 3, Ec + 6, c);
  out[0] = Ea[0] * c[0] + Ea[1] * c[1] + Ea[2] * c[2];
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[3 * i + j] = Ea[3 * i] * Eb[3 * j] + Ea[3 * i + 1] * Eb[3 * j + 1] + Ea[3 * i + 2] * Eb[3 * j + 2];
  const double tr = M[0] + M[4] + M[8];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      out[1 + 3 * i + j] = 2.0 * (M[3 * i] * Ec[j] + M[3 * i + 1] * Ec[3 + j] + M[3 * i + 2] * Ec[6 + j]) - tr * Ec[3 * i + j];
}

// ---- the triangulation of a pair under a pose and the measure

/** alpha, beta of triangulation.hpp:29-41 and the two points: a = fa, b = normalize(R fb) */
__device__ __forceinline__ void triangulatePair(const double *T, const double *fa, const double *fb, double &alpha, double &beta, double *XA, double *XB) {
  double b[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = T[3 * k] * fb[0] + T[3 * k + 1] * fb[1] + T[3 * k + 2] * fb[2];
  const double nb = sqrt(b[0] * b[0] + b[1] * b[1] + b[2] * b[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) b[k] = b[k] / nb;
  const double ab = dot3(fa, b), at = dot3(fa, T + 9), bt = dot3(b, T + 9);
  const double den = 1.0 / (1.0 - ab * ab);
  alpha = den * (at - ab * bt);
  beta = den * (ab * at - bt);
  double d[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    XA[k] = (alpha * fa[k] + beta * b[k] + T[9 + k]) / 2.0;
    d[k] = XA[k] - T[9 + k];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) XB[k] = T[k] * d[0] + T[3 + k] * d[1] + T[6 + k] * d[2];
}

/** d = (1 - fa . X_A / |X_A|) + (1 - fb . X_B / |X_B|) */
__device__ __forceinline__ double twoViewDistance(const double *T, const double *fa, const double *fb) {
  double alpha, beta, XA[3], XB[3];
  triangulatePair(T, fa, fb, alpha, beta, XA, XB);
  const double na = sqrt(XA[0] * XA[0] + XA[1] * XA[1] + XA[2] * XA[2]);
  const double nb = sqrt(XB[0] * XB[0] + XB[1] * XB[1] + XB[2] * XB[2]);
  return (1.0 - dot3(fa, XA) / na) + (1.0 - dot3(fb, XB) / nb);
}

/** the inlier test of pair j against pose T (strict; false for a NaN and for an observation outside the ROI) */
__device__ __forceinline__ bool isInlier(const double *T, const double *__restrict__ A, const double *__restrict__ B, int j, const TwoViewParams &p) {
  const double ax = A[2 * static_cast<size_t>(j)], ay = A[2 * static_cast<size_t>(j) + 1];
  const double bx = B[2 * static_cast<size_t>(j)], by = B[2 * static_cast<size_t>(j) + 1];
  if (!insideRoi(ax, ay, p) || !insideRoi(bx, by, p)) return false;
  double fa[3], fb[3];
  bearing(ax, ay, p, fa);
  bearing(bx, by, p, fb);
  return twoViewDistance(T, fa, fb) < p.t_ang;
}

// ---- the polynomial of degree 10 and its derivatives, in LDS

__device__ __forceinline__ double evalLevel(const WaveShared &s, int level, double x) {
  const int deg = 10 - level;
  double v = s.der[level][deg];
  for (int k = deg - 1; k >= 0; --k) v = v * x + s.der[level][k];
  return v;
}

/** the real roots of det B(z), one per lane (NaN = none), through the chain of derivatives */
__device__ __forceinline__ double realRoots(WaveShared &s, int lane) {
  int ncrit = 0, cur = 0;
  double root = NAN;
  for (int level = 9; level >= 0; --level) {
    const int deg = 10 - level;
    const double top = s.der[level][deg];
    double big = 0.0;
    for (int k = 0; k <= deg; ++k) big = fmax(big, fabs(s.der[level][k]));
    const double bound = 1.0 + big / fabs(top);  // Cauchy's: no root lies beyond
    const bool outer = top != 0.0 && bound < DBL_MAX;
    root = NAN;
    if (lane <= ncrit) {
      const bool first = lane == 0, last = lane == ncrit;
      const double lo = first ? -bound : s.crit[cur][lane - 1], hi = last ? bound : s.crit[cur][lane];
      if ((outer || (!first && !last)) && lo < hi) {
        const double flo = evalLevel(s, level, lo), fhi = evalLevel(s, level, hi);
        if (fhi == 0.0 && !last) {
          root = hi;  // (a root on a critical point belongs to the bracket below it)
        } else if (flo != 0.0 && fhi != 0.0 && (flo > 0.0) != (fhi > 0.0)) {
          root = bracketedRoot([&](double x) { return evalLevel(s, level, x); }, [&](double x) { return evalLevel(s, level + 1, x); }, lo, hi, flo);
        }
      }
    }
    const bool has = isFinite(root);
    const unsigned long long mask = __ballot(has);
    if (has) s.crit[cur ^ 1][__builtin_popcountll(mask & ((1ull << lane) - 1ull))] = root;
    ncrit = __builtin_popcountll(mask);
    cur ^= 1;
    waveSync();
  }
  return root;
}

// ---- a root's essential matrix and its pose

/** E = p0 basis[0] + p1 basis[1] + p2 basis[2] + basis[3] */
__device__ __forceinline__ void essentialOf(const WaveShared &s, const double *pt, double *E) {
#pragma unroll
  for (int e = 0; e < 9; ++e) E[e] = pt[0] * s.basis[0][e] + pt[1] * s.basis[1][e] + pt[2] * s.basis[2][e] + s.basis[3][e];
}

/** Gauss-Newton on the ten cubics in (x, y, z), until the point stops moving */
__device__ __forceinline__ void polish(const WaveShared &s, double *pt) {
  for (int it = 0; it < kPolishSteps; ++it) {
    double E[9], r[10], J[3][10];
    essentialOf(s, pt, E);
    trilinear(E, E, E, r);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      double Ek[9], t1[10], t2[10], t3[10];
#pragma unroll
      for (int e = 0; e < 9; ++e) Ek[e] = s.basis[k][e];
      trilinear(Ek, E, E, t1);
      trilinear(E, Ek, E, t2);
      trilinear(E, E, Ek, t3);
#pragma unroll
      for (int q = 0; q < 10; ++q) J[k][q] = t1[q] + t2[q] + t3[q];
    }
    double H[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, g[3] = {0.0, 0.0, 0.0};  // xx xy xz yy yz zz
#pragma unroll
    for (int q = 0; q < 10; ++q) {
      H[0] += J[0][q] * J[0][q];
      H[1] += J[0][q] * J[1][q];
      H[2] += J[0][q] * J[2][q];
      H[3] += J[1][q] * J[1][q];
      H[4] += J[1][q] * J[2][q];
      H[5] += J[2][q] * J[2][q];
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] += J[k][q] * r[q];
    }
    // the 3 x 3 normal equations by cofactors
    const double c00 = H[3] * H[5] - H[4] * H[4], c01 = H[2] * H[4] - H[1] * H[5], c02 = H[1] * H[4] - H[2] * H[3];
    const double c11 = H[0] * H[5] - H[2] * H[2], c12 = H[1] * H[2] - H[0] * H[4], c22 = H[0] * H[3] - H[1] * H[1];
    const double det = H[0] * c00 + H[1] * c01 + H[2] * c02;
    const double step[3] = {-(c00 * g[0] + c01 * g[1] + c02 * g[2]) / det, -(c01 * g[0] + c11 * g[1] + c12 * g[2]) / det,
                            -(c02 * g[0] + c12 * g[1] + c22 * g[2]) / det};
    if (!(isFinite(step[0]) && isFinite(step[1]) && isFinite(step[2]))) break;
#pragma unroll
    for (int k = 0; k < 3; ++k) pt[k] += step[k];
    if (dot3(step, step) <= 1e-28 * (1.0 + dot3(pt, pt))) break;
  }
}

/** the pose of E (|E|_F^2 = 2) under which the five pairs all have alpha > 0 and beta > 0; false when none of the four candidates does */
__device__ __forceinline__ bool poseOf(const WaveShared &s, const double *E, double *T) {
  // t spans the left null space of E: the normal of E's columns, from the pair of columns with the largest cross product
  const double c0[3] = {E[0], E[3], E[6]}, c1[3] = {E[1], E[4], E[7]}, c2[3] = {E[2], E[5], E[8]};
  double x01[3], x02[3], x12[3];
  cross3(c0, c1, x01);
  cross3(c0, c2, x02);
  cross3(c1, c2, x12);
  const double n01 = dot3(x01, x01), n02 = dot3(x02, x02), n12 = dot3(x12, x12);
  double t[3], nn = n01;
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = x01[k];
  if (n02 > nn) {
    nn = n02;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = x02[k];
  }
  if (n12 > nn) {
    nn = n12;
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = x12[k];
  }
  const double norm = sqrt(nn);
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = t[k] / norm;
  // R = Cof(E) -+ hat(t) E
  const double cof[9] = {E[4] * E[8] - E[5] * E[7], E[5] * E[6] - E[3] * E[8], E[3] * E[7] - E[4] * E[6],
                         E[2] * E[7] - E[1] * E[8], E[0] * E[8] - E[2] * E[6], E[1] * E[6] - E[0] * E[7],
                         E[1] * E[5] - E[2] * E[4], E[2] * E[3] - E[0] * E[5], E[0] * E[4] - E[1] * E[3]};
  double tE[9];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    tE[j] = t[1] * E[6 + j] - t[2] * E[3 + j];
    tE[3 + j] = t[2] * E[j] - t[0] * E[6 + j];
    tE[6 + j] = t[0] * E[3 + j] - t[1] * E[j];
  }
  bool found = false;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double sr = c < 2 ? -1.0 : 1.0, st = (c & 1) ? -1.0 : 1.0;
    double C[12];
#pragma unroll
    for (int e = 0; e < 9; ++e) C[e] = cof[e] + sr * tE[e];
#pragma unroll
    for (int k = 0; k < 3; ++k) C[9 + k] = st * t[k];
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      double alpha, beta, XA[3], XB[3];
      const double fa[3] = {s.fa[k][0], s.fa[k][1], s.fa[k][2]}, fb[3] = {s.fb[k][0], s.fb[k][1], s.fb[k][2]};
      triangulatePair(C, fa, fb, alpha, beta, XA, XB);
      ok = ok && alpha > 0.0 && beta > 0.0;
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) ok = ok && isFinite(C[e]);
    if (ok && !found) {
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = C[e];
      found = true;
    }
  }
  return found;
}

/** the wave's five-point solve: the poses of the sample into s.pose (descending trace, unused slots zero); returns their number */
__device__ __forceinline__ int solveFivePoint(WaveShared &s, int lane) {
  // -- the null space of Q: elimination with full pivoting, lane e < 45 owns entry (e / 9, e % 9)
  const int qr = lane / 9, qc = lane % 9;
  const bool owns = lane < 45;
  if (lane < 9) s.perm[lane] = lane;
  waveSync();
  bool regular = true;
  for (int k = 0; k < 5; ++k) {
    double v = owns && qr >= k && qc >= k ? fabs(s.Q[qr][qc]) : -1.0;
    int at = lane;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ov > v || (ov == v && oa < at)) {
        v = ov;
        at = oa;
      }
    }
    if (!(v > 0.0) || !isFinite(v)) {
      regular = false;
      break;
    }
    const int pr = at / 9, pc = at % 9;
    if (lane < 9 && pr != k) {
      const double u = s.Q[k][lane];
      s.Q[k][lane] = s.Q[pr][lane];
      s.Q[pr][lane] = u;
    }
    waveSync();
    if (lane < 5 && pc != k) {
      const double u = s.Q[lane][k];
      s.Q[lane][k] = s.Q[lane][pc];
      s.Q[lane][pc] = u;
    }
    if (lane == 0 && pc != k) {
      const int u = s.perm[k];
      s.perm[k] = s.perm[pc];
      s.perm[pc] = u;
    }
    waveSync();
    double mine = 0.0, factor = 0.0, row = 0.0;
    const double pivot = s.Q[k][k];
    if (owns) {
      mine = s.Q[qr][qc];
      factor = s.Q[qr][k];
      row = s.Q[k][qc] / pivot;
    }
    waveSync();
    if (owns) s.Q[qr][qc] = qr == k ? row : mine - factor * row;
    waveSync();
  }
  if (!regular) return 0;
  // null vector j (free column 5 + j): -Q[i][5 + j] at perm[i], 1 at perm[5 + j]; lane c < 9 holds component c of all four
  double nv[4] = {0.0, 0.0, 0.0, 0.0};
  {
    const int c = lane & 15;
    if (c < 9) {
      int where = 0;
      for (int i = 0; i < 9; ++i)
        if (s.perm[i] == c) where = i;
#pragma unroll
      for (int j = 0; j < 4; ++j) nv[j] = where < 5 ? -s.Q[where][5 + j] : (where == 5 + j ? 1.0 : 0.0);
    }
    // Gram-Schmidt, every projection taken twice; sums over the 16 lanes of a group (lanes 9..15 hold zeros)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
#pragma unroll
      for (int pass = 0; pass < 2; ++pass) {
#pragma unroll
        for (int i = 0; i < j; ++i) {
          double d = nv[i] * nv[j];
#pragma unroll
          for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o, 64);
          nv[j] = nv[j] - d * nv[i];
        }
      }
      double d = nv[j] * nv[j];
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) d += __shfl_xor(d, o, 64);
      nv[j] = nv[j] / sqrt(d);
    }
    // the elimination's null vectors each hold one free entry of E, so a ratio of two coordinates in them is a ratio of two entries of
    // E, which the solutions of a small-motion scene share to a part in a thousand: the hidden variable would not separate them.  A
    // Hadamard mix of the orthonormal basis makes every coordinate a generic direction of the null space
    if (lane < 9) {
      s.basis[0][lane] = 0.5 * (((nv[0] + nv[1]) + nv[2]) + nv[3]);
      s.basis[1][lane] = 0.5 * (((nv[0] - nv[1]) + nv[2]) - nv[3]);
      s.basis[2][lane] = 0.5 * (((nv[0] + nv[1]) - nv[2]) - nv[3]);
      s.basis[3][lane] = 0.5 * (((nv[0] - nv[1]) - nv[2]) + nv[3]);
    }
  }
  waveSync();
  // -- the ten cubics: lane (a, b, c) evaluates the polarised constraints, the monomial's permutations are summed
  {
    double Ea[9], Eb[9], Ec[9], out[10];
    const int a = lane >> 4, b = (lane >> 2) & 3, c = lane & 3;
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      Ea[e] = s.basis[a][e];
      Eb[e] = s.basis[b][e];
      Ec[e] = s.basis[c][e];
    }
    trilinear(Ea, Eb, Ec, out);
#pragma unroll
    for (int q = 0; q < 10; ++q) s.trio[q][lane] = out[q];
  }
  waveSync();
  for (int e = lane; e < 200; e += 64) {
    const int r = e / 20, m = e % 20;
    const int code = kMonomial[m], a = code >> 4, b = (code >> 2) & 3, c = code & 3;
    const int perms[6] = {16 * a + 4 * b + c, 16 * a + 4 * c + b, 16 * b + 4 * a + c, 16 * b + 4 * c + a, 16 * c + 4 * a + b, 16 * c + 4 * b + a};
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      bool fresh = true;
#pragma unroll
      for (int j = 0; j < i; ++j) fresh = fresh && perms[j] != perms[i];
      if (fresh) sum += s.trio[r][perms[i]];
    }
    s.A[r][m] = sum;
  }
  waveSync();
  // -- Gauss-Jordan with row pivoting: lane r < 10 offers |A[r][k]|, the lanes own the entries
  for (int k = 0; k < 10; ++k) {
    const int r16 = lane & 15;
    double v = r16 < 10 && r16 >= k ? fabs(s.A[r16][k]) : -1.0;
    int at = r16;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oa = __shfl_xor(at, o, 64);
      if (ov > v || (ov == v && oa < at)) {
        v = ov;
        at = oa;
      }
    }
    if (!(v > 0.0) || !isFinite(v)) {
      regular = false;
      break;
    }
    if (lane < 20 && at != k) {
      const double u = s.A[k][lane];
      s.A[k][lane] = s.A[at][lane];
      s.A[at][lane] = u;
    }
    waveSync();
    const double pivot = s.A[k][k];
    double mine[4], factor[4], row[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = lane + 64 * q, r = e / 20, c = e % 20;
      mine[q] = factor[q] = row[q] = 0.0;
      if (e < 200) {
        mine[q] = s.A[r][c];
        factor[q] = s.A[r][k];
        row[q] = s.A[k][c] / pivot;
      }
    }
    waveSync();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = lane + 64 * q, r = e / 20, c = e % 20;
      if (e < 200) s.A[r][c] = r == k ? row[q] : mine[q] - factor[q] * row[q];
    }
    waveSync();
  }
  if (!regular) return 0;
  // -- B(z): rows <e> - z <f> of (x^2z, x^2), (y^2z, y^2), (xyz, xy); columns the coefficients of x, of y and of 1
  if (lane < 9) {
    const int r = lane / 3, c = lane % 3, e = 4 + 2 * r, f = 5 + 2 * r, g = 10 + 3 * c;
    if (c < 2) {
      s.B[r][c][0] = s.A[e][g + 2];
      s.B[r][c][1] = s.A[e][g + 1] - s.A[f][g + 2];
      s.B[r][c][2] = s.A[e][g] - s.A[f][g + 1];
      s.B[r][c][3] = -s.A[f][g];
      s.B[r][c][4] = 0.0;
    } else {
      s.B[r][c][0] = s.A[e][19];
      s.B[r][c][1] = s.A[e][18] - s.A[f][19];
      s.B[r][c][2] = s.A[e][17] - s.A[f][18];
      s.B[r][c][3] = s.A[e][16] - s.A[f][17];
      s.B[r][c][4] = -s.A[f][16];
    }
  }
  waveSync();
  // -- det B(z): lane k < 11 sums the products of coefficient k over the six permutations
  double ck = 0.0;
  if (lane < 11) {
    const int perm3[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {1, 0, 2}, {2, 1, 0}};
    for (int q = 0; q < 6; ++q) {
      double sum = 0.0;
      for (int i = 0; i < 5; ++i)
        for (int j = 0; j < 5; ++j) {
          const int l = lane - i - j;
          if (l >= 0 && l < 5) sum += s.B[0][perm3[q][0]][i] * s.B[1][perm3[q][1]][j] * s.B[2][perm3[q][2]][l];
        }
      ck = q < 3 ? ck + sum : ck - sum;
    }
    s.der[0][lane] = ck;
  }
  waveSync();
  if (lane < 11) {
    for (int level = 1; level <= 10; ++level) {
      double value = 0.0;
      if (lane + level <= 10) {
        value = s.der[0][lane + level];
        for (int i = 1; i <= level; ++i) value = value * static_cast<double>(lane + i);
      }
      s.der[level][lane] = value;
    }
  }
  waveSync();
  bool usable = true;
  for (int k = 0; k < 11; ++k) usable = usable && isFinite(s.der[0][k]);
  if (!usable) return 0;
  const double z = realRoots(s, lane);
  // -- a lane per root: the point, its polish, the pose
  double T[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  bool valid = false;
  if (isFinite(z)) {
    double rows[3][3];
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        double v = s.B[r][c][4];
#pragma unroll
        for (int k = 3; k >= 0; --k) v = v * z + s.B[r][c][k];
        rows[r][c] = v;
      }
    double x01[3], x02[3], x12[3], best[3];
    cross3(rows[0], rows[1], x01);
    cross3(rows[0], rows[2], x02);
    cross3(rows[1], rows[2], x12);
#pragma unroll
    for (int k = 0; k < 3; ++k) best[k] = x01[k];
    if (fabs(x02[2]) > fabs(best[2])) {
#pragma unroll
      for (int k = 0; k < 3; ++k) best[k] = x02[k];
    }
    if (fabs(x12[2]) > fabs(best[2])) {
#pragma unroll
      for (int k = 0; k < 3; ++k) best[k] = x12[k];
    }
    double pt[3] = {best[0] / best[2], best[1] / best[2], z};
    if (isFinite(pt[0]) && isFinite(pt[1])) {
      polish(s, pt);
      double E[9], r[10];
      essentialOf(s, pt, E);
      double n2 = 0.0;
#pragma unroll
      for (int e = 0; e < 9; ++e) n2 += E[e] * E[e];
      const double scale = sqrt(2.0 / n2);
#pragma unroll
      for (int e = 0; e < 9; ++e) E[e] = E[e] * scale;
      trilinear(E, E, E, r);
      double worst = 0.0;
#pragma unroll
      for (int q = 0; q < 10; ++q) worst = fmax(worst, fabs(r[q]));
      // (an E the polish has not brought onto the constraints is none: !(<=) also drops a NaN)
      if (n2 > 0.0 && isFinite(scale) && worst <= kConstraintTolerance) valid = poseOf(s, E, T);
    }
  }
  // -- rank by descending trace (the lower lane first among equals) into the slots
  const double trace = valid ? T[0] + T[4] + T[8] : -4.0;
  int rank = 0;
  for (int o = 0; o < 11; ++o) {
    const double ot = __shfl(trace, o, 64);
    const int ov = __shfl(valid ? 1 : 0, o, 64);
    if (ov && o != lane && (ot > trace || (ot == trace && o < lane))) ++rank;
  }
  const int solutions = __builtin_popcountll(__ballot(valid));
  if (valid && rank < kMaxSolutions) {
#pragma unroll
    for (int e = 0; e < 12; ++e) s.pose[rank][e] = T[e];
  }
  waveSync();
  return solutions < kMaxSolutions ? solutions : kMaxSolutions;
}

// ---- the refinement: what refinePose (ransac_device.hpp) minimises

/** E = hat(t) R */
__device__ __forceinline__ void essentialOfPose(const double *T, double *E) {
  const double *t = T + 9;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * T[6 + j] - t[2] * T[3 + j];
    E[3 + j] = t[2] * T[j] - t[0] * T[6 + j];
    E[6 + j] = t[0] * T[3 + j] - t[1] * T[j];
  }
}

/** b1, b2 of the tangent plane at the unit vector d: k = the first axis with the smallest |d_k|, b1 = normalize(d x e_k), b2 = d x b1 */
__device__ __forceinline__ void sphereBasis(const double *d, double *b1, double *b2) {
  int k = 0;
  if (fabs(d[1]) < fabs(d[k])) k = 1;
  if (fabs(d[2]) < fabs(d[k])) k = 2;
  const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
  double c[3];
  cross3(d, e, c);
  const double norm = sqrt(dot3(c, c));
#pragma unroll
  for (int i = 0; i < 3; ++i) b1[i] = c[i] / norm;
  cross3(d, b1, b2);
}

struct SampsonTerms {
  double xa[3], xb[3], u[3], v[3], top, bottom;
};

/** the parts of the Sampson residual of pair j under E (sampson_distance_cost.hpp:17-28): fx divides both axes */
__device__ __forceinline__ void sampsonTerms(const double *E, const double *__restrict__ A, const double *__restrict__ B, int j, const TwoViewParams &p,
                                             SampsonTerms &s) {
  s.xa[0] = (A[2 * static_cast<size_t>(j)] - p.cx) / p.fx;
  s.xa[1] = (A[2 * static_cast<size_t>(j) + 1] - p.cy) / p.fx;
  s.xa[2] = 1.0;
  s.xb[0] = (B[2 * static_cast<size_t>(j)] - p.cx) / p.fx;
  s.xb[1] = (B[2 * static_cast<size_t>(j) + 1] - p.cy) / p.fx;
  s.xb[2] = 1.0;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    s.u[k] = E[3 * k] * s.xb[0] + E[3 * k + 1] * s.xb[1] + E[3 * k + 2] * s.xb[2];
    s.v[k] = E[k] * s.xa[0] + E[3 + k] * s.xa[1] + E[6 + k] * s.xa[2];
  }
  s.top = s.xa[0] * s.u[0] + s.xa[1] * s.u[1] + s.xa[2] * s.u[2];
  const double u0 = s.u[0] / p.fx, u1 = s.u[1] / p.fx, v0 = s.v[0] / p.fx, v1 = s.v[1] / p.fx;
  s.bottom = (u0 * u0 + u1 * u1) + (v0 * v0 + v1 * v1);
}

__device__ __forceinline__ double sampsonResidual(const SampsonTerms &s) { return s.bottom < 1e-16 ? s.top : s.top / sqrt(s.bottom); }

/** the Huber loss of the Sampson error over the five degrees of freedom of (R, t / |t|); s_sum: kWavesPerBlock x 20 doubles */
struct TwoViewRefinement {
  static constexpr int kUnknowns = 5;
  const double *A, *B;
  const TwoViewParams &p;
  double *s_sum;
  int tid;

  /** 1/2 sum rho(r^2) and the number of pairs over the inliers of `Tsel`, at pose T: (cost, count) on every thread */
  __device__ __forceinline__ void cost(const double *T, const double *Tsel, double &value, double &count) const {
    double E[9];
    essentialOfPose(T, E);
    double v[2] = {0.0, 0.0};
    for (int j = tid; j < p.n; j += kBlock) {
      if (!isInlier(Tsel, A, B, j, p)) continue;
      SampsonTerms st;
      sampsonTerms(E, A, B, j, p, st);
      const double r = sampsonResidual(st), sq = r * r;
      v[0] += sq > p.a * p.a ? 2.0 * p.a * sqrt(sq) - p.a * p.a : sq;
      v[1] += 1.0;
    }
    blockSum<2>(v, s_sum, tid & 63, tid >> 6);
    value = 0.5 * v[0];
    count = v[1];
  }

  /** H (upper triangle, row by row: 15) and b (5) over the inliers of `Tsel`, at pose T, with the Huber weights */
  __device__ __forceinline__ void linearise(const double *T, const double *Tsel, double (&Hb)[20]) const {
    double E[9], dE[5][9], b1[3], b2[3];
    essentialOfPose(T, E);
    sphereBasis(T + 9, b1, b2);
    // dE / d alpha = hat(b1) R, dE / d beta = hat(b2) R, dE / d omega_k = E hat(e_k)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dE[0][j] = b1[1] * T[6 + j] - b1[2] * T[3 + j];
      dE[0][3 + j] = b1[2] * T[j] - b1[0] * T[6 + j];
      dE[0][6 + j] = b1[0] * T[3 + j] - b1[1] * T[j];
      dE[1][j] = b2[1] * T[6 + j] - b2[2] * T[3 + j];
      dE[1][3 + j] = b2[2] * T[j] - b2[0] * T[6 + j];
      dE[1][6 + j] = b2[0] * T[3 + j] - b2[1] * T[j];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      // E hat(e_0) = (0, E_i2, -E_i1), E hat(e_1) = (-E_i2, 0, E_i0), E hat(e_2) = (E_i1, -E_i0, 0), row i
      dE[2][3 * i] = 0.0;
      dE[2][3 * i + 1] = E[3 * i + 2];
      dE[2][3 * i + 2] = -E[3 * i + 1];
      dE[3][3 * i] = -E[3 * i + 2];
      dE[3][3 * i + 1] = 0.0;
      dE[3][3 * i + 2] = E[3 * i];
      dE[4][3 * i] = E[3 * i + 1];
      dE[4][3 * i + 1] = -E[3 * i];
      dE[4][3 * i + 2] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 20; ++k) Hb[k] = 0.0;
    for (int j = tid; j < p.n; j += kBlock) {
      if (!isInlier(Tsel, A, B, j, p)) continue;
      SampsonTerms st;
      sampsonTerms(E, A, B, j, p, st);
      const bool small = st.bottom < 1e-16;
      const double r = sampsonResidual(st), sq = r * r;
      const double w = sq > p.a * p.a ? p.a / sqrt(sq) : 1.0;
      const double root = sqrt(small ? 1.0 : st.bottom), safe = small ? 1.0 : st.bottom;
      double J[5];
#pragma unroll
      for (int k = 0; k < 5; ++k) {
        double du[3], dv[3];
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          du[i] = dE[k][3 * i] * st.xb[0] + dE[k][3 * i + 1] * st.xb[1] + dE[k][3 * i + 2] * st.xb[2];
          dv[i] = dE[k][i] * st.xa[0] + dE[k][3 + i] * st.xa[1] + dE[k][6 + i] * st.xa[2];
        }
        const double dtop = st.xa[0] * du[0] + st.xa[1] * du[1] + st.xa[2] * du[2];
        const double dbottom = 2.0 * (st.u[0] * du[0] + st.u[1] * du[1] + st.v[0] * dv[0] + st.v[1] * dv[1]) / (p.fx * p.fx);
        J[k] = small ? dtop : dtop / root - 0.5 * st.top * dbottom / (safe * root);
      }
      int at = 0;
#pragma unroll
      for (int a = 0; a < 5; ++a)
#pragma unroll
        for (int b = a; b < 5; ++b) Hb[at++] += w * J[a] * J[b];
#pragma unroll
      for (int a = 0; a < 5; ++a) Hb[15 + a] += w * J[a] * r;
    }
    blockSum<20>(Hb, s_sum, tid & 63, tid >> 6);
  }

  /** R <- R Exp(omega), t <- normalize(t + alpha b1 + beta b2) */
  __device__ __forceinline__ void retract(const double *T, const double (&delta)[5], double *C) const {
    double b1[3], b2[3], tn[3];
    sphereBasis(T + 9, b1, b2);
#pragma unroll
    for (int k = 0; k < 3; ++k) tn[k] = T[9 + k] + delta[0] * b1[k] + delta[1] * b2[k];
    const double norm = sqrt(dot3(tn, tn));
    const double xi[6] = {0.0, 0.0, 0.0, delta[2], delta[3], delta[4]};
    const Rigid e = rigidExp(xi);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) C[3 * i + j] = T[3 * i] * e.R[j] + T[3 * i + 1] * e.R[3 + j] + T[3 * i + 2] * e.R[6 + j];
#pragma unroll
    for (int k = 0; k < 3; ++k) C[9 + k] = tn[k] / norm;
  }
};

__global__ void __launch_bounds__(kBlock) twoViewRansacKernel(const double *__restrict__ A, const double *__restrict__ B, const int *__restrict__ samples,
                                                              unsigned *ticket, int *hyp_num_solutions, double *hyp_poses, int *hyp_counts,
                                                              dsopp_hip_two_view_ransac_result *result, int *__restrict__ inliers,
                                                              const TwoViewParams p) {
  __shared__ WaveShared s_wave[kWavesPerBlock];
  __shared__ unsigned s_last;
  __shared__ int s_best_iteration, s_best_solution, s_best_count;
  __shared__ int s_wave_count[kWavesPerBlock];
  __shared__ double s_sum[kWavesPerBlock * 20];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int hyp = static_cast<int>(blockIdx.x) * kWavesPerBlock + wave;
  if (hyp < p.iterations) {
    WaveShared &s = s_wave[wave];
    bool inside = true;
    if (lane < 5) {
      const size_t j = static_cast<size_t>(samples[5 * static_cast<size_t>(hyp) + lane]);
      const double ax = A[2 * j], ay = A[2 * j + 1], bx = B[2 * j], by = B[2 * j + 1];
      inside = insideRoi(ax, ay, p) && insideRoi(bx, by, p);
      double fa[3], fb[3];
      bearing(ax, ay, p, fa);
      bearing(bx, by, p, fb);
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        s.fa[lane][i] = fa[i];
        s.fb[lane][i] = fb[i];
#pragma unroll
        for (int k = 0; k < 3; ++k) s.Q[lane][3 * i + k] = fa[i] * fb[k];
      }
    }
    for (int e = lane; e < kMaxSolutions * 12; e += 64) s.pose[e / 12][e % 12] = 0.0;
    const bool valid = __ballot(!inside) == 0ull;
    waveSync();
    int solutions = 0;
    if (valid) solutions = solveFivePoint(s, lane);
    int count = 0;  // lane k counts solution k
    if (solutions > 0) {
      for (int base = 0; base < p.n; base += 64) {
        const int j = base + lane;
        bool match = false;
        double fa[3] = {0.0, 0.0, 1.0}, fb[3] = {0.0, 0.0, 1.0};
        if (j < p.n) {
          const double ax = A[2 * static_cast<size_t>(j)], ay = A[2 * static_cast<size_t>(j) + 1];
          const double bx = B[2 * static_cast<size_t>(j)], by = B[2 * static_cast<size_t>(j) + 1];
          match = insideRoi(ax, ay, p) && insideRoi(bx, by, p);
          bearing(ax, ay, p, fa);
          bearing(bx, by, p, fb);
        }
        for (int k = 0; k < solutions; ++k) {
          double T[12];
#pragma unroll
          for (int e = 0; e < 12; ++e) T[e] = s.pose[k][e];
          const bool in = match && twoViewDistance(T, fa, fb) < p.t_ang;
          const int votes = __builtin_popcountll(__ballot(in));
          if (lane == k) count += votes;
        }
      }
    }
    if (lane == 0) hyp_num_solutions[hyp] = solutions;
    if (lane < kMaxSolutions) hyp_counts[kMaxSolutions * static_cast<size_t>(hyp) + lane] = count;
    for (int e = lane; e < kMaxSolutions * 12; e += 64) hyp_poses[kMaxSolutions * 12 * static_cast<size_t>(hyp) + e] = s.pose[e / 12][e % 12];
  }
  if (!lastWorkgroup(ticket, s_last)) return;

  if (wave == 0) selectBest<kMaxSolutions>(hyp_counts, p.iterations, lane, s_best_iteration, s_best_solution, s_best_count);
  __syncthreads();
  const int best_iteration = s_best_iteration, best_solution = s_best_solution;
  double T0[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0}, T1[12], T2[12];
  if (best_iteration >= 0) {
#pragma unroll
    for (int e = 0; e < 12; ++e)
      T0[e] = freshLoad(hyp_poses + kMaxSolutions * 12 * static_cast<size_t>(best_iteration) + 12 * best_solution + e);
  }
#pragma unroll
  for (int e = 0; e < 12; ++e) T1[e] = T2[e] = T0[e];
  int iterations[2] = {0, 0}, flags[2] = {0, 0}, total = 0;
  double cost_initial[2] = {0.0, 0.0}, cost[2] = {0.0, 0.0};
  if (best_iteration >= 0) {
    const TwoViewRefinement problem{A, B, p, s_sum, tid};
    refinePose(problem, T1, T0, iterations[0], flags[0], cost_initial[0], cost[0]);
#pragma unroll
    for (int e = 0; e < 12; ++e) T2[e] = T1[e];
    refinePose(problem, T2, T1, iterations[1], flags[1], cost_initial[1], cost[1]);
    total = listInliers(p.n, [&](int j) { return isInlier(T1, A, B, j, p); }, s_wave_count, tid, inliers);
  }
  if (tid == 0) {
    result->matches = 0;  // (the host counts them)
    result->best_iteration = best_iteration;
    result->best_solution = best_solution;
    result->ransac_inlier_count = s_best_count;
    result->inlier_count = total;
    result->reserved = 0;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      result->refine_iterations[k] = iterations[k];
      result->refine_flags[k] = flags[k];
      result->cost_initial[k] = cost_initial[k];
      result->cost_final[k] = cost[k];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) {
      result->pose_ransac[e] = T0[e];
      result->pose_reselect[e] = T1[e];
      result->pose[e] = T2[e];
    }
  }
}

/** the two-view triangulatePoints: a thread per pair */
__global__ void __launch_bounds__(kBlock) twoViewTriangulateKernel(const double *__restrict__ A, const double *__restrict__ B, double *__restrict__ X,
                                                                   unsigned char *__restrict__ keep, const double *__restrict__ poses,
                                                                   double cos_threshold, const TwoViewParams p) {
  const int j = static_cast<int>(blockIdx.x) * kBlock + static_cast<int>(threadIdx.x);
  if (j >= p.n) return;
  double T[12], W[12];
#pragma unroll
  for (int e = 0; e < 12; ++e) {
    T[e] = poses[e];
    W[e] = poses[12 + e];
  }
  const double ax = A[2 * static_cast<size_t>(j)], ay = A[2 * static_cast<size_t>(j) + 1];
  const double bx = B[2 * static_cast<size_t>(j)], by = B[2 * static_cast<size_t>(j) + 1];
  double fa[3], fb[3], alpha, beta, XA[3], XB[3], Xw[3];
  bearing(ax, ay, p, fa);
  bearing(bx, by, p, fb);
  triangulatePair(T, fa, fb, alpha, beta, XA, XB);
  const double ca = dot3(fa, XA) / sqrt(XA[0] * XA[0] + XA[1] * XA[1] + XA[2] * XA[2]);
  const double cb = dot3(fb, XB) / sqrt(XB[0] * XB[0] + XB[1] * XB[1] + XB[2] * XB[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) Xw[k] = W[3 * k] * XA[0] + W[3 * k + 1] * XA[1] + W[3 * k + 2] * XA[2] + W[9 + k];
  const bool ok = insideRoi(ax, ay, p) && insideRoi(bx, by, p) && XA[2] > 0.0 && ca > cos_threshold && cb > cos_threshold && isFinite(ca) && isFinite(cb) &&
                  isFinite(Xw[0]) && isFinite(Xw[1]) && isFinite(Xw[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) X[3 * static_cast<size_t>(j) + k] = Xw[k];
  keep[j] = ok ? 1 : 0;
}

}  // namespace
}  // namespace dsopp_hip

struct dsopp_hip_two_view_ransac : dsopp_hip::StagedCall {};

namespace dsopp_hip {
namespace {

/** in:  ticket (16 bytes) | two poses (192 bytes) | A | B | samples;   out: result (512 bytes) | inliers | hyp_poses | hyp_counts |
 *  hyp_num_solutions.  The per-hypothesis outputs come last, so a call that does not ask for them copies the head only.  triangulate uses
 *  the same blocks: out = positions | keep */
struct TwoViewLayout {
  size_t poses, a, b, samples, in_bytes;
  size_t inliers, hyp_poses, counts, solutions, head_bytes, out_bytes;
  TwoViewLayout(size_t n, size_t iterations) {
    poses = 16;
    a = poses + 192;
    b = a + 16 * n;
    samples = b + 16 * n;
    in_bytes = samples + 20 * iterations;
    static_assert(sizeof(dsopp_hip_two_view_ransac_result) <= 512, "the result's slot");
    inliers = 512;
    head_bytes = inliers + 4 * n;
    hyp_poses = (head_bytes + 7) / 8 * 8;
    counts = hyp_poses + 960 * iterations;
    solutions = counts + 40 * iterations;
    out_bytes = solutions + 4 * iterations;
    if (out_bytes < 25 * n) out_bytes = 25 * n;
  }
};

void defaultOptions(dsopp_hip_two_view_ransac_options *o) {
  o->a = 1.5;
  o->lambda_0 = 1e-4;
  o->function_tolerance = 1e-10;
  o->parameter_tolerance = 1e-10;
  o->decrease_factor = 2.0;
  o->increase_factor = 10.0;
  o->max_iterations = 40;
  o->reserved = 0;
}

/** the checks both calls share; returns the matches */
int checkPairs(double fx, double fy, double cx, double cy, int width, int height, int n, const double *points_a, const double *points_b) {
  if (n < 0 || n > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d pairs", n);
  if (!finite(fx) || !finite(fy) || !finite(cx) || !finite(cy)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "an intrinsic is not finite");
  if (n > 0 && (!points_a || !points_b)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  const double xmax = static_cast<double>(width) - 5.0, ymax = static_cast<double>(height) - 5.0;
  int matches = 0;
  for (size_t j = 0; j < static_cast<size_t>(n); ++j) {
    const double ax = points_a[2 * j], ay = points_a[2 * j + 1], bx = points_b[2 * j], by = points_b[2 * j + 1];
    if (!finite(ax) || !finite(ay) || !finite(bx) || !finite(by)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "pair %zu is not finite", j);
    if (ax >= 4.0 && ax <= xmax && ay >= 4.0 && ay <= ymax && bx >= 4.0 && bx <= xmax && by >= 4.0 && by <= ymax) ++matches;
  }
  return matches;
}

void fillCamera(TwoViewParams &p, double fx, double fy, double cx, double cy, int width, int height, int n) {
  p = TwoViewParams{};
  p.fx = fx;
  p.fy = fy;
  p.cx = cx;
  p.cy = cy;
  p.xmax = static_cast<double>(width) - 5.0;
  p.ymax = static_cast<double>(height) - 5.0;
  p.n = n;
}

void estimate(dsopp_hip_two_view_ransac *h, double fx, double fy, double cx, double cy, int width, int height, int n, const double *points_a,
              const double *points_b, int iterations, const int32_t *samples, double threshold_px, int min_matches,
              const dsopp_hip_two_view_ransac_options *options, dsopp_hip_two_view_ransac_result *result, int32_t *inlier_indices,
              int32_t *hyp_num_solutions, double *hyp_poses, int32_t *hyp_counts) {
  if (!h) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null two-view ransac");
  if (!result) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (iterations < 0 || iterations > (1 << 24)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d iterations", iterations);
  if (!finite(threshold_px)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the threshold is not finite");
  if (min_matches < 0) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "min_matches %d", min_matches);
  const int matches = checkPairs(fx, fy, cx, cy, width, height, n, points_a, points_b);
  if (n > 0 && !inlier_indices) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  dsopp_hip_two_view_ransac_options o;
  defaultOptions(&o);
  if (options) o = *options;
  if (!finite(o.a) || !finite(o.lambda_0) || !finite(o.function_tolerance) || !finite(o.parameter_tolerance) ||
      !finite(o.decrease_factor) || !finite(o.increase_factor) || !(o.a > 0.0) || o.lambda_0 < 0.0 || !(o.decrease_factor > 0.0) ||
      !(o.increase_factor > 0.0) || o.max_iterations < 0)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a refinement option is out of range");
  const bool enough = matches >= min_matches;  // (estimate_so3xs2.cpp:48: below it the samples are not looked at)
  if (enough && n > 0 && iterations > 0) {
    if (n < 5) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "%d pairs: a sample of distinct indices needs 5", n);
    checkSamples<5, false>(samples, iterations, n, "pairs");
  }
  std::memset(result, 0, sizeof(*result));
  result->matches = matches;
  result->best_iteration = -1;
  result->best_solution = -1;
  for (int k = 0; k < 9; ++k) result->pose_ransac[k] = result->pose_reselect[k] = result->pose[k] = k % 4 == 0 ? 1.0 : 0.0;
  const size_t count = static_cast<size_t>(n), hyps = static_cast<size_t>(iterations);
  if (hyp_num_solutions) std::memset(hyp_num_solutions, 0, 4 * hyps);
  if (hyp_poses) std::memset(hyp_poses, 0, 960 * hyps);
  if (hyp_counts) std::memset(hyp_counts, 0, 40 * hyps);
  if (!enough || n == 0 || iterations == 0) return;  // no hypothesis: the identity, no inliers, no refinement
  h->sr.use();
  const hipStream_t st = h->sr.stream;
  const TwoViewLayout lay(count, hyps);
  h->ensure(lay.in_bytes, lay.out_bytes);
  uint8_t *hi = h->h_in.get(), *di = h->d_in.get(), *ho = h->h_out.get(), *dout = h->d_out.get();
  std::memset(hi, 0, lay.a);  // (the ticket is armed by the upload)
  std::memcpy(hi + lay.a, points_a, 16 * count);
  std::memcpy(hi + lay.b, points_b, 16 * count);
  std::memcpy(hi + lay.samples, samples, 20 * hyps);
  HIP_CHECK(hipMemcpyAsync(di, hi, lay.in_bytes, hipMemcpyHostToDevice, st));
  TwoViewParams p;
  fillCamera(p, fx, fy, cx, cy, width, height, n);
  p.t_ang = 1.0 - std::cos(std::atan(threshold_px / fx));
  p.a = o.a;
  p.lambda_0 = o.lambda_0;
  p.function_tolerance = o.function_tolerance;
  p.parameter_tolerance = o.parameter_tolerance;
  p.decrease_factor = o.decrease_factor;
  p.increase_factor = o.increase_factor;
  p.iterations = iterations;
  p.max_iterations = o.max_iterations;
  const unsigned blocks = (static_cast<unsigned>(iterations) + kWavesPerBlock - 1) / kWavesPerBlock;
  twoViewRansacKernel<<<blocks, kBlock, 0, st>>>(reinterpret_cast<const double *>(di + lay.a), reinterpret_cast<const double *>(di + lay.b),
                                                 reinterpret_cast<const int *>(di + lay.samples), reinterpret_cast<unsigned *>(di),
                                                 reinterpret_cast<int *>(dout + lay.solutions), reinterpret_cast<double *>(dout + lay.hyp_poses),
                                                 reinterpret_cast<int *>(dout + lay.counts),
                                                 reinterpret_cast<dsopp_hip_two_view_ransac_result *>(dout), reinterpret_cast<int *>(dout + lay.inliers), p);
  HIP_CHECK(hipGetLastError());
  const bool with_hypotheses = hyp_num_solutions || hyp_poses || hyp_counts;
  HIP_CHECK(hipMemcpyAsync(ho, dout, with_hypotheses ? lay.solutions + 4 * hyps : lay.head_bytes, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipEventRecord(h->done.get(hipEventDisableTiming), st));
  HIP_CHECK(hipEventSynchronize(h->done.h));  // the one wait of the call
  std::memcpy(result, ho, sizeof(*result));
  result->matches = matches;
  if (result->inlier_count < 0 || result->inlier_count > n) fail(DSOPP_HIP_ERR_HIP, "the device returned %d inliers of %d pairs", result->inlier_count, n);
  std::memcpy(inlier_indices, ho + lay.inliers, 4 * static_cast<size_t>(result->inlier_count));
  if (hyp_num_solutions) std::memcpy(hyp_num_solutions, ho + lay.solutions, 4 * hyps);
  if (hyp_poses) std::memcpy(hyp_poses, ho + lay.hyp_poses, 960 * hyps);
  if (hyp_counts) std::memcpy(hyp_counts, ho + lay.counts, 40 * hyps);
}

void triangulate(dsopp_hip_two_view_ransac *h, double fx, double fy, double cx, double cy, int width, int height, int n, const double *points_a,
                 const double *points_b, const double *pose_a_b, const double *pose_world_a, double cos_threshold, double *positions, uint8_t *keep) {
  if (!h) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null two-view ransac");
  if (!pose_a_b || !pose_world_a) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  checkPairs(fx, fy, cx, cy, width, height, n, points_a, points_b);
  if (n > 0 && (!positions || !keep)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
  if (cos_threshold != cos_threshold) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the threshold is not a number");
  for (int e = 0; e < 12; ++e)
    if (!finite(pose_a_b[e]) || !finite(pose_world_a[e])) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a pose is not finite");
  if (n == 0) return;
  h->sr.use();
  const hipStream_t st = h->sr.stream;
  const size_t count = static_cast<size_t>(n);
  const TwoViewLayout lay(count, 0);
  h->ensure(lay.in_bytes, lay.out_bytes);
  uint8_t *hi = h->h_in.get(), *di = h->d_in.get(), *ho = h->h_out.get(), *dout = h->d_out.get();
  std::memset(hi, 0, 16);
  std::memcpy(hi + lay.poses, pose_a_b, 96);
  std::memcpy(hi + lay.poses + 96, pose_world_a, 96);
  std::memcpy(hi + lay.a, points_a, 16 * count);
  std::memcpy(hi + lay.b, points_b, 16 * count);
  HIP_CHECK(hipMemcpyAsync(di, hi, lay.samples, hipMemcpyHostToDevice, st));
  TwoViewParams p;
  fillCamera(p, fx, fy, cx, cy, width, height, n);
  const unsigned blocks = (static_cast<unsigned>(n) + kBlock - 1) / kBlock;
  twoViewTriangulateKernel<<<blocks, kBlock, 0, st>>>(reinterpret_cast<const double *>(di + lay.a), reinterpret_cast<const double *>(di + lay.b),
                                                      reinterpret_cast<double *>(dout), dout + 24 * count,
                                                      reinterpret_cast<const double *>(di + lay.poses), cos_threshold, p);
  HIP_CHECK(hipGetLastError());
  HIP_CHECK(hipMemcpyAsync(ho, dout, 25 * count, hipMemcpyDeviceToHost, st));
  HIP_CHECK(hipEventRecord(h->done.get(hipEventDisableTiming), st));
  HIP_CHECK(hipEventSynchronize(h->done.h));
  std::memcpy(positions, ho, 24 * count);
  std::memcpy(keep, ho + 24 * count, count);
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_two_view_ransac_default_iterations(void) { return 256; }

void dsopp_hip_two_view_ransac_default_options(dsopp_hip_two_view_ransac_options *options) {
  if (options) defaultOptions(options);
}

int dsopp_hip_two_view_ransac_create(int device, void *stream, dsopp_hip_two_view_ransac **out) { return createHandle(device, stream, out); }

void dsopp_hip_two_view_ransac_destroy(dsopp_hip_two_view_ransac *r) { destroyHandle(r); }

int dsopp_hip_two_view_ransac_estimate(dsopp_hip_two_view_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                       const double *points_a, const double *points_b, int iterations, const int32_t *samples, double threshold_px,
                                       int min_matches, const dsopp_hip_two_view_ransac_options *options,
                                       dsopp_hip_two_view_ransac_result *result, int32_t *inlier_indices, int32_t *hyp_num_solutions,
                                       double *hyp_poses, int32_t *hyp_counts) {
  return guarded([&] {
    estimate(r, fx, fy, cx, cy, width, height, n, points_a, points_b, iterations, samples, threshold_px, min_matches, options, result,
             inlier_indices, hyp_num_solutions, hyp_poses, hyp_counts);
  });
}

int dsopp_hip_two_view_ransac_triangulate(dsopp_hip_two_view_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                          const double *points_a, const double *points_b, const double pose_a_b[12], const double pose_world_a[12],
                                          double cos_threshold, double *positions, uint8_t *keep) {
  return guarded([&] {
    triangulate(r, fx, fy, cx, cy, width, height, n, points_a, points_b, pose_a_b, pose_world_a, cos_threshold, positions, keep);
  });
}

}  // extern "C"
