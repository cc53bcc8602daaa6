// The simple-radial camera's max_valid_radius_ (the constructor's constant, simple_radial.hpp:47-77) for the host and the device: the remap
// tables take it once per model on the host (camera_remap.hip), the geometric bundle adjustment for every candidate camera in a kernel
// (geometric_ba.hip).  One routine, one operation order, binary64 in single IEEE steps: both callers return the same bytes.
//   minimalPositiveRoot   src/energy/camera_model/include/energy/camera_model/polynomial_solver.hpp:11-41
#pragma once

#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <limits>

#pragma clang fp contract(off)

namespace dsopp_hip {
namespace radial {

constexpr int kBorderSize = 4;      // CameraModelBase::kBorderSize (camera_model_base.hpp:34)
constexpr int kMaxRootSteps = 200;  // as ransac_device.hpp: a bracket of doubles is exhausted long before

__host__ __device__ inline double evalPolynomial(const double *c, int n, double x) {
  double v = c[n];
  for (int i = n - 1; i >= 0; --i) v = v * x + c[i];
  return v;
}

__host__ __device__ inline double evalPolynomialDerivative(const double *c, int n, double x) {
  double v = n * c[n];
  for (int i = n - 1; i >= 1; --i) v = v * x + i * c[i];
  return v;
}

/** the middle of a bracket 0 <= lo < hi, geometric where the ends differ in magnitude (ransac_device.hpp: middlePositive) */
__host__ __device__ inline double middlePositive(double lo, double hi) {
  if (lo == 0.0) return hi > 2.0 ? 1.0 : 0.5 * hi;
  if (hi > 4.0 * lo) return sqrt(lo) * sqrt(hi);
  return 0.5 * (lo + hi);
}

/** the root inside (lo, hi) of the polynomial, which has the sign of flo at lo and the other sign at hi: the safeguarded Newton iteration
 *  of ransac_device.hpp (bracketedRoot) — bisection whenever Newton leaves the bracket or slows down, run to its fixed point */
__host__ __device__ inline double bracketedRoot(const double *c, int n, double lo, double hi, double flo) {
  double x = middlePositive(lo, hi), last_step = hi - lo;
  for (int it = 0; it < kMaxRootSteps; ++it) {
    const double f = evalPolynomial(c, n, x);
    if (f == 0.0) return x;
    if ((f > 0.0) == (flo > 0.0)) {
      lo = x;
    } else {
      hi = x;
    }
    const double mid = middlePositive(lo, hi);
    if (!(mid > lo && mid < hi)) break;  // neighbouring doubles
    double next = x - f / evalPolynomialDerivative(c, n, x);
    if (!(next > lo && next < hi) || !(fabs(next - x) <= 0.5 * fabs(last_step))) next = mid;
    if (next == x) break;
    last_step = next - x;
    x = next;
  }
  return x;
}

/** minimalPositiveRoot (polynomial_solver.hpp:11-41) of c[0] + c[1] r + c[3] r^3 + c[5] r^5 (c[2] = c[4] = 0): the polynomial is
 *  normalised, its leading coefficients below 1e-8 are dropped (:14-19), no coefficient left = 0 (:20-22), no root >= 0 = +inf (:30-40).
 *  Where the reference takes the companion matrix's eigenvalues, the roots of the derivative — a quadratic in r^2, closed form — cut
 *  r >= 0 into stretches on which the polynomial is monotone; the first stretch over which its sign changes holds the least root. */
__host__ __device__ inline double minimalPositiveRoot(double (&c)[6]) {
  double norm = 0.0;
  for (int i = 0; i < 6; ++i) norm += c[i] * c[i];
  norm = sqrt(norm);
  for (int i = 0; i < 6; ++i) c[i] /= norm;
  int n = 5;
  while (n > 0 && fabs(c[n]) < 1e-8) --n;
  if (n == 0) return 0.0;
  if (c[0] == 0.0) return 0.0;
  // the derivative in t = r^2: qa t^2 + qb t + qc
  const double qa = n >= 5 ? 5.0 * c[5] : 0.0, qb = n >= 3 ? 3.0 * c[3] : 0.0, qc = c[1];
  double t[2] = {-1.0, -1.0};
  if (qa != 0.0) {
    const double disc = qb * qb - 4.0 * qa * qc;
    if (disc >= 0.0) {
      const double q = -0.5 * (qb + copysign(sqrt(disc), qb));  // the root pair without cancellation
      t[0] = q / qa;
      if (q != 0.0) t[1] = qc / q;
    }
  } else if (qb != 0.0) {
    t[0] = -qc / qb;
  }
  double stops[3];
  int num_stops = 0;
  for (int i = 0; i < 2; ++i)
    if (t[i] > 0.0 && t[i] <= DBL_MAX) stops[num_stops++] = sqrt(t[i]);
  if (num_stops == 2 && stops[1] < stops[0]) {
    const double s = stops[0];
    stops[0] = stops[1];
    stops[1] = s;
  }
  double bound = 0.0;  // Cauchy: every root lies below 1 + max |c[i] / c[n]|
  for (int i = 0; i < n; ++i) bound = fmax(bound, fabs(c[i] / c[n]));
  stops[num_stops++] = fmin(1.0 + bound, DBL_MAX);
  double lo = 0.0, flo = c[0];
  for (int i = 0; i < num_stops; ++i) {
    const double hi = stops[i];
    if (!(hi > lo)) continue;
    const double fhi = evalPolynomial(c, n, hi);
    if (fhi == 0.0) return hi;
    if ((fhi > 0.0) != (flo > 0.0)) return bracketedRoot(c, n, lo, hi, flo);
    lo = hi;
    flo = fhi;
  }
  return std::numeric_limits<double>::infinity();
}

/** max_valid_radius_ of SimpleRadialCamera(width x height; f, cx, cy, k1, k2) (simple_radial.hpp:47-77): the least positive root of
 *  k2 r^5 + k1 r^3 + r - R, R = the farthest image corner's distance from the principal point over f, replaced by the first extremum of
 *  r + k1 r^3 + k2 r^5 less 4 / f where that lies below it.  As written there: with k2 == 0 the divisions give NaN or inf and the
 *  comparisons decide. */
__host__ __device__ inline double maxValidRadius(double width, double height, double f, double cx, double cy, double k1, double k2) {
  const double max_x = fmax(cx, width - cx), max_y = fmax(cy, height - cy);
  double radius = sqrt(max_x * max_x + max_y * max_y) / f;
  double polynomial[6] = {-radius, 1.0, 0.0, k1, 0.0, k2};
  radius = minimalPositiveRoot(polynomial);
  const double discriminant = 9.0 * k1 * k1 - 20.0 * k2;
  if (discriminant >= 0.0) {
    const double root1_2 = (-3.0 * k1 - sqrt(discriminant)) / 10.0 / k2;
    const double root2_2 = (-3.0 * k1 + sqrt(discriminant)) / 10.0 / k2;
    double root = radius;
    if (root1_2 > 0.0) {
      root = sqrt(root1_2);
    } else if (root2_2 > 0.0) {
      root = sqrt(root2_2);
    }
    if (root < radius) radius = root - static_cast<double>(kBorderSize) / f;
  }
  return radius;
}

}  // namespace radial
}  // namespace dsopp_hip
