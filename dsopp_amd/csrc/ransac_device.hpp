// Device tools the bootstrap's RANSAC units share (rotation_ransac.hip, pnp_ransac.hip, two_view_ransac.hip): the camera's region of
// interest, the hand-off to the closing workgroup, that workgroup's sums, selection, LM driver and inlier list, and the bracketed root
// finder of the polynomial solvers.  All of it binary64 in a stated order; this header sets no fp contract pragma, the including unit does.
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>
#include <cmath>

#include "../../include/dsopp_hip.h"

namespace dsopp_hip {
namespace ransac {  // (the units open it inside their own namespace: kBlock and the short helper names stay out of dsopp_hip)

// a wave owns one hypothesis, four waves a workgroup
constexpr int kBlock = 256;
constexpr int kWavesPerBlock = kBlock / 64;
constexpr int kMaxRootSteps = 200;  // a bracket of doubles is exhausted by ~64 bisections (geometric ones across magnitudes); the cap only bounds the loop

/** the pinhole camera and the observations' region of interest; the first part of every unit's kernel parameters */
struct PinholeRoi {
  double fx, fy, cx, cy, xmax, ymax;
};

__device__ __forceinline__ bool insideRoi(double x, double y, const PinholeRoi &p) { return x >= 4.0 && x <= p.xmax && y >= 4.0 && y <= p.ymax; }

__device__ __forceinline__ double dot3(const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double *a, const double *b, double *c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

/** f = normalize(unproject(x, y)) */
__device__ __forceinline__ void bearing(double x, double y, const PinholeRoi &p, double *f) {
  const double ux = (x - p.cx) / p.fx, uy = (y - p.cy) / p.fy;
  const double norm = sqrt(ux * ux + uy * uy + 1.0);
  f[0] = ux / norm;
  f[1] = uy / norm;
  f[2] = 1.0 / norm;
}

__device__ __forceinline__ bool isFinite(double v) { return fabs(v) <= DBL_MAX; }

/** a load that bypasses the vector cache: what the closing workgroup reads of the other workgroups' stores */
template <typename T>
__device__ __forceinline__ T freshLoad(const T *ptr) {
  return __hip_atomic_load(ptr, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

/** The hand-off to the workgroup that closes the call: true in the workgroup that draws the last ticket of the grid, which then sees
 *  every workgroup's plain stores from before its call (through freshLoad).  A ticket only: no workgroup waits for another.
 *    The order: the stores have left every wave (vmcnt(0)), a barrier, then one lane's release at agent scope and the ticket; behind the
 *  last ticket one acquire at agent scope, and a barrier that hands the verdict to the workgroup.  s_last: a __shared__ word */
__device__ __forceinline__ bool lastWorkgroup(unsigned *ticket, unsigned &s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const unsigned drawn = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    s_last = drawn == gridDim.x - 1 ? 1u : 0u;
    if (s_last) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
  }
  __syncthreads();
  return s_last != 0u;
}

// ---- the bracketed root of a polynomial

__device__ __forceinline__ double middlePositive(double lo, double hi) {
  if (lo == 0.0) return hi > 2.0 ? 1.0 : 0.5 * hi;
  if (hi > 4.0 * lo) return sqrt(lo) * sqrt(hi);
  return 0.5 * (lo + hi);
}

/** the middle of a bracket lo < hi: zero when it straddles zero, else geometric where the ends differ in magnitude, so that a bracket up
 *  to a polynomial's root bound is exhausted as fast as a narrow one */
__device__ __forceinline__ double middle(double lo, double hi) {
  if (lo < 0.0 && hi > 0.0) return 0.0;
  if (lo >= 0.0) return middlePositive(lo, hi);
  return -middlePositive(-hi, -lo);
}

/** the root inside (lo, hi) of the polynomial `eval` with the derivative `evalDerivative`, which has the sign of flo at lo and the other
 *  sign at hi: a safeguarded Newton iteration (bisection whenever Newton leaves the bracket or slows down), run to its fixed point.
 *  kNonNegative: the caller's brackets all have lo >= 0, where middle() is middlePositive(); the PnP's quartic chain, whose every lane
 *  runs it, measures 7 % of its call slower with the sign tests left in (profiles/ransac_shared/) */
template <bool kNonNegative = false, typename Eval, typename EvalDerivative>
__device__ __forceinline__ double bracketedRoot(Eval eval, EvalDerivative evalDerivative, double lo, double hi, double flo) {
  const auto middle = [](double a, double b) { return kNonNegative ? middlePositive(a, b) : ransac::middle(a, b); };
  double x = middle(lo, hi), last_step = hi - lo;
  for (int it = 0; it < kMaxRootSteps; ++it) {
    const double f = eval(x);
    if (f == 0.0) return x;
    if ((f > 0.0) == (flo > 0.0)) {
      lo = x;
    } else {
      hi = x;
    }
    const double mid = middle(lo, hi);
    if (!(mid > lo && mid < hi)) break;  // neighbouring doubles
    double next = x - f / evalDerivative(x);
    if (!(next > lo && next < hi) || !(fabs(next - x) <= 0.5 * fabs(last_step))) next = mid;
    if (next == x) break;
    last_step = next - x;
    x = next;
  }
  return x;
}

// ---- the closing workgroup's tools

/** every thread's v[k] becomes the sum over the workgroup, in one fixed order: a butterfly over the wave (both partners add the same two
 *  numbers), then the waves' sums in wave order.  s_sum: kWavesPerBlock x K doubles */
template <int K>
__device__ __forceinline__ void blockSum(double (&v)[K], double *s_sum, int lane, int wave) {
#pragma unroll
  for (int k = 0; k < K; ++k) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v[k] += __shfl_xor(v[k], o, 64);
  }
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) s_sum[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double total = s_sum[k];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) total += s_sum[w * K + k];
    v[k] = total;
  }
  __syncthreads();  // (s_sum is written again)
}

/** (H + lambda diag H) delta = -b by an unblocked right-looking Cholesky, Hb = H's upper triangle row by row, then b; false when a pivot
 *  is <= 0 or not finite */
template <int N>
__device__ __forceinline__ bool dampedSolve(const double (&Hb)[N * (N + 1) / 2 + N], double lambda, double (&delta)[N]) {
  double L[N][N];
  int at = 0;
#pragma unroll
  for (int a = 0; a < N; ++a)
#pragma unroll
    for (int b = a; b < N; ++b) {
      const double h = Hb[at++];
      L[b][a] = a == b ? h + lambda * h : h;
    }
  bool ok = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const double d = L[k][k];
    ok = ok && d > 0.0 && d <= DBL_MAX;
    const double root = sqrt(d);
    L[k][k] = root;
#pragma unroll
    for (int i = k + 1; i < N; ++i) L[i][k] /= root;
#pragma unroll
    for (int i = k + 1; i < N; ++i)
#pragma unroll
      for (int j = k + 1; j <= i; ++j) L[i][j] -= L[i][k] * L[j][k];
  }
  if (!ok) return false;
#pragma unroll
  for (int k = 0; k < N; ++k) delta[k] = -Hb[N * (N + 1) / 2 + k];
#pragma unroll
  for (int k = 0; k < N; ++k) {
    delta[k] /= L[k][k];
#pragma unroll
    for (int i = k + 1; i < N; ++i) delta[i] -= L[i][k] * delta[k];
  }
#pragma unroll
  for (int k = N - 1; k >= 0; --k) {
    delta[k] /= L[k][k];
#pragma unroll
    for (int i = 0; i < k; ++i) delta[i] -= L[k][i] * delta[k];
  }
  return true;
}

/** the indices j < n with isInlier(j), in ascending order: 256 per step, a wave's ballot places its lanes, the waves' counts place the
 *  waves; returns their number.  s_wave_count: kWavesPerBlock ints */
template <typename Predicate>
__device__ __forceinline__ int listInliers(int n, Predicate isInlier, int *s_wave_count, int tid, int *__restrict__ inliers) {
  const int lane = tid & 63, wave = tid >> 6;
  int total = 0;
  for (int base = 0; base < n; base += kBlock) {
    const int j = base + tid;
    const bool in = j < n && isInlier(j);
    const unsigned long long mask = __ballot(in);
    if (lane == 0) s_wave_count[wave] = __builtin_popcountll(mask);
    __syncthreads();
    int offset = total, step = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
      if (w < wave) offset += s_wave_count[w];
      step += s_wave_count[w];
    }
    if (in) inliers[offset + __builtin_popcountll(mask & ((1ull << lane) - 1ull))] = j;
    total += step;
    __syncthreads();  // (s_wave_count is written again)
  }
  return total;
}

/** the selection among kSolutions counts per hypothesis, by one wave: the greatest count, the lowest hypothesis among equals, the lowest
 *  solution among that one's.  Lane 0 writes the winner (-1, -1 when no count is positive) and its count */
template <int kSolutions>
__device__ __forceinline__ void selectBest(const int *hyp_counts, int iterations, int lane, int &s_best_iteration, int &s_best_solution,
                                           int &s_best_count) {
  int best = 0, best_i = INT_MAX;
  for (int i = lane; i < iterations; i += 64) {
    int c = 0;
#pragma unroll
    for (int s = 0; s < kSolutions; ++s) {
      const int cs = freshLoad(hyp_counts + kSolutions * static_cast<size_t>(i) + s);
      c = cs > c ? cs : c;
    }
    if (c > best) {
      best = c;
      best_i = i;
    }
  }
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int c = __shfl_xor(best, o, 64), i = __shfl_xor(best_i, o, 64);
    if (c > best || (c == best && i < best_i)) {
      best = c;
      best_i = i;
    }
  }
  if (lane == 0) {
    int solution = -1;
    if (best > 0) {
      for (int s = kSolutions - 1; s >= 0; --s)
        if (freshLoad(hyp_counts + kSolutions * static_cast<size_t>(best_i) + s) == best) solution = s;
    }
    s_best_iteration = best > 0 ? best_i : -1;
    s_best_solution = solution;
    s_best_count = best;
  }
}

/** The LM driver of the geometric BA over one pose T (12 doubles: R row-major, t), refined in place by the whole workgroup; every thread
 *  takes every decision from the same sums.  `problem` describes what is minimised over the inliers of the selection pose Tsel:
 *    kUnknowns                        the number of unknowns N
 *    cost(T, Tsel, cost, count)       the cost at T and the number of residuals that count, on every thread
 *    linearise(T, Tsel, Hb)           H (upper triangle, row by row) and b at T, on every thread
 *    retract(T, delta, C)             C = T moved by delta
 *    p                                lambda_0, function_tolerance, parameter_tolerance, decrease_factor, increase_factor, max_iterations */
template <typename Problem>
__device__ __forceinline__ void refinePose(const Problem &problem, double *T, const double *Tsel, int &iterations, int &flags, double &cost_initial,
                                           double &cost) {
  constexpr int N = Problem::kUnknowns;
  double counting, lambda = problem.p.lambda_0;
  iterations = 0;
  flags = 0;
  problem.cost(T, Tsel, cost, counting);
  cost_initial = cost;
  if (counting == 0.0) flags = DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL;
  bool linearise = true;
  double Hb[N * (N + 1) / 2 + N];
  while (iterations < problem.p.max_iterations && flags == 0) {
    if (linearise) problem.linearise(T, Tsel, Hb);
    linearise = false;
    double delta[N];
    ++iterations;
    if (!dampedSolve<N>(Hb, lambda, delta)) {
      lambda *= problem.p.increase_factor;
      continue;
    }
    double C[12], candidate_cost, candidate_counting;
    problem.retract(T, delta, C);
    problem.cost(C, Tsel, candidate_cost, candidate_counting);
    if (candidate_counting == 0.0) {
      flags = DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL;
      break;
    }
    int reason = fabs(cost - candidate_cost) / cost < problem.p.function_tolerance ? DSOPP_HIP_GEOMETRIC_BA_FUNCTION_TOLERANCE : 0;
    if (candidate_cost < cost) {
      double step = 0.0;
#pragma unroll
      for (int k = 0; k < N; ++k) step += delta[k] * delta[k];
      const double state = T[9] * T[9] + T[10] * T[10] + T[11] * T[11] + 1.0;
      if (step < problem.p.parameter_tolerance * (state + problem.p.parameter_tolerance)) reason |= DSOPP_HIP_GEOMETRIC_BA_PARAMETER_TOLERANCE;
#pragma unroll
      for (int e = 0; e < 12; ++e) T[e] = C[e];
      cost = candidate_cost;
      linearise = true;
      lambda /= problem.p.decrease_factor;
    } else {
      lambda *= problem.p.increase_factor;
    }
    flags = reason;
  }
}

}  // namespace ransac
}  // namespace dsopp_hip
