// The undistorter's remap tables from the camera model, on the device: dsopp_hip_camera_model_to_pinhole and
// dsopp_hip_undistorter_create_from_model.
//   Undistorter::constructRemaps / estimateRemaps   src/sensors/camera_calibration/include/sensors/camera_calibration/undistorter/undistorter.hpp:69-142
//   PinholeCamera::unproject                        src/energy/camera_model/include/energy/camera_model/pinhole/pinhole_camera.hpp:129-141
//   SimpleRadialCamera (ctor, project)              src/energy/camera_model/include/energy/camera_model/pinhole/simple_radial.hpp:39-83,134-160
//   TUMFovModel::project                            src/energy/camera_model/include/energy/camera_model/fisheye/tum_fov_model.hpp:72-82
//   AtanCamera::project                             src/energy/camera_model/include/energy/camera_model/fisheye/atan_camera.hpp:98-127
//   minimalPositiveRoot                             src/energy/camera_model/include/energy/camera_model/polynomial_solver.hpp:11-41
//
// The arithmetic is binary64 in the order include/dsopp_hip.h states, single IEEE steps (the file is built with -ffp-contract=off).
// One evaluation per output pixel, independent of every other: a thread takes 4 consecutive pixels of the row-major image — the granule
// undistortKernel reads — unprojects each through the target pinhole, projects the ray through the distorted model, rounds the point
// to float and folds it with the code dsopp_hip_undistorter_create runs on the host (remap_fold.hpp).  It stores the 32 bytes of table
// as two 16-byte words (a wave: 2 KiB contiguous) and, when the maps are asked for, 16 + 16 bytes of floats.  The N mod 4 pixels that
// are left are written entry by entry by the thread behind the last full granule.  The model's scalars are the kernel's arguments;
// the three projections are three instances of the kernel.  No LDS, no atomics, nothing between workgroups.
#include <cfloat>
#include <climits>
#include <cmath>
#include <limits>
#include <memory>

#include "pyramid.hpp"
#include "remap_fold.hpp"
#include "simple_radial_radius.hpp"
#include "undistort.hpp"

namespace dsopp_hip {
namespace {

constexpr int kBlock = 256;
constexpr int kBorder = 4;                   // CameraModelBase::kBorderSize (camera_model_base.hpp:34)
constexpr double kMaxCentre = 1048576.0;     // 2^20, the bound dsopp_hip_undistorter_create puts on a map entry

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

/** what the kernel needs of the model: everything a pixel's evaluation reads, passed by value */
struct RemapArgs {
  int w, h;
  double half_w, half_h, inv_fx, inv_fy;  // the target pinhole (undistorter.hpp:70-80, pinhole_camera.hpp:138)
  double fx, fy, cx, cy;                  // the distorted model (simple-radial: fx = fy = f)
  double roi_x, roi_y;                    // w - kBorder - 1, h - kBorder - 1
  double a, b;                            // simple-radial: max_valid_radius, unused | TUM-FOV: tan(fov / 2), fov
  double k[DSOPP_HIP_CAMERA_MAX_K];       // simple-radial: k1, k2 | atan: the polynomial, zero above num_k
};

__device__ __forceinline__ bool insideRoi(const RemapArgs &m, double x, double y) {
  return x >= kBorder && y >= kBorder && x <= m.roi_x && y <= m.roi_y;
}

/** the distorted model's projection of the ray (rx, ry, 1); false = the projection failed */
template <int kType>
__device__ __forceinline__ bool projectRay(const RemapArgs &m, double rx, double ry, double &px, double &py) {
  if constexpr (kType == DSOPP_HIP_CAMERA_SIMPLE_RADIAL) {
    const double r2 = rx * rx + ry * ry;
    const bool beyond = sqrt(r2) > m.a;
    const double d = (1.0 + m.k[0] * r2) + (m.k[1] * r2) * r2;
    px = (rx * d) * m.fx + m.cx;
    py = (ry * d) * m.fx + m.cy;
    return !beyond && insideRoi(m, px, py);
  } else if constexpr (kType == DSOPP_HIP_CAMERA_TUM_FOV) {
    const double ru = sqrt(rx * rx + ry * ry);
    if (ru < 1e-8) {
      px = m.cx;
      py = m.cy;
      return true;
    }
    const double rd = atan2((2.0 * ru) * m.a, 1.0) / m.b;
    const double q = rd / ru;
    px = (q * rx) * m.fx + m.cx;
    py = (q * ry) * m.fy + m.cy;
    return insideRoi(m, px, py);
  } else {
    const double n = sqrt((rx * rx + ry * ry) + 1.0);
    const double ax = rx / n, ay = ry / n, az = 1.0 / n;
    const double rho = sqrt(ax * ax + ay * ay);
    if (rho < 1e-6) {
      px = m.cx;
      py = m.cy;
      return true;
    }
    const double theta = atan2(rho, az);
    // Horner from the top of all 16 places: the places above num_k hold +0 and theta >= 0, so s stays +0 until the model's top
    // coefficient — the bits of a loop from num_k - 1, without an index into the arguments that depends on one
    double s = 0.0;
#pragma unroll
    for (int i = DSOPP_HIP_CAMERA_MAX_K - 1; i >= 0; --i) s = s * theta + m.k[i];
    s = theta * (1.0 + s * theta);
    px = ((ax * s) / rho) * m.fx + m.cx;
    py = ((ay * s) / rho) * m.fy + m.cy;
    return insideRoi(m, px, py);
  }
}

/** the map entry of output pixel (x, y): estimateRemaps (undistorter.hpp:126-141) */
template <int kType>
__device__ __forceinline__ void mapEntry(const RemapArgs &m, int x, int y, float &mx, float &my) {
  mx = my = -1.0f;
  if (x < kBorder || y < kBorder || x > m.w - kBorder - 1 || y > m.h - kBorder - 1) return;
  const double rx = (static_cast<double>(x) - m.half_w) * m.inv_fx, ry = (static_cast<double>(y) - m.half_h) * m.inv_fy;
  double px, py;
  if (!projectRay<kType>(m, rx, ry, px, py)) return;
  mx = static_cast<float>(px);
  my = static_cast<float>(py);
}

// (the parameters are plain pointers — a kernel's name must be the same in the host and the device pass — and are typed as HBM inside)
template <int kType>
__global__ void __launch_bounds__(kBlock) remapTableKernel(RemapArgs m, unsigned *__restrict__ table_, float *__restrict__ map_x_,
                                                           float *__restrict__ map_y_, unsigned words, unsigned tail) {
  const unsigned t = blockIdx.x * kBlock + threadIdx.x;
  if (t > words || (t == words && tail == 0)) return;
  const unsigned count = t < words ? 4u : tail;
  const unsigned first = 4u * t;  // < w * h <= INT_MAX
  int y = static_cast<int>(first / static_cast<unsigned>(m.w)), x = static_cast<int>(first - static_cast<unsigned>(y) * static_cast<unsigned>(m.w));
  float mx[4], my[4];
  unsigned e[8];
#pragma unroll
  for (unsigned k = 0; k < 4; ++k) {
    mx[k] = my[k] = -1.0f;
    e[2 * k] = e[2 * k + 1] = 0;
    if (k < count) {
      mapEntry<kType>(m, x, y, mx[k], my[k]);
      foldMapEntry(mx[k], my[k], m.w, m.h, e[2 * k], e[2 * k + 1]);
      if (++x == m.w) {
        x = 0;
        ++y;
      }
    }
  }
  if (t < words) {
    GlobalPtr<u32x4> out = reinterpret_cast<GlobalPtr<u32x4>>(glb(table_)) + 2 * static_cast<size_t>(t);
    out[0] = u32x4{e[0], e[1], e[2], e[3]};
    out[1] = u32x4{e[4], e[5], e[6], e[7]};
    if (map_x_) {
      reinterpret_cast<GlobalPtr<f32x4>>(glb(map_x_))[t] = f32x4{mx[0], mx[1], mx[2], mx[3]};
      reinterpret_cast<GlobalPtr<f32x4>>(glb(map_y_))[t] = f32x4{my[0], my[1], my[2], my[3]};
    }
  } else {
#pragma unroll
    for (unsigned k = 0; k < 3; ++k) {
      if (k < tail) {
        reinterpret_cast<GlobalPtr<u32x2>>(glb(table_))[first + k] = u32x2{e[2 * k], e[2 * k + 1]};
        if (map_x_) {
          glb(map_x_)[first + k] = mx[k];
          glb(map_y_)[first + k] = my[k];
        }
      }
    }
  }
}

// ---- the host side: the model's constants

int expectedNumK(int type) { return type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL ? 2 : type == DSOPP_HIP_CAMERA_TUM_FOV ? 1 : -1; }

/** the refusals of include/dsopp_hip.h */
void checkModel(const dsopp_hip_camera_model *m) {
  if (!m) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null camera model");
  if (m->type != DSOPP_HIP_CAMERA_SIMPLE_RADIAL && m->type != DSOPP_HIP_CAMERA_TUM_FOV && m->type != DSOPP_HIP_CAMERA_ATAN)
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "unknown camera model type %d", m->type);
  if (m->width < 2 || m->height < 2) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the image is %d x %d: reflection needs 2 x 2", m->width, m->height);
  if (static_cast<long long>(m->width) * m->height > INT_MAX) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "image too large");
  const int want = expectedNumK(m->type);
  if (m->num_k < 0 || m->num_k > DSOPP_HIP_CAMERA_MAX_K || (want >= 0 && m->num_k != want))
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "num_k = %d does not fit camera model type %d", m->num_k, m->type);
  const int num_params = m->type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL ? 3 : 4;
  for (int i = 0; i < num_params; ++i)
    if (!std::isfinite(m->params[i])) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "camera parameter %d is not finite", i);
  for (int i = 0; i < m->num_k; ++i)
    if (!std::isfinite(m->k[i])) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "distortion coefficient %d is not finite", i);
  const int num_focals = m->type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL ? 1 : 2;
  for (int i = 0; i < num_focals; ++i)
    if (!(m->params[i] > 0.0)) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "focal length %g is not positive", m->params[i]);
  for (int i = num_focals; i < num_params; ++i)
    if (std::fabs(m->params[i]) > kMaxCentre) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "principal point coordinate %g is beyond 2^20", m->params[i]);
  if (m->type == DSOPP_HIP_CAMERA_TUM_FOV && !(m->k[0] > 0.0 && m->k[0] < M_PI))
    fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "fov = %g is outside (0, pi)", m->k[0]);
}

/** the target pinhole of constructRemaps and, for simple-radial, the constructor's constants (simple_radial.hpp:47-82) */
void modelToPinhole(const dsopp_hip_camera_model *m, double pinhole[4], double derived[3]) {
  const bool radial = m->type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL;
  pinhole[0] = m->params[0];
  pinhole[1] = radial ? m->params[0] : m->params[1];
  pinhole[2] = static_cast<double>(m->width) / 2;
  pinhole[3] = static_cast<double>(m->height) / 2;
  derived[0] = derived[1] = derived[2] = 0.0;
  if (!radial) return;
  const double k1 = m->k[0], k2 = m->k[1];
  // the root finder and the extremum rule are simple_radial_radius.hpp's, shared with the geometric bundle adjustment's kernels
  const double radius = dsopp_hip::radial::maxValidRadius(static_cast<double>(m->width), static_cast<double>(m->height), m->params[0], m->params[1],
                                                          m->params[2], k1, k2);
  const double r2 = radius * radius, r4 = r2 * r2;
  derived[0] = radius;
  derived[1] = 1.0 + 3.0 * k1 * r2 + 5.0 * k2 * r4;
  derived[2] = radius * (1.0 + k1 * r2 + k2 * r4);
}

template <int kType>
void launchRemap(const RemapArgs &args, unsigned *table, float *map_x, float *map_y, hipStream_t stream) {
  const size_t n = static_cast<size_t>(args.w) * args.h;
  const unsigned words = static_cast<unsigned>(n / 4), tail = static_cast<unsigned>(n % 4);
  const unsigned threads = words + (tail ? 1u : 0u);
  remapTableKernel<kType><<<(threads + kBlock - 1) / kBlock, kBlock, 0, stream>>>(args, table, map_x, map_y, words, tail);
  HIP_CHECK(hipGetLastError());
}

}  // namespace
}  // namespace dsopp_hip

using namespace dsopp_hip;

extern "C" {

int dsopp_hip_camera_model_to_pinhole(const dsopp_hip_camera_model *model, double pinhole_intrinsics[4], double derived[3]) {
  return guarded([&] {
    checkModel(model);
    double pinhole[4], constants[3];
    modelToPinhole(model, pinhole, constants);
    for (int i = 0; i < 4 && pinhole_intrinsics; ++i) pinhole_intrinsics[i] = pinhole[i];
    for (int i = 0; i < 3 && derived; ++i) derived[i] = constants[i];
  });
}

int dsopp_hip_undistorter_create_from_model(int device, void *stream, const dsopp_hip_camera_model *model, float *map_x_out, float *map_y_out,
                                            double pinhole_intrinsics_out[4], dsopp_hip_undistorter **out) {
  return guarded([&] {
    if (!out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "null argument");
    checkModel(model);
    if (!map_x_out != !map_y_out) fail(DSOPP_HIP_ERR_INVALID_ARGUMENT, "one map without the other");
    double pinhole[4], derived[3];
    modelToPinhole(model, pinhole, derived);
    RemapArgs args = {};
    args.w = model->width;
    args.h = model->height;
    args.half_w = pinhole[2];
    args.half_h = pinhole[3];
    args.inv_fx = 1.0 / pinhole[0];
    args.inv_fy = 1.0 / pinhole[1];
    args.roi_x = static_cast<double>(model->width) - kBorder - 1;
    args.roi_y = static_cast<double>(model->height) - kBorder - 1;
    if (model->type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL) {
      args.fx = args.fy = model->params[0];
      args.cx = model->params[1];
      args.cy = model->params[2];
      args.a = derived[0];
      args.k[0] = model->k[0];
      args.k[1] = model->k[1];
    } else {
      args.fx = model->params[0];
      args.fy = model->params[1];
      args.cx = model->params[2];
      args.cy = model->params[3];
      if (model->type == DSOPP_HIP_CAMERA_TUM_FOV) {
        args.a = std::tan(model->k[0] / 2);
        args.b = model->k[0];
      } else {
        for (int i = 0; i < model->num_k; ++i) args.k[i] = model->k[i];
      }
    }
    const size_t n = static_cast<size_t>(model->width) * model->height;
    auto u = std::make_unique<dsopp_hip_undistorter>();
    u->sr.init(device, stream);
    u->in_w = u->out_w = model->width;
    u->in_h = u->out_h = model->height;
    u->table.alloc(2 * n * sizeof(uint32_t));
    DeviceMem<float> maps;  // both planes, the second from the next multiple of 4 floats: 16-byte stores
    const size_t plane = (n + 3) / 4 * 4;
    float *d_map_x = nullptr, *d_map_y = nullptr;
    if (map_x_out) {
      maps.alloc(2 * plane * sizeof(float));
      d_map_x = maps.get();
      d_map_y = maps.get() + plane;
    }
    if (model->type == DSOPP_HIP_CAMERA_SIMPLE_RADIAL) {
      launchRemap<DSOPP_HIP_CAMERA_SIMPLE_RADIAL>(args, u->table.get(), d_map_x, d_map_y, u->sr.stream);
    } else if (model->type == DSOPP_HIP_CAMERA_TUM_FOV) {
      launchRemap<DSOPP_HIP_CAMERA_TUM_FOV>(args, u->table.get(), d_map_x, d_map_y, u->sr.stream);
    } else {
      launchRemap<DSOPP_HIP_CAMERA_ATAN>(args, u->table.get(), d_map_x, d_map_y, u->sr.stream);
    }
    if (map_x_out) {
      HIP_CHECK(hipMemcpyAsync(map_x_out, d_map_x, n * sizeof(float), hipMemcpyDeviceToHost, u->sr.stream));
      HIP_CHECK(hipMemcpyAsync(map_y_out, d_map_y, n * sizeof(float), hipMemcpyDeviceToHost, u->sr.stream));
    }
    u->sr.sync();
    for (int i = 0; i < 4 && pinhole_intrinsics_out; ++i) pinhole_intrinsics_out[i] = pinhole[i];
    *out = u.release();
  });
}

}  // extern "C"
