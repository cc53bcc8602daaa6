// Host-side C++ mirror of the reference's solver interfaces over the C-ABI (include/dsopp_hip.h).
//
// The reference selects its solvers through two abstract class templates:
//   energy::problem::PhotometricBundleAdjustment<Precision, SE3, PinholeCamera, 8, PixelMap, true, true, true, 1>
//       virtuals  pushFrame(const ActiveKeyframe&, size_t level, const Model&, FrameParameterization)      PBA_INC/photometric_bundle_adjustment.hpp:55-56
//                 updateLocalFrame(const ActiveKeyframe&)                                                   :127
//                 solve(size_t number_of_threads) -> Precision                                              :154
//       services  updateFrame(ActiveKeyframe&), getPose(time), getAffineBrightness(time)                   PROB_SRC/photometric_bundle_adjustment.cpp:156-264
//   energy::problem::PoseAlignment<SE3, PinholeCamera, 1, PixelMap, 1>                                      PA_INC/pose_alignment.hpp:24-63
//       virtuals  solve -> rmse | kZeroCost, reset(), pushKnownPose(time, Motion), setRotationPrior(Matrix3)
// Those headers drag in Eigen / Sophus / glog / Ceres / OpenCV, none of which exist in this build environment, so this
// file states the SAME interface (names, argument meaning, error behaviour) over small value types that carry exactly
// what the solvers read from `track::ActiveKeyframe` / `sensors::calibration::CameraCalibration`.  INTEGRATION.md shows
// the ~60-line adapter that derives from the reference's real base classes and forwards to these.
//
// Ownership mirrors the reference: the solver copies what it needs at pushFrame, image pyramids are borrowed (they must
// outlive the frame's stay in the solver, as the keyframe's PixelMap does there), single-threaded use per object.
#pragma once
#include <algorithm>
#include <array>
#include <cstdint>
#include <cstdlib>
#include <deque>
#include <map>
#include <memory>
#include <sstream>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>
#include <limits>
#include <functional>

#include "../../include/dsopp_hip.h"

namespace dsopp_hip_host {

using time_point = int64_t;                 // dsopp::time (time_point of the keyframe), as integer ticks
using Motion = std::array<double, 7>;       // energy::motion::SE3<Precision>: Sophus storage (qx, qy, qz, qw, tx, ty, tz)
using Vector2 = std::array<double, 2>;
using Matrix6 = std::array<double, 36>;

enum class FrameParameterization { kFree = 0, kFixed = 1 };  // PBA_INC/frame_parameterization.hpp:9-12

/** energy::model::PinholeCamera<Precision> at a pyramid level (focal lengths, principal point), pinhole_camera.hpp:21-200 */
struct PinholeModel {
  double fx, fy, cx, cy;
};

struct SolverError : std::runtime_error {
  int code;
  SolverError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  // the reference aborts through glog CHECK on contract violations; a library cannot, so violations throw
  if (rc != DSOPP_HIP_OK) throw SolverError(rc, dsopp_hip_last_error());
}

/** sensors::calibration::Undistorter (undistorter.hpp:24-152) on the device: either the two remap tables of constructRemaps as the
 *  reference's host code fills them, folded into a device table once per camera (no maps = Undistorter::Identity), or constructRemaps
 *  itself from the distorted camera model, evaluated and folded on the device (dsopp_hip_undistorter_create_from_model). */
class HipUndistorter {
 public:
  HipUndistorter(int in_width, int in_height, int out_width, int out_height, const float *remap_x, const float *remap_y, int device = 0,
                 void *stream = nullptr)
      : out_width_(out_width), out_height_(out_height) {
    check(dsopp_hip_undistorter_create(device, stream, in_width, in_height, out_width, out_height, remap_x, remap_y, &u_));
  }
  /** Undistorter::constructRemaps(model) (undistorter.hpp:69-90): in size = out size = the model's; remap_x_out / remap_y_out (both or
   *  neither) receive the two float tables, pinhole_out the target pinhole's (fx, fy, cx, cy) */
  explicit HipUndistorter(const dsopp_hip_camera_model &model, int device = 0, void *stream = nullptr, float *remap_x_out = nullptr,
                          float *remap_y_out = nullptr, double *pinhole_out = nullptr)
      : out_width_(model.width), out_height_(model.height) {
    check(dsopp_hip_undistorter_create_from_model(device, stream, &model, remap_x_out, remap_y_out, pinhole_out, &u_));
  }
  ~HipUndistorter() { dsopp_hip_undistorter_destroy(u_); }
  HipUndistorter(const HipUndistorter &) = delete;
  HipUndistorter &operator=(const HipUndistorter &) = delete;
  /** undistort(img) of an 8-bit single-channel image, blocking: the static mask and the vignette (camera_fabric.cpp:164-167) */
  std::vector<uint8_t> undistort(const uint8_t *image) const {
    std::vector<uint8_t> out(static_cast<size_t>(out_width_) * static_cast<size_t>(out_height_));
    check(dsopp_hip_undistorter_undistort(u_, image, out.data()));
    return out;
  }
  /** the same between two 4-byte aligned device images; only enqueues on `stream` (nullptr = the undistorter's own) */
  void undistortDevice(const void *image_dev, void *out_dev, void *stream = nullptr) const {
    check(dsopp_hip_undistorter_undistort_device(u_, image_dev, out_dev, stream));
  }
  /** undistort(img) of an 8-bit BGR frame (CV_8UC3, interleaved; any alignment) between device images, as camera.cpp:70 calls it: the
   *  colour result, its grey conversion (camera_features.cpp:32), or both — nullptr = not wanted; outputs 4-byte aligned; only enqueues */
  void undistortBgrDevice(const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream = nullptr) const {
    check(dsopp_hip_undistorter_undistort_bgr_device(u_, bgr_in_dev, bgr_out_dev, grey_out_dev, stream));
  }
  const dsopp_hip_undistorter *handle() const { return u_; }

 private:
  dsopp_hip_undistorter *u_ = nullptr;
  int out_width_, out_height_;
};

/** The camera's image transformers (camera_transformers/fabric.cpp:12-31) on the device: a CameraResizer at `resize_ratio` (1.0 = the YAML
 *  has no resize_transformer) followed by the ImageCropper down to a multiple of 2^crop_levels (the reference: kNumberOfPyramidLevels = 4).
 *  Runs behind the undistorter on every frame, class image, static mask and vignette; the integer arithmetic is stated at
 *  dsopp_hip_transformer_create. */
class HipImageTransformer {
 public:
  HipImageTransformer(int in_width, int in_height, double resize_ratio = 1.0, int crop_levels = 4, int device = 0, void *stream = nullptr) {
    check(dsopp_hip_transformer_create(device, stream, in_width, in_height, resize_ratio, crop_levels, &t_));
    check(dsopp_hip_transformer_sizes(t_, nullptr, nullptr, nullptr, nullptr, &out_width_, &out_height_));
  }
  ~HipImageTransformer() { dsopp_hip_transformer_destroy(t_); }
  HipImageTransformer(const HipImageTransformer &) = delete;
  HipImageTransformer &operator=(const HipImageTransformer &) = delete;
  int outWidth() const { return out_width_; }
  int outHeight() const { return out_height_; }
  /** transformCalibration of both transformers on a pinhole calibration (camera_fabric.cpp:157-159); needs no device */
  static PinholeModel transformCalibration(int in_width, int in_height, double resize_ratio, int crop_levels, const PinholeModel &model,
                                           double image_size[2]) {
    const double in[4] = {model.fx, model.fy, model.cx, model.cy};
    double out[4];
    check(dsopp_hip_transform_calibration(in_width, in_height, resize_ratio, crop_levels, in, image_size, out, nullptr, nullptr));
    return PinholeModel{out[0], out[1], out[2], out[3]};
  }
  /** runImageTransformers (linear) of an 8-bit single-channel image, blocking: the undistorted vignette (camera_fabric.cpp:167) */
  std::vector<uint8_t> transformImage(const uint8_t *image) const {
    std::vector<uint8_t> out(static_cast<size_t>(out_width_) * static_cast<size_t>(out_height_));
    check(dsopp_hip_transformer_transform_image(t_, image, out.data()));
    return out;
  }
  /** runMaskTransformers (nearest), blocking: the undistorted static mask (camera_fabric.cpp:164) */
  std::vector<uint8_t> transformMask(const uint8_t *mask) const {
    std::vector<uint8_t> out(static_cast<size_t>(out_width_) * static_cast<size_t>(out_height_));
    check(dsopp_hip_transformer_transform_mask(t_, mask, out.data()));
    return out;
  }
  /** either between two 4-byte aligned device images (interpolation 0 = linear, 1 = nearest); only enqueues on `stream` */
  void transformDevice(const void *in_dev, void *out_dev, int interpolation, void *stream = nullptr) const {
    check(dsopp_hip_transformer_transform_device(t_, in_dev, out_dev, interpolation, stream));
  }
  /** runImageTransformers (linear) of an 8-bit BGR frame (CV_8UC3, interleaved; any alignment) between device images: the colour result,
   *  its grey conversion (camera_features.cpp:32), or both — nullptr = not wanted; outputs 4-byte aligned; only enqueues */
  void transformBgrDevice(const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream = nullptr) const {
    check(dsopp_hip_transformer_transform_bgr_device(t_, bgr_in_dev, bgr_out_dev, grey_out_dev, stream));
  }
  const dsopp_hip_transformer *handle() const { return t_; }

 private:
  dsopp_hip_transformer *t_ = nullptr;
  int out_width_ = 0, out_height_ = 0;
};

/** sensors::calibration::camera_calibration::create (src/sensors/camera_calibration/src/fabric.cpp:23-113) over the C-ABI: the text of a
 *  calibration file becomes the calibration the tracker runs on and the undistorter in front of it.
 *    pinhole        W H / fx fy cx cy            (:23-31)  a pinhole calibration, Undistorter::Identity: no undistorter here
 *    simple_radial  W H / f cx cy k1 k2          (:33-51)  with transform_to_pinhole the pinhole of constructRemaps and its undistorter,
 *                                                          else the simple-radial calibration itself and no undistorter
 *    tum_fov        W H / fx fy cx cy fov        (:53-72)  focals and centre relative to the image size (:59-64); always to a pinhole
 *  parse() needs no device; undistorter() builds the device table at its first call.  What the reference logs and answers with nullopt —
 *  an unknown model type, tum_fov without transform_to_pinhole — and a text that ends early throw SolverError. */
class HipCameraCalibration {
 public:
  enum class ModelType { kPinholeCamera, kSimpleRadialCamera };  // energy::model::ModelType of the resulting calibration

  static HipCameraCalibration parse(const std::string &text, bool transform_to_pinhole = true) {
    std::istringstream in(text);
    std::string model_type;
    in >> model_type;
    HipCameraCalibration c;
    double v[5] = {0, 0, 0, 0, 0};
    const auto read = [&](int count) {
      in >> c.image_size_[0] >> c.image_size_[1];
      for (int i = 0; i < count; ++i) in >> v[i];
      if (!in) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the " + model_type + " calibration ends early or holds no number");
    };
    if (model_type == "pinhole") {
      read(4);
      c.intrinsics_ = {v[0], v[1], v[2], v[3], 0.0};
      return c;
    }
    if (model_type == "simple_radial") {
      read(5);
      if (!transform_to_pinhole) {
        c.type_ = ModelType::kSimpleRadialCamera;
        c.intrinsics_ = {v[0], v[1], v[2], v[3], v[4]};
        return c;
      }
      c.model_.type = DSOPP_HIP_CAMERA_SIMPLE_RADIAL;
      c.model_.num_k = 2;
      for (int i = 0; i < 3; ++i) c.model_.params[i] = v[i];
      c.model_.k[0] = v[3];
      c.model_.k[1] = v[4];
    } else if (model_type == "tum_fov") {
      if (!transform_to_pinhole) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "can't create a TUM FOV model without an undistorter");
      read(5);
      c.model_.type = DSOPP_HIP_CAMERA_TUM_FOV;
      c.model_.num_k = 1;
      c.model_.params[0] = v[0] * c.image_size_[0];
      c.model_.params[1] = v[1] * c.image_size_[1];
      c.model_.params[2] = v[2] * c.image_size_[0];
      c.model_.params[3] = v[3] * c.image_size_[1];
      c.model_.k[0] = v[4];
    } else {
      throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "inappropriate model type for a camera sensor: '" + model_type + "'");
    }
    c.distorted_ = true;
    c.model_.width = static_cast<int32_t>(c.image_size_[0]);  // the maps' size, as constructRemaps casts it (undistorter.hpp:82-83)
    c.model_.height = static_cast<int32_t>(c.image_size_[1]);
    double pinhole[4];
    check(dsopp_hip_camera_model_to_pinhole(&c.model_, pinhole, nullptr));
    c.intrinsics_ = {pinhole[0], pinhole[1], pinhole[2], pinhole[3], 0.0};
    return c;
  }

  ModelType type() const { return type_; }
  /** CameraCalibration::image_size() */
  double imageWidth() const { return image_size_[0]; }
  double imageHeight() const { return image_size_[1]; }
  /** CameraCalibration's intrinsics: (fx, fy, cx, cy) of a pinhole calibration, (f, cx, cy, k1, k2) of a simple-radial one */
  const std::array<double, 5> &intrinsics() const { return intrinsics_; }
  /** the pinhole the tracker runs on (a kPinholeCamera calibration only) */
  PinholeModel pinhole() const {
    if (type_ != ModelType::kPinholeCamera) throw SolverError(DSOPP_HIP_ERR_STATE, "the calibration is not a pinhole");
    return PinholeModel{intrinsics_[0], intrinsics_[1], intrinsics_[2], intrinsics_[3]};
  }
  /** whether an undistorter stands in front of the calibration, and the distorted model it is built from */
  bool hasUndistorter() const { return distorted_; }
  const dsopp_hip_camera_model &model() const {
    if (!distorted_) throw SolverError(DSOPP_HIP_ERR_STATE, "the calibration has no distorted model");
    return model_;
  }
  /** calibration.undistorter(): built from the model on the device by the first call; nullptr = Undistorter::Identity, which every
   *  consumer of the library takes as "frames arrive undistorted" */
  const HipUndistorter *undistorter(int device = 0, void *stream = nullptr) {
    if (distorted_ && !undistorter_) undistorter_ = std::make_unique<HipUndistorter>(model_, device, stream);
    return undistorter_.get();
  }

 private:
  HipCameraCalibration() = default;
  ModelType type_ = ModelType::kPinholeCamera;
  double image_size_[2] = {0, 0};
  std::array<double, 5> intrinsics_{};
  bool distorted_ = false;
  dsopp_hip_camera_model model_{};
  std::unique_ptr<HipUndistorter> undistorter_;
};

/** The per-camera constants of the `segmentation:` block (camera_fabric.cpp:54-99,170-186) on the device: the static mask as the camera
 *  keeps it (already undistorted, camera_fabric.cpp:164; nullptr = all valid), SemanticFilter::is_filtered_ (256 bytes; nullptr =
 *  filterBySemantic() is false) and the undistorter the class images go through (nullptr = they arrive undistorted; it must outlive
 *  this object).  width and height must be divisible by 2^(levels - 1). */
class HipSemantics {
 public:
  HipSemantics(int width, int height, int levels, const uint8_t *static_mask, const uint8_t *is_filtered256, const HipUndistorter *undistorter = nullptr,
               int device = 0, void *stream = nullptr) {
    check(dsopp_hip_semantics_create(device, stream, width, height, levels, static_mask, is_filtered256, undistorter ? undistorter->handle() : nullptr, &s_));
  }
  /** for a camera with image transformers: the size is the transformer's output, static_mask already undistorted and transformed
   *  (HipImageTransformer::transformMask), class images are remapped, resized (nearest) and cropped; both helpers must outlive this object */
  HipSemantics(const HipImageTransformer &transformer, int levels, const uint8_t *static_mask, const uint8_t *is_filtered256,
               const HipUndistorter *undistorter = nullptr, int device = 0, void *stream = nullptr) {
    check(dsopp_hip_semantics_create_transformed(device, stream, levels, static_mask, is_filtered256, undistorter ? undistorter->handle() : nullptr,
                                                 transformer.handle(), &s_));
  }
  ~HipSemantics() { dsopp_hip_semantics_destroy(s_); }
  HipSemantics(const HipSemantics &) = delete;
  HipSemantics &operator=(const HipSemantics &) = delete;
  const dsopp_hip_semantics *handle() const { return s_; }

 private:
  dsopp_hip_semantics *s_ = nullptr;
};

/** device-resident pyramid of one frame = features::PixelDataFrame / ActiveKeyframe::pyramids() + masks */
class DevicePyramid {
 public:
  DevicePyramid(int width, int height, int levels, int device = 0, void *stream = nullptr, int dtype = DSOPP_HIP_F64) {
    check(dsopp_hip_pyramid_create(device, stream, width, height, levels, dtype, &p_));
  }
  ~DevicePyramid() { dsopp_hip_pyramid_destroy(p_); }
  DevicePyramid(const DevicePyramid &) = delete;
  DevicePyramid &operator=(const DevicePyramid &) = delete;
  /** PixelDataFrame(image, photometric_calibration, vignetting, levels) */
  void build(const uint8_t *image, const double *photometric_calibration256 = nullptr, const uint8_t *vignetting = nullptr) {
    check(dsopp_hip_pyramid_build(p_, image, photometric_calibration256, vignetting));
  }
  /** PixelDataFrame(undistorter.undistort(distorted_image), ...) — camera.cpp:70: the frame as the provider delivers it (grey), the
   *  vignette already undistorted */
  void buildUndistorted(const HipUndistorter &undistorter, const uint8_t *distorted_image, const double *photometric_calibration256 = nullptr,
                        const uint8_t *undistorted_vignetting = nullptr) {
    check(dsopp_hip_pyramid_build_undistorted(p_, undistorter.handle(), distorted_image, photometric_calibration256, undistorted_vignetting));
  }
  /** PixelDataFrame(runImageTransformers(transformers, undistorter.undistort(frame)), ...) — camera.cpp:70 in full: remap (nullptr =
   *  the frame arrives undistorted), resize and crop on the device, the vignette already undistorted and transformed */
  void buildTransformed(const HipUndistorter *undistorter, const HipImageTransformer &transformer, const uint8_t *frame,
                        const double *photometric_calibration256 = nullptr, const uint8_t *transformed_vignetting = nullptr) {
    check(dsopp_hip_pyramid_build_transformed(p_, undistorter ? undistorter->handle() : nullptr, transformer.handle(), frame,
                                              photometric_calibration256, transformed_vignetting));
  }
  /** the same for the 8-bit BGR frame a colour provider delivers (camera_fabric.cpp:35): all three channels go through the remap and the
   *  transformers (either may be nullptr) and the grey conversion of the CameraFeatures ctor comes last (camera_features.cpp:32);
   *  keep_colour: the transformed colour image stays on the device for image(3, ...), as CameraFeatures::image() keeps it */
  void buildColour(const HipUndistorter *undistorter, const HipImageTransformer *transformer, const uint8_t *bgr_frame,
                   const double *photometric_calibration256 = nullptr, const uint8_t *transformed_vignetting = nullptr, bool keep_colour = false) {
    check(dsopp_hip_pyramid_build_colour(p_, undistorter ? undistorter->handle() : nullptr, transformer ? transformer->handle() : nullptr, bgr_frame,
                                         photometric_calibration256, transformed_vignetting, keep_colour ? 1 : 0));
  }
  /** the 8-bit image the pyramid keeps: channels = 1 CameraFeatures::frameData() (behind buildUndistorted, buildTransformed and
   *  buildColour), channels = 3 CameraFeatures::image() (behind buildColour with keep_colour); false, and `out` untouched, when it keeps
   *  none.  Blocking. */
  bool image(int channels, std::vector<uint8_t> &out) const {
    int present = 0, width = 0, height = 0;
    check(dsopp_hip_pyramid_get_image(p_, channels, nullptr, &present));
    if (!present) return false;
    check(dsopp_hip_pyramid_level_size(p_, 0, &width, &height));
    out.resize(static_cast<size_t>(channels) * static_cast<size_t>(width) * static_cast<size_t>(height));
    check(dsopp_hip_pyramid_get_image(p_, channels, out.data(), &present));
    return present != 0;
  }
  /** adopt a PixelMap<1> level built on the host by the reference */
  void setLevel(int level, const double *pixelinfo) { check(dsopp_hip_pyramid_set_level(p_, level, pixelinfo)); }
  void setMask(int level, const uint8_t *mask) { check(dsopp_hip_pyramid_set_mask(p_, level, mask)); }
  /** the frame's semantics: the class image as the provider delivers it (nullptr = none for this frame) is undistorted and kept
   *  (camera.cpp:57-65), filtered classes leave the camera mask (camera_mask.cpp:31-39) and the masks of all levels are written
   *  (camera_features.cpp:71-84); only enqueues, in either order with build* */
  void setSemantics(const HipSemantics &semantics, const uint8_t *class_image) {
    check(dsopp_hip_pyramid_set_semantics(p_, semantics.handle(), class_image));
  }
  /** semanticsData(0) of the frame: false when it has none */
  bool semantics(std::vector<uint8_t> &class_image, int width, int height) const {
    int present = 0;
    class_image.resize(static_cast<size_t>(width) * static_cast<size_t>(height));
    check(dsopp_hip_pyramid_get_semantics(p_, class_image.data(), &present));
    return present != 0;
  }
  dsopp_hip_pyramid *handle() const { return p_; }

 private:
  dsopp_hip_pyramid *p_ = nullptr;
};

/** the same image on every device of a multi-device solver (HipPhotometricBundleAdjustment with a `devices` list): one
 *  device-resident copy per distinct device, each built on its own device */
class DevicePyramidGroup {
 public:
  DevicePyramidGroup(dsopp_hip_window_group *group, int width, int height, int levels) {
    check(dsopp_hip_pyramid_group_create(group, width, height, levels, &p_));
  }
  ~DevicePyramidGroup() { dsopp_hip_pyramid_group_destroy(p_); }
  DevicePyramidGroup(const DevicePyramidGroup &) = delete;
  DevicePyramidGroup &operator=(const DevicePyramidGroup &) = delete;
  void build(const uint8_t *image, const double *photometric_calibration256 = nullptr, const uint8_t *vignetting = nullptr) {
    check(dsopp_hip_pyramid_group_build(p_, image, photometric_calibration256, vignetting));
  }
  void setLevel(int level, const double *pixelinfo) { check(dsopp_hip_pyramid_group_set_level(p_, level, pixelinfo)); }
  void setMask(int level, const uint8_t *mask) { check(dsopp_hip_pyramid_group_set_mask(p_, level, mask)); }
  /** DevicePyramid::setSemantics on every device's copy (all on the semantics object's device) */
  void setSemantics(const HipSemantics &semantics, const uint8_t *class_image) {
    check(dsopp_hip_pyramid_group_set_semantics(p_, semantics.handle(), class_image));
  }
  dsopp_hip_pyramid_group *handle() const { return p_; }

 private:
  dsopp_hip_pyramid_group *p_ = nullptr;
};

/** what the solvers read from track::landmarks::ActiveTrackingLandmark */
struct LandmarkView {
  Vector2 projection;
  double idepth;
  std::array<double, DSOPP_HIP_PATTERN_SIZE> patch;
  bool is_marginalized;
  bool is_outlier;
};

/** what the solvers read from / write to track::ActiveKeyframe<Motion> (frames/include/track/frames/active_keyframe.hpp:36-274) */
struct KeyframeView {
  int32_t keyframe_id;
  time_point timestamp;
  Motion t_world_agent;
  double exposure_time;
  Vector2 affine_brightness;
  bool is_marginalized;
  const DevicePyramid *pyramids;
  const DevicePyramidGroup *pyramid_group = nullptr;  // multi-device bundle adjustment: the image on every device of the solver
  std::vector<LandmarkView> active_landmarks;
  /** connections: other keyframe id -> statuses of THIS frame's landmarks reprojected into the other frame
   *  (FrameConnection::referenceReprojectionStatuses / targetReprojectionStatuses, whichever side this frame is) */
  std::map<int32_t, std::vector<uint8_t>> reprojection_statuses;
  // --- written back by updateFrame ---
  std::vector<double> idepth_variance;
  std::vector<int32_t> inlier_residuals;
  std::vector<double> relative_baseline;
  std::map<int32_t, Matrix6> covariances;
};

/** TrustRegionPhotometricBundleAdjustmentOptions<Precision> — trust_region_photometric_bundle_adjustment_options.hpp:14-52 */
struct TrustRegionOptions {
  size_t max_iterations;
  double initial_trust_region_radius, function_tolerance, parameter_tolerance;
  Vector2 affine_brightness_regularizer;
  double fixed_state_regularizer;
  double sigma_huber_loss = 5;
};

/** mirror of EigenPhotometricBundleAdjustment<SE3, PinholeCamera, 8, PixelMap, true, true, true, 1> backed by HIP kernels */
/** track::landmarks::ImmatureTrackingLandmark as the depth estimator reads and writes it
 *  (src/track/landmarks/include/track/landmarks/immature_tracking_landmark.hpp:26-106) */
struct ImmatureLandmarkView {
  Vector2 projection{};
  std::array<double, 3> direction{};
  std::array<double, 8> patch{};
  Vector2 gradient{};
  double idepth_min = 0, idepth_max = 1. / 0.001;
  double uniqueness = std::numeric_limits<double>::max(), search_pixel_interval = std::numeric_limits<double>::max();
  uint8_t status = 5;  // ImmatureStatus::kUninitialized
  bool traced = false;
};

/** tracker::DepthEstimation (src/tracker/depth_estimators/include/tracker/depth_estimators/depth_estimation.hpp:24-58): same
 *  static entry point, the target frame given as its device pyramid (level 0 is used, as monocular_tracker.cpp:98-100 does) */
struct HipDepthEstimation {
  static void estimate(const DevicePyramid &target_frame, std::vector<std::reference_wrapper<ImmatureLandmarkView>> &reference_landmarks,
                       const Motion &t_t_r, double reference_exposure_time, const Vector2 &reference_affine_brightness,
                       double target_exposure_time, const Vector2 &target_affine_brightness, const PinholeModel &model,
                       double sigma_huber_loss) {
    const size_t n = reference_landmarks.size();
    std::vector<double> proj(2 * n), dir(3 * n), patch(8 * n), grad(2 * n), imin(n), imax(n), uniq(n), spi(n);
    std::vector<uint8_t> status(n), traced(n);
    for (size_t i = 0; i < n; ++i) {
      const ImmatureLandmarkView &l = reference_landmarks[i];
      for (int k = 0; k < 2; ++k) {
        proj[2 * i + k] = l.projection[static_cast<size_t>(k)];
        grad[2 * i + k] = l.gradient[static_cast<size_t>(k)];
      }
      for (int k = 0; k < 3; ++k) dir[3 * i + k] = l.direction[static_cast<size_t>(k)];
      for (int k = 0; k < 8; ++k) patch[8 * i + k] = l.patch[static_cast<size_t>(k)];
      imin[i] = l.idepth_min;
      imax[i] = l.idepth_max;
      uniq[i] = l.uniqueness;
      spi[i] = l.search_pixel_interval;
      status[i] = l.status;
      traced[i] = l.traced ? 1 : 0;
    }
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    check(dsopp_hip_estimate_depths(target_frame.handle(), 0, intr, t_t_r.data(), reference_exposure_time, reference_affine_brightness.data(),
                                    target_exposure_time, target_affine_brightness.data(), sigma_huber_loss, static_cast<int32_t>(n), proj.data(),
                                    dir.data(), patch.data(), grad.data(), imin.data(), imax.data(), uniq.data(), spi.data(), status.data(),
                                    traced.data()));
    for (size_t i = 0; i < n; ++i) {
      ImmatureLandmarkView &l = reference_landmarks[i];
      l.idepth_min = imin[i];
      l.idepth_max = imax[i];
      l.uniqueness = uniq[i];
      l.search_pixel_interval = spi[i];
      l.status = status[i];
      l.traced = traced[i] != 0;
    }
  }
};

/** Reference depth maps of the newest keyframe, resident on the device: what tracker::createReferenceDepthMaps
 *  (src/tracker/tracker/src/create_depth_maps.cpp:124-147) returns as std::vector<energy::problem::DepthMap>. */
class DeviceDepthMaps {
 public:
  explicit DeviceDepthMaps(dsopp_hip_depth_maps *m = nullptr) : m_(m) {}
  ~DeviceDepthMaps() { dsopp_hip_depth_maps_destroy(m_); }
  DeviceDepthMaps(const DeviceDepthMaps &) = delete;
  DeviceDepthMaps &operator=(const DeviceDepthMaps &) = delete;
  DeviceDepthMaps(DeviceDepthMaps &&o) noexcept : m_(o.m_) { o.m_ = nullptr; }
  const dsopp_hip_depth_maps *handle() const { return m_; }
  dsopp_hip_depth_maps *mutableHandle() { return m_; }
  /** calculateMeanSquareOpticalFlow(reference_frame_depth_map[level], t_t_r, model) — monocular_tracker.cpp:104-134 — for up
   *  to four relative poses in one pass over the device-resident map (the tracker needs t_t_r and t_t_r without rotation) */
  std::vector<double> meanSquareOpticalFlow(int level, const std::vector<Motion> &t_t_r, const PinholeModel &model) const {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    std::vector<double> T(7 * t_t_r.size()), flow(t_t_r.size());
    for (size_t i = 0; i < t_t_r.size(); ++i) std::copy(t_t_r[i].begin(), t_t_r[i].end(), T.begin() + 7 * static_cast<long>(i));
    check(dsopp_hip_depth_maps_mean_square_optical_flow(m_, level, intr, static_cast<int32_t>(t_t_r.size()), T.data(), flow.data()));
    return flow;
  }
  /** host copy of one level: two row-major H x W planes (DepthMap::map(x, y).idepth / .weight) */
  void level(int level, std::vector<double> &idepth_sum, std::vector<double> &weight, int &width, int &height) const {
    int32_t w = 0, h = 0;
    check(dsopp_hip_depth_maps_level_size(m_, level, &w, &h));
    idepth_sum.assign(static_cast<size_t>(w) * h, 0.0);
    weight.assign(static_cast<size_t>(w) * h, 0.0);
    check(dsopp_hip_depth_maps_get_level(m_, level, idepth_sum.data(), weight.data()));
    width = w;
    height = h;
  }

 private:
  dsopp_hip_depth_maps *m_;
};

/** The two images MonocularTracker::tick pushes to its camera_output_interface_, rendered on the device as interleaved 8-bit BGR:
 *  frame() stands where debugCurrentFrame(features) is called (monocular_tracker.cpp:485-487), keyframe() where
 *  debugCurrentKeyframe(features, reference_frame_depth_map_[0], maximum_visualized_idepth_) is (:511-514).  The object holds
 *  maximum_visualized_idepth_ (one per tracker); the depth maps are read where they lie.  A caller that links OpenCV passes its JET table
 *  (cv::applyColorMap of a 0 .. 255 ramp) and its radius-3 circle (cv::circle on a 7 x 7 image); nullptr = the library's own. */
class HipDebugViews {
 public:
  HipDebugViews(int width, int height, const uint8_t *colormap_bgr256 = nullptr, const uint8_t *stencil7x7 = nullptr, int device = 0,
                void *stream = nullptr)
      : width_(width), height_(height) {
    check(dsopp_hip_debug_views_create(device, stream, width, height, colormap_bgr256, stencil7x7, &v_));
  }
  ~HipDebugViews() { dsopp_hip_debug_views_destroy(v_); }
  HipDebugViews(const HipDebugViews &) = delete;
  HipDebugViews &operator=(const HipDebugViews &) = delete;
  /** debugCurrentFrame: the grey image the pyramid keeps, red where its level-0 mask is 0; height x width x 3 bytes.  Blocking. */
  std::vector<uint8_t> frame(const DevicePyramid &pyramid) {
    std::vector<uint8_t> bgr(size());
    check(dsopp_hip_debug_views_frame(v_, pyramid.handle(), nullptr, bgr.data()));
    return bgr;
  }
  /** debugCurrentKeyframe: the kept grey image under the jet-coloured circles of level 0 of `maps`; updates maximumIdepth().  Blocking. */
  std::vector<uint8_t> keyframe(const DevicePyramid &pyramid, const DeviceDepthMaps &maps) {
    std::vector<uint8_t> bgr(size());
    check(dsopp_hip_debug_views_keyframe(v_, pyramid.handle(), nullptr, maps.handle(), bgr.data(), nullptr, nullptr));
    return bgr;
  }
  /** maximum_visualized_idepth_ (0 = not set yet) */
  double maximumIdepth() const {
    double m = 0;
    check(dsopp_hip_debug_views_get_maximum_idepth(v_, &m));
    return m;
  }
  dsopp_hip_debug_views *handle() const { return v_; }

 private:
  size_t size() const { return 3 * static_cast<size_t>(width_) * static_cast<size_t>(height_); }
  int width_, height_;
  dsopp_hip_debug_views *v_ = nullptr;
};

class HipPhotometricBundleAdjustment {
 public:
  /** EigenPhotometricBundleAdjustment(options, estimate_uncertainty, force_accept) — eigen_photometric_bundle_adjustment.cpp:47-57 */
  HipPhotometricBundleAdjustment(const TrustRegionOptions &o, bool estimate_uncertainty = true, bool force_accept = true, int device = 0)
      : HipPhotometricBundleAdjustment(o, estimate_uncertainty, force_accept, std::vector<int>{device}) {}
  /** the single-process multi-GPU form (fabric_hip.patch: `devices: "0 1 2 3"`): the landmarks of every keyframe are sharded over
   *  `devices`, frames / images replicated, one all-reduce of the reduced system per Gauss-Newton iteration (dsopp_hip_window_group).
   *  `transport`: DSOPP_HIP_TRANSPORT_AUTO = RCCL between distinct devices */
  HipPhotometricBundleAdjustment(const TrustRegionOptions &o, bool estimate_uncertainty, bool force_accept, const std::vector<int> &devices,
                                 int transport = DSOPP_HIP_TRANSPORT_AUTO)
      : estimate_uncertainty_(estimate_uncertainty) {
    dsopp_hip_options c;
    dsopp_hip_default_pba_options(&c);
    c.max_iterations = static_cast<int32_t>(o.max_iterations);
    c.initial_trust_region_radius = o.initial_trust_region_radius;
    c.function_tolerance = o.function_tolerance;
    c.parameter_tolerance = o.parameter_tolerance;
    c.affine_brightness_regularizer[0] = o.affine_brightness_regularizer[0];
    c.affine_brightness_regularizer[1] = o.affine_brightness_regularizer[1];
    c.fixed_state_regularizer = o.fixed_state_regularizer;
    c.sigma_huber_loss = o.sigma_huber_loss;
    c.estimate_uncertainty = estimate_uncertainty ? 1 : 0;
    c.force_accept = force_accept ? 1 : 0;
    std::vector<int32_t> ids(devices.begin(), devices.end());
    check(dsopp_hip_window_group_create(&c, ids.data(), static_cast<int32_t>(ids.size()), transport, &g_));
    n_shards_ = static_cast<int>(ids.size());
    if (n_shards_ == 1) check(dsopp_hip_window_group_shard(g_, 0, &w_, nullptr));  // a group of one IS this window
  }
  ~HipPhotometricBundleAdjustment() { dsopp_hip_window_group_destroy(g_); }
  HipPhotometricBundleAdjustment(const HipPhotometricBundleAdjustment &) = delete;
  HipPhotometricBundleAdjustment &operator=(const HipPhotometricBundleAdjustment &) = delete;

  /** pushFrame(frame, level, model, frame_parameterization): local copy of the keyframe + residual lists between the new
   *  frame and all previous ones (photometric_bundle_adjustment.cpp:98-124); folds pending marginalisations first
   *  (eigen_photometric_bundle_adjustment.cpp:119-141) */
  void pushFrame(const KeyframeView &frame, size_t level, const PinholeModel &model,
                 FrameParameterization frame_parameterization = FrameParameterization::kFree) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    const int fixed = frame_parameterization == FrameParameterization::kFixed ? 1 : 0;
    if (frame.pyramid_group) {
      check(dsopp_hip_window_group_push_frame(g_, frame.keyframe_id, frame.timestamp, frame.pyramid_group->handle(), static_cast<int>(level), intr,
                                              frame.t_world_agent.data(), frame.exposure_time, frame.affine_brightness.data(), fixed,
                                              frame.is_marginalized ? 1 : 0));
    } else {
      if (!w_) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "a multi-device solver needs KeyframeView::pyramid_group (the image on every device)");
      check(dsopp_hip_window_push_frame(w_, frame.keyframe_id, frame.timestamp, frame.pyramids->handle(), static_cast<int>(level), intr,
                                        frame.t_world_agent.data(), frame.exposure_time, frame.affine_brightness.data(), fixed,
                                        frame.is_marginalized ? 1 : 0));
    }
    times_[frame.timestamp] = frame.keyframe_id;
    uploadLandmarks(frame);
    uploadConnections(frame);
  }
  /** updateLocalFrame(frame): freshly matured landmarks, marginalisation flags, new connections
   *  (eigen_photometric_bundle_adjustment.cpp:103-113, local_frame.hpp:484-521) */
  void updateLocalFrame(const KeyframeView &frame) {
    uploadLandmarks(frame);
    uploadConnections(frame);
    if (frame.is_marginalized) check(dsopp_hip_window_group_mark_frame_marginalized(g_, frame.keyframe_id));
  }
  /** tracker::createReferenceDepthMaps(active frames, calibration) for the window this solver holds, without leaving the
   *  device (monocular_tracker.cpp:465,509 call it right after the bundle adjustment, on the same keyframes) */
  DeviceDepthMaps createReferenceDepthMaps(int levels) {
    dsopp_hip_depth_maps *m = nullptr;
    check(dsopp_hip_window_group_create_reference_depth_maps(g_, levels, &m));
    return DeviceDepthMaps(m);
  }
  /** reference_frame_depth_map_ = createReferenceDepthMaps(...) into the object the tracker already holds (no allocation) */
  void createReferenceDepthMaps(DeviceDepthMaps &maps) { check(dsopp_hip_window_group_refill_reference_depth_maps(g_, maps.mutableHandle())); }
  /** solve(number_of_threads) -> final energy; number_of_threads is accepted and ignored, as in the Eigen backend */
  double solve(const size_t number_of_threads = 1) {
    (void)number_of_threads;
    double e = 0;
    int32_t it = 0, nv = 0;
    check(dsopp_hip_window_group_solve(g_, &e, &it, &nv));
    return e;
  }
  /** updateFrame(frame): poses, affine brightness, idepths, variances, inlier counts, baselines, statuses, covariances
   *  (photometric_bundle_adjustment.cpp:182-264) */
  void updateFrame(KeyframeView &frame) {
    check(dsopp_hip_window_group_get_pose(g_, frame.keyframe_id, frame.t_world_agent.data(), frame.affine_brightness.data()));
    int32_t n = 0;
    check(dsopp_hip_window_group_num_landmarks(g_, frame.keyframe_id, &n));
    std::vector<double> &idepth = scratch_idepth_, &inv_h = scratch_uv_, &baseline = scratch_patch_;  // (the solver's scratch: see uploadLandmarks)
    std::vector<int32_t> &inliers = scratch_inliers_;
    std::vector<uint8_t> &flags = scratch_flags_, &statuses = scratch_statuses_;
    idepth.resize(static_cast<size_t>(n));
    inv_h.resize(static_cast<size_t>(n));
    baseline.resize(static_cast<size_t>(n));
    inliers.resize(static_cast<size_t>(n));
    flags.resize(static_cast<size_t>(n));
    // one packed transfer for the landmark arrays and the statuses towards every connected frame
    std::vector<int32_t> &targets = scratch_targets_;
    targets.clear();
    for (const auto &kv : frame.reprojection_statuses)
      if (static_cast<int32_t>(kv.second.size()) == n && n > 0) targets.push_back(kv.first);
    statuses.resize(targets.size() * static_cast<size_t>(n));
    check(dsopp_hip_window_group_get_frame_update(g_, frame.keyframe_id, idepth.data(), inv_h.data(), baseline.data(), inliers.data(), flags.data(),
                                            static_cast<int32_t>(targets.size()), targets.data(), statuses.data()));
    // entries of landmarks the solver has not written yet start at the reference's defaults; entries of marginalised
    // landmarks are left as they are (photometric_bundle_adjustment.cpp:232-262 `continue`s before touching them)
    frame.idepth_variance.resize(n, 1e-5);
    frame.inlier_residuals.resize(n, 0);
    frame.relative_baseline.resize(n, 0.0);
    const double kIdepthEps = 1e-8;
    for (int32_t i = 0; i < n && i < static_cast<int32_t>(frame.active_landmarks.size()); ++i) {
      LandmarkView &lm = frame.active_landmarks[static_cast<size_t>(i)];
      if (flags[i] & 2) lm.is_outlier = true;
      if (flags[i] & 1) continue;  // marginalised landmarks keep their values
      if (std::abs(idepth[i]) < kIdepthEps)
        lm.idepth = 0;
      else if (idepth[i] < 0)
        lm.is_outlier = true;
      else
        lm.idepth = idepth[i];
      frame.idepth_variance[i] = estimate_uncertainty_ ? inv_h[i] : 1e-5;  // :252-254
      frame.inlier_residuals[i] = inliers[i];
      if (baseline[i] > frame.relative_baseline[i]) frame.relative_baseline[i] = baseline[i];
    }
    for (size_t k = 0; k < targets.size(); ++k)
      frame.reprojection_statuses[targets[k]].assign(statuses.begin() + static_cast<long>(k * static_cast<size_t>(n)),
                                                     statuses.begin() + static_cast<long>((k + 1) * static_cast<size_t>(n)));
    for (auto &kv : frame.reprojection_statuses) {
      if (kv.second.empty()) continue;
      Matrix6 cov;
      if (estimate_uncertainty_ && dsopp_hip_window_group_get_covariance(g_, frame.keyframe_id, kv.first, cov.data()) == DSOPP_HIP_OK)
        frame.covariances[kv.first] = cov;
    }
  }
  Motion getPose(time_point timestamp) const {
    Motion T;
    check(dsopp_hip_window_group_get_pose(g_, idOf(timestamp), T.data(), nullptr));
    return T;
  }
  Vector2 getAffineBrightness(time_point timestamp) const {
    Vector2 ab{0, 0};
    auto it = times_.find(timestamp);
    if (it == times_.end()) return ab;  // the reference returns zero for an unknown frame
    check(dsopp_hip_window_group_get_pose(g_, it->second, nullptr, ab.data()));
    return ab;
  }
  /** addSemanticObservations(track, marginalized_keyframes_ids, model) — monocular_tracker.cpp:263-305, called at :506 with the
   *  keyframes the marginalisation just chose, after updateLocalFrame has flagged them: the class codes under every reprojected pattern
   *  are counted on the device, from the class images the frames' pyramids keep */
  void addSemanticObservations(const std::vector<int32_t> &marginalized_keyframe_ids) {
    check(dsopp_hip_window_group_add_semantic_observations(g_, static_cast<int32_t>(marginalized_keyframe_ids.size()), marginalized_keyframe_ids.data()));
  }
  /** semantic_type_observations_ of every landmark of a keyframe (256 counters each), before the keyframe leaves the solver */
  std::vector<uint8_t> semanticObservations(int32_t keyframe_id) {
    int32_t n = 0;
    check(dsopp_hip_window_group_num_landmarks(g_, keyframe_id, &n));
    std::vector<uint8_t> hist(static_cast<size_t>(n) * 256);
    if (n) check(dsopp_hip_window_group_get_semantic_observations(g_, keyframe_id, hist.data()));
    return hist;
  }
  /** ActiveTrackingLandmark::semanticTypeId(legend) of every landmark of a keyframe; legend_weights256 = SemanticLegend::weights_,
   *  nullptr = no legend */
  std::vector<uint8_t> semanticTypes(int32_t keyframe_id, const uint64_t *legend_weights256 = nullptr) {
    int32_t n = 0;
    check(dsopp_hip_window_group_num_landmarks(g_, keyframe_id, &n));
    std::vector<uint8_t> type(static_cast<size_t>(n));
    if (n) check(dsopp_hip_window_group_get_semantic_types(g_, keyframe_id, legend_weights256, type.data()));
    return type;
  }
  /** the one device window of a single-device solver (nullptr for a multi-device one): what the device-resident landmark
   *  activation reads, which needs ALL active landmarks of the window on one device */
  dsopp_hip_window *handle() const { return w_; }
  dsopp_hip_window_group *group() const { return g_; }
  int numDevices() const { return n_shards_; }

 private:
  int32_t idOf(time_point t) const {
    auto it = times_.find(t);
    if (it == times_.end()) throw SolverError(DSOPP_HIP_ERR_NOT_FOUND, "no local copy of this frame in the solver");
    return it->second;
  }
  void uploadLandmarks(const KeyframeView &frame) {
    const size_t n = frame.active_landmarks.size();
    // flags of every landmark, coordinates / inverse depth / patch only of those the device does not hold yet (the C-ABI reads these
    // arrays from its own landmark count on)
    int32_t held = 0;
    check(dsopp_hip_window_group_num_landmarks(g_, frame.keyframe_id, &held));
    // (scratch kept with the solver: updateLocalFrame runs for every keyframe of the window three times per keyframe step, and four fresh
    // zero-filled arrays of all its landmarks per call were a measurable part of that step's host time)
    std::vector<double> &uv = scratch_uv_, &idepth = scratch_idepth_, &patch = scratch_patch_;
    std::vector<uint8_t> &flags = scratch_flags_;
    uv.resize(2 * n);
    idepth.resize(n);
    patch.resize(DSOPP_HIP_PATTERN_SIZE * n);
    flags.resize(n);
    for (size_t i = 0; i < n; ++i) {
      const LandmarkView &lm = frame.active_landmarks[i];
      flags[i] = static_cast<uint8_t>((lm.is_marginalized ? 1 : 0) | (lm.is_outlier ? 2 : 0));
      if (i < static_cast<size_t>(held)) continue;
      uv[2 * i] = lm.projection[0];
      uv[2 * i + 1] = lm.projection[1];
      idepth[i] = lm.idepth;
      for (int k = 0; k < DSOPP_HIP_PATTERN_SIZE; ++k) patch[DSOPP_HIP_PATTERN_SIZE * i + static_cast<size_t>(k)] = lm.patch[static_cast<size_t>(k)];
    }
    check(dsopp_hip_window_group_set_landmarks(g_, frame.keyframe_id, static_cast<int32_t>(n), uv.data(), idepth.data(), patch.data(), flags.data()));
  }
  void uploadConnections(const KeyframeView &frame) {
    int32_t nf = 0;
    check(dsopp_hip_window_group_num_frames(g_, &nf));
    for (const auto &kv : frame.reprojection_statuses) {
      if (kv.second.empty()) continue;
      const int rc = dsopp_hip_window_group_set_connection(g_, frame.keyframe_id, kv.first, static_cast<int32_t>(kv.second.size()), kv.second.data());
      if (rc != DSOPP_HIP_OK && rc != DSOPP_HIP_ERR_NOT_FOUND) check(rc);
    }
  }
  std::vector<double> scratch_uv_, scratch_idepth_, scratch_patch_;
  std::vector<uint8_t> scratch_flags_, scratch_statuses_;
  std::vector<int32_t> scratch_inliers_, scratch_targets_;
  dsopp_hip_window_group *g_ = nullptr;
  dsopp_hip_window *w_ = nullptr;  // shard 0's window when the group has one shard
  int n_shards_ = 1;
  bool estimate_uncertainty_;
  std::map<time_point, int32_t> times_;
};

/** what MonocularTracker::estimatePose leaves behind (monocular_tracker.cpp:179-245): the new frame's pose and affine brightness,
 *  whether an initialisation passed the per-level rmse gates, how many were tried and the LM iterations spent */
struct PoseEstimate {
  Motion t_world_target;
  Vector2 affine_brightness;
  bool success;
  int tries, lm_iterations;
};

/** mirror of EigenPoseAlignment<SE3, PinholeCamera, 1, PixelMap, 1, true> backed by HIP kernels */
class HipPoseAlignment {
 public:
  static constexpr double kZeroCost = -1;  // PA_INC/pose_alignment.hpp
  explicit HipPoseAlignment(const TrustRegionOptions &o, int device = 0, void *stream = nullptr) {
    dsopp_hip_options c;
    dsopp_hip_default_align_options(&c);
    c.max_iterations = static_cast<int32_t>(o.max_iterations);
    c.initial_trust_region_radius = o.initial_trust_region_radius;
    c.function_tolerance = o.function_tolerance;
    c.parameter_tolerance = o.parameter_tolerance;
    c.affine_brightness_regularizer[0] = o.affine_brightness_regularizer[0];
    c.affine_brightness_regularizer[1] = o.affine_brightness_regularizer[1];
    c.sigma_huber_loss = o.sigma_huber_loss;
    check(dsopp_hip_aligner_create(&c, device, stream, &a_));
  }
  ~HipPoseAlignment() { dsopp_hip_aligner_destroy(a_); }
  HipPoseAlignment(const HipPoseAlignment &) = delete;
  HipPoseAlignment &operator=(const HipPoseAlignment &) = delete;

  void reset() { check(dsopp_hip_aligner_reset(a_)); }
  /** pushFrame(timestamp, t_world_agent, pyramids, masks, depths_maps, exposure, affine, level, model, kFixed)
   *  — photometric_bundle_adjustment.cpp:58-74; depth maps are H_l x W_l {idepth sum, weight} (energy/problems/depth_map.hpp) */
  void pushFrame(time_point timestamp, const Motion &t_world_agent, const DevicePyramid &pyramids, const double *depth_idepth_sum,
                 const double *depth_weight, double exposure_time, const Vector2 &affine_brightness, size_t level, const PinholeModel &model) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    check(dsopp_hip_aligner_push_reference_depth_map(a_, timestamp, t_world_agent.data(), pyramids.handle(), static_cast<int>(level), intr,
                                                     depth_idepth_sum, depth_weight, exposure_time, affine_brightness.data()));
  }
  /** the same overload fed from device-resident maps (HipPhotometricBundleAdjustment::createReferenceDepthMaps) */
  void pushFrame(time_point timestamp, const Motion &t_world_agent, const DevicePyramid &pyramids, const DeviceDepthMaps &depth_maps,
                 double exposure_time, const Vector2 &affine_brightness, size_t level, const PinholeModel &model) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    check(dsopp_hip_aligner_push_reference_depth_maps(a_, timestamp, t_world_agent.data(), pyramids.handle(), static_cast<int>(level), intr,
                                                      depth_maps.handle(), exposure_time, affine_brightness.data()));
  }
  /** pushFrame(timestamp, t_world_agent_init, pyramids, masks, exposure, affine, level, model, kFree) — :131-154 */
  void pushFrame(time_point timestamp, const Motion &t_world_agent_init, const DevicePyramid &pyramids, double exposure_time,
                 const Vector2 &affine_brightness, size_t level, const PinholeModel &model) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    check(dsopp_hip_aligner_push_target(a_, timestamp, t_world_agent_init.data(), pyramids.handle(), static_cast<int>(level), intr,
                                        exposure_time, affine_brightness.data()));
    target_time_ = timestamp;
  }
  /** setRotationPrior(r_t_r) — pose_alignment.hpp:39, eigen_pose_alignment.cpp:254-257 (row-major 3x3) */
  void setRotationPrior(const std::array<double, 9> &r_t_r) { check(dsopp_hip_aligner_set_rotation_prior(a_, r_t_r.data())); }
  void pushKnownPose(time_point timestamp, const Motion &t_w_agent) { check(dsopp_hip_aligner_push_known_pose(a_, timestamp, t_w_agent.data())); }
  /** solve(number_of_threads) -> rmse, or kZeroCost when the pose was known */
  double solve(const size_t number_of_threads = 1) {
    (void)number_of_threads;
    check(dsopp_hip_aligner_solve(a_, &last_));
    return last_.rmse;
  }
  /** estimatePose of the tracker (monocular_tracker.cpp:179-245) as ONE call: for every initialisation in turn, coarse to fine over the
   *  levels of the target pyramid { reset; pushFrame(keyframe, depth map of the level); pushFrame(target, current estimate); solve; gate on
   *  2.5 x rmse_last_pose_estimation[level] } — the loop the tracker runs over this object, executed by one persistent launch per frame
   *  (up to 8 initialisations per launch once a first one has failed).  `rmse_last_pose_estimation` (one entry per level) is updated
   *  as the reference updates it. */
  PoseEstimate estimatePose(time_point reference_time, const Motion &t_world_reference, const DevicePyramid &reference_pyramids,
                            const DeviceDepthMaps &reference_depth_maps, double reference_exposure_time, const Vector2 &reference_affine_brightness,
                            time_point target_time, const DevicePyramid &target_pyramids, double target_exposure_time, const PinholeModel &model,
                            const std::vector<Motion> &initializations, const Vector2 &affine_brightness_init,
                            std::vector<double> &rmse_last_pose_estimation) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    std::vector<double> inits(7 * initializations.size());
    for (size_t i = 0; i < initializations.size(); ++i) std::copy(initializations[i].begin(), initializations[i].end(), inits.begin() + 7 * static_cast<long>(i));
    PoseEstimate out{};
    int32_t success = 0, tries = 0, its = 0;
    check(dsopp_hip_aligner_estimate_pose(a_, reference_time, t_world_reference.data(), reference_pyramids.handle(), reference_depth_maps.handle(),
                                          reference_exposure_time, reference_affine_brightness.data(), target_time, target_pyramids.handle(),
                                          target_exposure_time, intr, static_cast<int32_t>(initializations.size()), inits.data(),
                                          affine_brightness_init.data(), rmse_last_pose_estimation.data(), out.t_world_target.data(),
                                          out.affine_brightness.data(), &success, &tries, &its));
    out.success = success != 0;
    out.tries = tries;
    out.lm_iterations = its;
    return out;
  }
  Motion getPose(time_point) const {
    Motion T;
    for (int i = 0; i < 7; ++i) T[static_cast<size_t>(i)] = last_.T_world_target[i];
    return T;
  }
  Vector2 getAffineBrightness(time_point) const { return {last_.affine_brightness[0], last_.affine_brightness[1]}; }
  Matrix6 tTargetReferenceCovariance() const {
    Matrix6 c;
    for (int i = 0; i < 36; ++i) c[static_cast<size_t>(i)] = last_.covariance[i];
    return c;
  }

 private:
  dsopp_hip_aligner *a_ = nullptr;
  dsopp_hip_align_result last_{};
  time_point target_time_ = 0;
};

/** What both device tracking-feature extractors share (one handle type, dsopp_hip_feature_extractor): extract() mirrors
 *  TrackingFeaturesExtractor::extract(image, mask) and returns the features' coordinates (TrackingFeaturesFrame); the list also stays on
 *  the device for DeviceImmatureSet's constructor from an extractor. */
class HipTrackingFeaturesExtractor {
 public:
  using Feature = std::array<double, 2>;
  ~HipTrackingFeaturesExtractor() { dsopp_hip_feature_extractor_destroy(ex_); }
  HipTrackingFeaturesExtractor(const HipTrackingFeaturesExtractor &) = delete;
  HipTrackingFeaturesExtractor &operator=(const HipTrackingFeaturesExtractor &) = delete;
  /** image: W x H 8-bit grey (CameraFeatures::frame_data_); mask: the camera's level-0 CameraMask bytes, nullptr = all valid.  Without
   *  semantic filtering the mask is a per-camera constant (CameraFeatures::pyramidOfMasks()[0]): it is eroded again only when a
   *  different array is passed.  With it the mask is the frame's: setMaskFromPyramid. */
  std::vector<Feature> extract(const uint8_t *image, const uint8_t *mask) {
    return run(mask, [&](int32_t capacity, int32_t *n) { return dsopp_hip_feature_extractor_extract(ex_, image, capacity, xy_.data(), n); });
  }
  /** the same of the undistorted frame that `pyramid` kept from its last buildUndistorted: no second upload of the image */
  std::vector<Feature> extractFromPyramid(const DevicePyramid &pyramid, const uint8_t *mask) {
    return run(mask, [&](int32_t capacity, int32_t *n) {
      return dsopp_hip_feature_extractor_extract_from_pyramid(ex_, pyramid.handle(), capacity, xy_.data(), n);
    });
  }
  /** the frame's level-0 mask, which `pyramid` kept from its last setSemantics, eroded on the device with no host copy; it stays the
   *  extractor's mask for the extractFromPyramid(pyramid) that follows and until another mask is passed */
  void setMaskFromPyramid(const DevicePyramid &pyramid) {
    check(dsopp_hip_feature_extractor_set_mask_from_pyramid(ex_, pyramid.handle()));
    mask_ = &from_pyramid_;
    mask_set_ = true;
  }
  /** extractFromPyramid with the mask the extractor holds (the last setMaskFromPyramid or extract) */
  std::vector<Feature> extractFromPyramid(const DevicePyramid &pyramid) { return extractFromPyramid(pyramid, mask_set_ ? mask_ : nullptr); }
  const dsopp_hip_feature_extractor *handle() const { return ex_; }

 protected:
  HipTrackingFeaturesExtractor() = default;
  dsopp_hip_feature_extractor *ex_ = nullptr;

 private:
  /** set the mask when it changed, then `call(capacity, &n)`, once more with the room reported when the capacity was too small */
  template <typename Call>
  std::vector<Feature> run(const uint8_t *mask, Call call) {
    if (!mask_set_ || mask != mask_) {
      check(dsopp_hip_feature_extractor_set_mask(ex_, mask));
      mask_ = mask;
      mask_set_ = true;
    }
    int32_t n = 0;
    int rc = call(static_cast<int32_t>(xy_.size() / 2), &n);
    if (rc == DSOPP_HIP_ERR_CAPACITY) {  // the state is unchanged: run again with the room reported
      xy_.resize(2 * static_cast<size_t>(n));
      rc = call(n, &n);
    }
    check(rc);
    std::vector<Feature> out(static_cast<size_t>(n));
    for (size_t i = 0; i < out.size(); ++i) out[i] = {xy_[2 * i], xy_[2 * i + 1]};
    return out;
  }
  const uint8_t *mask_ = nullptr;
  bool mask_set_ = false;
  uint8_t from_pyramid_ = 0;  // its address stands for "the mask came from a pyramid" in mask_
  std::vector<double> xy_ = std::vector<double>(2 * 4096);
};

/** features::SobelTrackingFeaturesExtractor (src/features/src/sobel_tracking_features_extractor.cpp:70-134) on the device: the candidate
 *  pixels of a new keyframe.  Stateful as the reference: the first extract fixes the gradient-norm threshold and the window size, every
 *  later call adapts the threshold. */
class HipSobelTrackingFeaturesExtractor : public HipTrackingFeaturesExtractor {
 public:
  HipSobelTrackingFeaturesExtractor(int width, int height, double point_density_for_detector = 1500, double quantile_level = 0.6,
                                    int device = 0, void *stream = nullptr) {
    check(dsopp_hip_feature_extractor_create(device, stream, width, height, point_density_for_detector, quantile_level, &ex_));
  }
};

/** features::EigenTrackingFeaturesExtractor (src/features/src/eigen_tracking_features_extractor.cpp:432-469) on the device, the extractor
 *  camera_fabric.cpp:120-123 builds for `features_extractor: type: eigen`: DSO's pixel selector.  The window size (current_potential_)
 *  persists across calls; the list is in emission order. */
class HipEigenTrackingFeaturesExtractor : public HipTrackingFeaturesExtractor {
 public:
  HipEigenTrackingFeaturesExtractor(int width, int height, double point_density_for_detector, int device = 0, void *stream = nullptr) {
    check(dsopp_hip_feature_extractor_create_eigen(device, stream, width, height, point_density_for_detector, &ex_));
  }
};

/** The immature landmarks of one keyframe kept on the device for their lifetime (ActiveKeyframe::immature_landmarks_:
 *  created by pushImmatureLandmarks, traced every frame by the depth estimator, consumed by the activator). */
class DeviceImmatureSet {
 public:
  explicit DeviceImmatureSet(const std::vector<ImmatureLandmarkView> &landmarks, int device = 0, void *stream = nullptr)
      : n_(landmarks.size()) {
    std::vector<double> proj(2 * n_), dir(3 * n_), patch(8 * n_), grad(2 * n_);
    for (size_t i = 0; i < n_; ++i) {
      const ImmatureLandmarkView &l = landmarks[i];
      for (size_t k = 0; k < 2; ++k) {
        proj[2 * i + k] = l.projection[k];
        grad[2 * i + k] = l.gradient[k];
      }
      for (size_t k = 0; k < 3; ++k) dir[3 * i + k] = l.direction[k];
      for (size_t k = 0; k < 8; ++k) patch[8 * i + k] = l.patch[k];
    }
    check(dsopp_hip_immature_set_create(device, stream, static_cast<int32_t>(n_), proj.data(), dir.data(), patch.data(), grad.data(), &s_));
    upload(landmarks);
  }
  /** buildFeatures + pushImmatureLandmarks (build_features.hpp:20-32, active_keyframe.cpp:95-112) on the device for the extractor's last
   *  list over level 0 of the keyframe's pyramid: features outside insideCameraROI are dropped.  `landmarks` receives the host copy
   *  (projection, direction, patch, gradient; the estimator state at the constructor defaults) that the activator keeps. */
  DeviceImmatureSet(const HipTrackingFeaturesExtractor &extractor, const DevicePyramid &keyframe_pyramid, const PinholeModel &model,
                    std::vector<ImmatureLandmarkView> &landmarks, int device = 0, void *stream = nullptr) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    int32_t n = 0;
    check(dsopp_hip_immature_set_create_from_features(device, stream, extractor.handle(), keyframe_pyramid.handle(), intr, &s_, &n));
    n_ = static_cast<size_t>(n);
    std::vector<double> proj(2 * n_), dir(3 * n_), patch(8 * n_), grad(2 * n_);
    check(dsopp_hip_immature_set_download_inputs(s_, proj.data(), dir.data(), patch.data(), grad.data()));
    landmarks.assign(n_, ImmatureLandmarkView{});
    for (size_t i = 0; i < n_; ++i) {
      ImmatureLandmarkView &l = landmarks[i];
      for (size_t k = 0; k < 2; ++k) {
        l.projection[k] = proj[2 * i + k];
        l.gradient[k] = grad[2 * i + k];
      }
      for (size_t k = 0; k < 3; ++k) l.direction[k] = dir[3 * i + k];
      for (size_t k = 0; k < 8; ++k) l.patch[k] = patch[8 * i + k];
    }
  }
  ~DeviceImmatureSet() { dsopp_hip_immature_set_destroy(s_); }
  DeviceImmatureSet(const DeviceImmatureSet &) = delete;
  DeviceImmatureSet &operator=(const DeviceImmatureSet &) = delete;
  dsopp_hip_immature_set *handle() const { return s_; }
  size_t size() const { return n_; }
  /** DepthEstimator::estimate on the resident set (asynchronous) */
  void estimate(const DevicePyramid &target_frame, const Motion &t_t_r, double reference_exposure_time, const Vector2 &reference_affine_brightness,
                double target_exposure_time, const Vector2 &target_affine_brightness, const PinholeModel &model, double sigma_huber_loss) {
    const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
    check(dsopp_hip_immature_set_estimate(s_, target_frame.handle(), 0, intr, t_t_r.data(), reference_exposure_time, reference_affine_brightness.data(),
                                          target_exposure_time, target_affine_brightness.data(), sigma_huber_loss));
  }
  /** wait for the estimator launches enqueued on the set's stream (a download with no outputs) */
  void synchronize() const { check(dsopp_hip_immature_set_download_state(s_, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr)); }
  void upload(const std::vector<ImmatureLandmarkView> &landmarks) {
    std::vector<double> imin(n_), imax(n_), uniq(n_), spi(n_);
    std::vector<uint8_t> status(n_), traced(n_);
    for (size_t i = 0; i < n_; ++i) {
      const ImmatureLandmarkView &l = landmarks[i];
      imin[i] = l.idepth_min;
      imax[i] = l.idepth_max;
      uniq[i] = l.uniqueness;
      spi[i] = l.search_pixel_interval;
      status[i] = l.status;
      traced[i] = l.traced ? 1 : 0;
    }
    check(dsopp_hip_immature_set_upload_state(s_, imin.data(), imax.data(), uniq.data(), spi.data(), status.data(), traced.data()));
  }
  void download(std::vector<ImmatureLandmarkView> &landmarks) const {
    std::vector<double> imin(n_), imax(n_), uniq(n_), spi(n_);
    std::vector<uint8_t> status(n_), traced(n_);
    check(dsopp_hip_immature_set_download_state(s_, imin.data(), imax.data(), uniq.data(), spi.data(), status.data(), traced.data()));
    for (size_t i = 0; i < n_; ++i) {
      ImmatureLandmarkView &l = landmarks[i];
      l.idepth_min = imin[i];
      l.idepth_max = imax[i];
      l.uniqueness = uniq[i];
      l.search_pixel_interval = spi[i];
      l.status = status[i];
      l.traced = traced[i] != 0;
    }
  }

 private:
  size_t n_ = 0;
  dsopp_hip_immature_set *s_ = nullptr;
};

/** initializationPoses(track) — src/tracker/tracker/src/monocular_tracker.cpp:136-176: the hypotheses estimatePose tries in
 *  turn (113 for a track with at least two frames, else the identity).  Pass nullptr for a shorter track. */
inline std::vector<Motion> initializationPoses(const Motion *t_world_previous, const Motion *t_world_last, const Motion *t_world_keyframe) {
  std::vector<double> buf(7 * 128);
  int32_t n = 0;
  const bool two = t_world_previous && t_world_last && t_world_keyframe;
  check(dsopp_hip_initialization_poses(two ? t_world_previous->data() : nullptr, two ? t_world_last->data() : nullptr,
                                       two ? t_world_keyframe->data() : nullptr, 128, buf.data(), &n));
  std::vector<Motion> out(static_cast<size_t>(n));
  for (int32_t i = 0; i < n; ++i) std::copy(buf.begin() + 7 * i, buf.begin() + 7 * (i + 1), out[static_cast<size_t>(i)].begin());
  return out;
}

/** estimateDepths of the tracker (monocular_tracker.cpp:74-102) for all keyframes of the window in one launch:
 *  DepthEstimator::estimate(target_frame, keyframe k's immature landmarks, t_t_r[k], ...) for every k */
inline void estimateDepthsOfWindow(const DevicePyramid &target_frame, const std::vector<DeviceImmatureSet *> &keyframe_sets,
                                   const std::vector<Motion> &t_target_keyframe, const std::vector<double> &keyframe_exposure_times,
                                   const std::vector<Vector2> &keyframe_affine_brightness, double target_exposure_time,
                                   const Vector2 &target_affine_brightness, const PinholeModel &model, double sigma_huber_loss) {
  const size_t n = keyframe_sets.size();
  std::vector<dsopp_hip_immature_set *> sets(n);
  std::vector<double> T(7 * n), ab(2 * n);
  for (size_t k = 0; k < n; ++k) {
    sets[k] = keyframe_sets[k]->handle();
    std::copy(t_target_keyframe[k].begin(), t_target_keyframe[k].end(), T.begin() + 7 * static_cast<long>(k));
    ab[2 * k] = keyframe_affine_brightness[k][0];
    ab[2 * k + 1] = keyframe_affine_brightness[k][1];
  }
  const double intr[4] = {model.fx, model.fy, model.cx, model.cy};
  check(dsopp_hip_immature_sets_estimate(static_cast<int32_t>(n), sets.data(), target_frame.handle(), 0, intr, T.data(), keyframe_exposure_times.data(),
                                         ab.data(), target_exposure_time, target_affine_brightness.data(), sigma_huber_loss));
}

/** ActiveKeyframe::ImmatureLandmarkActivationStatus — src/track/frames/include/track/frames/active_keyframe.hpp:40-44 */
enum class ImmatureLandmarkActivationStatus : uint8_t { kActivate = 0, kSkip = 1, kDelete = 2 };

/**
 * tracker::LandmarksActivator<SE3, PinholeCamera, PixelMap, 1, REFINE>
 * (src/tracker/landmarks_activator/include/tracker/landmarks_activator/landmarks_activator.hpp:31-57): same constructor
 * arguments and the same persistent min_distance_to_neighbor_.  The track is what the HIP backend holds of it: the window
 * solver (poses, affine brightness, images and active landmarks of the older keyframes), their device-resident immature
 * sets, and the new keyframe that pushNewKeyframe just created (monocular_tracker.cpp:491-497 call order).
 */
template <bool REFINE = false>
class HipLandmarksActivator {
 public:
  struct Track {
    HipPhotometricBundleAdjustment *solver;          // holds every keyframe of activeFrames() but the newest
    std::vector<int32_t> keyframe_ids;               // oldest first
    std::vector<DeviceImmatureSet *> immature;       // per keyframe, nullptr = no immature landmarks
    const KeyframeView *newest;                      // pose, exposure, affine brightness, pyramid (>= 2 levels)
  };
  explicit HipLandmarksActivator(double sigma_huber_loss = 9, size_t number_of_desired_points = 2000)
      : sigma_huber_loss_(sigma_huber_loss), number_of_desired_points_(number_of_desired_points) {}
  /** activate(track): returns the statuses applyImmatureLandmarkActivationStatuses consumes, per keyframe; `idepths` (optional)
   *  receives landmark.idepth() after the refinement — what the new ActiveTrackingLandmark is constructed with */
  std::vector<std::vector<ImmatureLandmarkActivationStatus>> activate(const Track &track, std::vector<std::vector<double>> *idepths = nullptr) {
    const size_t n = track.keyframe_ids.size();
    std::vector<dsopp_hip_immature_set *> sets(n, nullptr);
    std::vector<std::vector<ImmatureLandmarkActivationStatus>> statuses(n);
    std::vector<uint8_t *> st_ptr(n, nullptr);
    std::vector<double *> id_ptr(n, nullptr);
    if (idepths) idepths->assign(n, {});
    for (size_t k = 0; k < n; ++k) {
      if (!track.immature[k]) continue;
      sets[k] = track.immature[k]->handle();
      statuses[k].resize(track.immature[k]->size());
      st_ptr[k] = reinterpret_cast<uint8_t *>(statuses[k].data());
      if (idepths) {
        (*idepths)[k].resize(track.immature[k]->size());
        id_ptr[k] = (*idepths)[k].data();
      }
    }
    const KeyframeView &nk = *track.newest;
    check(dsopp_hip_window_activate_landmarks(track.solver->handle(), static_cast<int32_t>(n), track.keyframe_ids.data(), sets.data(),
                                              nk.pyramids->handle(), nk.t_world_agent.data(), nk.exposure_time, nk.affine_brightness.data(),
                                              static_cast<int32_t>(number_of_desired_points_), &min_distance_to_neighbor_, REFINE ? 1 : 0,
                                              sigma_huber_loss_, st_ptr.data(), id_ptr.data(), &last_));
    return statuses;
  }
  double minDistanceToNeighbor() const { return min_distance_to_neighbor_; }
  const dsopp_hip_activation_result &lastResult() const { return last_; }

 private:
  double min_distance_to_neighbor_ = 2;  // landmarks_activator.hpp:51
  const double sigma_huber_loss_;
  const size_t number_of_desired_points_;
  dsopp_hip_activation_result last_{};
};

/**
 * marginalization::FrameMarginalizationStrategy<Motion> (src/marginalization/include/marginalization/frame_marginalization_strategy.hpp),
 * both kinds the fabric builds (src/marginalization/src/fabric.cpp:25-50), decided on the device from the solver's own state.
 * marginalize(track) replaces the whole of monocular_tracker.cpp:505 and :507 for the frames concerned — the strategy, updateLocalFrame of
 * the frames it marginalised (:317) and of the frames that stay (updateSolver): the solver is refreshed by the call, the views receive
 * the flags.  Do NOT send updateLocalFrame for these frames again before the next pushFrame: a second update clears to_marginalize, as
 * it does in the reference, and the landmarks would never reach the prior.  numberOfSuccessfulOptimizations lives in the solver: call
 * noteOptimization() once after every solve() (what updateFrame does for every landmark, photometric_bundle_adjustment.cpp:256).
 */
class HipFrameMarginalizationStrategy {
 public:
  struct Track {
    HipPhotometricBundleAdjustment *solver;     // single-device; holds every frame of activeFrames()
    std::vector<KeyframeView *> active_frames;  // track.activeFrames(), oldest first
    std::vector<int32_t> camera_frame_ids;      // ActiveKeyframe::id() per active frame; empty = the keyframe ids
    std::vector<DeviceImmatureSet *> immature;  // per active frame, nullptr = no immature landmarks; empty = none at all
  };
  /** SparseFrameMarginalizationStrategy(minimum_size, maximum_size, maximum_number_of_marginalized) */
  HipFrameMarginalizationStrategy(size_t minimum_size, size_t maximum_size, double maximum_share_marginalized) {
    dsopp_hip_marginalization_default_options(&options_);
    options_.minimum_size = static_cast<int32_t>(minimum_size);
    options_.maximum_size = static_cast<int32_t>(maximum_size);
    options_.maximum_share_marginalized = maximum_share_marginalized;
  }
  /** MaximumSizeFrameMarginalizationStrategy(maximum_size) */
  explicit HipFrameMarginalizationStrategy(size_t maximum_size) {
    dsopp_hip_marginalization_default_options(&options_);
    options_.strategy = DSOPP_HIP_MARGINALIZATION_MAXIMUM_SIZE;
    options_.maximum_size = static_cast<int32_t>(maximum_size);
  }
  /** the counting half of updateFrame for every frame of the solver */
  static void noteOptimization(HipPhotometricBundleAdjustment &solver) { check(dsopp_hip_window_note_optimization(window(solver))); }
  /** marginalize(track): the keyframe ids marginalised, in the order marginalizeFrame() hit them (what addSemanticObservations takes) */
  std::vector<int32_t> marginalize(const Track &track) {
    dsopp_hip_window *w = window(*track.solver);
    int32_t nf = 0;
    check(dsopp_hip_window_num_frames(w, &nf));
    std::vector<int32_t> ids(static_cast<size_t>(std::max(nf, 1)));
    check(dsopp_hip_window_frame_ids(w, nf, ids.data(), &nf));
    // the C-ABI takes one entry per frame of the window, which may still hold frames marginalised earlier
    std::vector<int32_t> camera_ids(ids.begin(), ids.begin() + nf), counts(static_cast<size_t>(nf), 0);
    std::vector<dsopp_hip_immature_set *> sets(static_cast<size_t>(nf), nullptr);
    std::vector<KeyframeView *> views(static_cast<size_t>(nf), nullptr);
    size_t total = 0;
    for (int32_t s = 0; s < nf; ++s) {
      check(dsopp_hip_window_num_landmarks(w, ids[static_cast<size_t>(s)], &counts[static_cast<size_t>(s)]));
      total += static_cast<size_t>(counts[static_cast<size_t>(s)]);
      for (size_t a = 0; a < track.active_frames.size(); ++a) {
        if (track.active_frames[a]->keyframe_id != ids[static_cast<size_t>(s)]) continue;
        views[static_cast<size_t>(s)] = track.active_frames[a];
        if (a < track.camera_frame_ids.size()) camera_ids[static_cast<size_t>(s)] = track.camera_frame_ids[a];
        if (a < track.immature.size() && track.immature[a]) sets[static_cast<size_t>(s)] = track.immature[a]->handle();
      }
    }
    std::vector<uint8_t> flags(std::max<size_t>(total, 1));
    check(dsopp_hip_window_choose_marginalization(w, &options_, camera_ids.data(), sets.data(), 1, &last_, flags.data()));
    size_t offset = 0;
    for (int32_t s = 0; s < nf; ++s) {
      const size_t n = static_cast<size_t>(counts[static_cast<size_t>(s)]);
      if (KeyframeView *view = views[static_cast<size_t>(s)])
        for (size_t i = 0; i < n && i < view->active_landmarks.size(); ++i) {
          view->active_landmarks[i].is_marginalized = (flags[offset + i] & 1) != 0;
          if (flags[offset + i] & 2) view->active_landmarks[i].is_outlier = true;
        }
      offset += n;
    }
    std::vector<int32_t> marginalized(last_.marginalized_ids, last_.marginalized_ids + last_.n_marginalized);
    for (KeyframeView *view : track.active_frames)
      for (int32_t id : marginalized)
        if (view->keyframe_id == id) view->is_marginalized = true;
    return marginalized;
  }
  const dsopp_hip_marginalization_result &lastResult() const { return last_; }

 private:
  static dsopp_hip_window *window(const HipPhotometricBundleAdjustment &solver) {
    if (!solver.handle()) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the marginalisation strategy needs a single-device solver");
    return solver.handle();
  }
  dsopp_hip_marginalization_options options_;
  dsopp_hip_marginalization_result last_{};
};

/** storage::PointStorageType and one class of storage::PointsStorage (the viewer's input, one sensor): what Frame::buildPoints fills
 *  (src/track/frames/src/frame.cpp:190-216) */
enum class PointStorageType { kActive = DSOPP_HIP_MAP_CLASS_ACTIVE, kMarginalized = DSOPP_HIP_MAP_CLASS_MARGINALIZED, kOutlier = DSOPP_HIP_MAP_CLASS_OUTLIER };
struct PointsStorage {
  std::vector<std::array<double, 3>> points;                                   // keyframe-local: direction / idepth
  std::vector<std::array<uint8_t, 3>> colors, default_colors, semantics_colors;  // getColor(landmark, true, false) | (false, false) | (false, true)
  std::vector<double> idepth_variances, relative_baselines;
};

/** a packed export of the map (dsopp_hip_map_export) */
struct PointCloud {
  std::vector<std::array<double, 3>> xyz;
  std::vector<std::array<uint8_t, 3>> rgb;
  std::vector<uint8_t> type;
  std::vector<double> relative_baseline, idepth_variance;
  std::vector<int32_t> keyframe_index, record_index, per_keyframe_counts;
};

/** The track's side of the map on the device: the ActiveTrackingLandmark records of every keyframe, kept where the bundle adjustment
 *  leaves them and for good once the keyframe left the window, and their point cloud — what Frame::buildPoints hands the viewer
 *  (points()) and what pydsopp/utils/point_cloud_exporter.py writes (exportWorld()).  Call order of a keyframe step:
 *    solver.pushFrame(new keyframe); map.addKeyframe(solver, id, &pyramid); ... solver.solve(); map.update(solver);
 *    strategy.marginalize(track); map.update(solver);   (then the next pushFrame, which erases the marginalised keyframes) */
class HipMap {
 public:
  explicit HipMap(bool estimate_uncertainty = true, int channels = 1, double min_relative_baseline = 0.1, int device = 0, void *stream = nullptr) {
    dsopp_hip_map_options o;
    dsopp_hip_map_default_options(&o);
    o.estimate_uncertainty = estimate_uncertainty ? 1 : 0;
    o.channels = channels;
    o.min_relative_baseline = min_relative_baseline;
    check(dsopp_hip_map_create(device, stream, &o, &m_));
  }
  ~HipMap() { dsopp_hip_map_destroy(m_); }
  HipMap(const HipMap &) = delete;
  HipMap &operator=(const HipMap &) = delete;
  /** after solver.pushFrame of that keyframe; the pyramid's kept 8-bit image (colour before grey) is copied, nullptr = no image colours */
  void addKeyframe(const HipPhotometricBundleAdjustment &solver, int32_t keyframe_id, const DevicePyramid *pyramid = nullptr) {
    check(dsopp_hip_map_add_keyframe(m_, window(solver), keyframe_id, pyramid ? pyramid->handle() : nullptr));
  }
  /** the landmark half of updateFrame for every keyframe of the window at once (photometric_bundle_adjustment.cpp:223-263), on the device;
   *  legend_weights = SemanticLegend::weights_ (256) or nullptr */
  void update(const HipPhotometricBundleAdjustment &solver, const uint64_t *legend_weights = nullptr) {
    check(dsopp_hip_map_update(m_, window(solver), legend_weights));
  }
  void setPose(int32_t keyframe_id, const Motion &t_world_agent) { check(dsopp_hip_map_set_pose(m_, keyframe_id, t_world_agent.data())); }
  std::vector<int32_t> keyframeIds() const {
    int32_t n = 0;
    check(dsopp_hip_map_num_keyframes(m_, &n));
    std::vector<int32_t> ids(static_cast<size_t>(std::max(n, 1)));
    check(dsopp_hip_map_keyframe_ids(m_, n, ids.data(), &n));
    ids.resize(static_cast<size_t>(n));
    return ids;
  }
  int32_t numRecords(int32_t keyframe_id) const {
    int32_t n = 0;
    check(dsopp_hip_map_num_records(m_, keyframe_id, &n));
    return n;
  }
  /** the packed export of `keyframe_ids` (empty = every keyframe, in insertion order) under `options` */
  PointCloud exportCloud(const dsopp_hip_map_export_options &options, const std::vector<int32_t> &keyframe_ids = {}) const {
    const std::vector<int32_t> ids = keyframe_ids.empty() ? keyframeIds() : keyframe_ids;
    int64_t capacity = 0;
    for (int32_t id : ids) capacity += numRecords(id);
    const size_t cap = static_cast<size_t>(capacity);
    PointCloud c;
    c.xyz.resize(cap), c.rgb.resize(cap), c.type.resize(cap), c.relative_baseline.resize(cap), c.idepth_variance.resize(cap);
    c.keyframe_index.resize(cap), c.record_index.resize(cap), c.per_keyframe_counts.resize(std::max<size_t>(ids.size(), 1));
    int64_t count = 0;
    check(dsopp_hip_map_export(m_, &options, static_cast<int32_t>(ids.size()), ids.data(), capacity, cap ? c.xyz[0].data() : nullptr,
                               cap ? c.rgb[0].data() : nullptr, c.type.data(), c.relative_baseline.data(), c.idepth_variance.data(),
                               c.keyframe_index.data(), c.record_index.data(), &count, c.per_keyframe_counts.data()));
    const size_t n = static_cast<size_t>(count);
    c.xyz.resize(n), c.rgb.resize(n), c.type.resize(n), c.relative_baseline.resize(n), c.idepth_variance.resize(n);
    c.keyframe_index.resize(n), c.record_index.resize(n), c.per_keyframe_counts.resize(ids.size());
    return c;
  }
  /** the exporter's cloud (point_cloud_exporter.py:83-107): world coordinates, image colours (or the semantic ones), active and
   *  marginalised landmarks, with `filtration` the confident filter at the exporter's thresholds */
  PointCloud exportWorld(bool filtration, bool semantic_colours = false, double max_idepth_variance = 5e-8, double min_relative_baseline = 0.15) const {
    dsopp_hip_map_export_options o;
    dsopp_hip_map_default_export_options(&o);
    o.apply_filters = filtration ? 1 : 0;
    o.max_idepth_variance = max_idepth_variance;
    o.min_relative_baseline_filter = min_relative_baseline;
    o.frame = DSOPP_HIP_MAP_FRAME_WORLD;
    o.colours = semantic_colours ? DSOPP_HIP_MAP_COLOURS_SEMANTIC : DSOPP_HIP_MAP_COLOURS_IMAGE;
    return exportCloud(o);
  }
  /** Frame::buildPoints of one keyframe and one class, appended to `storage`: three exports, one per colour set */
  void points(int32_t keyframe_id, PointStorageType type, PointsStorage &storage) const {
    dsopp_hip_map_export_options o;
    dsopp_hip_map_default_export_options(&o);
    o.classes = static_cast<int32_t>(type);
    o.frame = DSOPP_HIP_MAP_FRAME_KEYFRAME;
    o.colours = DSOPP_HIP_MAP_COLOURS_LANDMARK_TYPE;
    const PointCloud by_type = exportCloud(o, {keyframe_id});
    o.colours = DSOPP_HIP_MAP_COLOURS_CONSTANT;
    const PointCloud constant = exportCloud(o, {keyframe_id});
    o.colours = DSOPP_HIP_MAP_COLOURS_SEMANTIC;
    const PointCloud semantic = exportCloud(o, {keyframe_id});
    storage.points.insert(storage.points.end(), by_type.xyz.begin(), by_type.xyz.end());
    storage.colors.insert(storage.colors.end(), by_type.rgb.begin(), by_type.rgb.end());
    storage.default_colors.insert(storage.default_colors.end(), constant.rgb.begin(), constant.rgb.end());
    storage.semantics_colors.insert(storage.semantics_colors.end(), semantic.rgb.begin(), semantic.rgb.end());
    storage.idepth_variances.insert(storage.idepth_variances.end(), by_type.idepth_variance.begin(), by_type.idepth_variance.end());
    storage.relative_baselines.insert(storage.relative_baselines.end(), by_type.relative_baseline.begin(), by_type.relative_baseline.end());
  }
  dsopp_hip_map *handle() const { return m_; }

 private:
  static dsopp_hip_window *window(const HipPhotometricBundleAdjustment &solver) {
    if (!solver.handle()) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the map needs a single-device solver");
    return solver.handle();
  }
  dsopp_hip_map *m_ = nullptr;
};

/** features::Correspondence (feature_based_slam/features/correspondence.hpp:12-19) */
struct FlowCorrespondence {
  bool is_inlier;
  size_t idx_from, idx_to;
};

/** features::OpticalFlowMatch (src/feature_based_slam/features/src/optical_flow.cpp:11-42) on the device, its Lucas-Kanade half: the
 *  features of frame_from tracked into image_to by cv::calcOpticalFlowPyrLK(..., Size(15, 15), 3, TermCriteria(COUNT + EPS, 10, 0.01)),
 *  a feature and a correspondence {true, i, features.size() - 1} for every status != 0, in the order of frame_from.  image_from is the
 *  first track frame for the whole bootstrap (monocular_initializer.cpp:47-51), so it is set once and its levels stay on the device.
 *  The refill from a fresh ORB detection (optical_flow.cpp:44-53) is HipFindCorrespondences below. */
class HipOpticalFlowMatch {
 public:
  struct Result {
    std::vector<std::array<float, 2>> features;  // DistinctFeature coordinates in image_to
    std::vector<FlowCorrespondence> correspondences;
  };
  HipOpticalFlowMatch(int width, int height, int device = 0, void *stream = nullptr) : width_(width) {
    check(dsopp_hip_flow_tracker_create(width, height, 15, 3, 10, 0.01, 1e-4, device, stream, &t_));
  }
  ~HipOpticalFlowMatch() { dsopp_hip_flow_tracker_destroy(t_); }
  HipOpticalFlowMatch(const HipOpticalFlowMatch &) = delete;
  HipOpticalFlowMatch &operator=(const HipOpticalFlowMatch &) = delete;
  /** image_from as a continuous 8-bit Mat, or the grey image a pyramid keeps (CameraFeatures::frameData()) */
  void setImageFrom(const uint8_t *image_from) { check(dsopp_hip_flow_tracker_set_reference(t_, image_from, static_cast<size_t>(width_))); }
  void setImageFrom(const DevicePyramid &frame_from) { check(dsopp_hip_flow_tracker_set_reference_from_pyramid(t_, frame_from.handle())); }
  /** features_from: (x, y) per feature of frame_from */
  Result match(const std::vector<std::array<float, 2>> &features_from, const uint8_t *image_to) {
    prepare(features_from.size());
    check(dsopp_hip_flow_tracker_track(t_, image_to, static_cast<size_t>(width_), static_cast<int>(features_from.size()), flat(features_from),
                                       to_.data(), status_.data(), err_.data(), nullptr));
    return collect(features_from.size());
  }
  Result match(const std::vector<std::array<float, 2>> &features_from, const DevicePyramid &frame_to) {
    prepare(features_from.size());
    check(dsopp_hip_flow_tracker_track_from_pyramid(t_, frame_to.handle(), static_cast<int>(features_from.size()), flat(features_from), to_.data(),
                                                    status_.data(), err_.data(), nullptr));
    return collect(features_from.size());
  }
  /** status and err of the last match, per feature of frame_from */
  const std::vector<uint8_t> &status() const { return status_; }
  const std::vector<float> &error() const { return err_; }
  dsopp_hip_flow_tracker *handle() const { return t_; }

 private:
  static const float *flat(const std::vector<std::array<float, 2>> &v) { return v.empty() ? nullptr : v.front().data(); }
  void prepare(size_t n) {
    to_.assign(2 * n, 0.0f);
    status_.assign(n, 0);
    err_.assign(n, 0.0f);
  }
  Result collect(size_t n) const {
    Result r;
    for (size_t i = 0; i < n; ++i) {
      if (status_[i] == 0) continue;
      r.features.push_back({to_[2 * i], to_[2 * i + 1]});
      r.correspondences.push_back({true, i, r.features.size() - 1});
    }
    return r;
  }
  dsopp_hip_flow_tracker *t_ = nullptr;
  int width_;
  std::vector<float> to_, err_;
  std::vector<uint8_t> status_;
};

/** DistinctFeaturesExtractorORB (src/feature_based_slam/features/src/distinct_features_extractor_orb.cpp:11-38) on the device:
 *  cv::ORB::create(number_of_features, 2.0f, 5)->detect, of which the reference uses keypoint.pt alone.  The detections come in the
 *  canonical order of include/dsopp_hip.h (level, y, x), not in the order retainBest leaves them in; the set is the same. */
class HipDistinctFeaturesExtractorORB {
 public:
  using Feature = std::array<float, 2>;
  HipDistinctFeaturesExtractorORB(int width, int height, size_t number_of_features = 500, int device = 0, void *stream = nullptr, int levels = 5,
                                  int edge_threshold = 31, int fast_threshold = 20)
      : width_(width), number_of_features_(number_of_features) {
    check(dsopp_hip_orb_detector_create(width, height, static_cast<int>(number_of_features), levels, edge_threshold, fast_threshold, device, stream, &d_));
    reserve(2 * number_of_features + 256);
  }
  ~HipDistinctFeaturesExtractorORB() { dsopp_hip_orb_detector_destroy(d_); }
  HipDistinctFeaturesExtractorORB(const HipDistinctFeaturesExtractorORB &) = delete;
  HipDistinctFeaturesExtractorORB &operator=(const HipDistinctFeaturesExtractorORB &) = delete;
  /** the CameraMask bytes every later extract honours (W x H, 0 = masked), nullptr = none; or the level-0 mask a pyramid keeps */
  void setMask(const uint8_t *mask) { check(dsopp_hip_orb_detector_set_mask(d_, mask)); }
  void setMaskFromPyramid(const DevicePyramid &pyramid) { check(dsopp_hip_orb_detector_set_mask_from_pyramid(d_, pyramid.handle())); }
  /** extract(image, mask, ...) of a continuous 8-bit Mat, or of the grey image a pyramid keeps (CameraFeatures::frameData()) */
  std::vector<Feature> extract(const uint8_t *image) {
    return run([&](int32_t capacity, int32_t *n) {
      return dsopp_hip_orb_detector_detect(d_, image, static_cast<size_t>(width_), capacity, xy_.data(), level_.data(), response_.data(), n);
    });
  }
  std::vector<Feature> extract(const DevicePyramid &frame) {
    return run([&](int32_t capacity, int32_t *n) {
      return dsopp_hip_orb_detector_detect_from_pyramid(d_, frame.handle(), capacity, xy_.data(), level_.data(), response_.data(), n);
    });
  }
  size_t featureCount() const { return number_of_features_; }
  /** level and Harris response of the last extract, per feature */
  const std::vector<int32_t> &levels() const { return level_; }
  const std::vector<float> &responses() const { return response_; }
  dsopp_hip_orb_detector *handle() const { return d_; }

 private:
  void reserve(size_t n) {
    xy_.resize(2 * n);
    level_.resize(n);
    response_.resize(n);
  }
  /** `call(capacity, &n)`, once more with the room reported when the capacity was too small */
  template <typename Call>
  std::vector<Feature> run(Call call) {
    reserve(capacity_ > level_.size() ? capacity_ : level_.size());
    int32_t n = 0;
    int rc = call(static_cast<int32_t>(level_.size()), &n);
    if (rc == DSOPP_HIP_ERR_CAPACITY) {
      capacity_ = static_cast<size_t>(n);
      reserve(capacity_);
      rc = call(static_cast<int32_t>(level_.size()), &n);
    }
    check(rc);
    capacity_ = level_.size();
    std::vector<Feature> out(static_cast<size_t>(n));
    for (size_t i = 0; i < out.size(); ++i) out[i] = {xy_[2 * i], xy_[2 * i + 1]};
    level_.resize(out.size());
    response_.resize(out.size());
    return out;
  }
  dsopp_hip_orb_detector *d_ = nullptr;
  int width_;
  size_t number_of_features_, capacity_ = 0;
  std::vector<float> xy_, response_;
  std::vector<int32_t> level_;
};

/** features::findCorrespondences (src/feature_based_slam/features/src/correspondences_finder.cpp:7-18) with features::OpticalFlowMatch
 *  as its finder (optical_flow.cpp:11-56), whole, on the device: without features of a previous frame the detection of image_to and no
 *  correspondences; otherwise the flow's feature and correspondence per status != 0, in the order of features_from, then a refill from
 *  a fresh detection of image_to: new[indices[i]] while fewer than featureCount() are held, indices = the std::shuffle of 0 .. m - 1
 *  under a default-constructed std::default_random_engine (dsopp_hip_features_shuffle_order).  No duplicate test, as in the reference.
 *  image_from is set once (monocular_initializer.cpp:47-51).  The random subset a refill draws differs from the reference's because the
 *  order of the detections does (HipDistinctFeaturesExtractorORB). */
class HipFindCorrespondences {
 public:
  using Feature = std::array<float, 2>;
  using Result = HipOpticalFlowMatch::Result;
  HipFindCorrespondences(int width, int height, size_t number_of_features = 500, int device = 0, void *stream = nullptr, int levels = 5,
                         int edge_threshold = 31, int fast_threshold = 20)
      : flow_(width, height, device, stream), extractor_(width, height, number_of_features, device, stream, levels, edge_threshold, fast_threshold) {}
  void setImageFrom(const uint8_t *image_from) { flow_.setImageFrom(image_from); }
  void setImageFrom(const DevicePyramid &frame_from) { flow_.setImageFrom(frame_from); }
  /** features_from == nullptr: the reference frame does not exist yet */
  Result find(const std::vector<Feature> *features_from, const uint8_t *image_to) { return findIn(features_from, image_to); }
  Result find(const std::vector<Feature> *features_from, const DevicePyramid &frame_to) { return findIn(features_from, frame_to); }
  HipOpticalFlowMatch &flow() { return flow_; }
  HipDistinctFeaturesExtractorORB &extractor() { return extractor_; }

 private:
  template <typename Image>
  Result findIn(const std::vector<Feature> *features_from, const Image &image_to) {
    if (!features_from) {
      Result r;
      r.features = extractor_.extract(image_to);
      return r;
    }
    Result r = flow_.match(*features_from, image_to);
    const std::vector<Feature> fresh = extractor_.extract(image_to);
    std::vector<int32_t> indices(fresh.size());
    if (!fresh.empty()) check(dsopp_hip_features_shuffle_order(static_cast<int32_t>(fresh.size()), indices.data()));
    for (size_t i = 0; r.features.size() < extractor_.featureCount() && i < indices.size(); ++i)
      r.features.push_back(fresh[static_cast<size_t>(indices[i])]);
    return r;
  }
  HipOpticalFlowMatch flow_;
  HipDistinctFeaturesExtractorORB extractor_;
};

/** FrameStatus of the initialiser's keyframe strategies (initialization_strategy/frame_status.hpp) */
enum class FrameStatus { kDropFrame, kKeepFrame, kFinish };

/** The bootstrap's standstill test on the device: estimateSO3inlierCount<3> (src/feature_based_slam/tracker/src/estimate_so3_inlier_count.cpp:17-48),
 *  that is ransac::ransac (ransac.hpp:27-56) over the three-point PureRorationSolver (pure_rotation_estimator.cpp:14-67), and the two
 *  decisions that consume its counts.  The reference calls ransac(solver, target_points, reference_points, ...): points_new are the new
 *  frame's points, points_keyframe the last bootstrap keyframe's, and the rotation maps bearings of the new frame onto bearings of the
 *  keyframe (the reference stores it as rotation_t_r all the same).
 *  One deviation: all sample triples are drawn ahead of the launch.  Given the same std::rand() state at entry the hypotheses examined and
 *  the result equal the reference's; after an early stop the state of std::rand() left behind is not the reference's, which draws a
 *  triple only for an iteration it runs. */
class HipRotationStandstill {
 public:
  struct Result {
    size_t inliers, matches;          // estimateSO3inlierCount's pair
    std::array<double, 9> rotation;   // rotation_t_r, row-major
    std::vector<int32_t> inlier_indices;
    int iterations_run, best_iteration;
  };
  /** width, height: the image size of `model` (CameraModelBase::image_size), which bounds the ROI */
  HipRotationStandstill(int width, int height, int device = 0, void *stream = nullptr) : width_(width), height_(height) {
    check(dsopp_hip_rotation_ransac_create(device, stream, &r_));
  }
  ~HipRotationStandstill() { dsopp_hip_rotation_ransac_destroy(r_); }
  HipRotationStandstill(const HipRotationStandstill &) = delete;
  HipRotationStandstill &operator=(const HipRotationStandstill &) = delete;

  /** generateRandomSequence<3>(n) (ransac/random_sequence_generator.hpp:17-34), `iterations` times: rand() % n, redrawn on a repeat */
  static std::vector<int32_t> drawSamples(size_t n, size_t iterations) {
    if (iterations > 0 && n < 3) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "fewer than 3 points: the reference's sampler never returns");
    std::vector<int32_t> samples(3 * iterations);
    for (size_t i = 0; i < iterations; ++i) {
      size_t sequence[3];
      sequence[0] = static_cast<size_t>(std::rand()) % n;
      for (size_t k = 1; k < 3; ++k) {
        size_t next = static_cast<size_t>(std::rand()) % n;
        auto repeats = [&] {
          for (size_t j = 0; j < k; ++j)
            if (sequence[j] == next) return true;
          return false;
        };
        while (repeats()) next = static_cast<size_t>(std::rand()) % n;
        sequence[k] = next;
      }
      for (size_t k = 0; k < 3; ++k) samples[3 * i + k] = static_cast<int32_t>(sequence[k]);
    }
    return samples;
  }

  /** estimateSO3inlierCount<3>(keyframe, new frame, ...): the triples come from std::rand() */
  Result estimate(const std::vector<Vector2> &points_new, const std::vector<Vector2> &points_keyframe, const PinholeModel &model,
                  size_t iterations = 200, double threshold = 1.5) {
    return estimate(points_new, points_keyframe, model, points_new.empty() ? std::vector<int32_t>() : drawSamples(points_new.size(), iterations),
                    threshold);
  }
  /** the same over the caller's triples (3 indices per hypothesis) */
  Result estimate(const std::vector<Vector2> &points_new, const std::vector<Vector2> &points_keyframe, const PinholeModel &model,
                  const std::vector<int32_t> &samples, double threshold = 1.5, double inliers_tolerance = 0.95) {
    if (points_new.size() != points_keyframe.size()) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the two point sets differ in size");
    const size_t n = points_new.size();
    Result out;
    out.inlier_indices.assign(n, 0);
    dsopp_hip_rotation_ransac_result res;
    check(dsopp_hip_rotation_ransac_estimate(r_, model.fx, model.fy, model.cx, model.cy, width_, height_, static_cast<int>(n),
                                             n ? points_new.front().data() : nullptr, n ? points_keyframe.front().data() : nullptr,
                                             static_cast<int>(samples.size() / 3), samples.data(), threshold, inliers_tolerance, &res,
                                             out.inlier_indices.data(), nullptr, nullptr, nullptr));
    out.inlier_indices.resize(static_cast<size_t>(res.inlier_count));
    out.inliers = static_cast<size_t>(res.inlier_count);
    out.matches = static_cast<size_t>(res.matches);
    for (int k = 0; k < 9; ++k) out.rotation[static_cast<size_t>(k)] = res.rotation[k];
    out.iterations_run = res.iterations_run;
    out.best_iteration = res.best_iteration;
    return out;
  }

  /** WaitForMovementInitializerKeyframeStrategy::needNewFrame (wait_for_movement_keyframe_strategy.cpp:13-29) */
  static FrameStatus needNewFrame(size_t previous_frames, size_t inliers, size_t matches, size_t sliding_window_length = 5,
                                  double rotation_inlier_ratio = 0.7) {
    if (previous_frames == 0) return FrameStatus::kKeepFrame;
    if (inliers > static_cast<size_t>(rotation_inlier_ratio * static_cast<double>(matches))) return FrameStatus::kDropFrame;
    if (sliding_window_length <= previous_frames + 1) return FrameStatus::kFinish;
    return FrameStatus::kKeepFrame;
  }
  /** addNewFrame's standstill test (add_new_frame.cpp:36-45): the frame is attached to the last keyframe */
  static bool isStandstill(size_t inliers, size_t matches, double max_ratio_of_so3_inliers = 0.7) {
    return static_cast<double>(inliers) / static_cast<double>(matches) > max_ratio_of_so3_inliers;
  }
  dsopp_hip_rotation_ransac *handle() const { return r_; }

 private:
  dsopp_hip_rotation_ransac *r_ = nullptr;
  int width_, height_;
};

/** A frame of the bootstrap's track (feature_based_slam::track::Frame): t_world_agent as 12 doubles, R row-major then t */
struct RefineFrame {
  size_t frame_id = 0;
  std::array<double, 12> t_world_agent{1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0};
  bool initialized = false;
};
/** A landmark of the bootstrap's track (track::Landmark): an optional position and its projections (frame id, pixel) */
struct RefineLandmark {
  bool has_position = false;
  std::array<double, 3> position{0, 0, 0};
  std::vector<std::pair<size_t, Vector2>> projections;
  const Vector2 *projection(size_t frame_id) const {
    for (const auto &p : projections)
      if (p.first == frame_id) return &p.second;
    return nullptr;
  }
};

/** The refinement of the bootstrap's track on the device, the three steps MonocularTracker runs after estimateSE3PnP
 *  (src/feature_based_slam/tracker/src/monocular_tracker.cpp:54-68): triangulatePoints (triangulate_points.cpp:47-71),
 *  optimizeTransformations (refine_track.cpp:16-83) and removeOutliers (remove_outliers.cpp:15-47), over dsopp_hip_geometric_ba.
 *  The object takes at most 16 frames per call (DSOPP_HIP_ERR_CAPACITY beyond): triangulatePoints reads every frame it is given, the
 *  other two the initialised ones among the last number_of_frames.
 *  Deviations: the solve is the library's LM over the Huber IRLS blocks, not Ceres's trust region with its loss corrector (include/dsopp_hip.h);
 *  with fewer than two initialised frames in the window optimizeTransformations changes nothing (Ceres would still move the landmarks
 *  against the one fixed frame); a second local frame whose t_agent_world has no translation (|t_1| = 0: no direction to hold) is
 *  DSOPP_HIP_ERR_INVALID_ARGUMENT. */
class HipRefineTrack {
 public:
  /** width, height: the image size of `model`, which bounds the ROI */
  HipRefineTrack(int width, int height, int device = 0, void *stream = nullptr) : width_(width), height_(height) {
    check(dsopp_hip_geometric_ba_create(device, stream, &b_));
  }
  ~HipRefineTrack() { dsopp_hip_geometric_ba_destroy(b_); }
  HipRefineTrack(const HipRefineTrack &) = delete;
  HipRefineTrack &operator=(const HipRefineTrack &) = delete;

  /** triangulatePoints(landmarks, frames, model, min_number_of_projections, retriangulation); returns how many positions were set */
  size_t triangulatePoints(std::vector<RefineLandmark> &landmarks, const std::deque<RefineFrame> &frames, const PinholeModel &model,
                           size_t min_number_of_projections, bool retriangulation) {
    std::vector<size_t> local;  // every frame takes part, initialised or not, as in the reference
    for (size_t i = 0; i < frames.size(); ++i) local.push_back(i);
    std::vector<size_t> chosen(landmarks.size());
    for (size_t l = 0; l < landmarks.size(); ++l) chosen[l] = l;
    Problem p = gather(landmarks, frames, local, chosen, model, false);
    std::vector<uint8_t> has(chosen.size()), done(chosen.size(), 0);
    for (size_t k = 0; k < chosen.size(); ++k) has[k] = landmarks[chosen[k]].has_position ? 1 : 0;
    check(dsopp_hip_geometric_ba_triangulate(b_, &p.c, has.data(), static_cast<int>(min_number_of_projections), retriangulation ? 1 : 0, done.data()));
    size_t count = 0;
    for (size_t k = 0; k < chosen.size(); ++k)
      if (done[k]) {
        RefineLandmark &lm = landmarks[chosen[k]];
        lm.has_position = true;
        for (size_t r = 0; r < 3; ++r) lm.position[r] = p.positions[3 * k + r];
        ++count;
      }
    return count;
  }

  /** optimizeTransformations<PinholeCamera, false>(landmarks, ..., frames, reprojection_threshold, number_of_frames_to_optimize, ...):
   *  the window of the last frames, the landmarks with a position and a projection in it (exists_in_window), the initialised frames as
   *  local frames, write-back of poses and positions.  `options` (NULL = the defaults with a = reprojection_threshold) */
  dsopp_hip_geometric_ba_result optimizeTransformations(std::vector<RefineLandmark> &landmarks, std::deque<RefineFrame> &frames, const PinholeModel &model,
                                                        double reprojection_threshold = 1.5, size_t number_of_frames_to_optimize = 10,
                                                        const dsopp_hip_geometric_ba_options *options = nullptr) {
    return optimize(landmarks, frames, model, nullptr, reprojection_threshold, number_of_frames_to_optimize, options);
  }

  /** ParameterParameterization (ceres_geometric_bundle_adjustment.hpp:16-27) with the reference's defaults */
  struct ParameterParameterization {
    bool fix_focal = true, fix_center = true, fix_model_specific = true, fix_poses = false, fix_landmarks = false;
    int32_t bits() const {
      return (fix_focal ? DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL : 0) | (fix_center ? DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER : 0) |
             (fix_model_specific ? DSOPP_HIP_GEOMETRIC_BA_FIX_MODEL_SPECIFIC : 0) | (fix_poses ? DSOPP_HIP_GEOMETRIC_BA_FIX_POSES : 0) |
             (fix_landmarks ? DSOPP_HIP_GEOMETRIC_BA_FIX_LANDMARKS : 0);
    }
  };
  /** the camera model of the OPTIMIZE_CAMERA form: PinholeCamera (fx, fy, cx, cy) or SimpleRadialCamera (f, cx, cy, k1, k2) */
  enum class CameraModel { kPinhole = DSOPP_HIP_GEOMETRIC_BA_PINHOLE, kSimpleRadial = DSOPP_HIP_GEOMETRIC_BA_SIMPLE_RADIAL };

  /** optimizeTransformations<Model, true>(landmarks, camera_intrinsics, image_size, frames, reprojection_threshold,
   *  number_of_frames_to_optimize, parameterization): as above with the intrinsics as a third parameter block, written back as
   *  refine_track.cpp:80-82 does.  `max_valid_radius` (NULL-able) receives the simple-radial constant of the intrinsics left. */
  dsopp_hip_geometric_ba_result optimizeTransformations(std::vector<RefineLandmark> &landmarks, std::vector<double> &camera_intrinsics,
                                                        CameraModel camera_model, std::deque<RefineFrame> &frames,
                                                        const ParameterParameterization &parameterization, double reprojection_threshold = 1.5,
                                                        size_t number_of_frames_to_optimize = 10,
                                                        const dsopp_hip_geometric_ba_options *options = nullptr, double *max_valid_radius = nullptr) {
    const size_t count = camera_model == CameraModel::kPinhole ? 4 : 5;
    if (camera_intrinsics.size() != count) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "the camera model takes other intrinsics");
    dsopp_hip_geometric_ba_camera camera{};
    camera.model = static_cast<int32_t>(camera_model);
    camera.fixed = parameterization.bits();
    for (size_t k = 0; k < count; ++k) camera.intrinsics[k] = camera_intrinsics[k];
    const dsopp_hip_geometric_ba_result result =
        optimize(landmarks, frames, PinholeModel{}, &camera, reprojection_threshold, number_of_frames_to_optimize, options);
    for (size_t k = 0; k < count; ++k) camera_intrinsics[k] = camera.intrinsics[k];
    if (max_valid_radius) *max_valid_radius = camera.max_valid_radius;
    return result;
  }

  /** removeOutliers(landmarks, model, frames, last_frames_to_filter, outlier_threshold); returns how many projections were removed */
  size_t removeOutliers(std::vector<RefineLandmark> &landmarks, const std::deque<RefineFrame> &frames, const PinholeModel &model,
                        size_t last_frames_to_filter = 10, double outlier_threshold = 0.5) {
    const size_t number_of_frames = std::min(frames.size(), last_frames_to_filter), start = frames.size() - number_of_frames;
    std::vector<size_t> chosen, local;
    for (size_t i = start; i < frames.size(); ++i)
      if (frames[i].initialized) local.push_back(i);
    for (size_t l = 0; l < landmarks.size(); ++l)
      if (landmarks[l].has_position) chosen.push_back(l);
    if (local.empty()) return 0;
    Problem p = gather(landmarks, frames, local, chosen, model, true);
    std::vector<uint8_t> flags(p.obs_frame.size(), 0);
    int32_t flagged = 0;
    check(dsopp_hip_geometric_ba_flag_outliers(b_, &p.c, outlier_threshold, flags.data(), &flagged));
    for (size_t k = 0; k < chosen.size(); ++k) {
      RefineLandmark &lm = landmarks[chosen[k]];
      for (int32_t o = p.offsets[k]; o < p.offsets[k + 1]; ++o)
        if (flags[static_cast<size_t>(o)]) {
          const size_t frame_id = frames[local[static_cast<size_t>(p.obs_frame[static_cast<size_t>(o)])]].frame_id;
          lm.projections.erase(std::remove_if(lm.projections.begin(), lm.projections.end(), [&](const auto &q) { return q.first == frame_id; }),
                               lm.projections.end());
        }
    }
    return static_cast<size_t>(flagged);
  }
  dsopp_hip_geometric_ba *handle() const { return b_; }

  /** the inverse of a rigid transform given as 12 doubles */
  static std::array<double, 12> inverse(const double *T) {
    std::array<double, 12> out{};
    for (size_t r = 0; r < 3; ++r) {
      for (size_t c = 0; c < 3; ++c) out[3 * r + c] = T[3 * c + r];
      out[9 + r] = -(T[r] * T[9] + T[3 + r] * T[10] + T[6 + r] * T[11]);
    }
    return out;
  }

 private:
  struct Problem {
    std::vector<double> poses, positions, obs_xy;
    std::vector<int32_t> offsets, obs_frame;
    dsopp_hip_geometric_ba_problem c;
  };
  /** the problem of local frames `local` (indices into `frames`) and landmarks `chosen`: t_agent_world per local frame, the observations
   *  grouped by landmark in the local frames' order */
  Problem gather(const std::vector<RefineLandmark> &landmarks, const std::deque<RefineFrame> &frames, const std::vector<size_t> &local,
                 const std::vector<size_t> &chosen, const PinholeModel &model, bool positions_required) const {
    Problem p;
    for (size_t i : local) {
      const std::array<double, 12> t_agent_world = inverse(frames[i].t_world_agent.data());
      p.poses.insert(p.poses.end(), t_agent_world.begin(), t_agent_world.end());
    }
    p.offsets.push_back(0);
    for (size_t l : chosen) {
      const RefineLandmark &lm = landmarks[l];
      for (size_t r = 0; r < 3; ++r) p.positions.push_back(lm.has_position || positions_required ? lm.position[r] : 0.0);
      for (size_t f = 0; f < local.size(); ++f)
        if (const Vector2 *xy = lm.projection(frames[local[f]].frame_id)) {
          p.obs_frame.push_back(static_cast<int32_t>(f));
          p.obs_xy.push_back((*xy)[0]);
          p.obs_xy.push_back((*xy)[1]);
        }
      p.offsets.push_back(static_cast<int32_t>(p.obs_frame.size()));
    }
    p.c = dsopp_hip_geometric_ba_problem{model.fx, model.fy, model.cx, model.cy, width_, height_, static_cast<int32_t>(local.size()),
                                         static_cast<int32_t>(chosen.size()), static_cast<int32_t>(p.obs_frame.size()), 0, p.poses.data(),
                                         p.positions.data(), p.offsets.data(), p.obs_frame.data(), p.obs_xy.data()};
    return p;
  }
  /** the body both forms of optimizeTransformations share: the window, exists_in_window, the local frames, the solve — with `camera` as
   *  a parameter block when one is given (the problem's own camera is then not read) — and the write-back of poses and positions */
  dsopp_hip_geometric_ba_result optimize(std::vector<RefineLandmark> &landmarks, std::deque<RefineFrame> &frames, const PinholeModel &model,
                                         dsopp_hip_geometric_ba_camera *camera, double reprojection_threshold, size_t number_of_frames_to_optimize,
                                         const dsopp_hip_geometric_ba_options *options) {
    const size_t number_of_frames = std::min(frames.size(), number_of_frames_to_optimize), start = frames.size() - number_of_frames;
    std::vector<size_t> chosen, local;
    for (size_t l = 0; l < landmarks.size(); ++l) {
      bool exists_in_window = false;
      for (size_t i = start; i < frames.size(); ++i)
        if (landmarks[l].has_position && landmarks[l].projection(frames[i].frame_id)) exists_in_window = true;
      if (exists_in_window) chosen.push_back(l);
    }
    for (size_t i = start; i < frames.size(); ++i)
      if (frames[i].initialized) local.push_back(i);
    dsopp_hip_geometric_ba_result result{};
    if (local.size() < 2) return result;
    Problem p = gather(landmarks, frames, local, chosen, model, true);
    dsopp_hip_geometric_ba_options o;
    if (options) {
      o = *options;
    } else {
      dsopp_hip_geometric_ba_default_options(&o);
      o.a = reprojection_threshold;
    }
    check(camera ? dsopp_hip_geometric_ba_solve_camera(b_, &p.c, camera, &o, &result, nullptr) : dsopp_hip_geometric_ba_solve(b_, &p.c, &o, &result, nullptr));
    for (size_t f = 0; f < local.size(); ++f) frames[local[f]].t_world_agent = inverse(p.poses.data() + 12 * f);
    for (size_t k = 0; k < chosen.size(); ++k)
      for (size_t r = 0; r < 3; ++r) landmarks[chosen[k]].position[r] = p.positions[3 * k + r];
    return result;
  }
  dsopp_hip_geometric_ba *b_ = nullptr;
  int width_, height_;
};

/** The pose of a bootstrap frame on the device: estimateSE3PnP (src/feature_based_slam/tracker/src/estimate_se3_pnp.cpp:23-77), the step
 *  MonocularTracker runs ahead of HipRefineTrack's three (monocular_tracker.cpp:54-56) and initializePoses for every intermediate frame
 *  (initialize_poses.cpp:47-73), over dsopp_hip_pnp_ransac.
 *  Deviations: the solver is the library's three-point RANSAC with an LM refinement, not OpenGV's EPnP RANSAC (include/dsopp_hip.h);
 *  every hypothesis is scored, there is no adaptive stop; the sample triples come from std::rand(), the sampler the rotation RANSAC
 *  mirrors, not from OpenGV's own generator. */
class HipEstimateSE3PnP {
 public:
  struct Result {
    size_t inliers, matches;  // estimateSE3PnP's pair: RANSAC's inliers (not the re-selected ones) and the matches
    dsopp_hip_pnp_ransac_result record;
    std::vector<size_t> inlier_landmarks;  // the landmarks that keep their projection: the refined pose's inliers, ascending
  };
  /** width, height: the image size of `model`, which bounds the ROI */
  HipEstimateSE3PnP(int width, int height, int device = 0, void *stream = nullptr) : width_(width), height_(height) {
    check(dsopp_hip_pnp_ransac_create(device, stream, &r_));
  }
  ~HipEstimateSE3PnP() { dsopp_hip_pnp_ransac_destroy(r_); }
  HipEstimateSE3PnP(const HipEstimateSE3PnP &) = delete;
  HipEstimateSE3PnP &operator=(const HipEstimateSE3PnP &) = delete;

  /** the landmarks with a position and a projection in frame `frame_id`, in landmark order: the candidates of estimateSE3PnP's first
   *  loop.  Those whose projection fails the ROI are no matches of the reference; the device leaves them out of every count. */
  static std::vector<size_t> candidates(size_t frame_id, const std::vector<RefineLandmark> &landmarks) {
    std::vector<size_t> out;
    for (size_t l = 0; l < landmarks.size(); ++l)
      if (landmarks[l].has_position && landmarks[l].projection(frame_id)) out.push_back(l);
    return out;
  }

  /** estimateSE3PnP(frame_id, landmarks, frame.t_world_agent, model, pnp_ransac_threshold): the triples come from std::rand() */
  Result estimate(size_t frame_id, std::vector<RefineLandmark> &landmarks, RefineFrame &frame, const PinholeModel &model,
                  double pnp_ransac_threshold = 0.5) {
    const size_t n = candidates(frame_id, landmarks).size();
    const size_t iterations = static_cast<size_t>(dsopp_hip_pnp_ransac_default_iterations());
    return estimate(frame_id, landmarks, frame, model, n < 3 ? std::vector<int32_t>() : HipRotationStandstill::drawSamples(n, iterations),
                    pnp_ransac_threshold);
  }
  /** the same over the caller's triples (3 indices per hypothesis, into the candidates) */
  Result estimate(size_t frame_id, std::vector<RefineLandmark> &landmarks, RefineFrame &frame, const PinholeModel &model,
                  const std::vector<int32_t> &samples, double pnp_ransac_threshold = 0.5, const dsopp_hip_pnp_ransac_options *options = nullptr) {
    const std::vector<size_t> chosen = candidates(frame_id, landmarks);
    const size_t n = chosen.size();
    std::vector<double> positions(3 * n), observations(2 * n);
    for (size_t k = 0; k < n; ++k) {
      const RefineLandmark &lm = landmarks[chosen[k]];
      const Vector2 &xy = *lm.projection(frame_id);
      for (size_t r = 0; r < 3; ++r) positions[3 * k + r] = lm.position[r];
      observations[2 * k] = xy[0];
      observations[2 * k + 1] = xy[1];
    }
    Result out;
    std::vector<int32_t> indices(n, 0);
    check(dsopp_hip_pnp_ransac_estimate(r_, model.fx, model.fy, model.cx, model.cy, width_, height_, static_cast<int>(n), positions.data(),
                                        observations.data(), static_cast<int>(samples.size() / 3), samples.data(), pnp_ransac_threshold, options,
                                        &out.record, indices.data(), nullptr, nullptr, nullptr));
    out.inliers = static_cast<size_t>(out.record.ransac_inlier_count);
    out.matches = static_cast<size_t>(out.record.matches);
    frame.t_world_agent = HipRefineTrack::inverse(out.record.pose);
    // every landmark with a position that is not a final inlier loses its projection in this frame (:64-74), a non-match too
    std::vector<uint8_t> keeps(n, 0);
    for (int32_t k = 0; k < out.record.refined_inlier_count; ++k) keeps[static_cast<size_t>(indices[static_cast<size_t>(k)])] = 1;
    for (size_t k = 0; k < n; ++k) {
      if (keeps[k]) {
        out.inlier_landmarks.push_back(chosen[k]);
        continue;
      }
      auto &projections = landmarks[chosen[k]].projections;
      projections.erase(std::remove_if(projections.begin(), projections.end(), [&](const auto &q) { return q.first == frame_id; }), projections.end());
    }
    return out;
  }

  /** initializePoses' test of the returned pair (initialize_poses.cpp:47-73): inliers > (size_t)(ratio * matches) */
  static bool initialised(size_t inliers, size_t matches, double ratio = 0.5) {
    return inliers > static_cast<size_t>(ratio * static_cast<double>(matches));
  }
  dsopp_hip_pnp_ransac *handle() const { return r_; }

 private:
  dsopp_hip_pnp_ransac *r_ = nullptr;
  int width_, height_;
};

/** The two-view pose that initialises a track, on the device: estimateSO3xS2 (src/feature_based_slam/tracker/src/estimate_so3xs2.cpp:23-110)
 *  and the two-view triangulatePoints (triangulate_points.cpp:18-45), steps I and II of initializePoses, over dsopp_hip_two_view_ransac.
 *  The reference calls its result t_t_r, but it maps the target (last) frame into the reference (first) frame and is stored as the last
 *  frame's t_world_agent (initialize_poses.cpp:31-33, include/dsopp_hip.h): so it is here.
 *  Deviations: the solver is the library's five-point RANSAC with its own LM refinements, not OpenGV's and Ceres's (include/dsopp_hip.h);
 *  every hypothesis is scored, there is no adaptive stop; the samples come from std::rand(), as HipEstimateSE3PnP's do. */
class HipEstimateSO3xS2 {
 public:
  struct Result {
    size_t inliers, matches;  // estimateSO3xS2's pair: the re-selected inliers and the matches
    dsopp_hip_two_view_ransac_result record;
    std::vector<size_t> inlier_landmarks;  // the landmarks that keep their projection in the target frame, ascending
  };
  /** width, height: the image size of `model`, which bounds the ROI */
  HipEstimateSO3xS2(int width, int height, int device = 0, void *stream = nullptr) : width_(width), height_(height) {
    check(dsopp_hip_two_view_ransac_create(device, stream, &r_));
  }
  ~HipEstimateSO3xS2() { dsopp_hip_two_view_ransac_destroy(r_); }
  HipEstimateSO3xS2(const HipEstimateSO3xS2 &) = delete;
  HipEstimateSO3xS2 &operator=(const HipEstimateSO3xS2 &) = delete;

  /** getLandmarksFromTwoFrames: the landmarks with a projection in both frames, in landmark order.  Those with an observation outside the
   *  ROI are no matches of the reference (:40-41); the device leaves them out of every count. */
  static std::vector<size_t> candidates(size_t reference_frame_id, size_t target_frame_id, const std::vector<RefineLandmark> &landmarks) {
    std::vector<size_t> out;
    for (size_t l = 0; l < landmarks.size(); ++l)
      if (landmarks[l].projection(reference_frame_id) && landmarks[l].projection(target_frame_id)) out.push_back(l);
    return out;
  }

  /** `iterations` samples of five distinct indices < n from std::rand(), drawn as HipRotationStandstill::drawSamples draws its triples */
  static std::vector<int32_t> drawSamples(size_t n, size_t iterations) {
    if (iterations > 0 && n < 5) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "fewer than 5 pairs: no sample of distinct indices");
    std::vector<int32_t> samples(5 * iterations);
    for (size_t i = 0; i < iterations; ++i) {
      size_t sequence[5];
      for (size_t k = 0; k < 5; ++k) {
        size_t next = static_cast<size_t>(std::rand()) % n;
        auto repeats = [&] {
          for (size_t j = 0; j < k; ++j)
            if (sequence[j] == next) return true;
          return false;
        };
        while (repeats()) next = static_cast<size_t>(std::rand()) % n;
        sequence[k] = next;
      }
      for (size_t k = 0; k < 5; ++k) samples[5 * i + k] = static_cast<int32_t>(sequence[k]);
    }
    return samples;
  }

  /** estimateSO3xS2(reference_frame_id, target_frame_id, landmarks, target.t_world_agent, ..., min_ransac_matches,
   *  essential_matrix_ransac_threshold, reprojection_threshold): the samples come from std::rand() */
  Result estimate(size_t reference_frame_id, size_t target_frame_id, std::vector<RefineLandmark> &landmarks, RefineFrame &target,
                  const PinholeModel &model, size_t min_ransac_matches = 50, double essential_matrix_ransac_threshold = 0.5,
                  double reprojection_threshold = 1.5) {
    const size_t n = candidates(reference_frame_id, target_frame_id, landmarks).size();
    const size_t iterations = static_cast<size_t>(dsopp_hip_two_view_ransac_default_iterations());
    return estimate(reference_frame_id, target_frame_id, landmarks, target, model, n < 5 ? std::vector<int32_t>() : drawSamples(n, iterations),
                    min_ransac_matches, essential_matrix_ransac_threshold, reprojection_threshold);
  }
  /** the same over the caller's samples (5 indices per hypothesis, into the candidates) */
  Result estimate(size_t reference_frame_id, size_t target_frame_id, std::vector<RefineLandmark> &landmarks, RefineFrame &target,
                  const PinholeModel &model, const std::vector<int32_t> &samples, size_t min_ransac_matches = 50,
                  double essential_matrix_ransac_threshold = 0.5, double reprojection_threshold = 1.5) {
    const std::vector<size_t> chosen = candidates(reference_frame_id, target_frame_id, landmarks);
    const size_t n = chosen.size();
    std::vector<double> a(2 * n), b(2 * n);
    for (size_t k = 0; k < n; ++k) {
      const Vector2 &pa = *landmarks[chosen[k]].projection(reference_frame_id), &pb = *landmarks[chosen[k]].projection(target_frame_id);
      a[2 * k] = pa[0];
      a[2 * k + 1] = pa[1];
      b[2 * k] = pb[0];
      b[2 * k + 1] = pb[1];
    }
    dsopp_hip_two_view_ransac_options options;
    dsopp_hip_two_view_ransac_default_options(&options);
    options.a = reprojection_threshold;
    Result out;
    std::vector<int32_t> indices(n, 0);
    check(dsopp_hip_two_view_ransac_estimate(r_, model.fx, model.fy, model.cx, model.cy, width_, height_, static_cast<int>(n), a.data(), b.data(),
                                             static_cast<int>(samples.size() / 5), samples.data(), essential_matrix_ransac_threshold,
                                             static_cast<int>(min_ransac_matches), &options, &out.record, indices.data(), nullptr, nullptr, nullptr));
    out.matches = static_cast<size_t>(out.record.matches);
    // too few matches: {0, matches}, the pose and the projections untouched (:48)
    if (out.matches < min_ransac_matches) {
      out.inliers = 0;
      return out;
    }
    out.inliers = static_cast<size_t>(out.record.inlier_count);
    for (size_t e = 0; e < 12; ++e) target.t_world_agent[e] = out.record.pose[e];
    // every landmark of the two frames that is not an inlier loses its projection in the target frame (:77-86), a non-match too
    std::vector<uint8_t> keeps(n, 0);
    for (int32_t k = 0; k < out.record.inlier_count; ++k) keeps[static_cast<size_t>(indices[static_cast<size_t>(k)])] = 1;
    for (size_t k = 0; k < n; ++k) {
      if (keeps[k]) {
        out.inlier_landmarks.push_back(chosen[k]);
        continue;
      }
      auto &projections = landmarks[chosen[k]].projections;
      projections.erase(std::remove_if(projections.begin(), projections.end(), [&](const auto &q) { return q.first == target_frame_id; }),
                        projections.end());
    }
    return out;
  }

  /** triangulatePoints(reference_frame_id, target_frame_id, landmarks, reference.t_world_agent, target.t_world_agent, model,
   *  triangulation_cos_threshold): sets the position of every kept landmark of the two frames; returns their number */
  size_t triangulatePoints(size_t reference_frame_id, size_t target_frame_id, std::vector<RefineLandmark> &landmarks, const RefineFrame &reference,
                           const RefineFrame &target, const PinholeModel &model, double triangulation_cos_threshold = 0.9999) {
    const std::vector<size_t> chosen = candidates(reference_frame_id, target_frame_id, landmarks);
    const size_t n = chosen.size();
    std::vector<double> a(2 * n), b(2 * n), positions(3 * n);
    std::vector<uint8_t> keep(n, 0);
    for (size_t k = 0; k < n; ++k) {
      const Vector2 &pa = *landmarks[chosen[k]].projection(reference_frame_id), &pb = *landmarks[chosen[k]].projection(target_frame_id);
      a[2 * k] = pa[0];
      a[2 * k + 1] = pa[1];
      b[2 * k] = pb[0];
      b[2 * k + 1] = pb[1];
    }
    // t_r_t = t_w_r^-1 t_w_t (:21)
    const std::array<double, 12> inv = HipRefineTrack::inverse(reference.t_world_agent.data());
    std::array<double, 12> t_r_t{};
    for (size_t i = 0; i < 3; ++i) {
      for (size_t j = 0; j < 3; ++j)
        t_r_t[3 * i + j] = inv[3 * i] * target.t_world_agent[j] + inv[3 * i + 1] * target.t_world_agent[3 + j] + inv[3 * i + 2] * target.t_world_agent[6 + j];
      t_r_t[9 + i] = inv[3 * i] * target.t_world_agent[9] + inv[3 * i + 1] * target.t_world_agent[10] + inv[3 * i + 2] * target.t_world_agent[11] + inv[9 + i];
    }
    check(dsopp_hip_two_view_ransac_triangulate(r_, model.fx, model.fy, model.cx, model.cy, width_, height_, static_cast<int>(n), a.data(), b.data(),
                                                t_r_t.data(), reference.t_world_agent.data(), triangulation_cos_threshold, positions.data(), keep.data()));
    size_t count = 0;
    for (size_t k = 0; k < n; ++k)
      if (keep[k]) {
        RefineLandmark &lm = landmarks[chosen[k]];
        lm.has_position = true;
        for (size_t r = 0; r < 3; ++r) lm.position[r] = positions[3 * k + r];
        ++count;
      }
    return count;
  }

  /** initializePoses' test of the returned pair (initialize_poses.cpp:37): false iff inliers < (size_t)(ratio * matches) */
  static bool accepted(size_t inliers, size_t matches, double ratio = 0.6) { return !(inliers < static_cast<size_t>(ratio * static_cast<double>(matches))); }
  dsopp_hip_two_view_ransac *handle() const { return r_; }

 private:
  dsopp_hip_two_view_ransac *r_ = nullptr;
  int width_, height_;
};

/** initializePoses (src/feature_based_slam/tracker/src/initialize_poses.cpp:17-78) composed from the library: I. HipEstimateSO3xS2 between
 *  the first and the last frame, II. its triangulation, III. HipEstimateSE3PnP for every frame between them, IV. HipRefineTrack's
 *  optimizeTransformations over all frames (refine_track's defaults: the last 10), V. the PnP again for the frames III left uninitialised.
 *  The samples of every step come from std::rand(), which the caller seeds. */
class HipInitializePoses {
 public:
  struct Options {  // feature_based_slam/tracker/initializer.hpp:25-39
    double reprojection_threshold = 1.5;
    size_t min_ransac_matches = 50;
    double se3_inlier_ratio = 0.6;
    double essential_matrix_ransac_threshold = 0.5;
    double triangulation_cos_threshold = 0.9999;
    double pnp_inlier_ratio = 0.5;
    double pnp_ransac_threshold = 0.5;
  };
  struct Result {
    bool success = false;
    HipEstimateSO3xS2::Result two_view{};
    size_t triangulated = 0, pnp_initialized = 0;
    std::vector<HipEstimateSE3PnP::Result> pnp, second_pnp;  // per intermediate frame of III; per frame V ran for
    dsopp_hip_geometric_ba_result refinement{};
  };
  HipInitializePoses(int width, int height, int device = 0, void *stream = nullptr)
      : two_view_(width, height, device, stream), pnp_(width, height, device, stream), refine_(width, height, device, stream) {}

  Result run(std::deque<RefineFrame> &frames, std::vector<RefineLandmark> &landmarks, const PinholeModel &model) {
    return run(frames, landmarks, model, Options{});
  }
  Result run(std::deque<RefineFrame> &frames, std::vector<RefineLandmark> &landmarks, const PinholeModel &model, const Options &options) {
    Result out;
    if (frames.size() < 2) throw SolverError(DSOPP_HIP_ERR_INVALID_ARGUMENT, "initializePoses needs two frames");
    RefineFrame &first = frames.front(), &last = frames.back();
    /* I. */
    out.two_view = two_view_.estimate(first.frame_id, last.frame_id, landmarks, last, model, options.min_ransac_matches,
                                      options.essential_matrix_ransac_threshold, options.reprojection_threshold);
    if (!HipEstimateSO3xS2::accepted(out.two_view.inliers, out.two_view.matches, options.se3_inlier_ratio)) return out;
    first.initialized = true;
    last.initialized = true;
    /* II. */
    out.triangulated = two_view_.triangulatePoints(first.frame_id, last.frame_id, landmarks, first, last, model, options.triangulation_cos_threshold);
    /* III. */
    for (size_t i = 1; i + 1 < frames.size(); ++i) {
      out.pnp.push_back(pnp_.estimate(frames[i].frame_id, landmarks, frames[i], model, options.pnp_ransac_threshold));
      if (HipEstimateSE3PnP::initialised(out.pnp.back().inliers, out.pnp.back().matches, options.pnp_inlier_ratio)) {
        frames[i].initialized = true;
        ++out.pnp_initialized;
      }
    }
    if (out.pnp_initialized < 1) return out;
    /* IV. */
    out.refinement = refine_.optimizeTransformations(landmarks, frames, model, options.reprojection_threshold);
    /* V. */
    for (size_t i = 1; i + 1 < frames.size(); ++i) {
      if (frames[i].initialized) continue;
      out.second_pnp.push_back(pnp_.estimate(frames[i].frame_id, landmarks, frames[i], model, options.pnp_ransac_threshold));
    }
    out.success = true;
    return out;
  }

 private:
  HipEstimateSO3xS2 two_view_;
  HipEstimateSE3PnP pnp_;
  HipRefineTrack refine_;
};

}  // namespace dsopp_hip_host
