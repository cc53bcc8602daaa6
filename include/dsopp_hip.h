/* dsopp_hip.h — C-ABI of the MI355X-native photometric bundle adjustment / direct image alignment hot path.
 *
 * This is the drop-in boundary: a thin `extern "C"` layer with plain pointers and sizes that a
 * `solver: hip` backend of DSOPP binds to.  The reference itself has no FFI; its plugin API is a pair of C++ abstract
 * class templates selected by a YAML string in a factory (src/tracker/tracker/src/fabric.cpp:58-180).  Each entry point
 * below cites the reference member function whose work it replaces.  INTEGRATION.md shows the reference-side adapter
 * classes (`HipPhotometricBundleAdjustment`, `HipPoseAlignment`, mirrored in dsopp_amd/host/) that call these.
 *
 * Path shorthands used in citations:
 *   PBA_INC  = src/energy/problems/include/energy/problems/photometric_bundle_adjustment
 *   PBA_INT  = src/energy/problems/internal/energy/problems/photometric_bundle_adjustment
 *   PA_INC   = src/energy/problems/include/energy/problems/pose_alignment
 *   PROB_SRC = src/energy/problems/src
 *
 * Conventions
 *   - every function returns DSOPP_HIP_OK (0) or a negative error code; dsopp_hip_last_error() gives the message
 *     (thread-local).  No exceptions cross the boundary.
 *   - all host buffers are caller-owned and only read/written during the call; handles are opaque and used from one
 *     thread at a time (the reference calls its solvers from the single tracker thread only).
 *   - poses are 7 doubles in Sophus::SE3 storage order (qx, qy, qz, qw, tx, ty, tz); tangent vectors are
 *     (translation, rotation); per-frame state blocks are 8 doubles (6 pose + affine a, b); K = 8 * number of frames.
 *   - matrices are row-major doubles.
 *   - there is NO CPU fallback: every entry point that computes fails with DSOPP_HIP_ERR_HIP when no gfx950 device
 *     is available.
 */
#ifndef DSOPP_HIP_H
#define DSOPP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSOPP_HIP_PATTERN_SIZE 8 /* Pattern::kSize — src/common/pattern/include/common/pattern/pattern.hpp:17 */
#define DSOPP_HIP_BLOCK_SIZE 8   /* Motion::DoF + 2 */
#define DSOPP_HIP_MAX_FRAMES 16  /* window capacity (reference configs use 5..15 keyframes) */
#define DSOPP_HIP_MAX_LEVELS 5   /* PixelDataFrame::kMaxPyramidDepth — src/features/include/features/camera/pixel_data_frame.hpp:26 */

enum {
  DSOPP_HIP_OK = 0,
  DSOPP_HIP_ERR_INVALID_ARGUMENT = -1,
  DSOPP_HIP_ERR_NOT_FOUND = -2,
  DSOPP_HIP_ERR_ORDER = -3,    /* frames must be pushed in ascending timestamp order (PROB_SRC/photometric_bundle_adjustment.cpp:101-102) */
  DSOPP_HIP_ERR_HIP = -4,      /* HIP runtime failure / no device */
  DSOPP_HIP_ERR_CAPACITY = -5, /* window full */
  DSOPP_HIP_ERR_STATE = -6     /* call sequence violation (e.g. stage call before begin) */
};

/* track::PointConnectionStatus — src/track/connections/include/track/connections/frame_connection.hpp:19-25 */
enum { DSOPP_HIP_STATUS_OK = 0, DSOPP_HIP_STATUS_OUTLIER = 1, DSOPP_HIP_STATUS_OCCLUDED = 2, DSOPP_HIP_STATUS_OOB = 3, DSOPP_HIP_STATUS_UNKNOWN = 4 };

/* storage / evaluation scalar of the device images and sweeps.  F64 matches the reference's default build
 * (Precision = double, src/common/include/common/settings.hpp:10-14); F32 matches its -DUSE_FLOAT=ON build.
 * Normal equations are accumulated in fp64 in both. */
enum { DSOPP_HIP_F64 = 0, DSOPP_HIP_F32 = 1 };

const char *dsopp_hip_last_error(void);
int dsopp_hip_device_count(int *count);
const char *dsopp_hip_version(void);

/* TrustRegionPhotometricBundleAdjustmentOptions (PBA_INC/trust_region_photometric_bundle_adjustment_options.hpp:14-52)
 * + the EigenPhotometricBundleAdjustment ctor flags (PROB_SRC/eigen_photometric_bundle_adjustment.cpp:47-57)
 * + the class template switches FIRST_ESTIMATE_JACOBIANS / OPTIMIZE_IDEPTHS */
typedef struct dsopp_hip_options {
  int32_t max_iterations;
  double initial_trust_region_radius;
  double function_tolerance;
  double parameter_tolerance;
  double affine_brightness_regularizer[2];
  double fixed_state_regularizer;
  double sigma_huber_loss;
  int32_t estimate_uncertainty;
  int32_t force_accept;
  int32_t first_estimate_jacobians;
  int32_t optimize_idepths;
  int32_t dtype; /* DSOPP_HIP_F64 | DSOPP_HIP_F32 */
} dsopp_hip_options;

/* production values of createPhotometricBundleAdjustment / createPoseAlignment — src/tracker/tracker/src/fabric.cpp:63-79,127-142 */
void dsopp_hip_default_pba_options(dsopp_hip_options *o);
void dsopp_hip_default_align_options(dsopp_hip_options *o);

/* ------------------------------------------------------------------------------------------------------------------
 * Image pyramid of one frame, resident in HBM (replaces features::PixelDataFrame / PixelMap<1> levels + CameraMask)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_pyramid dsopp_hip_pyramid;

/* allocate `levels` (<= DSOPP_HIP_MAX_LEVELS) texel images of width>>l x height>>l on `device`.
 * `stream` is a hipStream_t (NULL = the library creates its own non-blocking stream). */
int dsopp_hip_pyramid_create(int device, void *stream, int width, int height, int levels, int dtype, dsopp_hip_pyramid **out);
void dsopp_hip_pyramid_destroy(dsopp_hip_pyramid *p);
/* PixelDataFrame ctor (src/features/src/pixel_data_frame.cpp:12-31): photometric correction LUT[u8] * vmax/(vignette+1)
 * (src/features/src/photometrically_corrected_image.cpp:9-29), 2x2 box pyramid (downscale_image.hpp:16-33), per-level
 * (I, dI/dx, dI/dy) (src/features/src/calculate_pixelinfo.cpp:340-374).  lut256 / vignetting may be NULL.
 * The host arrays are consumed before the call returns (the image through a pinned copy: its upload and the build run behind the call on
 * the pyramid's stream; every consumer of the library orders itself behind them). */
int dsopp_hip_pyramid_build(dsopp_hip_pyramid *p, const uint8_t *image_host, const double *lut256, const uint8_t *vignetting_host);
/* same, the u8 image (and vignette) already in HBM: no PCIe transfer of pixels inside the call and no host sync
 * (the call only enqueues work on the pyramid's stream).  vignetting_max = max over the vignette image
 * (cv::minMaxLoc in the reference, a per-camera constant); ignored when vignetting_dev is NULL. */
int dsopp_hip_pyramid_build_device(dsopp_hip_pyramid *p, const void *image_dev, const double *lut256, const void *vignetting_dev,
                                   double vignetting_max);
/* adopt a level built by the reference's host code: pixelinfo = H_l x W_l x (I, dx, dy) doubles = PixelInfo<1>::data_
 * (src/features/include/features/camera/pixel_map.hpp:79-132) */
int dsopp_hip_pyramid_set_level(dsopp_hip_pyramid *p, int level, const double *pixelinfo_host);
/* CameraMask of a level (src/sensors/camera_calibration/include/sensors/camera_calibration/mask/camera_mask.hpp:48-89);
 * NULL = all valid */
int dsopp_hip_pyramid_set_mask(dsopp_hip_pyramid *p, int level, const uint8_t *mask_host);
int dsopp_hip_pyramid_get_level(dsopp_hip_pyramid *p, int level, double *pixelinfo_host);
int dsopp_hip_pyramid_level_size(dsopp_hip_pyramid *p, int level, int *width, int *height);

/* ------------------------------------------------------------------------------------------------------------------
 * Image undistortion (replaces sensors::calibration::Undistorter::undistort — src/sensors/camera_calibration/src/undistorter.cpp:7-18 —
 * which src/sensors/camera/src/camera.cpp:70 runs on every frame and src/sensors/sensors_builder/src/camera_fabric.cpp:164-167 once
 * on the static mask and the vignette; src/sensors/camera_calibration/src/fabric.cpp:45-49,67-71 builds one for every simple_radial
 * and TUM-FOV calibration)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_undistorter dsopp_hip_undistorter;
/* Undistorter(remapX, remapY, input_width, input_height) (undistorter.hpp:35-36): map_x / map_y are the two CV_32F remap tables
 * (out_h x out_w floats, row-major) that constructRemaps (undistorter.hpp:69-142) fills on the host (dsopp_hip_undistorter_create_from_model
 * builds them from the camera model on the device instead); the reference has out == in,
 * both sizes are taken as cv::remap takes them.  NULL, NULL = Undistorter::Identity (undistorter.cpp:20-22; out must equal in).
 * The arithmetic of every later undistort is integer and fixed here, for a single-channel 8-bit image (cv::remap INTER_LINEAR,
 * BORDER_REFLECT_101, undistorter.cpp:16):
 *   sx = rint(map_x * 32.0f) (half to even), ix = sx >> 5 (arithmetic: the floor), fx = sx & 31; sy, iy, fy alike;
 *   taps (ix, iy), (ix + 1, iy), (ix, iy + 1), (ix + 1, iy + 1), each coordinate reflected on its own with period 2 (n - 1);
 *   out = (sum of weight * tap + 16384) >> 15, weights (32 - fx)(32 - fy) * 32, fx (32 - fy) * 32, (32 - fx) fy * 32, fx fy * 32.
 * So a map entry without fractions copies a pixel, and the failure marker (-1, -1) of estimateRemaps (undistorter.hpp:138-139)
 * yields src[1, 1].  The maps are folded into a device table before the call returns and are not needed afterwards.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: a non-finite map entry, |entry| > 2^20, in_w < 2 or in_h < 2, only one of the two maps. */
int dsopp_hip_undistorter_create(int device, void *stream, int in_w, int in_h, int out_w, int out_h, const float *map_x, const float *map_y,
                                 dsopp_hip_undistorter **out);
void dsopp_hip_undistorter_destroy(dsopp_hip_undistorter *u);
/* input_width() / input_height() (undistorter.cpp:24-26) and the size of the maps; any pointer may be NULL */
int dsopp_hip_undistorter_sizes(const dsopp_hip_undistorter *u, int *in_w, int *in_h, int *out_w, int *out_h);
/* Undistorter::undistort(img) (undistorter.cpp:7-18) of an in_h x in_w 8-bit image into out_h x out_w bytes, blocking: the
 * once-per-camera form for the static mask and the vignette (camera_fabric.cpp:164-167). */
int dsopp_hip_undistorter_undistort(dsopp_hip_undistorter *u, const uint8_t *image_host, uint8_t *out_host);
/* same, both images in HBM: the call only enqueues one launch on `stream` (a hipStream_t; NULL = the undistorter's own).  Both
 * pointers must be 4-byte aligned, else DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_undistorter_undistort_device(dsopp_hip_undistorter *u, const void *image_dev, void *out_dev, void *stream);
/* The per-frame path, camera.cpp:70 followed by the PixelDataFrame ctor: dsopp_hip_pyramid_build of undistort(distorted_host).  The
 * distorted in_h x in_w image goes through the pyramid's pinned buffer as in build, is remapped on the pyramid's stream into an 8-bit
 * image the pyramid keeps (dsopp_hip_feature_extractor_extract_from_pyramid reads it), and the levels are built from that.
 * vignetting_host is the vignette already undistorted, as the reference keeps it (undistorted_vignetting_,
 * src/features/src/pixel_data_frame_extractor.cpp:8-14).  f64 and f32 pyramids.  The pyramid and the undistorter must be on one
 * device and the pyramid's size must be the undistorter's out size, else DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_pyramid_build_undistorted(dsopp_hip_pyramid *p, const dsopp_hip_undistorter *u, const uint8_t *distorted_host, const double *lut256,
                                        const uint8_t *vignetting_host);

/* ------------------------------------------------------------------------------------------------------------------
 * The undistorter's remap tables from the camera model (replaces Undistorter::constructRemaps / estimateRemaps — src/sensors/
 * camera_calibration/include/sensors/camera_calibration/undistorter/undistorter.hpp:69-142 —, which src/sensors/camera_calibration/src/
 * fabric.cpp:45-49,67-71 runs once for every simple_radial and TUM-FOV calibration, with the projections of CAM = src/energy/camera_model/
 * include/energy/camera_model: CAM/pinhole/pinhole_camera.hpp:129-141, CAM/pinhole/simple_radial.hpp:39-83,134-160,
 * CAM/fisheye/tum_fov_model.hpp:72-82, CAM/fisheye/atan_camera.hpp:98-127, CAM/polynomial_solver.hpp:11-41).  The maps are evaluated on
 * the device, one independent evaluation per pixel, and folded there into the table dsopp_hip_undistorter_create folds on the host.
 *
 * The arithmetic, binary64 in the order written, every product, sum, quotient and square root one IEEE step (nothing is fused):
 *   the target pinhole (undistorter.hpp:70-80) is (focalX, focalY, width / 2, height / 2) at the model's own size (w, h);
 *   per output pixel (x, y) (undistorter.hpp:124-141, pinhole_camera.hpp:129-141): the unprojection fails unless 4 <= x <= w - 5 and
 *   4 <= y <= h - 5;  rx = (x - w / 2) * (1 / fx), ry = (y - h / 2) * (1 / fy) — a product with the inverse, not a division; the ray
 *   is (rx, ry, 1).  "ROI" of a point p: 4 <= px <= w - 5 and 4 <= py <= h - 5 (camera_model_base.hpp:52-60).
 *   simple-radial (simple_radial.hpp:134-160): r2 = rx rx + ry ry; fail if sqrt(r2) > max_valid_radius; d = (1 + k1 r2) + (k2 r2) r2;
 *     p = ((rx d) f + cx, (ry d) f + cy); fail unless p is in the ROI.
 *   TUM-FOV (tum_fov_model.hpp:72-82): ru = sqrt(rx rx + ry ry); ru < 1e-8: p = (cx, cy), success, no ROI test; else
 *     rd = atan2((2 ru) T, 1) / fov with T = tan(fov / 2) computed once on the host; q = rd / ru; p = ((q rx) fx + cx, (q ry) fy + cy);
 *     fail unless p is in the ROI.
 *   atan (atan_camera.hpp:98-127): n = sqrt((rx rx + ry ry) + 1); a = (rx / n, ry / n, 1 / n); rho = sqrt(ax ax + ay ay); rho < 1e-6:
 *     p = (cx, cy), success, no ROI test; else theta = atan2(rho, az); Horner from the top coefficient, s = 0, s = s theta + k[i];
 *     s = theta (1 + s theta); p = (((ax s) / rho) fx + cx, ((ay s) / rho) fy + cy); fail unless p is in the ROI.
 *   The map entry is ((float)px, (float)py), round to nearest even; either failure gives (-1, -1) (undistorter.hpp:134-140), which the
 *   remap turns into src[1, 1] as stated at dsopp_hip_undistorter_create.  The fold into the table is the statement given there
 *   (sx = rint(map * 32.0f), the split, the reflection), run by the same code on the host and on the device.
 * What this does not pin: the reference's own build may contract products and sums into fused operations (the GCC default), so its last
 * bit is not pinned by this statement; atan2 on the device is the device math library's (OCML), so TUM-FOV and atan maps are not
 * bit-pinned to any host libm (simple-radial maps are: sqrt, products and sums only); and max_valid_radius below comes from this
 * library's own root finder, whose parity with the eigenvalues of Eigen's companion matrix (polynomial_solver.hpp:23-28) is unpinned —
 * both are roots of one polynomial to about an ulp, and a pixel whose radius lies between the two would differ.
 * ---------------------------------------------------------------------------------------------------------------- */
#define DSOPP_HIP_CAMERA_MAX_K 16
enum { DSOPP_HIP_CAMERA_SIMPLE_RADIAL = 0, DSOPP_HIP_CAMERA_TUM_FOV = 1, DSOPP_HIP_CAMERA_ATAN = 2 };
/* SimpleRadialCamera (simple_radial.hpp:39-46): params = (f, cx, cy), k = (k1, k2), num_k = 2.
 * TUMFovModel (tum_fov_model.hpp:37-43): params = (fx, fy, cx, cy) in pixels, k = (fov), num_k = 1.
 * AtanCamera (atan_camera.hpp:86-88): params = (fx, fy, cx, cy) in pixels, k = the polynomial data_[4 ...], num_k = 0 .. 16. */
typedef struct dsopp_hip_camera_model {
  int32_t type; /* DSOPP_HIP_CAMERA_* */
  int32_t width, height;
  int32_t num_k;
  double params[4];
  double k[DSOPP_HIP_CAMERA_MAX_K];
} dsopp_hip_camera_model;
/* The pinhole of constructRemaps (undistorter.hpp:70-80): pinhole_intrinsics = (focalX, focalY, width / 2, height / 2).  Needs no device.
 * derived: for simple-radial the constructor's constants (simple_radial.hpp:47-82) max_valid_radius_, line_after_radius_(0),
 * line_after_radius_(1); zeros for the other types.  max_valid_radius_ is the least positive root of k2 r^5 + k1 r^3 + r - R, R the
 * corner radius (:47-50), found by bracketing between the roots of the derivative (a quadratic in r^2) and a safeguarded Newton
 * iteration in the bracket; as in the reference the polynomial is normalised and its leading coefficients below 1e-8 are dropped
 * (polynomial_solver.hpp:14-19), and no positive root gives +inf (:30-40).  The extremum rule (simple_radial.hpp:62-77) is applied as
 * written in IEEE arithmetic: with k2 == 0 its divisions give NaN or inf and the comparisons decide.  Either output may be NULL.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: the model errors listed below. */
int dsopp_hip_camera_model_to_pinhole(const dsopp_hip_camera_model *model, double pinhole_intrinsics[4], double derived[3]);
/* constructRemaps(model) (undistorter.hpp:69-90): the undistorter of the model, in size = out size = (width, height) as in the
 * reference.  One launch evaluates every pixel and writes the folded table; nothing but the kernel's arguments goes to the device.
 * map_x_out / map_y_out (height x width floats each, row-major; both or neither) receive the two CV_32F tables when given, else
 * nothing comes back; pinhole_intrinsics_out (may be NULL) as above.  Blocking.  The handle is the one dsopp_hip_undistorter_create
 * returns and every consumer takes it unchanged.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: an unknown type, a non-finite parameter or coefficient, a focal length <= 0, a principal point
 * coordinate beyond 2^20 in magnitude (the bound on a map entry), fov outside (0, pi), num_k wrong for the type or above 16, width or
 * height < 2, more than INT_MAX pixels, a NULL model or out, only one of the two map outputs. */
int dsopp_hip_undistorter_create_from_model(int device, void *stream, const dsopp_hip_camera_model *model, float *map_x_out, float *map_y_out,
                                            double pinhole_intrinsics_out[4], dsopp_hip_undistorter **out);

/* ------------------------------------------------------------------------------------------------------------------
 * Image transformers: the resize and the crop behind the undistortion (replaces CameraResizer — src/sensors/camera_transformers/src/
 * camera_resizer.cpp:7-20 — and ImageCropper — src/sensors/camera_transformers/src/image_cropper.cpp:7-18 —, the list that
 * src/sensors/camera_transformers/src/fabric.cpp:12-31 builds for every camera: a resizer when the YAML has a `resize_transformer`,
 * then always the cropper.  src/sensors/camera/src/camera.cpp:57-70 runs it on every frame and every class image,
 * src/sensors/sensors_builder/src/camera_fabric.cpp:157-167 once on the calibration, the static mask and the vignette)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_transformer dsopp_hip_transformer;
/* resize_ratio: CameraResizer's new_to_old_size_ratio (1.0 = no resizer configured); crop_levels: the ImageCropper's shift (the
 * reference: kNumberOfPyramidLevels = 4; 0 = no crop).  Sizes, per axis (camera_resizer.cpp:9-10, camera_image_crop.hpp:16-20):
 *   resized = (int)((double)in * resize_ratio), truncated;  out = (resized >> crop_levels) << crop_levels.
 * The arithmetic of every later transform is integer and fixed here, for a single-channel 8-bit image.
 * Linear (the camera image and the vignette; cv::resize INTER_LINEAR, camera_resizer.cpp:12), per axis n_in -> n_resized:
 *   scale = 1.0 / ((double)n_resized / n_in);  for the output index d:  f = (float)((d + 0.5) * scale - 0.5), s = floor(f), f -= s
 *   in float;  s < 0: s = 0, f = 0;  s >= n_in - 1: s = n_in - 1, f = 0 (the second tap then has weight 0 and is not read outside
 *   the image);  weights w1 = rint(f * 2048.0f), w0 = rint((1.0f - f) * 2048.0f), both half to even.
 *   With (sx, a0, a1) of column x and (sy, b0, b1) of row y:  r(v) = a0 * S[v, sx] + a1 * S[v, sx + 1],
 *   out[y, x] = (((b0 * (r(sy) >> 4)) >> 16) + ((b1 * (r(sy + 1) >> 4)) >> 16) + 2) >> 2, always within 0 .. 255.
 *   So ratio 1 is the identity and ratio 0.5 of an even size is (a + b + c + d + 2) >> 2 of every 2 x 2 block.
 * Nearest (the static mask and the class image; INTER_NEAREST, camera_resizer.cpp:16): s = min(floor(d * scale), n_in - 1), out = S[sy, sx].
 * The crop keeps rows [0, out_h) and columns [0, out_w) of the resized image (image_cropper.cpp:12); only those are computed.
 * Both axes are folded into device tables of out_w + out_h entries before the call returns.  With nothing to do (resized == out ==
 * in) no kernel is ever launched.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: a ratio that is not finite or not positive, in_w or in_h < 1, crop_levels outside 0 .. 8, an
 * output axis of 0 pixels, an input or resized image of more than INT_MAX pixels. */
int dsopp_hip_transformer_create(int device, void *stream, int in_w, int in_h, double resize_ratio, int crop_levels, dsopp_hip_transformer **out);
void dsopp_hip_transformer_destroy(dsopp_hip_transformer *t);
/* the three sizes above; any pointer may be NULL */
int dsopp_hip_transformer_sizes(const dsopp_hip_transformer *t, int *in_w, int *in_h, int *resized_w, int *resized_h, int *out_w, int *out_h);
/* transformCalibration of every transformer (camera_fabric.cpp:157-159) on a pinhole calibration; needs no device.
 * CameraCalibration::resize (src/sensors/camera_calibration/src/camera_calibration.cpp:33-42): image_size = in * ratio, NOT truncated,
 * and all four intrinsics (fx, fy, cx, cy) times the ratio — the reference shifts cx, cy by no half pixel, and neither does this.
 * CameraCalibration::crop (:44-46): image_size = ((size_t)image_size >> crop_levels) << crop_levels; the origin stays at the top-left
 * pixel, so the intrinsics do not change.  out_w / out_h are the transformer's output size.  (simple_radial scales only its first three
 * intrinsics, :37-38: not built.)  Any output pointer may be NULL; intrinsics_out is written only with intrinsics_in.  The argument
 * errors of dsopp_hip_transformer_create. */
int dsopp_hip_transform_calibration(int in_w, int in_h, double resize_ratio, int crop_levels, const double intrinsics_in[4], double image_size_out[2],
                                    double intrinsics_out[4], int *out_w, int *out_h);
/* runImageTransformers (linear) and runMaskTransformers (nearest) of an in_h x in_w 8-bit image into out_h x out_w bytes, blocking:
 * the once-per-camera forms for the vignette and the static mask (camera_fabric.cpp:164-167), behind dsopp_hip_undistorter_undistort */
int dsopp_hip_transformer_transform_image(dsopp_hip_transformer *t, const uint8_t *image_host, uint8_t *out_host);
int dsopp_hip_transformer_transform_mask(dsopp_hip_transformer *t, const uint8_t *mask_host, uint8_t *out_host);
/* same, both images in HBM: the call only enqueues on `stream` (a hipStream_t; NULL = the transformer's own) one launch, or one copy
 * when there is nothing to do.  interpolation: 0 = linear, 1 = nearest.  Both pointers must be 4-byte aligned, else
 * DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_transformer_transform_device(dsopp_hip_transformer *t, const void *in_dev, void *out_dev, int interpolation, void *stream);
/* The per-frame path, camera.cpp:70 followed by the PixelDataFrame ctor: dsopp_hip_pyramid_build of
 * runImageTransformers(undistort(frame_host)).  u = NULL: frames arrive undistorted (t's input size), else u's input size.  The frame
 * goes through the pyramid's pinned buffer as in build_undistorted; on the pyramid's stream follow the remap (with u), the transformer's
 * launch (unless it has nothing to do) and the level build; the call does not wait for them.  The pyramid keeps the transformed 8-bit
 * image, the one the reference extracts features from: dsopp_hip_feature_extractor_extract_from_pyramid reads it as it reads
 * build_undistorted's.  vignetting_host is the vignette already undistorted and transformed (camera_fabric.cpp:167).  f64 and f32
 * pyramids.  DSOPP_HIP_ERR_INVALID_ARGUMENT unless all three live on one device, u writes t's input size and t writes the pyramid's. */
int dsopp_hip_pyramid_build_transformed(dsopp_hip_pyramid *p, const dsopp_hip_undistorter *u, const dsopp_hip_transformer *t, const uint8_t *frame_host,
                                        const double *lut256, const uint8_t *vignetting_host);

/* ------------------------------------------------------------------------------------------------------------------
 * Colour frames: the camera delivers 8-bit BGR (the image provider is created with read_grayscale = false —
 * src/sensors/sensors_builder/src/camera_fabric.cpp:35 — so cv::imread and cv::VideoCapture::read hand over CV_8UC3), the frame is
 * undistorted and transformed in colour (src/sensors/camera/src/camera.cpp:70) and converted to grey last, by the CameraFeatures ctor
 * (cv::cvtColor(raw_image_, frame_data_, cv::COLOR_BGR2GRAY), src/features/src/camera_features.cpp:32); the colour image stays with the
 * frame (CameraFeatures::image(), camera_features.cpp:49; src/tracker/tracker/src/monocular_tracker.cpp:63,460,493).
 * An image here is a continuous CV_8UC3 Mat: 3 * w * h bytes, interleaved, channel c (0 = B, 1 = G, 2 = R) of pixel o at byte 3 * o + c.
 * The arithmetic is integer and fixed here:
 *   remap and resize + crop are the single-channel statements of dsopp_hip_undistorter_create and dsopp_hip_transformer_create (linear)
 *   applied to B, G and R on their own — coordinates, reflection and weights are shared between the channels, as cv::remap and cv::resize
 *   share them for CV_8UC3 — each rounded to 8 bits as stated there; the handles' device tables are used as they are;
 *   grey = (3735 * B + 19235 * G + 9798 * R + 16384) >> 15 of the 8-bit result of the last stage (the 15-bit fixed point of OpenCV 4's
 *   8-bit BGR2GRAY; the weights sum to 32768, so (v, v, v) -> v, and pure blue, green and red give 29, 150 and 76).  It is within 0.505
 *   of 0.114 B + 0.587 G + 0.299 R.  The 14-bit form of OpenCV 3 (1868, 9617, 4899) is not built.
 * Converting last is not converting first: after a resize about a quarter of the grey bytes differ by one level between the two orders.
 * Not built: RGB, BGRA and planar layouts, 16-bit images, dsopp_hip_pyramid_group_* forms.  The class image, the static mask and the
 * vignette are single-channel in the reference and stay on the entry points above.
 * ---------------------------------------------------------------------------------------------------------------- */
/* Undistorter::undistort of a CV_8UC3 frame (undistorter.cpp:7-18 as camera.cpp:70 calls it), both images in HBM: the call only
 * enqueues one launch on `stream` (a hipStream_t; NULL = the undistorter's own).  bgr_out_dev (3 * out_w * out_h bytes) takes the
 * remapped colour image, grey_out_dev (out_w * out_h bytes) its grey conversion (camera_features.cpp:32); either may be NULL, both NULL
 * or a NULL input is DSOPP_HIP_ERR_INVALID_ARGUMENT, and so is an output that is not 4-byte aligned.  The input may have any alignment. */
int dsopp_hip_undistorter_undistort_bgr_device(dsopp_hip_undistorter *u, const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream);
/* runImageTransformers of a CV_8UC3 frame (camera.cpp:70; camera_resizer.cpp:12, image_cropper.cpp:12), linear interpolation only, with
 * the same conventions.  A transformer with nothing to do enqueues the plain conversion for grey_out_dev and one copy for bgr_out_dev
 * (none when it is the input). */
int dsopp_hip_transformer_transform_bgr_device(dsopp_hip_transformer *t, const void *bgr_in_dev, void *bgr_out_dev, void *grey_out_dev, void *stream);
/* The per-frame path for a colour camera, camera.cpp:70 followed by the CameraFeatures and PixelDataFrame ctors
 * (camera_features.cpp:19-47): dsopp_hip_pyramid_build of BGR2GRAY(runImageTransformers(undistort(bgr_host))).  u and t may each be
 * NULL (frames arrive undistorted / there is no transformer list); the frame has u's input size, else t's, else the pyramid's.  The
 * 3 * w * h bytes go through the pyramid's pinned buffer in pieces as in build; on the pyramid's stream follow at most two launches —
 * with u and a t that has work the remap BGR -> BGR and the resize + crop BGR -> grey; with one of them that stage BGR -> grey; with
 * neither the plain conversion — and the level build.  The conversion is the last stage's epilogue, never a pass of its own behind a
 * stage.  The call does not wait, unless lut256 or vignetting_host is given (they are read straight from the caller's arrays, as in
 * build_transformed; vignetting_host is the single-channel vignette already undistorted and transformed).  The pyramid keeps the grey
 * image as build_transformed keeps its image (dsopp_hip_feature_extractor_extract_from_pyramid and _set_mask_from_pyramid work
 * unchanged) and, with keep_colour != 0, the transformed colour image too (without a stage that is the uploaded frame itself: no
 * copy).  f64 and f32 pyramids.  DSOPP_HIP_ERR_INVALID_ARGUMENT: a NULL frame, handles on different devices, u not writing t's input
 * size, the last stage not writing the pyramid's size. */
int dsopp_hip_pyramid_build_colour(dsopp_hip_pyramid *p, const dsopp_hip_undistorter *u, const dsopp_hip_transformer *t, const uint8_t *bgr_host,
                                   const double *lut256, const uint8_t *vignetting_host, int keep_colour);
/* The 8-bit image the pyramid keeps, blocking.  channels = 1: the grey image the levels were built from (CameraFeatures::frameData(),
 * camera_features.cpp:51), width * height bytes, kept by build_undistorted, build_transformed and build_colour.  channels = 3: the
 * colour image (CameraFeatures::image(), camera_features.cpp:49), 3 * width * height bytes, kept by build_colour with keep_colour.
 * *present = 0 and out_host untouched when the pyramid keeps no such image: after build, build_device, set_level — every other
 * rewrite of the image drops both — and channels = 3 after any build but a build_colour with keep_colour.  Other values of channels
 * are DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_pyramid_get_image(dsopp_hip_pyramid *p, int channels, uint8_t *out_host, int *present);

/* ------------------------------------------------------------------------------------------------------------------
 * Optical flow of the bootstrap: pyramidal Lucas-Kanade tracking of the first frame's features into every new frame (replaces the
 * cv::calcOpticalFlowPyrLK(image_from, image_to, pts_from, pts_to, status, err, Size(15, 15), 3, TermCriteria(COUNT + EPS, 10, 0.01))
 * of features::OpticalFlowMatch — src/feature_based_slam/features/src/optical_flow.cpp:11-42 — which MonocularInitializer::tick —
 * src/feature_based_slam/tracker/src/monocular_initializer.cpp:36-102 — runs on every frame until the sequence is initialised)
 * The refill of lost features from a fresh ORB detection (optical_flow.cpp:44-53) is dsopp_hip_orb_detector_* below, and
 * estimateSO3inlierCount dsopp_hip_rotation_ransac_*, estimateSE3PnP dsopp_hip_pnp_ransac_*, and the refinement behind them dsopp_hip_geometric_ba_*.  estimateSO3xS2 and the two-view triangulation of initializePoses dsopp_hip_two_view_ransac_*.  Not built: a dsopp_hip_pyramid_group_* form, OPTFLOW_USE_INITIAL_FLOW, OPTFLOW_LK_GET_MIN_EIGENVALS, multi-channel images.
 *
 * The arithmetic is fixed here, a restatement of OpenCV 4's calcOpticalFlowPyrLK (the scalar path of lkpyramid.cpp) for 8-bit
 * single-channel images; tests/optical_flow_model.py is its NumPy form and the device is held to it bit for bit.  OpenCV sums the window
 * in float in raster order (its SIMD paths in other orders); the exact integer sums below are the order-free statement of those, so
 * parity with OpenCV itself is not pinned.  win = the window side, half = (win - 1) * 0.5f, reflect = BORDER_REFLECT_101,
 * DESCALE(x, n) = (x + (1 << (n - 1))) >> n (arithmetic), rn = round to nearest, ties to even; every float step is one IEEE binary32
 * operation in the written order, never fused; division and square root are correctly rounded.
 *   Levels: level 0 is the image; level l + 1 is ((w + 1) / 2) x ((h + 1) / 2), pyrDown of level l: r = s[2x-2] + s[2x+2] +
 *     4 (s[2x-1] + s[2x+1]) + 6 s[2x] along rows, the same taps over rows 2y-2 .. 2y+2 of r, (sum + 128) >> 8, source indices reflected.
 *     After level l the size is halved; a halved width or height <= win makes l the last level, and there are at most max_level + 1.
 *   Scharr planes of the reference's levels, int16 pairs: t0 = (s[y-1][x] + s[y+1][x]) * 3 + s[y][x] * 10, t1 = s[y+1][x] - s[y-1][x],
 *     dx = t0[x+1] - t0[x-1], dy = (t1[x+1] + t1[x-1]) * 3 + t1[x] * 10, neighbours reflected.
 *   Window sample at integer origin (ix, iy) and f32 fractions (a, b): iw00 = rn((1-a)(1-b) * 16384), iw01 = rn(a (1-b) * 16384),
 *     iw10 = rn((1-a) b * 16384), iw11 = 16384 - iw00 - iw01 - iw10; v = p[y][x] iw00 + p[y][x+1] iw01 + p[y+1][x] iw10 + p[y+1][x+1] iw11
 *     for 0 <= x, y < win at (ix + x, iy + y); an image plane is read through reflect, a derivative plane reads 0 outside the level;
 *     an intensity is DESCALE(v, 9) (5 fraction bits), a derivative DESCALE(v, 14).
 *   Per point, from the top level down to 0, status = 1, err = 0, S = 2^-20:
 *     1. prev = pt * 2^-level; next = prev at the top level, else 2 * the result of the level above; the result is next.
 *     2. prev -= half, ip = floor(prev).  Range test: ip.x < -win || ip.x >= W_l || ip.y < -win || ip.y >= H_l: at level 0 status = 0,
 *        err = 0; at any level go on with the next level.
 *     3. I, Ix, Iy over the window at ip; A11, A12, A22 = (float)(the exact sum of Ix Ix, Ix Iy, Iy Iy) * S.
 *     4. D = A11 A22 - A12 A12, minEig = (A22 + A11 - sqrt((A11 - A22)(A11 - A22) + 4 A12 A12)) / (float)(2 win win).
 *        (double)minEig < min_eig_threshold || D < FLT_EPSILON: at level 0 status = 0; at any level go on with the next level.  D = 1 / D.
 *     5. next -= half, prevDelta = 0; for j < max_iterations: in = floor(next); the range test on `in` (at level 0 status = 0) ends the
 *        loop; diff = DESCALE(J sample at in, 9) - I; b1, b2 = (float)(the exact sum of diff Ix, diff Iy) * S;
 *        delta = ((A12 b2 - A22 b1) D, (A12 b1 - A11 b2) D); next += delta; result = next + half;
 *        (double)dx dx + (double)dy dy <= epsilon^2 (in double) ends the loop; so does, for j > 0, fabs(delta + prevDelta) < 0.01 on both
 *        axes (the sums in float), after result -= delta * 0.5f; prevDelta = delta.
 *     6. at level 0 with status 1: q = result - half; the range test on floor(q) gives status = 0, else
 *        err = (float)(the exact sum of |DESCALE(J sample at q, 9) - I|) / (float)(32 win win).
 *   A coordinate that is not finite fails the range test.  max_iterations is clamped to 0 .. 100 and epsilon to 0 .. 10, as OpenCV does.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_flow_tracker dsopp_hip_flow_tracker;
/* The tracker of one image size.  The reference's values (optical_flow.cpp:19-22 and OpenCV's default minEigThreshold): window 15,
 * max_level 3, max_iterations 10, epsilon 0.01, min_eig_threshold 1e-4.  `stream` is a hipStream_t (NULL = a stream of its own); all
 * work of the object runs on it.  DSOPP_HIP_ERR_INVALID_ARGUMENT: an even window or one outside 3 .. 15, width or height < 2, max_level
 * outside 0 .. 5, a threshold that is not a number. */
int dsopp_hip_flow_tracker_create(int width, int height, int window, int max_level, int max_iterations, double epsilon, double min_eig_threshold,
                                  int device, void *stream, dsopp_hip_flow_tracker **out);
void dsopp_hip_flow_tracker_destroy(dsopp_hip_flow_tracker *t);
/* the number of levels the stop rule above leaves for this size (buildOpticalFlowPyramid) */
int dsopp_hip_flow_tracker_num_levels(const dsopp_hip_flow_tracker *t, int *n);
/* image_from (optical_flow.cpp:30; the first track frame, monocular_initializer.cpp:47-51): its levels and Scharr planes are built once
 * and kept, so every later frame costs one pyramid and one tracking launch.  `stride` = bytes between rows, >= width.  The host image
 * is copied before the call returns, which only enqueues. */
int dsopp_hip_flow_tracker_set_reference(dsopp_hip_flow_tracker *t, const uint8_t *image_host, size_t stride);
/* same, the image already in HBM (any alignment): it is read on the tracker's stream, and has been read when the call returns */
int dsopp_hip_flow_tracker_set_reference_device(dsopp_hip_flow_tracker *t, const void *image_dev, size_t stride);
/* same, the 8-bit grey image `pyramid` keeps (CameraFeatures::frameData(), the image dsopp_hip_pyramid_get_image(p, 1, ...) returns),
 * read behind the pyramid's build with no host copy.  DSOPP_HIP_ERR_STATE when the pyramid keeps none, DSOPP_HIP_ERR_INVALID_ARGUMENT
 * when its size or device is not the tracker's. */
int dsopp_hip_flow_tracker_set_reference_from_pyramid(dsopp_hip_flow_tracker *t, const dsopp_hip_pyramid *pyramid);
/* calcOpticalFlowPyrLK(reference, image, points_from, ...) (optical_flow.cpp:30-31), blocking: points_from / points_to are n x 2 floats
 * (x, y), status n bytes (1 = tracked), err n floats, iterations n x num_levels int32 or NULL — the passes of step 5 per level, there
 * so that a divergence from the stated arithmetic can be located.  The results come back through one pinned buffer with one wait.
 * n = 0 builds the target's levels only.  DSOPP_HIP_ERR_STATE before a reference was set. */
int dsopp_hip_flow_tracker_track(dsopp_hip_flow_tracker *t, const uint8_t *image_host, size_t stride, int n, const float *points_from, float *points_to,
                                 uint8_t *status, float *err, int32_t *iterations);
/* same, the image in HBM / the grey image a pyramid keeps, with the conventions and errors of the set_reference twins */
int dsopp_hip_flow_tracker_track_device(dsopp_hip_flow_tracker *t, const void *image_dev, size_t stride, int n, const float *points_from, float *points_to,
                                        uint8_t *status, float *err, int32_t *iterations);
int dsopp_hip_flow_tracker_track_from_pyramid(dsopp_hip_flow_tracker *t, const dsopp_hip_pyramid *pyramid, int n, const float *points_from,
                                              float *points_to, uint8_t *status, float *err, int32_t *iterations);
/* For tests, blocking: level `level` of the reference (which = 0) or of the last tracked frame (which = 1) as w_l x h_l dense bytes,
 * and of the reference its Scharr plane as w_l x h_l (dx, dy) int16 pairs.  Either pointer may be NULL; deriv_out with which = 1 is
 * DSOPP_HIP_ERR_INVALID_ARGUMENT; DSOPP_HIP_ERR_STATE when that image was never set. */
int dsopp_hip_flow_tracker_get_level(dsopp_hip_flow_tracker *t, int which, int level, uint8_t *image_out, int16_t *deriv_out);

/* ------------------------------------------------------------------------------------------------------------------
 * ORB keypoints of the bootstrap: the detection that gives the first frame its features and refills, on every later frame, the
 * features the flow lost (replaces the cv::ORB::create(nfeatures, 2.0f, 5)->detect of DistinctFeaturesExtractorORB —
 * src/feature_based_slam/features/src/distinct_features_extractor_orb.cpp:11-38 —, which features::OpticalFlowMatch —
 * src/feature_based_slam/features/src/optical_flow.cpp:44-53 — and the first frame — correspondences_finder.cpp:12-15 — run;
 * MonocularInitializer::tick — monocular_initializer.cpp:47-53 — and the feature-based tracker — add_new_frame.cpp:31 — go through
 * them on every frame; ORB is the one extractor the factory knows, feature_based_slam/tracker/src/fabric.cpp:97-102)
 * Only keypoint.pt is used by the reference, so only positions (with level and response) are computed.  Not built: descriptors and
 * angles, scale factors other than 2, FAST_SCORE, a dsopp_hip_pyramid_group_* form, the ORB brute-force matcher (features/src/orb.cpp).
 *
 * The arithmetic is fixed here, a restatement of OpenCV 4's orb.cpp, fast.cpp and keypoint.cpp; tests/orb_model.py is its NumPy form
 * and the device is held to it bit for bit.  Parity with OpenCV itself is not pinned.  All integers are exact; every float step is one
 * IEEE binary32 operation in the written order, never fused; cvRound rounds to nearest, ties to even.  e = edge_threshold, t =
 * fast_threshold.
 *   1. Features per level: factor = 0.5f; nd = nfeatures * (1 - factor) / (1 - (float)pow((double)factor, (double)nlevels)) in float;
 *      for l < nlevels - 1: n_l = cvRound(nd), nd *= factor; n_last = max(nfeatures - sum n_l, 0).  (500 over 5: 258, 129, 65, 32, 16.)
 *   2. Levels: level 0 is the image; level l is cvRound(W / 2^l) x cvRound(H / 2^l), the linear resize of level l - 1 in the arithmetic
 *      of dsopp_hip_transformer_create (cv::resize INTER_LINEAR, 11-bit weights); at a ratio of exactly 2 that is (a + b + c + d + 2) >> 2.
 *      Deviation: OpenCV resizes these levels with INTER_LINEAR_EXACT; the two agree where every halving is exact (every shipped
 *      configuration: ImageCropper leaves multiples of 2^4) and may differ by a grey level elsewhere.
 *   3. Masks: level 0 is the mask bytes; level l the same resize of level l - 1's bytes followed by m > 254 ? m : 0
 *      (threshold(254, THRESH_TOZERO)).  A point is masked where the byte at its pixel is 0.
 *   4. FAST-9/16 per level, centres 3 <= x < w - 3, 3 <= y < h - 3, ring (0,3) (1,3) (2,2) (3,1) (3,0) (3,-1) (2,-2) (1,-3) (0,-3)
 *      (-1,-3) (-2,-2) (-3,-1) (-3,0) (-3,1) (-2,2) (-1,3): m = the maximum, over the 16 circular arcs of 9 ring pixels and both signs
 *      s, of the arc's minimum of s (p_k - v).  A corner iff m > t, its score m - 1; every other pixel scores 0.
 *   5. Non-maximum suppression: a corner survives iff its score is strictly greater than the scores of its 8 neighbours (masked
 *      corners take part).
 *   6. Filters: survivors on a masked pixel are dropped, and so are those outside e <= x < w - e, e <= y < h - e (a level with
 *      w <= 2 e or h <= 2 e keeps nothing).
 *   7. First cut, retainBest(2 n_l): when more than 2 n_l remain, n_l = 0 keeps none, else every point whose score is >= the
 *      2 n_l-th largest score stays (ties at the boundary all stay).
 *   8. Harris response at (x, y) of the level image p, over the 7 x 7 block centred there:
 *      Ix = 2 (p[y][x+1] - p[y][x-1]) + (p[y-1][x+1] - p[y-1][x-1]) + (p[y+1][x+1] - p[y+1][x-1]), Iy its transpose;
 *      a = sum Ix^2, b = sum Iy^2, c = sum Ix Iy in int32; scale = 1.f / (4 * 7 * 255.f), s4 = scale * scale * scale * scale (left to
 *      right); r = (((float)a (float)b - (float)c (float)c) - (0.04f ((float)a + (float)b)) ((float)a + (float)b)) s4.
 *   9. Second cut, retainBest(n_l) on r by the rule of 7 (float ties all stay; -0 equals +0).
 *  10. Output (x 2^l, y 2^l) as floats with l and r, in the canonical order: levels ascending, within a level ascending y, then x.
 *      Deviation: the reference's order is what std::nth_element and std::partition leave inside retainBest; the set is the same, the
 *      random subset a refill draws from it is not.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_orb_detector dsopp_hip_orb_detector;
/* step 1 (orb.cpp's computeKeyPoints; distinct_features_extractor_orb.cpp:13), out = nlevels int32: host arithmetic, the one entry
 * point of this section that needs no device.  DSOPP_HIP_ERR_INVALID_ARGUMENT: nfeatures < 0, nlevels outside 1 .. 8. */
int dsopp_hip_orb_features_per_level(int nfeatures, int nlevels, int32_t *out);
/* The detector of one image size (DistinctFeaturesExtractorORB's constructor, distinct_features_extractor_orb.cpp:11-14).  The
 * reference's values: nfeatures 500 (YAML number_of_features, fabric.cpp:97-102), nlevels 5, edge_threshold 31, fast_threshold 20.
 * `stream` is a hipStream_t (NULL = a stream of its own); all work of the object runs on it.  Its internal lists hold ceil(w / 2) *
 * ceil(h / 2) survivors per level, the most step 5 can leave: no input overflows them.  DSOPP_HIP_ERR_INVALID_ARGUMENT: nlevels
 * outside 1 .. 8, edge_threshold < 4 (the Harris block must stay inside the level), fast_threshold outside 0 .. 255, nfeatures < 0,
 * width or height outside 1 .. 65535, a size whose last level would be empty. */
int dsopp_hip_orb_detector_create(int width, int height, int nfeatures, int nlevels, int edge_threshold, int fast_threshold, int device, void *stream,
                                  dsopp_hip_orb_detector **out);
void dsopp_hip_orb_detector_destroy(dsopp_hip_orb_detector *d);
/* The mask of every later detect (the `mask` of extract(), distinct_features_extractor_orb.cpp:16-24): width x height bytes, dense,
 * copied before the call returns, which only enqueues the mask levels of step 3.  NULL = no mask. */
int dsopp_hip_orb_detector_set_mask(dsopp_hip_orb_detector *d, const uint8_t *mask_host);
/* The same from the level-0 mask `pyramid` kept from its last dsopp_hip_pyramid_set_semantics, taken as validity: a non-zero byte is
 * 255.  A mask byte of 1 .. 254 is valid at level 0 and, by the threshold of step 3, masks every pixel of the levels above that it
 * touches; a caller whose mask holds such bytes and wants that hands the bytes over with set_mask.  Only enqueues, behind the
 * pyramid's ready event.  DSOPP_HIP_ERR_INVALID_ARGUMENT when the pyramid never had set_semantics, or its size or device is not the
 * detector's. */
int dsopp_hip_orb_detector_set_mask_from_pyramid(dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *pyramid);
/* detect (distinct_features_extractor_orb.cpp:16-38; optical_flow.cpp:44-46; correspondences_finder.cpp:12-15), blocking: *n
 * detections in the canonical order, xy n x 2 floats, level n int32, response n floats.  `stride` = bytes between rows, >= width.  The
 * results come back through one pinned block with one wait (a second only when boundary ties keep more than nfeatures + 256).  More
 * detections than `capacity`: DSOPP_HIP_ERR_CAPACITY, *n = the count needed, nothing else written. */
int dsopp_hip_orb_detector_detect(dsopp_hip_orb_detector *d, const uint8_t *image_host, size_t stride, int32_t capacity, float *xy, int32_t *level,
                                  float *response, int32_t *n);
/* same, the image in HBM (any alignment) / the grey image a pyramid keeps, with the conventions and errors of
 * dsopp_hip_flow_tracker_set_reference_device and _from_pyramid */
int dsopp_hip_orb_detector_detect_device(dsopp_hip_orb_detector *d, const void *image_dev, size_t stride, int32_t capacity, float *xy, int32_t *level,
                                         float *response, int32_t *n);
int dsopp_hip_orb_detector_detect_from_pyramid(dsopp_hip_orb_detector *d, const dsopp_hip_pyramid *pyramid, int32_t capacity, float *xy,
                                               int32_t *level, float *response, int32_t *n);
/* For tests, blocking: of level `level` the image and the FAST score plane (step 4, before the suppression) of the last detect, and
 * the mask bytes (all 255 without a mask), each w_l x h_l dense bytes; any pointer may be NULL, *w and *h take the level's size.
 * DSOPP_HIP_ERR_STATE for an image or score plane before the first detect. */
int dsopp_hip_orb_detector_get_level(dsopp_hip_orb_detector *d, int level, uint8_t *image_out, uint8_t *mask_out, uint8_t *score_out, int *w, int *h);

/* ------------------------------------------------------------------------------------------------------------------
 * The bootstrap's standstill test: the pure-rotation RANSAC over the matches of two frames (replaces estimateSO3inlierCount<3> —
 * src/feature_based_slam/tracker/src/estimate_so3_inlier_count.cpp:17-48 —, that is ransac::ransac — src/ransac/include/ransac/ransac.hpp:27-56 —
 * over the three-point PureRorationSolver — src/energy/n_point_solvers/src/pure_rotation_estimator.cpp:14-67 —, which
 * MonocularInitializer::tick — monocular_initializer.cpp:71-94 — and the feature-based tracker — add_new_frame.cpp:36-45 — run on every
 * frame).  Not built: ORB descriptors and matching, the SimpleRadialCamera instantiation
 * (triangulation and the refinement are dsopp_hip_geometric_ba_* below, the PnP RANSAC dsopp_hip_pnp_ransac_* below them, the
 * essential-matrix RANSAC dsopp_hip_two_view_ransac_* below those).
 *
 * The arithmetic is fixed here; tests/rotation_ransac_model.py is its NumPy form.  Everything is binary64 (the reference's Precision);
 * float points of the flow tracker are widened by the caller.
 *   Inputs: a pinhole camera fx, fy, cx, cy, width, height; n pairs A[j], B[j] (x, y); `iterations` sample triples S[i] = (s0, s1, s2) of
 *     distinct indices < n, drawn by the caller; threshold in pixels (the reference's default 1.5); inliers_tolerance (0.95).
 *   Roles: the reference calls ransac(solver, target_points, reference_points, ...): A is the NEW frame's points, B the last bootstrap
 *     keyframe's, and the returned rotation maps bearings of A onto bearings of B.  The reference stores it under the name rotation_t_r
 *     all the same; it is kept that way here.
 *   roi(p) = 4 <= x <= width - 5 && 4 <= y <= height - 5 (camera_model_base.hpp:53-60); unproject(p) = ((x - cx) / fx, (y - cy) / fy, 1).
 *   Hypothesis i (solve): invalid when any of its six sample points fails roi.  Otherwise a_k, b_k = the normalised bearings of
 *     A[S[i][k]], B[S[i][k]]; H = sum_k a_k b_k^T / 9 (the reference divides by Matrix::size()); H = U S V^T; Q = V U^T;
 *     R_i = det(Q) Q — the whole matrix flips, this is not Kabsch's diag(1, 1, d).  For a non-singular H, Q is the orthogonal polar
 *     factor of H^T; any backward-stable route to it serves (the device: a one-sided Jacobi SVD).  With a vanishing smallest singular
 *     value the result depends on the decomposition and is not pinned, but it is a rotation.
 *   Score of R (findBest): point j is an inlier iff roi(A[j]) and, with (x, y, z) = R unproject(A[j]) and
 *     q = (fx x / z + cx, fy y / z + cy), sqrt(|q - B[j]|^2) < threshold (strict; a NaN is no inlier).  No depth test, no roi test on q
 *     or on B[j].  One deviation: for a point that fails roi(A[j]) the reference reads an uninitialised vector; here it is never an inlier.
 *   An invalid hypothesis carries the rotation and the count of its nearest valid predecessor (the reference ignores solve's return value
 *     and scores the solver's previous solution), and the identity and its count when no valid one precedes it.
 *   Selection, the serial loop's meaning: walk i = 0, 1, ...; stop before i when (double)best / (double)n >= inliers_tolerance;
 *     hypothesis i replaces the best iff its count is strictly greater.  best_iteration is -1 when no count exceeded 0: the rotation is
 *     then the identity and there are no inliers, as with the reference's default-constructed Solution.
 *   n = 0 runs no iteration (0 / 0 < 0.95 is false).  For n = 1, 2 the reference's sampler never returns: DSOPP_HIP_ERR_INVALID_ARGUMENT
 *     when iterations > 0.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_rotation_ransac dsopp_hip_rotation_ransac;
typedef struct dsopp_hip_rotation_ransac_result {
  int32_t iterations_run; /* hypotheses examined before the tolerance stopped the walk */
  int32_t best_iteration; /* the winning hypothesis, -1 when no count exceeded 0 */
  int32_t inlier_count;
  int32_t matches;        /* n, the reference's matching number */
  double rotation[9];     /* the winner's R, row-major */
} dsopp_hip_rotation_ransac_result;
/* `stream` is a hipStream_t (NULL = a stream of its own); all work of the object runs on it.  Its buffers grow with n and iterations. */
int dsopp_hip_rotation_ransac_create(int device, void *stream, dsopp_hip_rotation_ransac **out);
void dsopp_hip_rotation_ransac_destroy(dsopp_hip_rotation_ransac *r);
/* One launch and one wait, blocking.  points_a / points_b: n x 2 doubles; samples: iterations x 3 int32; inlier_indices: room for n int32,
 * the first result->inlier_count of which are written, ascending.  Optional (NULL) per-hypothesis outputs, there so that a divergence
 * from the stated arithmetic can be located: hyp_counts (iterations int32), hyp_rotations (iterations x 9 doubles, row-major), hyp_valid
 * (iterations bytes); they cover every hypothesis, also those behind an early stop.  DSOPP_HIP_ERR_INVALID_ARGUMENT: n < 0,
 * iterations < 0, 0 < n < 3 with iterations > 0, a sample index outside 0 .. n - 1 or repeated within its triple, a threshold or
 * inliers_tolerance that is not a number, a NULL required argument. */
int dsopp_hip_rotation_ransac_estimate(dsopp_hip_rotation_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                       const double *points_a, const double *points_b, int iterations, const int32_t *samples, double threshold,
                                       double inliers_tolerance, dsopp_hip_rotation_ransac_result *result, int32_t *inlier_indices,
                                       int32_t *hyp_counts, double *hyp_rotations, uint8_t *hyp_valid);

/* ------------------------------------------------------------------------------------------------------------------
 * The bootstrap's geometric bundle adjustment: the reprojection-error refinement of the last frames' poses and of every landmark seen in
 * them, with the triangulation before it and the pruning after it (replaces, per bootstrap frame once the initialiser has succeeded —
 * src/feature_based_slam/tracker/src/monocular_tracker.cpp:54-68 —, triangulatePoints — triangulate_points.cpp:47-71, triangulation.hpp:52-64 —,
 * optimizeTransformations — refine_track.cpp:16-83, which runs Ceres SPARSE_SCHUR with a Huber loss through
 * ceres_geometric_bundle_adjustment_solver.cpp:33-108 — and removeOutliers — remove_outliers.cpp:15-47).  The OPTIMIZE_CAMERA form of
 * optimizeTransformations — the intrinsics as a third parameter block, PinholeCamera or SimpleRadialCamera, with
 * ParameterParameterization's fix_focal, fix_center, fix_model_specific, fix_poses and fix_landmarks — is the pair
 * dsopp_hip_geometric_ba_evaluate_camera / _solve_camera, stated under "The camera block" below.  Not built: triangulation and pruning
 * with a simple-radial camera (they need unproject), the autocalibration initialiser (estimateSE3PnP is dsopp_hip_pnp_ransac_* below;
 * the essential-matrix RANSAC and the two-view triangulatePoints that only initializePoses calls are dsopp_hip_two_view_ransac_* below it).
 *
 * The arithmetic is fixed here; tests/geometric_ba_model.py is its NumPy form.  Everything is binary64.
 *   Problem: a pinhole camera fx, fy, cx, cy, width, height; F frames, 2 <= F <= 16 (a 17th is DSOPP_HIP_ERR_CAPACITY; the reference uses
 *     at most 10), each with its t_agent_world (world to camera) as 12 doubles: R row-major, then t; L landmark positions X; M observations
 *     (frame, landmark, x, y), every (frame, landmark) pair at most once, listed grouped by landmark: landmark l owns observations
 *     landmark_offsets[l] .. landmark_offsets[l + 1] - 1.  The caller passes the participating frames only, in the reference's order:
 *     frame 0 is local_frames[0].
 *   Residual (bundle_adjustment_geometric_cost_functor.hpp:41-60, pinhole_camera.hpp:78-90): p = R_f X_l + t_f,
 *     q = (fx p_x / p_z + cx, fy p_y / p_z + cy); the observation is valid iff p_z >= 0.001 and roi(q), roi(q) = 4 <= q_x <= width - 5 &&
 *     4 <= q_y <= height - 5; r = obs - q when valid, else r = 0 with a zero Jacobian.
 *   Cost: s = |r|^2, rho(s) = s for s <= a^2 and 2 a sqrt(s) - a^2 otherwise (ceres::HuberLoss(a), a = reprojection_threshold = 1.5),
 *     cost = 1/2 sum rho(s) over the valid observations.  The linearisation is plain IRLS: w = rho'(s) = 1 or a / sqrt(s), blocks J^T w J
 *     and J^T w r.  Deviation: Ceres also applies its second-order corrector to outliers; that is not built.
 *   Degrees of freedom (ceres_geometric_bundle_adjustment_solver.cpp:41-53): frame 0 is fixed.  A frame f >= 2 has six, delta = (upsilon,
 *     omega), T <- T exp(delta) (a right increment, LocalParameterizationSE3), so dp = R (upsilon + omega x X): J_x = -G R with
 *     G = dq / dp, J_p = J_x [I | -hat(X)].  Frame 1 has five, (alpha, beta, omega): R <- R Exp(omega), and with n = |t_1| on entry and
 *     d = t_1 / |t_1|: t_1 <- n normalize(d + alpha b1 + beta b2), where k = the first axis with the smallest |d_k|, b1 = normalize(d x e_k),
 *     b2 = d x b1.  In the six components of a free frame that is upsilon = n R^T (alpha b1 + beta b2): the 6 x 5 basis B through which
 *     frame 1's blocks pass.  (Ceres spans the same plane with a Householder basis.)  |t_1| = 0 or a non-finite input is
 *     DSOPP_HIP_ERR_INVALID_ARGUMENT.  Every landmark has three.
 *   System: H = sum J^T w J, b = sum J^T w r, damped H + lambda diag(H) on pose and landmark blocks alike (for frame 1 the diagonal of
 *     B^T H_pp B), step (H + lambda D) delta = -b, solved through the Schur complement on the landmarks: with
 *     L_l L_l^T = H_ll + lambda diag(H_ll), the reduced system is B^T (H_pp - sum_l W_l (L_l L_l^T)^-1 W_l^T) B + lambda diag(B^T H_pp B),
 *     its right-hand side -B^T (b_p - sum_l W_l (L_l L_l^T)^-1 b_l), in the order (alpha, beta, omega) of frame 1, then (upsilon, omega) of
 *     frames 2, 3, ...; delta_l = -(L_l L_l^T)^-1 (b_l + sum_f W_lf^T delta_f).  A landmark whose 3 x 3 Cholesky meets a pivot that is <= 0
 *     or not finite (no valid observation, H_ll = 0, ...) takes no step and adds nothing to the reduced system.  A reduced system whose
 *     Cholesky meets such a pivot (a free frame without a valid observation, ...) gives no step: the iteration counts as rejected, with
 *     an infinite candidate cost in the trace.
 *   Control, the reference's own LM driver (levenberg_marquardt_algorithm.hpp:77-128), not Ceres's trust-region loop: lambda_0 = 1e-4 (the
 *     reciprocal of Ceres's default radius); E = the cost; the loop runs while iterations remain, nothing has converged and a residual is
 *     valid.  Per iteration: linearise unless the last step was rejected; solve; E' = the candidate's cost; no valid candidate residual
 *     ends the loop with the step rejected; |E - E'| / E < function_tolerance converges (accepted or not); E' < E accepts: step norm
 *     |delta_p|^2 + sum_l |delta_l|^2 (delta_p in the reduced coordinates) < parameter_tolerance * (state norm + parameter_tolerance)
 *     converges, with the state norm sum over the free frames (|t|^2 + 1) + sum_l |X_l|^2 of the state the step left; lambda /= 2;
 *     otherwise lambda *= 10 and the Jacobians are kept.  function_tolerance = parameter_tolerance = 1e-10 (the reference's solver
 *     options), max_iterations 50 (the driver's default).  Parity with Ceres's iteration path is unpinned: only the minimiser is shared.
 *   Triangulation: for every landmark without a position (all of them with retriangulation) and MORE than min_number_of_projections
 *     observations (the tracker passes 4): A = sum_i A_i^T A_i, A_i = P_i - v_i v_i^T P_i, P_i the 3 x 4 [R | t] of the observation's
 *     frame, v_i = normalize((x - cx) / fx, (y - cy) / fy, 1) (no roi test: the reference ignores unproject's result there); X = the
 *     eigenvector of A's smallest eigenvalue divided by its last entry.  Any backward-stable route serves (the device: cyclic Jacobi);
 *     the result is unpinned where the two smallest eigenvalues nearly coincide.
 *   Pruning: observation (f, l) is flagged iff it is not valid or sqrt(|obs - q|^2) > outlier_threshold (0.5, strict).
 *   The camera block (evaluate_camera, solve_camera; tests/geometric_ba_camera_model.py is its NumPy form).  The camera is the call's
 *     dsopp_hip_geometric_ba_camera; problem->fx .. cy are ignored, width and height bound the ROI as above.
 *     Pinhole, intrinsics (fx, fy, cx, cy): residual and validity as above; with u = p_x / p_z, v = p_y / p_z,
 *     dr/d(fx, fy, cx, cy) = -[[u, 0, 1, 0], [0, v, 0, 1]].
 *     Simple radial, intrinsics (f, cx, cy, k1, k2) (simple_radial.hpp:133-160, the projection without a Jacobian, which the cost functor
 *     calls): rho2 = u u + v v, d = (1 + k1 rho2) + (k2 rho2) rho2, q = f (d (u, v)) + (cx, cy); valid iff sqrt(rho2) <= max_valid_radius
 *     and roi(q).  There is no test on p_z (the reference has none): p_z = 0 gives a q that is not finite and fails roi.
 *     dq/df = d (u, v), dq/d(cx, cy) = I, dq/dk1 = (f rho2) (u, v), dq/dk2 = (f (rho2 rho2)) (u, v); G = dq / dp as simple_radial.hpp:190-199
 *     writes it: c = (2 k1 + 4 k2 rho2) / p_z / p_z, G_00 = f (p_x p_x c + d) / p_z, G_01 = G_10 = f p_x p_y c / p_z,
 *     G_11 = f (p_y p_y c + d) / p_z, G_i2 = f p_i / p_z / p_z (-3 k1 rho2 - 5 k2 rho2 rho2 - 1).  max_valid_radius is the constructor's
 *     constant (simple_radial.hpp:47-77, the routine stated with dsopp_hip_camera_model_to_pinhole above, dsopp_amd/csrc/
 *     simple_radial_radius.hpp) of the CURRENT intrinsics and the problem's width and height — Ceres rebuilds the model at every
 *     evaluation —; it enters the validity branch only, no derivative flows through it.
 *     Free intrinsics (constantParameterSet): pinhole focal = {fx, fy}, centre = {cx, cy}, FIX_MODEL_SPECIFIC ignored; simple radial
 *     focal = {f}, centre = {cx, cy}, model-specific = {k1, k2}.  The free ones, in parameter order, follow the pose unknowns in the
 *     reduced system: n = (pose unknowns) + Dc <= 94.  With FIX_POSES there are no pose unknowns (frame 1's basis and |t_1| are unused,
 *     |t_1| = 0 is allowed); the increment is additive, c <- c + delta_c.
 *     System: H_cc = sum w J_c^T J_c, b_c = sum w J_c^T r, H_pc = sum w J_p^T J_c per frame, W_lc = sum_o w J_x^T J_c over all of a
 *     landmark's observations; damping lambda diag(H_cc) like everywhere else.  The Schur complement takes the camera as one more block
 *     row and column: Y_c,l = L_l^-1 W_lc, S_fc = sum_l Y_f^T Y_c, S_cc = sum_l Y_c^T Y_c, the right-hand side alike;
 *     delta_l = -(L_l L_l^T)^-1 (b_l + sum_f W_lf^T delta_f + W_lc delta_c).  With FIX_LANDMARKS there is no elimination: the system is
 *     H + lambda D over poses and camera and delta_l = 0.  A pivot that is <= 0 or not finite — now also a camera diagonal that carries no
 *     information — fails the step as above.
 *     Candidate: the step also fails when the candidate camera has a focal length <= 0, an intrinsic that is not finite or, simple radial,
 *     a max_valid_radius that is not finite or <= 0 (the candidate poses and intrinsics are still handed out as computed).
 *     Control: the driver above; the step norm gains |delta_c|^2, the state norm sum c_i^2 over the free intrinsics; fixed poses and fixed
 *     landmarks contribute to neither norm.
 *     Pinning: a pinhole with FIX_FOCAL | FIX_CENTER | FIX_MODEL_SPECIFIC and free poses and landmarks returns the bytes of
 *     dsopp_hip_geometric_ba_solve given the same intrinsics: poses, positions, result and trace.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_geometric_ba dsopp_hip_geometric_ba;
typedef struct dsopp_hip_geometric_ba_problem {
  double fx, fy, cx, cy;
  int32_t width, height;
  int32_t num_frames, num_landmarks, num_observations, reserved;
  double *poses;                   /* num_frames x 12: R row-major, t; solve updates them in place */
  double *positions;               /* num_landmarks x 3; solve and triangulate update them in place */
  const int32_t *landmark_offsets; /* num_landmarks + 1, ascending from 0 to num_observations */
  const int32_t *obs_frame;        /* num_observations, 0 .. num_frames - 1 */
  const double *obs_xy;            /* num_observations x 2 */
} dsopp_hip_geometric_ba_problem;
typedef struct dsopp_hip_geometric_ba_options {
  double a;                   /* the Huber width, 1.5 */
  double lambda_0;            /* 1e-4 */
  double function_tolerance;  /* 1e-10 */
  double parameter_tolerance; /* 1e-10 */
  double decrease_factor;     /* lambda is divided by it on accept, 2 */
  double increase_factor;     /* lambda is multiplied by it on reject, 10 */
  int32_t max_iterations;     /* 50 */
  int32_t iteration_group;    /* iterations enqueued between two reads of the state record; 0 = the library's choice */
} dsopp_hip_geometric_ba_options;
enum {
  DSOPP_HIP_GEOMETRIC_BA_FUNCTION_TOLERANCE = 1,
  DSOPP_HIP_GEOMETRIC_BA_PARAMETER_TOLERANCE = 2,
  DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL = 4
};
typedef struct dsopp_hip_geometric_ba_result {
  double initial_cost, final_cost, final_lambda;
  int32_t valid_residuals; /* valid observations at the final state */
  int32_t iterations;      /* iterations run, accepted or not */
  int32_t accepted_steps;
  int32_t converged;       /* a tolerance was reached */
  int32_t reason;          /* the DSOPP_HIP_GEOMETRIC_BA_* bits that ended the loop; 0 = max_iterations */
  int32_t reserved;
} dsopp_hip_geometric_ba_result;
typedef struct dsopp_hip_geometric_ba_trace {
  double cost_before, cost_candidate, lambda; /* lambda = the one the iteration's system was damped with */
  int32_t accepted, reserved;
} dsopp_hip_geometric_ba_trace;
/* Optional outputs of solve, each NULL-able, there so that a divergence from the stated arithmetic can be located.  All but the trace and
 * the candidate belong to the LAST linearisation (the state the last iteration started from): obs_valid (M bytes), obs_residual (M x 2),
 * obs_weight (M), landmark_H (L x 6: xx xy xz yy yz zz, undamped) and landmark_b (L x 3); reduced_H (n x n, row-major, damped with
 * *system_lambda), reduced_b (n) and pose_step (n) of the last iteration's solve, n = 6 (F - 1) - 1; candidate_poses (F x 12) and
 * candidate_positions (L x 3) that iteration evaluated; trace (max_iterations records, result->iterations of them written).  Without an
 * iteration the system and the step are zero and the candidate is the state. */
typedef struct dsopp_hip_geometric_ba_debug {
  uint8_t *obs_valid;
  double *obs_residual, *obs_weight, *landmark_H, *landmark_b, *reduced_H, *reduced_b, *pose_step, *system_lambda, *candidate_poses, *candidate_positions;
  dsopp_hip_geometric_ba_trace *trace;
} dsopp_hip_geometric_ba_debug;
void dsopp_hip_geometric_ba_default_options(dsopp_hip_geometric_ba_options *options);
/* `stream` is a hipStream_t (NULL = a stream of its own); all work of the object runs on it.  Its buffers grow with F, L and M. */
int dsopp_hip_geometric_ba_create(int device, void *stream, dsopp_hip_geometric_ba **out);
void dsopp_hip_geometric_ba_destroy(dsopp_hip_geometric_ba *b);
/* Every call below is blocking.  DSOPP_HIP_ERR_CAPACITY: more than 16 frames.  DSOPP_HIP_ERR_INVALID_ARGUMENT: fewer frames than the call
 * needs (solve 2, the others 1), negative counts, an image without a region of interest, a camera, pose, observation or (where the call
 * reads them) position that is not finite, offsets that do not ascend from 0 to num_observations, a frame index out of range, a
 * (frame, landmark) pair listed twice, a NULL required argument, and what each call adds below. */
/* cost and valid observations of the state as given; one wait.  Optional per-observation outputs as in the debug record. */
int dsopp_hip_geometric_ba_evaluate(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem, double a, double *cost,
                                    int32_t *valid_residuals, uint8_t *obs_valid, double *obs_residual, double *obs_weight);
/* The LM solve; poses and positions are updated in place.  The iterations are enqueued in groups of options->iteration_group with one
 * wait after each group but the last and one at the end.  Also invalid: |t_1| = 0, an option that is not finite, a <= 0, lambda_0 < 0,
 * a factor <= 0, max_iterations < 0, iteration_group < 0.  M = 0 returns at once with DSOPP_HIP_GEOMETRIC_BA_NO_VALID_RESIDUAL. */
int dsopp_hip_geometric_ba_solve(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, const dsopp_hip_geometric_ba_options *options,
                                 dsopp_hip_geometric_ba_result *result, const dsopp_hip_geometric_ba_debug *debug);
/* The camera block: evaluate and solve with the camera as a parameter block of its own (optimizeTransformations<Model, OPTIMIZE_CAMERA>). */
enum { DSOPP_HIP_GEOMETRIC_BA_PINHOLE = 0, DSOPP_HIP_GEOMETRIC_BA_SIMPLE_RADIAL = 1 };
enum {
  DSOPP_HIP_GEOMETRIC_BA_FIX_FOCAL = 1,
  DSOPP_HIP_GEOMETRIC_BA_FIX_CENTER = 2,
  DSOPP_HIP_GEOMETRIC_BA_FIX_MODEL_SPECIFIC = 4,
  DSOPP_HIP_GEOMETRIC_BA_FIX_POSES = 8,
  DSOPP_HIP_GEOMETRIC_BA_FIX_LANDMARKS = 16
};
typedef struct dsopp_hip_geometric_ba_camera {
  int32_t model, fixed;    /* fixed: the DSOPP_HIP_GEOMETRIC_BA_FIX_* bits (ParameterParameterization) */
  double intrinsics[5];    /* pinhole fx fy cx cy (the fifth is ignored and kept) | simple radial f cx cy k1 k2; solve updates them in place */
  double max_valid_radius; /* out: simple radial, of the intrinsics the call leaves; 0 for a pinhole */
} dsopp_hip_geometric_ba_camera;
/* The debug record of solve_camera: base as above with reduced_H, reduced_b and pose_step at n = (pose unknowns: 6 (F - 1) - 1, or 0 with
 * FIX_POSES) + (free intrinsics), the camera's rows last; obs_camera_jacobian (M x 2 x 5: dr/dc of the last linearisation over all five
 * parameter slots, fixed ones included, a pinhole's fifth zero, zero where not valid); candidate_intrinsics (5) and
 * candidate_max_valid_radius (1) of the last iteration's candidate. */
typedef struct dsopp_hip_geometric_ba_camera_debug {
  dsopp_hip_geometric_ba_debug base;
  double *obs_camera_jacobian, *candidate_intrinsics, *candidate_max_valid_radius;
} dsopp_hip_geometric_ba_camera_debug;
/* Both calls are also invalid with an unknown model or fixed bit, an intrinsic that is not finite, a focal length <= 0, or a simple-radial
 * camera whose max_valid_radius is not finite or not positive.  evaluate_camera: as evaluate; writes camera->max_valid_radius. */
int dsopp_hip_geometric_ba_evaluate_camera(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem,
                                           dsopp_hip_geometric_ba_camera *camera, double a, double *cost, int32_t *valid_residuals,
                                           uint8_t *obs_valid, double *obs_residual, double *obs_weight);
/* As solve; the intrinsics are updated in place with poses and positions.  Also invalid: nothing free (FIX_POSES, FIX_LANDMARKS and every
 * intrinsic fixed).  |t_1| = 0 is invalid only when the poses are free.  Two frames are required with fixed poses too. */
int dsopp_hip_geometric_ba_solve_camera(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, dsopp_hip_geometric_ba_camera *camera,
                                        const dsopp_hip_geometric_ba_options *options, dsopp_hip_geometric_ba_result *result,
                                        const dsopp_hip_geometric_ba_camera_debug *debug);
/* has_position, triangulated: num_landmarks bytes.  Writes problem->positions of the landmarks it triangulated (triangulated[l] = 1) and
 * leaves the others; positions are not read.  Also invalid: min_number_of_projections < 2 (the reference's CHECK_GE).  One wait. */
int dsopp_hip_geometric_ba_triangulate(dsopp_hip_geometric_ba *b, dsopp_hip_geometric_ba_problem *problem, const uint8_t *has_position,
                                       int min_number_of_projections, int retriangulation, uint8_t *triangulated);
/* flags: num_observations bytes, 1 = the reference would remove the projection; *flagged (NULL-able) = their number.  Also invalid: a
 * threshold that is not a number.  One wait. */
int dsopp_hip_geometric_ba_flag_outliers(dsopp_hip_geometric_ba *b, const dsopp_hip_geometric_ba_problem *problem, double outlier_threshold,
                                         uint8_t *flags, int32_t *flagged);

/* ------------------------------------------------------------------------------------------------------------------
 * The pose of a bootstrap frame: a PnP RANSAC over the frame's landmarks with a position, with the refinement and the re-selection behind
 * it (replaces estimateSE3PnP — src/feature_based_slam/tracker/src/estimate_se3_pnp.cpp:23-77 —, which the feature-based tracker runs
 * first on every bootstrap frame once the initialiser has succeeded — monocular_tracker.cpp:54-56 — and initializePoses for every
 * intermediate frame — initialize_poses.cpp:47-73).  The reference hands its matches to OpenGV: EPnP inside OpenGV's RANSAC, then
 * optimizeModelCoefficients and selectWithinDistance.  OpenGV is not part of the reference's tree, so, like the bundle adjustment above,
 * this is the library's own algorithm for the same job: a three-point pose per hypothesis and an LM refinement of the winner.  Parity
 * with OpenGV's iteration path (its EPnP solutions, its sampler, its adaptive stopping rule, its refinement) is unpinned.  What is
 * mirrored is everything around the solver: which landmarks are matches (:31-43), the threshold's conversion (:45), the error measure,
 * refine-then-reselect (:56-60), which projections are removed (:64-74, in the host mirror) and the returned pair (:76).
 * Not built: the autocalibration variant, the SimpleRadialCamera instantiation.
 *
 * The arithmetic is fixed here; tests/pnp_ransac_model.py is its NumPy form.  Everything is binary64.
 *   Inputs: a pinhole camera fx, fy, cx, cy, width, height; n matches: the world position X[j] (3 doubles) and the observation obs[j]
 *     (x, y); `iterations` sample triples S[i] = (s1, s2, s3) of distinct indices < n, drawn by the caller; threshold_px (the reference's
 *     pnp_ransac_threshold, 0.5); the refinement's options.
 *   roi(p) and unproject(p) as in the rotation RANSAC's block; f_j = normalize(unproject(obs[j])).  A match whose observation fails roi is
 *     no match of the reference (unproject returns false, :38): it is never an inlier, a triple that holds one is invalid, and it does
 *     not count in `matches`.
 *   Threshold and measure (:45, OpenGV's absolute-pose distance): t_ang = 1 - cos(atan(threshold_px / fx)), computed once on the host.
 *     For a pose (R, t), world to camera: p = R X_j + t, d_j = 1 - f_j . p / |p|; point j is an inlier iff d_j < t_ang (strict; a NaN is
 *     no inlier).  No depth test: a point behind the camera has d near 2.
 *   Hypothesis i, the three-point pose by Grunert's elimination over the points 1, 2, 3 of its triple: a^2 = |X2 - X3|^2,
 *     b^2 = |X1 - X3|^2, c^2 = |X1 - X2|^2; ca = f2 . f3, cb = f1 . f3, cg = f1 . f2; the depths are s1, s2 = u s1, s3 = v s1.  With
 *     K = (a^2 - c^2) / b^2: N(v) = (K - 1) v^2 - 2 K cb v + 1 + K, D(v) = 2 (cg - v ca), Q(v) = v^2 - 2 cb v + 1; u = N / D, and v is a
 *     real root of the quartic D^2 + N^2 - 2 cg N D - (c^2 / b^2) Q D^2 = 0.  The roots with v > 0, u > 0, Q(v) > 0 are kept, in
 *     ascending v: at most four solutions.  s1 = sqrt(b^2 / Q(v)), the camera-frame points are Y_k = s_k f_k, and the pose comes from
 *     the two congruent triangles by frames: e1 = normalize(X2 - X1), e3 = normalize(e1 x (X3 - X1)), e2 = e3 x e1, E_w = [e1 e2 e3];
 *     the same from Y gives E_c; R = E_c E_w^T, t = Y_1 - R X_1.  A solution whose pose is not finite is dropped.  The triple is
 *     invalid, with zero solutions, when one of its observations fails roi, when b^2 = 0, or when
 *     |(X2 - X1) x (X3 - X1)|^2 <= 1e-12 |X2 - X1|^2 |X3 - X1|^2 (a degenerate world triangle).  Any route to the quartic's real roots
 *     that reaches them to rounding serves (the device: brackets from the derivatives' roots, a safeguarded Newton iteration in each; the
 *     model: numpy.roots); where two roots nearly coincide their number and the poses are unpinned.
 *   Score and selection: every solution of every hypothesis is scored against all n points.  A hypothesis's count is its best solution's,
 *     the lower solution index winning a tie; the winner is the hypothesis with the greatest count, the lowest index winning a tie.
 *     Deviation: there is no early stop — all hypotheses are scored in one launch anyway, and OpenGV's serial adaptive stopping rule has
 *     nothing to mirror here.  best_iteration = -1 when no count exceeds 0: the pose is then the identity, there are no inliers and
 *     there is no refinement.  dsopp_hip_pnp_ransac_default_iterations() = 256: log(0.01) / log(1 - w^3) <= 256 down to an inlier share
 *     w = 0.262 (OpenGV's confidence 0.99 with a three-point sample; w = 0.26 would take 260).
 *   Refinement (the role of optimizeModelCoefficients, :57-58), over the winner's inliers only, the landmarks fixed: the pixel residual
 *     r = obs - q with q and G = dq / dp as in the geometric BA's block; a point counts iff p_z >= 0.001 (no roi test on q, no robust
 *     loss); cost = 1/2 sum |r|^2.  Right increment T <- T exp(delta), delta = (upsilon, omega): J = -G R [I | -hat(X)], H = sum J^T J,
 *     b = sum J^T r in a fixed order of summation (the same input gives the same bits on every run); (H + lambda diag H) delta = -b by
 *     a 6 x 6 Cholesky; a pivot <= 0 or not finite gives no step and the iteration counts as rejected.  Control is the geometric BA's
 *     driver with one free frame: lambda_0 = 1e-4, / 2 on accept, x 10 on reject; |E - E'| / E < function_tolerance converges (accepted
 *     or not); E' < E accepts, and |delta|^2 < parameter_tolerance (|t|^2 + 1 + parameter_tolerance) converges, t of the state the step
 *     left; no counting point, at the start or at a candidate, ends the loop (the candidate rejected); function_tolerance =
 *     parameter_tolerance = 1e-10; max_iterations 10.  refine_flags are the DSOPP_HIP_GEOMETRIC_BA_* bits, 0 = max_iterations.
 *   Final selection (selectWithinDistance on the refined model, :59-60): the same test with the refined pose; its inliers, ascending, are
 *     the call's index list.  ransac_inlier_count, the first number the reference returns, is the winner's count, not the re-selected one.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_pnp_ransac dsopp_hip_pnp_ransac;
typedef struct dsopp_hip_pnp_ransac_options {
  double lambda_0;            /* 1e-4 */
  double function_tolerance;  /* 1e-10 */
  double parameter_tolerance; /* 1e-10 */
  double decrease_factor;     /* lambda is divided by it on accept, 2 */
  double increase_factor;     /* lambda is multiplied by it on reject, 10 */
  int32_t max_iterations;     /* 10 */
  int32_t reserved;
} dsopp_hip_pnp_ransac_options;
typedef struct dsopp_hip_pnp_ransac_result {
  int32_t matches;              /* the observations inside the ROI, the reference's matching number */
  int32_t best_iteration;       /* the winning hypothesis, -1 when no count exceeded 0 */
  int32_t best_solution;        /* its solution, 0 .. 3; -1 without a winner */
  int32_t ransac_inlier_count;  /* the winner's count */
  int32_t refined_inlier_count; /* the inliers of the refined pose: the length of the index list */
  int32_t refine_iterations;    /* iterations run, accepted or not */
  int32_t refine_flags;         /* the DSOPP_HIP_GEOMETRIC_BA_* bits that ended the loop; 0 = max_iterations */
  int32_t reserved;
  double cost_initial, cost_final; /* 1/2 sum |r|^2 over the winner's inliers, before and after */
  double pose_ransac[12];       /* the winner's pose, world to camera: R row-major, then t (the t_agent_world layout above) */
  double pose[12];              /* the refined pose */
} dsopp_hip_pnp_ransac_result;
int dsopp_hip_pnp_ransac_default_iterations(void);
void dsopp_hip_pnp_ransac_default_options(dsopp_hip_pnp_ransac_options *options);
/* `stream` is a hipStream_t (NULL = a stream of its own); all work of the object runs on it.  Its buffers grow with n and iterations. */
int dsopp_hip_pnp_ransac_create(int device, void *stream, dsopp_hip_pnp_ransac **out);
void dsopp_hip_pnp_ransac_destroy(dsopp_hip_pnp_ransac *r);
/* One launch and one wait, blocking.  positions: n x 3 doubles; observations: n x 2; samples: iterations x 3 int32; options: NULL = the
 * defaults; inlier_indices: room for n int32, the first result->refined_inlier_count of which are written, ascending.  Optional (NULL)
 * per-hypothesis outputs, there so that a divergence from the stated arithmetic can be located: hyp_num_solutions (iterations int32),
 * hyp_poses (iterations x 4 x 12 doubles, unused slots zero), hyp_counts (iterations x 4 int32, unused slots zero); they cover every
 * hypothesis.  n = 0 or iterations = 0 returns at once without a winner.  DSOPP_HIP_ERR_INVALID_ARGUMENT: n < 0, iterations < 0,
 * 0 < n < 3 with iterations > 0, a sample index outside 0 .. n - 1 or repeated within its triple, a position, observation, threshold or
 * intrinsic that is not finite, an option that is not finite or out of range (lambda_0 < 0, a factor <= 0, max_iterations < 0), a NULL
 * required argument. */
int dsopp_hip_pnp_ransac_estimate(dsopp_hip_pnp_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                  const double *positions, const double *observations, int iterations, const int32_t *samples, double threshold_px,
                                  const dsopp_hip_pnp_ransac_options *options, dsopp_hip_pnp_ransac_result *result, int32_t *inlier_indices,
                                  int32_t *hyp_num_solutions, double *hyp_poses, int32_t *hyp_counts);

/* ------------------------------------------------------------------------------------------------------------------
 * The two-view pose that initialises a track: a five-point essential-matrix RANSAC over the matches of the first and the last bootstrap
 * frame, the Sampson refinement around its re-selection, and the two-view triangulation behind it (replaces estimateSO3xS2 —
 * src/feature_based_slam/tracker/src/estimate_so3xs2.cpp:23-110 —, refineSO3xS2 — src/energy/problems/src/so3xs2_refinement.cpp:13-50 with
 * cost_functors/sampson_distance_cost.hpp:17-66 — and the two-view triangulatePoints — triangulate_points.cpp:18-45 with
 * epipolar_geometry/triangulation.hpp:26-42: steps I and II of initializePoses, initialize_poses.cpp:29-45; steps III to V are
 * dsopp_hip_pnp_ransac_* and dsopp_hip_geometric_ba_* above).  The reference hands step I to OpenGV (Stewenius' five-point solver inside
 * OpenGV's RANSAC, then optimizeModelCoefficients and selectWithinDistance) and refines with Ceres (Sampson error, Huber loss, quaternion
 * x S^2 parameterisation).  Neither library is part of the reference's tree, so, like the bundle adjustment and the PnP above, this is the
 * library's own algorithm for the same job.  Mirrored: which landmarks are matches (:33-46), the minimum number of matches (:48), the
 * threshold's conversion (:55-56), refine-then-reselect (:58-68), the normalised translation (:70-71), which projections are removed
 * (:77-86, in the host mirror), the refinement's residual, loss, threshold and iteration limit (:88-105) and the returned pair (:109).
 * The library's own: the five-point solver, the two-view measure, both refinements' iteration.  Unpinned: OpenGV's sampler, its three
 * extra disambiguation points, its stopping rule and its optimiser; Ceres' second-order corrector and its trust-region path.
 * Not built: the SimpleRadialCamera instantiation, the focal-length refinement.
 *
 * Direction.  The reference names the result t_t_r, but it maps the TARGET (last) frame into the REFERENCE (first) frame: OpenGV's
 * central relative pose is frame 2 seen from frame 1 with (reference_bearings, target_bearings) as frames 1 and 2 (:52); the refinement
 * is handed its two point lists swapped (:93-99), so its cost x_first . E x_last with E = hat(t) R (sampson_distance_cost.hpp:52-59) is the
 * epipolar constraint of exactly that direction; and initialize_poses.cpp:31-33 stores the result as last_frame.t_world_agent with the
 * first frame at the identity.  The same holds for the triangulation, whose `target` is the first frame's ray and whose t_t_r argument is
 * t_first_last (triangulate_points.cpp:22-37).  That direction is kept here.
 *
 * The arithmetic is fixed here; tests/two_view_ransac_model.py is its NumPy form.  Everything is binary64.
 *   Inputs: a pinhole camera fx, fy, cx, cy, width, height; n matches: A[j], the first frame's observation, and B[j], the last frame's
 *     (x, y); `iterations` samples S[i] of five distinct indices < n, drawn by the caller; threshold_px (the reference's
 *     essential_matrix_ransac_threshold, 0.5); min_matches (min_ransac_matches, 50); the refinement's options.
 *   Pose: (R, t) with |t| = 1 and p_A = R p_B + t, as 12 doubles: R row-major, then t.  E = hat(t) R, and f_A . E f_B = 0.
 *   roi(p) and unproject(p) as in the rotation RANSAC's block; f_A = normalize(unproject(A[j])), f_B likewise.  A match with an
 *     observation that fails roi is no match of the reference (:40-41): it is never an inlier, a sample that holds one is invalid, and it
 *     does not count in `matches`.  matches < min_matches returns without a winner and without looking at the samples.
 *   Triangulation of a pair under a pose (triangulation.hpp:29-41): a = f_A, b = normalize(R f_B), den = 1 / (1 - (a.b)^2),
 *     alpha = den (a.t - (a.b)(b.t)), beta = den ((a.b)(a.t) - b.t), X_A = (alpha a + beta b + t) / 2, X_B = R^T (X_A - t).
 *   Threshold and measure: t_ang = 1 - cos(atan(threshold_px / fx)), computed once on the host;
 *     d_j = (1 - f_A . X_A / |X_A|) + (1 - f_B . X_B / |X_B|), the role of OpenGV's two-view reprojection distance; a match is an inlier
 *     iff d_j < t_ang (strict; a NaN is no inlier, and parallel rays give one).
 *   Hypothesis i: its essential matrices are the real E in the four-dimensional null space of the five constraints f_A (x) f_B that
 *     satisfy det E = 0 and 2 E E^T E - tr(E E^T) E = 0, at most ten.  With an orthonormal basis E_1 .. E_4 of the null space and
 *     E = x E_1 + y E_2 + z E_3 + E_4 these are ten cubics in (x, y, z).  Each solution is polished on those ten cubics, evaluated on E
 *     itself, by Gauss-Newton (3 x 3 normal equations; at most 12 steps, until |step|^2 <= 1e-28 (1 + |(x, y, z)|^2)), so the route that
 *     found it contributes second-order error only; E is then scaled to |E|_F^2 = 2, and an E on which a constraint still exceeds 1e-9 in
 *     magnitude is dropped.  Any basis serves, and any route to the solutions that reaches them to rounding (the model: the 10 x 10 action
 *     matrix from the Gauss-Jordan-reduced 10 x 20 coefficient matrix and numpy.linalg.eig; the device: the hidden-variable form, a
 *     polynomial of degree 10 in z whose real roots are bracketed through the chain of its derivatives and closed by the PnP's safeguarded
 *     Newton iteration).  Per E = U diag(s, s, 0) V^T the four candidates are R in {U W V^T, U W^T V^T}, signs fixed so that det R = +1,
 *     with t = +-u_3 (the device takes them in closed form: t the unit normal of E's columns, R = Cof(E) -+ hat(t) E); the one candidate
 *     under which all five sample pairs have alpha > 0 and beta > 0 is kept, an E without one is dropped.  Non-finite poses are dropped;
 *     the surviving poses are listed in descending trace R.  A sample with an observation outside roi is invalid, with zero solutions.
 *     Where two solutions nearly coincide their number and the poses are unpinned; a rank-deficient sample (a repeated pair of
 *     observations, ...) is unpinned too, but yields either nothing or finite poses with an orthonormal R and a unit t.
 *   Score and selection as in the PnP's block: every solution is scored against all n matches; a hypothesis counts its best solution, the
 *     lower index winning a tie; the winner is the greatest count, the lowest hypothesis winning a tie; best_iteration = -1 when no count
 *     exceeds 0; no early stop.  dsopp_hip_two_view_ransac_default_iterations() = 256: log(0.01) / log(1 - w^5) <= 256 down to an inlier
 *     share w = 0.447, well under the 0.6 below which initializePoses rejects the result anyway (:37).
 *   Refinement, one routine run twice.  Residual (sampson_distance_cost.hpp:17-28, 52-66): x_A = ((A - c) / fx, 1), x_B = ((B - c) / fx, 1) —
 *     fx divides both axes, as in the reference —, top = x_A . E x_B, bottom = |(E x_B)_xy / fx|^2 + |(x_A^T E)_xy / fx|^2,
 *     r = top / sqrt(bottom), or top when bottom < 1e-16: pixels.  Cost = 1/2 sum rho(r^2) with the geometric BA's Huber rho (a = 1.5, the
 *     reference's reprojection_threshold) and plain IRLS weights.  Five degrees of freedom (alpha, beta, omega): R <- R Exp(omega),
 *     t <- normalize(t + alpha b1 + beta b2), b1 and b2 by the geometric BA's rule for its frame 1 with d = t; the Jacobian is analytic
 *     (dE = hat(b1) R, hat(b2) R, E hat(e_k)).  H = sum w J^T J and b = sum w J^T r in a fixed order of summation; (H + lambda diag H)
 *     delta = -b by a 5 x 5 Cholesky.  Control is the PnP block's driver: lambda_0 = 1e-4, / 2, x 10, both tolerances 1e-10, the state norm
 *     |t|^2 + 1; max_iterations 40 (so3xs2_refinement.cpp:41); no pair to sum over ends the loop.  The flags are the
 *     DSOPP_HIP_GEOMETRIC_BA_* bits, 0 = max_iterations.
 *   Sequence: 1. the winner, pose_ransac; 2. the refinement over the winner's inliers (the role of optimizeModelCoefficients),
 *     pose_reselect; 3. the re-selection with pose_reselect: its ascending index list is the call's inlier list and its length
 *     inlier_count, the first number the reference returns; 4. the refinement over the re-selected inliers (refineSO3xS2), pose.  There
 *     is no third selection.  Without a winner the three poses are the identity rotation with a zero translation.
 *   Two-view triangulation (step II): for each pair X_A by the formulas above under pose_a_b; keep iff both observations pass roi,
 *     X_A.z > 0, f_A . X_A / |X_A| > cos_threshold and f_B . X_B / |X_B| > cos_threshold (triangulation_cos_threshold, 0.9999; strict)
 *     and everything is finite; X_world = pose_world_a X_A is written for every pair.
 * There is no CPU fallback: without a device create fails with DSOPP_HIP_ERR_HIP.
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_two_view_ransac dsopp_hip_two_view_ransac;
typedef struct dsopp_hip_two_view_ransac_options {
  double a;                   /* the Huber width, 1.5 */
  double lambda_0;            /* 1e-4 */
  double function_tolerance;  /* 1e-10 */
  double parameter_tolerance; /* 1e-10 */
  double decrease_factor;     /* lambda is divided by it on accept, 2 */
  double increase_factor;     /* lambda is multiplied by it on reject, 10 */
  int32_t max_iterations;     /* 40, of either refinement */
  int32_t reserved;
} dsopp_hip_two_view_ransac_options;
typedef struct dsopp_hip_two_view_ransac_result {
  int32_t matches;              /* the pairs with both observations inside the ROI, the reference's matching number */
  int32_t best_iteration;       /* the winning hypothesis, -1 when no count exceeded 0 */
  int32_t best_solution;        /* its solution, 0 .. 9; -1 without a winner */
  int32_t ransac_inlier_count;  /* the winner's count */
  int32_t inlier_count;         /* the inliers of pose_reselect: the length of the index list, the reference's first number */
  int32_t refine_iterations[2]; /* per stage: iterations run, accepted or not */
  int32_t refine_flags[2];      /* per stage: the DSOPP_HIP_GEOMETRIC_BA_* bits that ended the loop; 0 = max_iterations */
  int32_t reserved;
  double cost_initial[2], cost_final[2]; /* per stage: 1/2 sum rho(r^2) over the stage's inliers, before and after */
  double pose_ransac[12];       /* the winner's pose: R row-major, then t; p_A = R p_B + t */
  double pose_reselect[12];     /* after the first refinement: the pose of the re-selection */
  double pose[12];              /* after the second refinement: the call's pose */
} dsopp_hip_two_view_ransac_result;
int dsopp_hip_two_view_ransac_default_iterations(void);
void dsopp_hip_two_view_ransac_default_options(dsopp_hip_two_view_ransac_options *options);
/* `stream` is a hipStream_t (NULL = a stream of its own); all work of the object runs on it.  Its buffers grow with n and iterations. */
int dsopp_hip_two_view_ransac_create(int device, void *stream, dsopp_hip_two_view_ransac **out);
void dsopp_hip_two_view_ransac_destroy(dsopp_hip_two_view_ransac *r);
/* One launch and one wait, blocking.  points_a, points_b: n x 2 doubles; samples: iterations x 5 int32; options: NULL = the defaults;
 * inlier_indices: room for n int32, the first result->inlier_count of which are written, ascending.  Optional (NULL) per-hypothesis
 * outputs, there so that a divergence from the stated arithmetic can be located: hyp_num_solutions (iterations int32), hyp_poses
 * (iterations x 10 x 12 doubles, unused slots zero), hyp_counts (iterations x 10 int32, unused slots zero); they cover every hypothesis.
 * n = 0, iterations = 0 or matches < min_matches returns at once without a winner (the samples are then not read).
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: n < 0, iterations < 0, min_matches < 0, 0 < n < 5 with iterations > 0, a sample index outside
 * 0 .. n - 1 or repeated within its sample, an observation, threshold or intrinsic that is not finite, an option that is not finite or
 * out of range (a <= 0, lambda_0 < 0, a factor <= 0, max_iterations < 0), a NULL required argument. */
int dsopp_hip_two_view_ransac_estimate(dsopp_hip_two_view_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                       const double *points_a, const double *points_b, int iterations, const int32_t *samples, double threshold_px,
                                       int min_matches, const dsopp_hip_two_view_ransac_options *options,
                                       dsopp_hip_two_view_ransac_result *result, int32_t *inlier_indices, int32_t *hyp_num_solutions,
                                       double *hyp_poses, int32_t *hyp_counts);
/* The two-view triangulation; one launch and one wait, blocking.  pose_a_b: the pose above (the last frame into the first);
 * pose_world_a: the first frame's t_world_agent, 12 doubles; positions: n x 3 doubles, X_world of every pair; keep: n bytes, 1 = the
 * reference would set the landmark's position.  DSOPP_HIP_ERR_INVALID_ARGUMENT: n < 0, an observation, intrinsic or pose entry that is
 * not finite, a cos_threshold that is not a number, a NULL required argument. */
int dsopp_hip_two_view_ransac_triangulate(dsopp_hip_two_view_ransac *r, double fx, double fy, double cx, double cy, int width, int height, int n,
                                          const double *points_a, const double *points_b, const double pose_a_b[12], const double pose_world_a[12],
                                          double cos_threshold, double *positions, uint8_t *keep);

/* ------------------------------------------------------------------------------------------------------------------
 * Semantic segmentation: the per-frame camera mask and the class image of a frame (replaces, per frame, the undistortion of the class
 * image — src/sensors/camera/src/camera.cpp:57-65 —, CameraMask::filterSemanticObjects —
 * src/sensors/camera_calibration/src/camera_mask.cpp:31-39 — and the mask pyramid of src/features/src/camera_features.cpp:71-84; the
 * `segmentation:` block that configures them is read by src/sensors/sensors_builder/src/camera_fabric.cpp:54-99,170-186)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_semantics dsopp_hip_semantics;
/* The per-camera constants.  static_mask_host: the camera's W x H mask bytes, already undistorted as camera_fabric.cpp:164 keeps them
 * (NULL = all 255).  is_filtered256: SemanticFilter::is_filtered_ (src/common/semantics/src/semantic_filter.cpp:5-14), one byte per class
 * code, non-zero = pixels of that class leave the mask (NULL = filterBySemantic() is false: nothing is filtered).  undistorter: the
 * remap every class image goes through (NULL = class images arrive undistorted, W x H); it is BORROWED and must outlive this object,
 * live on `device` and write width x height.  levels in 1 .. DSOPP_HIP_MAX_LEVELS, and width and height must be divisible by
 * 2^(levels - 1) — for other sizes the reference's own mask sizes (cvRound of the scaled size) differ from its image level sizes —
 * else DSOPP_HIP_ERR_INVALID_ARGUMENT.  Both host arrays are copied before the call returns. */
int dsopp_hip_semantics_create(int device, void *stream, int width, int height, int levels, const uint8_t *static_mask_host,
                               const uint8_t *is_filtered256, const dsopp_hip_undistorter *undistorter, dsopp_hip_semantics **out);
/* The same for a camera with image transformers (camera.cpp:57-65: the class image is undistorted, then goes through
 * runMaskTransformers).  Width and height are the transformer's output size; static_mask_host is the mask already undistorted and
 * transformed (dsopp_hip_transformer_transform_mask, camera_fabric.cpp:164).  dsopp_hip_pyramid_set_semantics then takes the class
 * image at the undistorter's input size (without one: the transformer's), remaps it, resizes it with INTER_NEAREST and crops it, and
 * the pyramid keeps that as the frame's semanticsData.  Both are BORROWED, must outlive this object and live on `device`; the
 * undistorter (may be NULL) must write the transformer's input size, and the output size must be divisible by 2^(levels - 1) — which
 * the crop provides for crop_levels >= levels - 1 — else DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_semantics_create_transformed(int device, void *stream, int levels, const uint8_t *static_mask_host, const uint8_t *is_filtered256,
                                           const dsopp_hip_undistorter *undistorter, const dsopp_hip_transformer *transformer,
                                           dsopp_hip_semantics **out);
void dsopp_hip_semantics_destroy(dsopp_hip_semantics *s);
/* The frame's class image and the masks of all its levels.  class_image_host: the distorted in_h x in_w class codes (W x H without an
 * undistorter); it goes through a pinned buffer of the pyramid, is remapped on the pyramid's stream by the undistorter's kernel (the
 * reference runs the same cv::remap(INTER_LINEAR) over class codes, camera.cpp:57-65: the integer arithmetic stated at
 * dsopp_hip_undistorter_create applies unchanged) and is kept by the pyramid as the frame's semanticsData.  NULL = the frame has no
 * semantic data.  Then ONE launch writes the mask lane of every level and the level-0 mask bytes, in exact integer arithmetic:
 *   m0[y, x]  = is_filtered[c[y, x]] ? 0 : static[y, x]        (camera_mask.cpp:31-39; without a filter or a class image m0 = static,
 *                                                                the copy of pyramid_of_static_masks_, camera_features.cpp:73)
 *   m_l[y, x] = (m0[cy, cx] + m0[cy, cx + 1] + m0[cy + 1, cx] + m0[cy + 1, cx + 1] + 2) >> 2,  cx = 2^l x + 2^(l-1) - 1, cy alike
 * — every level from level 0 directly, which is CameraMask::resize(1 / 2^l) = cv::resize(INTER_LINEAR) at these ratios
 * (camera_features.cpp:76-82) — and a texel is valid iff m_l != 0.  The build kernels keep the mask lane, so build* and set_semantics
 * work in either order.  The call only enqueues on the pyramid's stream and records the pyramid's ready event; it does not wait.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: another device, another size, or more levels than the semantics object was created for. */
int dsopp_hip_pyramid_set_semantics(dsopp_hip_pyramid *p, const dsopp_hip_semantics *s, const uint8_t *class_image_host);
/* the undistorted class image the pyramid keeps (W x H bytes; out_host may be NULL); *present = 0 when the last set_semantics had
 * no class image or there was none: out_host is then left alone */
int dsopp_hip_pyramid_get_semantics(dsopp_hip_pyramid *p, uint8_t *out_host, int *present);
/* the mask lane of a level's texels as bytes: 1 = valid, 0 = masked (CameraMask::valid) */
int dsopp_hip_pyramid_get_mask(dsopp_hip_pyramid *p, int level, uint8_t *out_host);

/* ------------------------------------------------------------------------------------------------------------------
 * Sliding-window photometric bundle adjustment
 * (replaces EigenPhotometricBundleAdjustment<SE3, PinholeCamera, 8, PixelMap, true, true, true, 1>)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_window dsopp_hip_window;

int dsopp_hip_window_create(const dsopp_hip_options *options, int device, void *stream, dsopp_hip_window **out);
void dsopp_hip_window_destroy(dsopp_hip_window *w);

/* pushFrame(ActiveKeyframe, level, model, parameterization) — PBA_INC/photometric_bundle_adjustment.hpp:55-56,
 * PROB_SRC/eigen_photometric_bundle_adjustment.cpp:119-141: when the window already holds > 1 frame, first folds the
 * landmarks/frames flagged for marginalisation into the marginal prior (updateMarginalizedLinearSystem,
 * PBA_INT/eigen_photometric_bundle_adjustment_problem.hpp:146-203), then appends the frame.
 * The pyramid is BORROWED: it must outlive the frame's stay in the window (the reference keeps raw pointers to the
 * keyframe's PixelMap levels, PBA_INT/local_frame.hpp:323-325).  intrinsics = (fx, fy, cx, cy) of that level. */
int dsopp_hip_window_push_frame(dsopp_hip_window *w, int32_t frame_id, int64_t timestamp, const dsopp_hip_pyramid *pyramid,
                                int level, const double intrinsics[4], const double T_world_agent[7], double exposure_time,
                                const double affine_brightness[2], int fixed, int is_marginalized);
/* LocalFrame ctor landmark copy + LocalFrame::update (PBA_INT/local_frame.hpp:309-335,484-505).  n_total >= current count;
 * existing landmarks only get their flags refreshed (to_marginalize = newly marginalised && !outlier), new ones are
 * appended.  uv = landmark.projection(), patch = 8 intensities of the host level-0 image (src/track/frames/src/
 * active_keyframe.cpp:96-110).  flags bit0 = isMarginalized, bit1 = isOutlier.
 * The arrays are copied before the call returns; the device side of set_landmarks / set_connection is QUEUED and applied — one transfer,
 * one launch for everything queued — in front of the next call that uses the window's device state (any solve / stage / getter /
 * push_frame / activation call): a keyframe step's ~120 appends cost host time only.  A device error of a queued append is reported by
 * that later call. */
int dsopp_hip_window_set_landmarks(dsopp_hip_window *w, int32_t frame_id, int32_t n_total, const double *uv, const double *idepth,
                                   const double *patch, const uint8_t *flags);
/* residual lists from FrameConnection statuses (PROB_SRC/photometric_bundle_adjustment.cpp:109-123, local_frame.hpp:507-519):
 * appends entries [current size, n) of the (reference, target) connection.  A target that is not in the window (not pushed yet, or
 * folded into the prior) is legal, as in LocalFrame::update, which keeps the list of every connection: the statuses are kept on the
 * host as given — they become the device list when a frame with that id is pushed, and they are what get_frame_update returns
 * for such a target. */
int dsopp_hip_window_set_connection(dsopp_hip_window *w, int32_t reference_id, int32_t target_id, int32_t n, const uint8_t *statuses);
/* updateLocalFrame's frame flags (PROB_SRC/eigen_photometric_bundle_adjustment.cpp:106-113) */
int dsopp_hip_window_mark_frame_marginalized(dsopp_hip_window *w, int32_t frame_id);
int dsopp_hip_window_num_frames(dsopp_hip_window *w, int32_t *n);
/* ids of the frames currently in the window, oldest first (frames_ of PBA_INC/photometric_bundle_adjustment.hpp:181 after
 * the fold-in of pushFrame erased the marginalised ones): a caller that owns the borrowed pyramids learns here which of them the
 * window has let go of.  At most `capacity` ids are written, *n receives the count. */
int dsopp_hip_window_frame_ids(dsopp_hip_window *w, int32_t capacity, int32_t *ids, int32_t *n);

/* solve(number_of_threads) -> final energy — PBA_INC/photometric_bundle_adjustment.hpp:154,
 * PROB_SRC/eigen_photometric_bundle_adjustment.cpp:61-101 (FEJ, LM loop on device, relinearise, covariances, point statuses) */
int dsopp_hip_window_solve(dsopp_hip_window *w, double *energy, int32_t *iterations, int32_t *n_valid);

/* stage-level entry points = PhotometricBundleAdjustmentProblem methods (PBA_INT/eigen_photometric_bundle_adjustment_problem.hpp:290-402)
 * for host-driven LM and stage-by-stage parity checks */
int dsopp_hip_window_begin(dsopp_hip_window *w);                                           /* problem ctor + firstEstimateJacobians */
int dsopp_hip_window_calculate_energy(dsopp_hip_window *w, double *energy, int32_t *n_valid); /* :290-317 */
int dsopp_hip_window_linearize(dsopp_hip_window *w);                                        /* :322-336 */
int dsopp_hip_window_get_system(dsopp_hip_window *w, double *H_pp, double *b_pp, double *H_schur, double *b_schur);
int dsopp_hip_window_calculate_step(dsopp_hip_window *w, double lambda, double *step);     /* :342-361 */
int dsopp_hip_window_accept_step(dsopp_hip_window *w, double *state_sq, double *step_sq);  /* :366-388 */
int dsopp_hip_window_reject_step(dsopp_hip_window *w);                                      /* :392-402 */
int dsopp_hip_window_update_point_statuses(dsopp_hip_window *w);                            /* PROB_SRC/photometric_bundle_adjustment.cpp:321-406 */

/* read-back = PhotometricBundleAdjustment::updateFrame / getPose / getAffineBrightness
 * (PROB_SRC/photometric_bundle_adjustment.cpp:156-264) */
int dsopp_hip_window_get_frame_state(dsopp_hip_window *w, int32_t frame_id, double T0[7], double ab0[2], double eps[8], double step[8]);
int dsopp_hip_window_get_pose(dsopp_hip_window *w, int32_t frame_id, double T_world_agent[7], double affine_brightness[2]);
int dsopp_hip_window_num_landmarks(dsopp_hip_window *w, int32_t frame_id, int32_t *n);
/* updateFrame in one transfer (PROB_SRC/photometric_bundle_adjustment.cpp:182-264 reads, per keyframe: idepths, H_dd^-1 for the
 * idepth variance, relative baselines, inlier counts, outlier flags and the connection statuses towards every other frame):
 * a gather kernel packs everything of one frame, one pinned device-to-host copy, one synchronisation.  Any landmark array may
 * be NULL; statuses receives n_targets rows of n bytes in the order of target_ids.  (The per-array getters below cost one
 * copy + wait each.) */
int dsopp_hip_window_get_frame_update(dsopp_hip_window *w, int32_t frame_id, double *idepth, double *inv_hessian_idepth, double *relative_baseline,
                                      int32_t *n_inliers, uint8_t *flags_out, int32_t n_targets, const int32_t *target_ids, uint8_t *statuses);
/* any output may be NULL.  flags_out bit0 marginalized, bit1 outlier, bit2 to_marginalize, bit3 ill_conditioned;
 * hpib (hessian_poses_idepth_block) is n x K */
int dsopp_hip_window_get_landmarks(dsopp_hip_window *w, int32_t frame_id, double *idepth, double *idepth_step, double *inv_hessian_idepth,
                                   double *b_idepth, double *relative_baseline, int32_t *n_inliers, uint8_t *flags_out, double *hpib);
int dsopp_hip_window_get_residuals(dsopp_hip_window *w, int32_t reference_id, int32_t target_id, int32_t n, uint8_t *status,
                                   uint8_t *candidate, double *energy);
int dsopp_hip_window_get_marginalized(dsopp_hip_window *w, double *H, double *b, double *energy, int32_t *size);
int dsopp_hip_window_get_covariance(dsopp_hip_window *w, int32_t reference_id, int32_t target_id, double cov[36]);

/* ---- class observations of the landmarks (semantic segmentation) ----
 * addSemanticObservations(track, marginalized_keyframes_ids, model) — src/tracker/tracker/src/monocular_tracker.cpp:263-305, called at
 * :506 for the keyframes the marginalisation strategy just chose — on the window's own state.  For every listed frame M and every
 * frame X of the window that is neither flagged marginalised nor listed (:298-300), both directions (reference M, target X) and
 * (reference X, target M): for every landmark i of the reference whose connection status towards the target is kOk, the 8 pattern
 * points are reprojected by the checked pinhole reprojector (validIdepth, reference and target insideCameraROI, z > 0 —
 * src/energy/projector/include/energy/projector/camera_reproject.hpp:270-293) with the intrinsics the frames were pushed with (level 0,
 * else DSOPP_HIP_ERR_INVALID_ARGUMENT), T_target^-1 * T_reference of the current estimates (dsopp_hip_window_get_pose) and the
 * landmark's current inverse depth; on success hist[i][class_target[int(v_k), int(u_k)]] is incremented for the 8 points.  class_target
 * is the class image the target's pyramid keeps (dsopp_hip_pyramid_set_semantics); a target without one is skipped (:268-269).  The
 * counters are bytes and wrap modulo 256, as the reference's std::array<uint8_t, 256> does.  A landmark's 256 counters are written by
 * the one work item that owns the landmark, which walks the partner frames itself: no atomics, bit-exact, independent of any order.
 * One deviation: the reference reads the KEYFRAME's inverse depth, which for a landmark whose solved inverse depth went negative still
 * holds the previous value (updateFrame marks it outlier instead of copying); the window uses its own value.  Such landmarks are
 * outliers and are never exported.
 * The counters live with the frame while it is in the window (read them before the push_frame that folds the frame out), follow their
 * landmarks through every internal re-ordering and through appends (new landmarks start at zero), and are allocated by the first add:
 * a window that never uses semantics pays nothing.  dsopp_hip_window_snapshot / _restore leave them alone. */
int dsopp_hip_window_add_semantic_observations(dsopp_hip_window *w, int32_t n, const int32_t *marginalized_frame_ids);
/* semantic_type_observations_ of every landmark of a frame: n_landmarks x 256 bytes in the caller's landmark order (all zero
 * before the first add) */
int dsopp_hip_window_get_semantic_observations(dsopp_hip_window *w, int32_t frame_id, uint8_t *hist);
/* ActiveTrackingLandmark::semanticTypeId(legend) (src/track/landmarks/src/active_tracking_landmark.cpp:71-88) for every landmark
 * of a frame, on the device: weights256 = SemanticLegend::weights_ as 256 uint64 (std::array<size_t, 256> weights_ = {1}: only code 0 has a default weight,
 * every other code the legend does not list weighs 0), NULL = no legend.
 * Without weights the first maximal count; with weights the first i with the strictly largest count[i] * weight[i], the first
 * maximal count when every product is 0.  type: n_landmarks bytes. */
int dsopp_hip_window_get_semantic_types(dsopp_hip_window *w, int32_t frame_id, const uint64_t *weights256, uint8_t *type);

/* multi-GPU: landmarks are sharded across ranks by the caller (each rank uploads only its shard; frames and images are
 * replicated).  The library calls `allreduce_sum` on its stream whenever partial sums over landmarks must be combined
 * (the reduced normal equations once per linearisation, energy + valid count once per energy sweep).  `device_buffer`
 * is device memory holding `count` doubles to be summed in place across ranks.  With no callback the window is single-GPU. */
typedef int (*dsopp_hip_allreduce_fn)(void *user, void *device_buffer, size_t count, void *stream);
int dsopp_hip_window_set_allreduce(dsopp_hip_window *w, dsopp_hip_allreduce_fn fn, void *user, int rank, int world_size);

/* The same exchange as native code: a communicator of one rank per GPU (one process per GPU) whose all-reduce the library
 * enqueues itself — ncclAllReduce(sum, double) over RCCL / xGMI on the window's stream, no callback into the host language.
 * Replaces the mutex reduction of the per-thread partial systems (PBA_INT/hessian_block_evaluation.hpp:101-145,178-235) across
 * GPUs.  Rank 0 obtains an id (dsopp_hip_comm_unique_id), hands it to the other ranks by any means (MPI, a file, a socket),
 * then EVERY rank calls dsopp_hip_comm_create (collective).  dsopp_hip_comm_adopt wraps an ncclComm_t the host program
 * already owns (not destroyed with the wrapper): the communicator must come from the SAME loaded librccl this library resolves
 * (the instance already mapped into the process — e.g. PyTorch's — else /opt/rocm/lib/librccl.so.1); a handle of another RCCL
 * build (statically linked, differently named) must not be adopted.  `device` is the device the communicator's rank runs on.
 * librccl is loaded on first use only. */
#define DSOPP_HIP_COMM_ID_BYTES 128
typedef struct dsopp_hip_comm dsopp_hip_comm;
int dsopp_hip_comm_unique_id(uint8_t id[DSOPP_HIP_COMM_ID_BYTES]);
int dsopp_hip_comm_create(const uint8_t id[DSOPP_HIP_COMM_ID_BYTES], int rank, int world_size, int device, dsopp_hip_comm **out);
int dsopp_hip_comm_adopt(void *nccl_comm, int device, dsopp_hip_comm **out);
void dsopp_hip_comm_destroy(dsopp_hip_comm *c);
/* ncclCommAbort: releases collectives the other ranks have enqueued and that this rank will never join (it failed between two of
 * them); the handle can only be destroyed afterwards, a window it is attached to fails its next collective with an error instead of
 * enqueueing it.  What dsopp_hip_window_group does with every shard's communicator when one shard fails. */
int dsopp_hip_comm_abort(dsopp_hip_comm *c);
int dsopp_hip_comm_rank(const dsopp_hip_comm *c, int *rank, int *world_size);
/* in-place sum of `count` doubles in device memory across the ranks, ordered on `stream` (a hipStream_t) */
int dsopp_hip_comm_allreduce(dsopp_hip_comm *c, void *device_buffer, size_t count, void *stream);
/* attach (NULL: detach) a communicator: the window sums its partial systems / energy scalars through it.  The communicator
 * must outlive its use by the window; landmarks are sharded by the caller exactly as with dsopp_hip_window_set_allreduce. */
int dsopp_hip_window_set_comm(dsopp_hip_window *w, dsopp_hip_comm *comm);

/* ------------------------------------------------------------------------------------------------------------------
 * Window group: ONE host process, n landmark shards of one sliding window on n devices
 *
 * The reference builds ONE solver object in ONE process (createPhotometricBundleAdjustment, src/tracker/tracker/src/fabric.cpp:58-121,
 * moved into the tracker that src/application/dsopp_main.cpp:114-119 runs), so the multi-GPU form of the drop-in has to live behind
 * one object too.  A group has the calls of dsopp_hip_window (same argument meaning and error codes; every dsopp_hip_window_group_X
 * replaces what dsopp_hip_window_X replaces) and does the sharding itself:
 *   - frames, images, poses, the marginal prior: replicated on every device (dsopp_hip_pyramid_group = one pyramid per distinct device);
 *   - landmarks and their connection statuses: landmark j of a keyframe lives on shard j % n at local index j / n (balanced to +-1 and
 *     stable under the appends of PROB_SRC/photometric_bundle_adjustment.cpp:109-123); the getters interleave them back;
 *   - every Gauss-Newton iteration sums the partial combined systems with ONE collective (F(F+1)/2 * 64 + K + 4 doubles), every shard
 *     then takes the same LM decision, solves the same K x K system and back-substitutes its own landmarks.
 * One worker thread per shard enqueues that shard's launches.  transport: RCCL = ncclAllReduce on the shards' streams over xGMI, one
 * rank per device (all device ids distinct); LOCAL = an event-ordered sum kernel inside the process (peer access between the
 * devices; the only choice when shards share a device, e.g. to exercise the sharded path on a single GPU); AUTO = RCCL when the ids
 * are distinct (falling back to LOCAL when no communicator can be created, e.g. no librccl on the node — an explicit RCCL request
 * fails instead), else LOCAL.  P2P = the one-shot all-reduce: every shard stores its partial sums (15 .. 41 KB per Gauss-Newton
 * iteration) straight into every peer's receive area over the direct xGMI links and adds up what the others stored into its own — one
 * kernel per shard and collective, no ring, no host barrier (fine-grained device memory, system-scope flags, every wait bounded: a
 * time-out is reported as an error and leaves the group unusable); buffers beyond the receive area take the LOCAL reducer.  Never
 * chosen by AUTO.  EXPERIMENTAL across distinct devices: that branch has never run on a multi-GPU node, so a P2P request with distinct
 * device ids is refused (DSOPP_HIP_ERR_INVALID_ARGUMENT) unless the process sets DSOPP_HIP_P2P_EXPERIMENTAL=1; with all shards on one
 * device (what the one-GPU tests execute) it needs no opt-in.
 * dsopp_hip_window_group_size reports the transport in use.  A group of one shard is a plain window.
 * ---------------------------------------------------------------------------------------------------------------- */
enum { DSOPP_HIP_TRANSPORT_AUTO = 0, DSOPP_HIP_TRANSPORT_RCCL = 1, DSOPP_HIP_TRANSPORT_LOCAL = 2, DSOPP_HIP_TRANSPORT_P2P = 3 };
typedef struct dsopp_hip_window_group dsopp_hip_window_group;
typedef struct dsopp_hip_pyramid_group dsopp_hip_pyramid_group;
typedef struct dsopp_hip_depth_maps dsopp_hip_depth_maps;

int dsopp_hip_window_group_create(const dsopp_hip_options *options, const int32_t *device_ids, int32_t n, int32_t transport,
                                  dsopp_hip_window_group **out);
void dsopp_hip_window_group_destroy(dsopp_hip_window_group *g);
int dsopp_hip_window_group_size(const dsopp_hip_window_group *g, int32_t *n, int32_t *transport);
/* introspection: the shard's own window (owned by the group; for read-only calls and tests) and its device */
int dsopp_hip_window_group_shard(dsopp_hip_window_group *g, int32_t shard, dsopp_hip_window **window, int32_t *device);

/* the keyframe's image pyramid on every device of the group (PixelDataFrame is one host object in the reference; here one
 * device-resident copy per distinct device, each built on its own device from the same u8 image / adopted host levels) */
int dsopp_hip_pyramid_group_create(dsopp_hip_window_group *g, int width, int height, int levels, dsopp_hip_pyramid_group **out);
void dsopp_hip_pyramid_group_destroy(dsopp_hip_pyramid_group *pg);
int dsopp_hip_pyramid_group_build(dsopp_hip_pyramid_group *pg, const uint8_t *image_host, const double *lut256, const uint8_t *vignetting_host);
int dsopp_hip_pyramid_group_set_level(dsopp_hip_pyramid_group *pg, int level, const double *pixelinfo_host);
int dsopp_hip_pyramid_group_set_mask(dsopp_hip_pyramid_group *pg, int level, const uint8_t *mask_host);
int dsopp_hip_pyramid_group_get(dsopp_hip_pyramid_group *pg, int32_t shard, dsopp_hip_pyramid **pyramid);

/* pushFrame / LocalFrame landmark copy / residual lists / updateLocalFrame flags — as the dsopp_hip_window_ calls of the same name;
 * landmark arrays and status lists are the WHOLE keyframe's (the group deals them out) */
int dsopp_hip_window_group_push_frame(dsopp_hip_window_group *g, int32_t frame_id, int64_t timestamp, const dsopp_hip_pyramid_group *pyramids,
                                      int level, const double intrinsics[4], const double T_world_agent[7], double exposure_time,
                                      const double affine_brightness[2], int fixed, int is_marginalized);
int dsopp_hip_window_group_set_landmarks(dsopp_hip_window_group *g, int32_t frame_id, int32_t n_total, const double *uv, const double *idepth,
                                         const double *patch, const uint8_t *flags);
int dsopp_hip_window_group_set_connection(dsopp_hip_window_group *g, int32_t reference_id, int32_t target_id, int32_t n, const uint8_t *statuses);
int dsopp_hip_window_group_mark_frame_marginalized(dsopp_hip_window_group *g, int32_t frame_id);
int dsopp_hip_window_group_num_frames(dsopp_hip_window_group *g, int32_t *n);
int dsopp_hip_window_group_frame_ids(dsopp_hip_window_group *g, int32_t capacity, int32_t *ids, int32_t *n);
int dsopp_hip_window_group_num_landmarks(dsopp_hip_window_group *g, int32_t frame_id, int32_t *n);
/* solve(number_of_threads) and the stage entry points (PBA_INT/eigen_photometric_bundle_adjustment_problem.hpp:290-402) */
int dsopp_hip_window_group_solve(dsopp_hip_window_group *g, double *energy, int32_t *iterations, int32_t *n_valid);
int dsopp_hip_window_group_optimize(dsopp_hip_window_group *g, double *energy, int32_t *iterations, int32_t *n_valid);
int dsopp_hip_window_group_begin(dsopp_hip_window_group *g);
int dsopp_hip_window_group_calculate_energy(dsopp_hip_window_group *g, double *energy, int32_t *n_valid);
int dsopp_hip_window_group_linearize(dsopp_hip_window_group *g);
int dsopp_hip_window_group_get_system(dsopp_hip_window_group *g, double *H_pp, double *b_pp, double *H_schur, double *b_schur);
int dsopp_hip_window_group_calculate_step(dsopp_hip_window_group *g, double lambda, double *step);
int dsopp_hip_window_group_accept_step(dsopp_hip_window_group *g, double *state_sq, double *step_sq);
int dsopp_hip_window_group_reject_step(dsopp_hip_window_group *g);
int dsopp_hip_window_group_update_point_statuses(dsopp_hip_window_group *g);
/* updateFrame / getPose / getAffineBrightness read-back; landmark arrays come back in the keyframe's own landmark order */
int dsopp_hip_window_group_get_frame_state(dsopp_hip_window_group *g, int32_t frame_id, double T0[7], double ab0[2], double eps[8], double step[8]);
int dsopp_hip_window_group_get_pose(dsopp_hip_window_group *g, int32_t frame_id, double T_world_agent[7], double affine_brightness[2]);
int dsopp_hip_window_group_get_landmarks(dsopp_hip_window_group *g, int32_t frame_id, double *idepth, double *idepth_step, double *inv_hessian_idepth,
                                         double *b_idepth, double *relative_baseline, int32_t *n_inliers, uint8_t *flags_out, double *hpib);
int dsopp_hip_window_group_get_frame_update(dsopp_hip_window_group *g, int32_t frame_id, double *idepth, double *inv_hessian_idepth,
                                            double *relative_baseline, int32_t *n_inliers, uint8_t *flags_out, int32_t n_targets,
                                            const int32_t *target_ids, uint8_t *statuses);
int dsopp_hip_window_group_get_residuals(dsopp_hip_window_group *g, int32_t reference_id, int32_t target_id, int32_t n, uint8_t *status,
                                         uint8_t *candidate, double *energy);
int dsopp_hip_window_group_get_marginalized(dsopp_hip_window_group *g, double *H, double *b, double *energy, int32_t *size);
int dsopp_hip_window_group_get_covariance(dsopp_hip_window_group *g, int32_t reference_id, int32_t target_id, double cov[36]);
/* the class observations, as the dsopp_hip_window_ calls of the same name: every shard counts for its own landmarks, the getters
 * interleave.  The class image is replicated with the pyramid: dsopp_hip_pyramid_group_set_semantics runs
 * dsopp_hip_pyramid_set_semantics on every pyramid of the group, which must all live on the semantics object's device (a group over
 * several devices sets each device's pyramid — dsopp_hip_pyramid_group_get — with that device's own object). */
int dsopp_hip_pyramid_group_set_semantics(dsopp_hip_pyramid_group *pg, const dsopp_hip_semantics *s, const uint8_t *class_image_host);
int dsopp_hip_window_group_add_semantic_observations(dsopp_hip_window_group *g, int32_t n, const int32_t *marginalized_frame_ids);
int dsopp_hip_window_group_get_semantic_observations(dsopp_hip_window_group *g, int32_t frame_id, uint8_t *hist);
int dsopp_hip_window_group_get_semantic_types(dsopp_hip_window_group *g, int32_t frame_id, const uint64_t *weights256, uint8_t *type);
/* createReferenceDepthMaps over all shards: the level-0 splat planes are summed across the shards, the maps returned live on
 * device_ids[0] (where the tracker's aligner runs); refill needs maps this group created */
int dsopp_hip_window_group_create_reference_depth_maps(dsopp_hip_window_group *g, int32_t levels, dsopp_hip_depth_maps **out);
int dsopp_hip_window_group_refill_reference_depth_maps(dsopp_hip_window_group *g, dsopp_hip_depth_maps *maps);
/* settings / measurement aids, as the dsopp_hip_window_ calls of the same name */
int dsopp_hip_window_group_set_lm_mode(dsopp_hip_window_group *g, int mode);
int dsopp_hip_window_group_set_deterministic(dsopp_hip_window_group *g, int enable);
int dsopp_hip_window_group_set_max_iterations(dsopp_hip_window_group *g, int32_t max_iterations);
int dsopp_hip_window_group_snapshot(dsopp_hip_window_group *g);
int dsopp_hip_window_group_restore(dsopp_hip_window_group *g);
int dsopp_hip_window_group_optimize_repeated(dsopp_hip_window_group *g, int32_t iterations_target, int32_t *iterations_done, double *last_energy);
int dsopp_hip_window_group_last_solve_ms(dsopp_hip_window_group *g, float *ms);

/* the Levenberg-Marquardt loop of solve() alone (firstEstimateJacobians + levenberg_marquardt_algorithm::solve,
 * PROB_SRC/eigen_photometric_bundle_adjustment.cpp:83-86) without the post-processing (relinearise, covariance, statuses).
 * One loop body = one Gauss-Newton iteration = linearize + calculateStep + calculateEnergy + accept/reject. */
int dsopp_hip_window_optimize(dsopp_hip_window *w, double *energy, int32_t *iterations, int32_t *n_valid);
/* the same split in two for callers that drive several independent windows from one host thread (a mapping server with many
 * sessions per GPU): _async enqueues the whole LM loop on the window's stream and returns, _wait is the one host
 * synchronisation and returns the results.  One window is latency-bound (three dependent launches per iteration), so
 * windows on different streams overlap: 8 C1 windows reach ~3x the single-window rate on one MI355X (bench.py,
 * "concurrent_windows").  No other call on this window between the two. */
int dsopp_hip_window_optimize_async(dsopp_hip_window *w);
int dsopp_hip_window_optimize_wait(dsopp_hip_window *w, double *energy, int32_t *iterations, int32_t *n_valid);
/* 0 (default): fused device-side LM loop — 3 launches per Gauss-Newton iteration, one read-back per solve;
 * 1: control flow on the host through the stage entry points (one small read-back per energy evaluation).  Same arithmetic in
 * both; 1 is kept for debugging and as the parity cross-check of the fused control logic.  Any other value:
 * DSOPP_HIP_ERR_INVALID_ARGUMENT, the mode stays as it was */
int dsopp_hip_window_set_lm_mode(dsopp_hip_window *w, int mode);
/* Summation order of the reduced normal equations inside the fused LM loop.  0 (default): windows of up to 192 chunks of 64
 * landmarks accumulate H_schur with fp64 atomics (fewest launches; the sum order, hence the last bits, vary from run to run — the
 * reference's own reduction under a mutex, hessian_block_evaluation.hpp:101-145, has the same property), larger windows use the
 * two-stage build (per-workgroup partial systems, then one ordered sum per entry: no atomics, bit-reproducible, and faster there).
 * 1: the two-stage build at every size — the fused LM loop (lm_mode 0, the default), the host-driven loop (lm_mode 1) and the stage
 * entry point dsopp_hip_window_linearize are then bit-reproducible from run to run, at the cost of two more launches per Gauss-Newton
 * iteration.  Not covered: the fold-in of marginalised landmarks inside push_frame, which keeps the atomic accumulation. */
int dsopp_hip_window_set_deterministic(dsopp_hip_window *w, int enable);
/* TrustRegion...Options::max_iterations of an existing window */
int dsopp_hip_window_set_max_iterations(dsopp_hip_window *w, int32_t max_iterations);
/* Measurement aid (bench.py): repeats { dsopp_hip_window_restore; dsopp_hip_window_optimize } from the snapshot until exactly
 * `iterations_target` Gauss-Newton iterations have run (the last solve's max_iterations is capped accordingly, then the
 * window's setting is put back).  Same work as calling the two entry points in a loop, without the caller's per-call
 * overhead between solves; every solve still ends with its own read-back + stream synchronisation. */
int dsopp_hip_window_optimize_repeated(dsopp_hip_window *w, int32_t iterations_target, int32_t *iterations_done, double *last_energy);

/* device-side snapshot / restore of the mutable solver state (poses, affine, idepths, flags, connection statuses);
 * device-to-device copies only.  Lets a caller re-run a solve from the same starting point (benchmark loops, the
 * tracker's re-tracking tries) without re-uploading the window.  The class observations of
 * dsopp_hip_window_add_semantic_observations are not part of it: neither call touches them. */
int dsopp_hip_window_snapshot(dsopp_hip_window *w);
int dsopp_hip_window_restore(dsopp_hip_window *w);

/* timing / introspection for bench.py */
int dsopp_hip_window_last_solve_ms(dsopp_hip_window *w, float *ms); /* HIP-event time of the last LM loop */
enum {
  DSOPP_HIP_KERNEL_PAIR_SETUP = 0,
  DSOPP_HIP_KERNEL_FEJ,
  DSOPP_HIP_KERNEL_SWEEP_LINEARIZE,
  DSOPP_HIP_KERNEL_SWEEP_ENERGY,
  DSOPP_HIP_KERNEL_SCHUR,
  DSOPP_HIP_KERNEL_ASSEMBLE,
  DSOPP_HIP_KERNEL_ASSEMBLE_SOLVE,
  DSOPP_HIP_KERNEL_BACKSUB,
  DSOPP_HIP_KERNEL_ENERGY_REDUCE,
  DSOPP_HIP_KERNEL_ACCEPT,
  DSOPP_HIP_KERNEL_SWEEP_LINEARIZE_LOOP, /* the linearisation sweep as the fused LM loop runs it: back-substitution of the pending step
                                          * (calculateIdepths) + linearisation at the candidate state in one pass */
  DSOPP_HIP_NUM_KERNEL_CLASSES
};
/* when enabled every kernel launch is bracketed by HIP events on the window's stream; get_profile returns the summed
 * device time and launch count of one kernel class since profiling was (re-)enabled */
int dsopp_hip_window_set_profiling(dsopp_hip_window *w, int enable);
int dsopp_hip_window_get_profile(dsopp_hip_window *w, int kernel_class, double *total_ms, int64_t *launches);
const char *dsopp_hip_kernel_class_name(int kernel_class);
/* average duration (microseconds) of `repeats` back-to-back launches of one kernel class at the window's current state,
 * bracketed by ONE pair of HIP events on the window's stream (amortises the ~5 us an event pair costs around a single
 * short kernel).  Supported: SWEEP_LINEARIZE, SWEEP_LINEARIZE_LOOP, SWEEP_ENERGY, SCHUR, ASSEMBLE_SOLVE.  The window state is
 * left unchanged. */
int dsopp_hip_window_time_kernel(dsopp_hip_window *w, int kernel_class, int repeats, double *avg_us);

/* ---- reference depth maps of the newest keyframe (row a21) ----
 * createReferenceDepthMaps (src/tracker/tracker/src/create_depth_maps.cpp:124-147) on the device, from the window's own
 * state: the active landmarks of every older keyframe (connection status kOk towards the newest keyframe, not outlier, not
 * marginalized — :36-38) are reprojected into the newest keyframe and splatted with weight sqrt(1e-3 / (variance + 1e-12))
 * (:51-53; variance = H_dd^-1 of the last linearisation when estimate_uncertainty, else 1e-5 —
 * PROB_SRC/photometric_bundle_adjustment.cpp:252-254), sum-pooled to `levels` pyramid levels (:70-88) and dilated (:90-122).
 * The maps stay in HBM; dsopp_hip_aligner_push_reference_depth_maps hands a level to the tracker without a host round trip. */
/* (typedef struct dsopp_hip_depth_maps dsopp_hip_depth_maps: declared with the window group above) */
int dsopp_hip_window_create_reference_depth_maps(dsopp_hip_window *w, int32_t levels, dsopp_hip_depth_maps **out);
void dsopp_hip_depth_maps_destroy(dsopp_hip_depth_maps *m);
int dsopp_hip_depth_maps_level_size(const dsopp_hip_depth_maps *m, int32_t level, int32_t *width, int32_t *height);
/* copies one level to the host: two row-major H x W planes (energy::problem::DepthMap::map(x, y).{idepth, weight}) */
/* the same into an existing object of the same image size (the tracker keeps ONE reference_frame_depth_map_ and reassigns it
 * after every keyframe, monocular_tracker.cpp:465,509): no allocation, cached reference points are invalidated */
int dsopp_hip_window_refill_reference_depth_maps(dsopp_hip_window *w, dsopp_hip_depth_maps *maps);
/* calculateMeanSquareOpticalFlow (src/tracker/tracker/src/monocular_tracker.cpp:104-134) of one level of the device-resident
 * maps — the parallax measure the keyframe strategy reads for every tracked frame (:474-479: once for t_t_r, once for t_t_r
 * with the rotation removed) — for n_transforms <= 4 relative poses T_target_reference (7 each) in one pass.
 * flow[i] = sqrt(mean |bearing(pixel) - bearing(reprojection)|^2) over the map's pixels that reproject (NaN for none). */
int dsopp_hip_depth_maps_mean_square_optical_flow(const dsopp_hip_depth_maps *m, int32_t level, const double intrinsics[4], int32_t n_transforms,
                                                  const double *T_target_reference, double *flow);
int dsopp_hip_depth_maps_get_level(const dsopp_hip_depth_maps *m, int32_t level, double *idepth_sum, double *weight);

/* ---- depth estimation of immature landmarks (row f-1) ----
 * DepthEstimation::estimate (src/tracker/depth_estimators/src/depth_estimation.cpp:363-381) for the immature landmarks of one
 * keyframe against level `level` (0 in the tracker, monocular_tracker.cpp:98-100) of a new frame's device pyramid:
 * epipolar segment (epipolar_line_builder_pinhole_se3.hpp:296-372), discrete search (findBest, :36-76), sub-pixel
 * refinement on the epipolar tangent (refine, :184-221), uniqueness, error model and re-triangulated [idepth_min, idepth_max]
 * (estimateLandmark, :223-357).  T_target_reference = T_new_frame^-1 * T_keyframe.  The landmark arrays are the
 * struct-of-arrays view of track::landmarks::ImmatureTrackingLandmark and are updated in place:
 * status: 0 good, 1 out of boundary, 2 outlier, 3 skipped, 4 ill conditioned, 5 uninitialized, 6 delete
 * (immature_tracking_landmark.hpp:14-22).  One wavefront per landmark. */
/* the same on a device-resident landmark set (the immature landmarks of a keyframe persist over many frames: only their
 * estimator state changes).  create() initialises the state to the ImmatureTrackingLandmark constructor defaults;
 * estimate() is asynchronous on the set's stream; upload / download move the state (any pointer may be NULL). */
typedef struct dsopp_hip_immature_set dsopp_hip_immature_set;
int dsopp_hip_immature_set_create(int device, void *stream, int32_t n, const double *projection, const double *direction, const double *patch,
                                  const double *gradient, dsopp_hip_immature_set **out);
void dsopp_hip_immature_set_destroy(dsopp_hip_immature_set *s);
int dsopp_hip_immature_set_upload_state(dsopp_hip_immature_set *s, const double *idepth_min, const double *idepth_max, const double *uniqueness,
                                        const double *search_pixel_interval, const uint8_t *status, const uint8_t *traced);
int dsopp_hip_immature_set_download_state(dsopp_hip_immature_set *s, double *idepth_min, double *idepth_max, double *uniqueness,
                                          double *search_pixel_interval, uint8_t *status, uint8_t *traced);
int dsopp_hip_immature_set_estimate(dsopp_hip_immature_set *s, const dsopp_hip_pyramid *target_pyramid, int level, const double intrinsics[4],
                                    const double T_target_reference[7], double reference_exposure, const double reference_affine[2],
                                    double target_exposure, const double target_affine[2], double sigma_huber_loss);
/* estimateDepths of the tracker (monocular_tracker.cpp:74-102: the estimator runs for EVERY keyframe of the window on every
 * frame) as one call and one launch over n_sets sets: T_target_reference 7 per set, reference_exposure 1 per set,
 * reference_affine 2 per set.  Runs on the first set's stream; asynchronous when all sets share it. */
int dsopp_hip_immature_sets_estimate(int32_t n_sets, dsopp_hip_immature_set *const *sets, const dsopp_hip_pyramid *target_pyramid, int level,
                                     const double intrinsics[4], const double *T_target_reference, const double *reference_exposure,
                                     const double *reference_affine, double target_exposure, const double target_affine[2],
                                     double sigma_huber_loss);
/* one-shot form over host arrays (temporary set: upload, estimate, download) */
int dsopp_hip_estimate_depths(const dsopp_hip_pyramid *target_pyramid, int level, const double intrinsics[4],
                              const double T_target_reference[7], double reference_exposure, const double reference_affine[2],
                              double target_exposure, const double target_affine[2], double sigma_huber_loss, int32_t n,
                              const double *projection /* 2n */, const double *direction /* 3n */, const double *patch /* 8n */,
                              const double *gradient /* 2n */, double *idepth_min, double *idepth_max, double *uniqueness,
                              double *search_pixel_interval, uint8_t *status, uint8_t *traced);

/* the input planes of a set as create() took them (projection 2n, direction 3n, patch 8n, gradient 2n); any pointer may be NULL.
 * What fills the host copy of a set built on the device by dsopp_hip_immature_set_create_from_features: the keyframe keeps its
 * ImmatureTrackingLandmark objects on the host (immature_tracking_landmark.hpp:26-106), and the host mirror's activator reads
 * their projection and patch (ImmatureLandmarkView, dsopp_amd/host/dsopp_hip_solvers.hpp). */
int dsopp_hip_immature_set_download_inputs(const dsopp_hip_immature_set *s, double *projection, double *direction, double *patch,
                                           double *gradient);

/* ---- tracking-feature extraction (the candidate pixels of a new keyframe) ----
 * features::SobelTrackingFeaturesExtractor (src/features/src/sobel_tracking_features_extractor.cpp:70-134), the extractor
 * camera_fabric.cpp:103-123 builds when nothing else is configured, run once per keyframe on the 8-bit grey image
 * (camera_features.cpp:36-41).  Stateful as the reference: the first extract() fixes the gradient-norm threshold (the
 * quantile_level quantile of |Sx| + |Sy|) and the window size sqrt(W * H * (1 - q) / density); every later call adapts the
 * threshold.  The `eigen` extractor (DSO's pixel selector) is the second kind of the same handle: see
 * dsopp_hip_feature_extractor_create_eigen.
 * width, height >= 16; point_density_for_detector > 0; quantile_level in (0, 1), else DSOPP_HIP_ERR_INVALID_ARGUMENT.
 * Before the first extract the state reads initialized 0, threshold 0, window size 15 (tracking_features_extractor.hpp:51). */
typedef struct dsopp_hip_feature_extractor dsopp_hip_feature_extractor;
int dsopp_hip_feature_extractor_create(int device, void *stream, int width, int height, double point_density_for_detector, double quantile_level,
                                       dsopp_hip_feature_extractor **out);
/* features::EigenTrackingFeaturesExtractor (src/features/src/eigen_tracking_features_extractor.cpp:432-469), the extractor
 * camera_fabric.cpp:120-123 builds for `features_extractor: type: eigen`: DSO's pixel selector over the extractor's own raw pyramid
 * (5 levels, identity LUT, no vignette), a (W/32) x (H/32) gradient threshold map, 16 directions picked by a fixed random pattern
 * (srand(3141592)) and a window size (current_potential_, 15 before the first call) adapted by at most one re-sampling per call; a
 * final random reduction when the list is still too long.  The list is in emission order, neither shuffled nor truncated.  The
 * same handle as the Sobel extractor: set_mask, extract, get_state, destroy and dsopp_hip_immature_set_create_from_features serve
 * both kinds, with the same capacity contract.  For this kind get_state reads threshold 0, window size = current_potential_, and
 * found_last = the emissions of the last pass before the reduction.  width, height >= 32 and point_density_for_detector > 0, else
 * DSOPP_HIP_ERR_INVALID_ARGUMENT.  The projection |cos dx + sin dy| rounds each product and the sum (no fused multiply-add); a
 * reference compiled with FMA contraction may differ where that rounding decides a comparison. */
int dsopp_hip_feature_extractor_create_eigen(int device, void *stream, int width, int height, double point_density_for_detector,
                                             dsopp_hip_feature_extractor **out);
/* the passes of the last extract of an eigen extractor (1 or 2), the window size and emission count of each (0 for a pass not run),
 * and the number of top windows whose emission count depended on the directions and were walked in order; DSOPP_HIP_ERR_STATE for a
 * Sobel extractor.  Any pointer may be NULL. */
int dsopp_hip_feature_extractor_get_eigen_stats(const dsopp_hip_feature_extractor *ex, int32_t *passes, int32_t potentials[2], int32_t found[2],
                                                int32_t *chained_windows);
/* The eigen extractor's random pattern: srand(3141592), then width * height bytes (uint8_t)rand() of glibc's generator, written out in
 * the library (no libc state is touched).  Needs no device. */
int dsopp_hip_eigen_random_pattern(int width, int height, uint8_t *out);
void dsopp_hip_feature_extractor_destroy(dsopp_hip_feature_extractor *ex);
/* the camera mask the extractor erodes (CameraMask::getEroded(4).getEroded(3), camera_mask.cpp:20-29: a 15 x 15 erosion whose
 * image edge never erodes) and uses for every later extract; NULL = all pixels valid (CameraMask(rows, cols)).  W x H bytes,
 * non-zero = valid. */
int dsopp_hip_feature_extractor_set_mask(dsopp_hip_feature_extractor *ex, const uint8_t *mask_host);
/* SobelTrackingFeaturesExtractor::extract(image, mask): the first pixel (raster order) with |Sx| + |Sy| above the threshold and
 * inside the eroded mask of every window, in window order, shuffled by std::shuffle with a fresh std::default_random_engine and cut
 * to (long)point_density_for_detector.  xy = (x, y) per feature (2 * capacity doubles), *n = their number.  A capacity below the
 * result returns DSOPP_HIP_ERR_CAPACITY with *n = the number needed and the extractor state unchanged.  One deliberate deviation:
 * where the reference's threshold update is undefined (no feature found: an integer division by zero; a non-finite or
 * out-of-range quotient) the threshold is kept.  The list stays on the device for dsopp_hip_immature_set_create_from_features. */
int dsopp_hip_feature_extractor_extract(dsopp_hip_feature_extractor *ex, const uint8_t *image_host, int32_t capacity, double *xy, int32_t *n);
/* extract() of the undistorted 8-bit image that `p` kept from its last dsopp_hip_pyramid_build_undistorted — the reference extracts
 * from the undistorted frame (camera.cpp:70, src/features/src/camera_features.cpp:36-41) — read on the device behind the pyramid's
 * build, with no second upload.  Both kinds of extractor; lists, capacity contract and state as extract() of the same image from
 * the host.  DSOPP_HIP_ERR_INVALID_ARGUMENT when the pyramid's last build was not build_undistorted, or its size or device is not
 * the extractor's. */
int dsopp_hip_feature_extractor_extract_from_pyramid(dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *p, int32_t capacity, double *xy,
                                                     int32_t *n);
/* The extractor's mask from the level-0 mask bytes that `p` kept from its last dsopp_hip_pyramid_set_semantics (the per-frame camera
 * mask the reference hands to extract(), camera_features.cpp:36-41,71-74): eroded on the device for both kinds of extractor, behind
 * the pyramid's ready event, with no host copy; the call only enqueues.  DSOPP_HIP_ERR_INVALID_ARGUMENT when the pyramid never had
 * set_semantics, or its size or device is not the extractor's. */
int dsopp_hip_feature_extractor_set_mask_from_pyramid(dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *p);
/* the extractor's state after the last extract (any pointer may be NULL): initialized_, grad_norm_threshold_, current_potential_
 * (the window size), point_density_for_detector_ (lowered by the first call when the window would be below one pixel), and the
 * number of windows with a hit before the truncation */
int dsopp_hip_feature_extractor_get_state(const dsopp_hip_feature_extractor *ex, int32_t *initialized, int32_t *grad_norm_threshold,
                                          int32_t *window_size, double *point_density, int32_t *found_last);
/* The permutation std::shuffle(first, first + n, std::default_random_engine{}) applies (libstdc++), written as perm[i] = the
 * original index at position i: the reference's shuffle of step :127.  It states the reference's ordering for tests and
 * callers and computes nothing the device would; the one entry point of this section that needs no device. */
int dsopp_hip_features_shuffle_order(int32_t n, int32_t *perm);
/* buildFeatures (src/tracker/tracker/internal/tracker/build_features.hpp:20-32: features outside insideCameraROI dropped, order
 * kept; direction = ((x - cx) / fx, (y - cy) / fy, 1) with the inverse focal lengths precomputed) + pushImmatureLandmarks
 * (src/track/frames/src/active_keyframe.cpp:95-112: patch = level-0 intensities at the 8 pattern pixels, gradient = the sum of their
 * (dI/dx, dI/dy) in the image scalar) for the last extract of `ex`, read from level 0 of `pyramid` (f64 or f32, the extractor's size,
 * same device) after its build: a new set in the ImmatureTrackingLandmark constructor state, *n landmarks, no host round trip of
 * the patches.  intrinsics = (fx, fy, cx, cy). */
int dsopp_hip_immature_set_create_from_features(int device, void *stream, const dsopp_hip_feature_extractor *ex, const dsopp_hip_pyramid *pyramid,
                                                const double intrinsics[4], dsopp_hip_immature_set **out, int32_t *n);

/* ---- activation of immature landmarks (row f-3) ----
 * LandmarksActivator<SE3, PinholeCamera, PixelMap, 1, REFINE>::activate (src/tracker/landmarks_activator/src/landmarks_activator.cpp:351-391),
 * called once per new keyframe after pushNewKeyframe and before the keyframe enters the bundle adjustment
 * (monocular_tracker.cpp:491-497).  track.activeFrames() = the listed window keyframes (oldest first; poses, affine
 * brightness, exposure, level-0 images and active landmarks are the window's own) + the newest keyframe given explicitly.
 *   1. reprojectActivePoints (:51-87) into the newest keyframe at pyramid level 1, number_of_active_points;
 *   2. recalculateMinDistanceToNeighbor (:29-39): *min_distance_to_neighbor is LandmarksActivator::min_distance_to_neighbor_ (in/out);
 *   3. activationStatus (:89-126) of every immature landmark in keyframe / landmark order, the greedy sparsity test
 *      haveNoNeighbors (:41-49) through a uniform grid (identical result to the sequential O(n^2) loop);
 *   4. refine != 0: optimizeImmatureLandmark (:279-311), a 3-iteration LM on the inverse depth over all other keyframes.
 * activation_status[k][i]: 0 activate, 1 skip, 2 delete (ActiveKeyframe::ImmatureLandmarkActivationStatus, active_keyframe.hpp:40-44);
 * idepth[k][i] = landmark.idepth() after the call (refined for activated landmarks).  Either array (or an entry) may be NULL.
 * The sets are updated the way applyImmatureLandmarkActivationStatuses (active_keyframe.cpp:209-239) leaves the immature
 * landmarks: idepth_min = idepth_max = refined value for activated ones, status := delete for activated and deleted ones.
 * Creating the ActiveTrackingLandmark objects (and dsopp_hip_window_set_landmarks for them) stays with the caller. */
typedef struct dsopp_hip_activation_result {
  int32_t number_of_active_points;
  int32_t n_activated, n_skipped, n_deleted;
  int32_t selection_rounds; /* parallel rounds the greedy selection needed */
  double min_distance_to_neighbor;
} dsopp_hip_activation_result;
int dsopp_hip_window_activate_landmarks(dsopp_hip_window *w, int32_t n_keyframes, const int32_t *frame_ids,
                                        dsopp_hip_immature_set *const *immature /* n_keyframes, entries may be NULL */,
                                        const dsopp_hip_pyramid *newest_pyramid, const double T_world_newest[7], double exposure_newest,
                                        const double affine_newest[2], int32_t number_of_desired_points, double *min_distance_to_neighbor,
                                        int32_t refine, double sigma_huber_loss, uint8_t *const *activation_status, double *const *idepth,
                                        dsopp_hip_activation_result *result);

/* ---- the keyframes and landmarks that leave the window (marginalisation strategy) ----
 * marginalize(solver, track, marginalizer) — src/tracker/tracker/src/monocular_tracker.cpp:308-321, called at :505 after every
 * bundle adjustment of a new keyframe — decided on the window's own state: landmark flags, n_inliers, the connection statuses towards
 * the newest keyframe, inverse depths, 1 / H_dd, the poses, and the immature sets' estimator state.
 *
 * The counting half of updateFrame: ActiveTrackingLandmark::setNumberOfInlierResidualsInTheLastOptimization
 * (src/track/landmarks/src/active_tracking_landmark.cpp:42-49, called by photometric_bundle_adjustment.cpp:256 for every landmark
 * that is not marginalised) increments numberOfSuccessfulOptimizations() when the landmark had more than 3 inlier residuals.
 * note_optimization does that for every landmark of every frame of the window that is not flagged marginalised, from the window's
 * n_inliers; call it once after each solve (no solve calls it).  The counters live with the frame like the class observations above:
 * rows in the caller's landmark order, allocated by the first call, zero for landmarks appended later, untouched by internal
 * re-ordering and by dsopp_hip_window_snapshot / _restore, released when the frame leaves the window. */
int dsopp_hip_window_note_optimization(dsopp_hip_window *w);
/* numberOfSuccessfulOptimizations() of every landmark of a frame (n_landmarks values, the caller's order; zero before the first note) */
int dsopp_hip_window_get_optimization_counts(dsopp_hip_window *w, int32_t frame_id, int32_t *counts);

/* marginalization_strategy of the tracker's configuration (src/marginalization/src/fabric.cpp):
 * `sparse` = SparseFrameMarginalizationStrategy(minimum_size, maximum_size, maximum_percentage_of_marginalized_points_in_frame),
 * `maximum_size` = MaximumSizeFrameMarginalizationStrategy(maximum_size).  Defaults: sparse, 5, 7, 0.95
 * (test/test_data/tummono/mono.yaml:39-43). */
enum { DSOPP_HIP_MARGINALIZATION_SPARSE = 0, DSOPP_HIP_MARGINALIZATION_MAXIMUM_SIZE = 1 };
typedef struct dsopp_hip_marginalization_options {
  int32_t strategy;
  int32_t minimum_size, maximum_size;
  double maximum_share_marginalized;
} dsopp_hip_marginalization_options;
void dsopp_hip_marginalization_default_options(dsopp_hip_marginalization_options *o);

/* Everything below is indexed by ACTIVE frame: the window's frames that are not flagged marginalised, oldest first
 * (track.activeFrames()); n_active of them. */
typedef struct dsopp_hip_marginalization_result {
  int32_t n_active;
  int32_t active_ids[DSOPP_HIP_MAX_FRAMES]; /* window ids of the active frames */
  int32_t n_selected;
  int32_t selected[DSOPP_HIP_MAX_FRAMES]; /* the strategy's set `to_marginalize`: active indices, ascending */
  int32_t n_marginalized;
  int32_t marginalized_ids[DSOPP_HIP_MAX_FRAMES]; /* window ids of the frames marginalizeFrame() hit, in erase order */
  double scores[DSOPP_HIP_MAX_FRAMES]; /* distance_score of findFramesToMarginalize; NaN where it computes none */
  int32_t n_active_landmarks[DSOPP_HIP_MAX_FRAMES];       /* numberOfActiveAndImmatureLandmarks */
  int32_t n_marginalized_landmarks[DSOPP_HIP_MAX_FRAMES]; /* numberOfMarginalizedLandmarks */
  int32_t n_newly_marginalized, n_newly_outlier;          /* landmarks of the whole window */
} dsopp_hip_marginalization_result;

/* FrameMarginalizationStrategy::marginalize(track) for the window's active frames.
 *
 * sparse (src/marginalization/src/sparse_frame_marginalization_strategy.cpp):
 *  - findFramesWithSmallNumberOfActivePoints (:38-53, counts :16-35): frame i (i + 2 < n_active) joins the set when
 *    kept < (1 - maximum_share_marginalized) * (kept + gone) and n_active - |set| > minimum_size, serially in i; kept = landmarks that
 *    are neither outlier nor marginalised + immature landmarks with readyForActivation(), gone = outlier or marginalised landmarks.
 *  - findFramesToMarginalize (:101-140), only when n_active > maximum_size + |set|: kEps 1e-5, kKeepFramesFromStart 2, kMinFrameAge 1;
 *    score(r) = sqrt(|t_r - t_last|) * sum over t != r of 1 / (kEps + |t_r - t_t|), r and t over the active frames but the last two, the
 *    sum in window order; the first r with score > max_score (from 0) wins, and index 0 joins the set when no score exceeds 0 —
 *    also when every candidate was skipped.  The age test reads camera_frame_ids (the keyframes' frame ids, one per WINDOW frame,
 *    ids >= 0); NULL = the window's own ids.
 *  - marginalizeLandmarks (:56-91), when n_active > 2, for every active frame but the last and every landmark that is neither
 *    marginalised nor outlier: out_of_boundary = the frame is in the set, or the landmark's status towards the last active keyframe is
 *    not kOk; valid = n_inliers >= (minimum_size + 1) / 2 and successful optimisations > 2 * maximum_size; sufficient = successful
 *    optimisations > 0.  out_of_boundary and not sufficient: outlier.  Else out_of_boundary or valid: marginalize().
 *    A landmark without an entry in that connection (the list is shorter than the frame, or there is no connection) counts as not
 *    kOk; the reference's .at() would throw.
 *  - ActiveTrackingLandmark::marginalize() (active_tracking_landmark.cpp:55-63) also marks the landmark outlier when
 *    variance / idepth > 1e-3 or idepth < 0.  As the class observations above, the window reads its own values, in binary64: its
 *    inverse depth and variance = 1 / H_dd (what updateFrame hands the keyframe with estimate_uncertainty, :252), not the keyframe's
 *    copies in Precision, which lag for landmarks whose solved inverse depth went negative or below 1e-8 in magnitude.
 *  - the erase loop (:165-167, ActiveOdometryTrack::marginalizeFrame, src/track/track/src/active_odometry_track.cpp:70-75) erases
 *    the set's indices in ascending order from a list that shrinks as it goes: the second index of a set hits the frame one place
 *    later.  `selected` is the set, `marginalized_ids` the frames hit (an index past the end of the shrunken list, undefined in the
 *    reference, hits nothing).  ActiveKeyframe::marginalize (src/track/frames/src/active_keyframe.cpp:176-184) calls marginalize()
 *    on EVERY landmark of a frame hit, whatever its flags.
 * maximum_size (src/marginalization/src/maximum_size_frame_marginalization_strategy.cpp:16-20): marginalizeFrame(0) until
 * n_active <= maximum_size; `selected` lists the active indices of those oldest frames, no landmark rule but ActiveKeyframe::marginalize.
 *
 * immature: one set per WINDOW frame (entries or the array may be NULL: no immature landmarks); their state is read behind
 * whatever their streams hold.  flags (may be NULL): the new flag byte of every landmark of every window frame, frame after frame in
 * window order, each frame in the caller's landmark order — bit0 marginalised, bit1 outlier; the frames flagged earlier report
 * the bits they have.
 * apply = 0 changes nothing in the window.  apply != 0 leaves the window as one dsopp_hip_window_set_landmarks flag refresh with
 * those bytes would, for every frame that was active (to_marginalize = newly marginalised and not outlier, assigned for each of them),
 * followed by dsopp_hip_window_mark_frame_marginalized for the frames in marginalized_ids: updateLocalFrame of monocular_tracker.cpp
 * :317 and :507.  As in that refresh (PBA_INT/local_frame.hpp:492-497) the outlier bit of a landmark the window already holds only
 * decides to_marginalize; the window's own outlier flags are the solver's.  A second refresh of those frames would clear
 * to_marginalize, as it does in the reference.
 * One launch counts and lets the workgroup that finishes last choose, a second writes the landmarks' flags; nothing waits on the host
 * in between, and one pinned transfer brings everything back. */
int dsopp_hip_window_choose_marginalization(dsopp_hip_window *w, const dsopp_hip_marginalization_options *options,
                                            const int32_t *camera_frame_ids, dsopp_hip_immature_set *const *immature, int32_t apply,
                                            dsopp_hip_marginalization_result *result, uint8_t *flags);

/* ------------------------------------------------------------------------------------------------------------------
 * Two-frame direct image alignment of one pyramid level
 * (replaces EigenPoseAlignment<SE3, PinholeCamera, 1, PixelMap, 1, true>, PROB_SRC/eigen_pose_alignment.cpp:26-329)
 * ---------------------------------------------------------------------------------------------------------------- */
typedef struct dsopp_hip_aligner dsopp_hip_aligner;

typedef struct dsopp_hip_align_result {
  double rmse; /* sqrt(E / n_valid / PatternSize) — eigen_pose_alignment.cpp:328; -1 (kZeroCost) for a known pose */
  double energy;
  int32_t n_valid;
  int32_t iterations;
  double T_world_target[7];
  double affine_brightness[2];
  double covariance[36]; /* tTargetReferenceCovariance — eigen_pose_alignment.cpp:320-323 */
  double H[64];
} dsopp_hip_align_result;

int dsopp_hip_aligner_create(const dsopp_hip_options *options, int device, void *stream, dsopp_hip_aligner **out);
void dsopp_hip_aligner_destroy(dsopp_hip_aligner *a);
/* reset() — PA_INC/pose_alignment.hpp, eigen_pose_alignment.cpp:261-264 */
int dsopp_hip_aligner_reset(dsopp_hip_aligner *a);
/* pushFrame(timestamp, pose, pyramids, masks, depth maps, ...) for the fixed reference frame
 * (PROB_SRC/photometric_bundle_adjustment.cpp:58-74 + LocalFrame depth-map ctor PBA_INT/local_frame.hpp:350-393): every
 * pixel with weight > 0 and idepth_sum/weight >= 1e-6 inside the 4-px border becomes a reference point whose intensity
 * is sampled from the reference pyramid level on the device.  depth maps are H_l x W_l row-major host arrays. */
int dsopp_hip_aligner_push_reference_depth_map(dsopp_hip_aligner *a, int64_t timestamp, const double T_world_agent[7],
                                               const dsopp_hip_pyramid *pyramid, int level, const double intrinsics[4],
                                               const double *idepth_sum, const double *weight, double exposure_time,
                                               const double affine_brightness[2]);
/* same, from device-resident maps (dsopp_hip_window_create_reference_depth_maps): the scan / compaction of the LocalFrame
 * depth-map constructor runs on the device and keeps the reference's row-major point order */
int dsopp_hip_aligner_push_reference_depth_maps(dsopp_hip_aligner *a, int64_t timestamp, const double T_world_agent[7],
                                                const dsopp_hip_pyramid *pyramid, int level, const double intrinsics[4],
                                                const dsopp_hip_depth_maps *maps, double exposure_time, const double affine_brightness[2]);
/* same with an explicit point list (u, v, idepth); intensity sampled on the device.  A point outside the reference camera's ROI
 * (4 <= u <= width - 5, 4 <= v <= height - 5) is kept in the list, never contributes (as in the reference) and is not sampled: its
 * intensity is 0.  A coordinate or inverse depth that is not finite, or beyond 1e15 in magnitude: DSOPP_HIP_ERR_INVALID_ARGUMENT. */
int dsopp_hip_aligner_push_reference_points(dsopp_hip_aligner *a, int64_t timestamp, const double T_world_agent[7],
                                            const dsopp_hip_pyramid *pyramid, int level, const double intrinsics[4], int32_t n,
                                            const double *u, const double *v, const double *idepth, double exposure_time,
                                            const double affine_brightness[2]);
/* pushFrame(timestamp, initial pose, pyramids, masks, ...) for the free target frame (photometric_bundle_adjustment.cpp:131-154) */
int dsopp_hip_aligner_push_target(dsopp_hip_aligner *a, int64_t timestamp, const double T_world_agent_init[7],
                                  const dsopp_hip_pyramid *pyramid, int level, const double intrinsics[4], double exposure_time,
                                  const double affine_brightness[2]);
/* pushKnownPose — eigen_pose_alignment.cpp:268-271 */
int dsopp_hip_aligner_push_known_pose(dsopp_hip_aligner *a, int64_t timestamp, const double T_world_agent[7]);
/* setRotationPrior — eigen_pose_alignment.cpp:254-257: the rotation of t_target_reference is replaced by fitToSO3(R) (3x3
 * row-major, det > 0) at the start of solve (:309-311); reset() clears it (:262), as does a NULL pointer */
int dsopp_hip_aligner_set_rotation_prior(dsopp_hip_aligner *a, const double *R_target_reference);
/* solve -> rmse (or kZeroCost = -1) — eigen_pose_alignment.cpp:275-329 */
int dsopp_hip_aligner_solve(dsopp_hip_aligner *a, dsopp_hip_align_result *result);
/* initializationPoses (src/tracker/tracker/src/monocular_tracker.cpp:136-176): the pose hypotheses estimatePose tries in turn —
 * previous motion, doubled, halved (exp(log/2)), zero motion, the keyframe's pose, then the previous motion perturbed by
 * rotations of 1, 1.5, 2, 2.5 degrees about every axis combination: 5 + 4 * 27 = 113 poses.  T_world_previous / T_world_last are
 * track.getFrame(-2) / (-1); any of the three NULL = fewer than two frames in the track -> the single identity pose.
 * Host arithmetic (no device work); *n receives the count, at most `capacity` poses (7 doubles each) are written. */
int dsopp_hip_initialization_poses(const double T_world_previous[7], const double T_world_last[7], const double T_world_keyframe[7],
                                   int32_t capacity, double *poses, int32_t *n);
/* Coarse-to-fine pose estimation of a new frame against the last keyframe: estimatePose of the tracker
 * (src/tracker/tracker/src/monocular_tracker.cpp:179-245).  For every initialisation in turn (until one succeeds): from the
 * coarsest level of the target pyramid down to level 0 { reset; push the keyframe's depth map of that level; push the target
 * with the current estimate; solve; accept the level when rmse < 2.5 * rmse_last_pose_estimation[level] }.  The camera model
 * of level l is the level-0 one scaled by 2^-l.  rmse_last_pose_estimation (one per level) is updated as the reference
 * does (multiplied by 2.5 when every initialisation failed; then the result of the FIRST initialisation is returned). */
int dsopp_hip_aligner_estimate_pose(dsopp_hip_aligner *a, int64_t reference_time, const double T_world_reference[7],
                                    const dsopp_hip_pyramid *reference_pyramid, const dsopp_hip_depth_maps *reference_depth_maps,
                                    double reference_exposure, const double reference_affine[2], int64_t target_time,
                                    const dsopp_hip_pyramid *target_pyramid, double target_exposure, const double intrinsics[4],
                                    int32_t n_initializations, const double *T_world_target_init, const double affine_init[2],
                                    double *rmse_last_pose_estimation, double T_world_target[7], double affine_brightness[2],
                                    int32_t *success, int32_t *tries, int32_t *lm_iterations);
/* Initialisations estimate_pose evaluates per launch.  The reference tries them one after the other until one passes its per-level
 * energy gates (monocular_tracker.cpp:193-243); they are independent of each other, so up to 8 run concurrently — one per XCD of the
 * device, each with its own exchange buffers — and the lowest-index success is taken: pose, `tries`, `lm_iterations` and the updated
 * rmse_last_pose_estimation are those of the sequential loop.  0 (default): automatic — the first initialisation alone while
 * tracking holds (it succeeds; nothing is computed in vain), 8 at a time as soon as a first try failed in this or the previous call
 * (re-localisation: up to 113 initialisations); 1: strictly one per launch; 2 .. 8: that many per launch from the first one on. */
int dsopp_hip_aligner_set_hypothesis_width(dsopp_hip_aligner *a, int32_t width);
/* 0 (default): the whole LM loop of a solve runs in ONE launch of one workgroup when the reference has at most 16384 points
 * (a launch per iteration costs more than the iteration at that size); 1: always one launch per LM iteration (multi-workgroup).
 * Same state machine and arithmetic on both paths (parity cross-check in tests/test_gpu_tracker.py). */
int dsopp_hip_aligner_set_lm_path(dsopp_hip_aligner *a, int path);
int dsopp_hip_aligner_num_points(dsopp_hip_aligner *a, int32_t *n);

/* ---- the tracker's debug views (row o-1) ----
 * The two images MonocularTracker::tick pushes to its camera_output_interface_ (the viewer), as interleaved 8-bit BGR of width x height:
 *   debugCurrentFrame(features), every frame                                   src/tracker/tracker/src/monocular_tracker.cpp:323-333, 485-487
 *   debugCurrentKeyframe(features, depth_map[0], maximum_visualized_idepth_)   src/tracker/tracker/src/monocular_tracker.cpp:335-374, 511-514
 * The arithmetic is stated here as the library's own (parity with OpenCV's circle rasteriser and colour table is NOT pinned: both are
 * creation parameters, see below).  tests/debug_views_model.py is the NumPy statement the kernels are held to byte for byte.
 *
 * Frame view.  g = the grey byte, m = (the level-0 mask byte is 0; a pyramid's mask lane is 0).  BGR = (g, g, g) where !m and
 * (max(g - 128, 0), max(g - 128, 0), g) where m: `debug - ((mask == 0) - Scalar(0, 0, 255)) / 2` in saturating 8-bit arithmetic with
 * 127.5 rounded to 128.  Without a mask every pixel is valid and the view is plain grey.
 *
 * Keyframe view, over the level-0 map {idepth_sum, weight} (two row-major height x width planes, as dsopp_hip_depth_maps_get_level
 * returns them) and the state M (the tracker's maximum_visualized_idepth_, 0 = unset, 0 at creation):
 *   1 the cells with idepth_sum > 0 qualify; q = idepth_sum / weight; avg = (sum of q) / cells.  (A map the library fills has weight > 0
 *     wherever idepth_sum > 0; a caller's cell with idepth_sum > 0 and weight 0 has q = inf, as in the reference.)  The sum is taken in a
 *     FIXED order, whatever the device does: with i = y * width + x and q = 0.0 for a cell that does not qualify,
 *       chunk b (4096 cells), thread t < 256:  s = 0; for k = 0 .. 15: s += q[4096 b + 256 k + t]
 *       64 consecutive threads (a wave):       for off = 32, 16, 8, 4, 2, 1: s[l] += s[l + off], l < off; the wave's sum is s[0]
 *       the chunk:                             ((wave 0 + wave 1) + wave 2) + wave 3
 *     and the chunks' sums are added the same way: thread j < 256 adds chunks j, j + 256, j + 512, ... in that order, then the waves and
 *     the four wave sums as above.
 *   2 if M == 0: M = 2 avg.  Then M = 0.9 M + 0.1 (2 avg): binary64, single operations, the two products first.
 *   3 a qualifying cell's level = rint(clamp((255 q) / M, 0, 255)) with the NEW M: half to even, a NaN gives 0.
 *   4 the cells are painted in raster order (y outer, x inner), each as the stencil's footprint around (x, y), clipped to the image,
 *     later over earlier.  (The device gathers instead: a pixel p takes, among the cells p - offset of the set stencil taps, the
 *     occupied one with the largest (y, x) — the same image, in any execution order.)
 *   5 a covered pixel is colormap[level of the last footprint over it], every other pixel (g, g, g).
 * With NO qualifying cell the reference divides 0 by 0 and its M is NaN from then on.  The library instead leaves M as it is, returns the
 * plain grey view and reports cells = 0.
 *
 * create: colormap_bgr = 256 x {B, G, R}, the colour of every level; NULL = the library's jet, x = v / 255,
 *   r = clamp(1.5 - |4 x - 3|, 0, 1), g = clamp(1.5 - |4 x - 2|, 0, 1), b = clamp(1.5 - |4 x - 1|, 0, 1), each channel rint(255 c)
 * — NOT claimed to be OpenCV's COLORMAP_JET table: a caller that links OpenCV passes cv::applyColorMap of a 0 .. 255 ramp.
 * stencil = 7 x 7 bytes, a circle's footprint: a nonzero byte at (dy + 3, dx + 3) means the circle at c covers c + (dx, dy); NULL =
 * dx^2 + dy^2 <= 9 (29 pixels); need not be symmetric (a caller that links OpenCV passes one cv::circle of radius 3 on a 7 x 7 image).
 * `stream` NULL = a stream of the object's own.  All buffers are sized here from width x height; only the staging planes of
 * keyframe_planes are allocated by its first call.
 *
 * frame: blocking.  Reads the 8-bit grey image `pyramid` keeps (the one dsopp_hip_pyramid_get_image(p, 1, ...) returns) and the mask lane
 * of its level-0 texels behind the pyramid's stream; grey_host, unless NULL, is width * height bytes that replace the kept image.
 * frame_device: enqueues only, on `stream` (NULL = the object's); mask_dev NULL = all valid; bgr_out_dev must be 4-byte aligned.
 * keyframe: blocking.  Reads level 0 of `maps` where it lies (the planes are never copied to the host), ordered behind the pyramid's and
 * the maps' streams by events; grey_host as for frame.  maximum_idepth and cells (either may be NULL) receive the new M and the number
 * of qualifying cells.
 * keyframe_device: enqueues only (both launches), ordered behind the maps' stream and, on another stream than the object's previous
 * keyframe view, behind that view (they share M and the partial sums); the new M is read with get_maximum_idepth, which waits for it.
 * keyframe_planes: blocking; the two planes from the host in the layout dsopp_hip_depth_maps_get_level returns, for callers whose maps
 * live on the host and for exact test inputs; the same kernels.
 * get_ / set_maximum_idepth: the state M (set 0 for "unset"); both wait for a keyframe view in flight.
 * One thread drives an object at a time.
 * DSOPP_HIP_ERR_INVALID_ARGUMENT: a NULL handle, image or output, a pyramid or maps of another size or on another device than the object,
 * a pyramid that keeps no grey image while grey_host is NULL, a stencil whose centre byte is 0, an unaligned device output, width or
 * height < 1 or more than 2^31 - 1 pixels.  There is no CPU path: without a device create fails with DSOPP_HIP_ERR_HIP. */
typedef struct dsopp_hip_debug_views dsopp_hip_debug_views;
int dsopp_hip_debug_views_create(int device, void *stream, int width, int height, const uint8_t *colormap_bgr, const uint8_t *stencil,
                                 dsopp_hip_debug_views **out);
void dsopp_hip_debug_views_destroy(dsopp_hip_debug_views *v);
int dsopp_hip_debug_views_frame(dsopp_hip_debug_views *v, const dsopp_hip_pyramid *pyramid, const uint8_t *grey_host, uint8_t *bgr_out_host);
int dsopp_hip_debug_views_frame_device(dsopp_hip_debug_views *v, const void *grey_dev, const void *mask_dev, void *bgr_out_dev, void *stream);
int dsopp_hip_debug_views_keyframe(dsopp_hip_debug_views *v, const dsopp_hip_pyramid *pyramid, const uint8_t *grey_host,
                                   const dsopp_hip_depth_maps *maps, uint8_t *bgr_out_host, double *maximum_idepth, int64_t *cells);
int dsopp_hip_debug_views_keyframe_device(dsopp_hip_debug_views *v, const void *grey_dev, const dsopp_hip_depth_maps *maps, void *bgr_out_dev,
                                          void *stream);
int dsopp_hip_debug_views_keyframe_planes(dsopp_hip_debug_views *v, const uint8_t *grey_host, const double *idepth_sum_host,
                                          const double *weight_host, uint8_t *bgr_out_host, double *maximum_idepth, int64_t *cells);
int dsopp_hip_debug_views_get_maximum_idepth(dsopp_hip_debug_views *v, double *maximum_idepth);
int dsopp_hip_debug_views_set_maximum_idepth(dsopp_hip_debug_views *v, double maximum_idepth);

/* ---- the map: keyframe landmark records that outlive the window, and their point cloud (row o-2) ----
 * What the reference keeps in its track (ActiveTrackingLandmark of every keyframe) and hands to its viewer and its exporter:
 *   PhotometricBundleAdjustment::updateFrame, the landmark rules        src/energy/problems/src/photometric_bundle_adjustment.cpp:223-263
 *   ActiveTrackingLandmark::marginalize / semanticTypeId               src/track/landmarks/src/active_tracking_landmark.cpp:55-63, 71-88
 *   Frame::buildPoints / validForVisualization / getColor              src/track/frames/src/frame.cpp:19-82, 190-216
 *   initializeVisiblePointsStorage                                     src/output/visualizer/src/local_track.cpp:139-158
 *   the exporter's loop                                                pydsopp/utils/point_cloud_exporter.py:83-107
 * tests/point_cloud_model.py is the NumPy statement of everything below; the device is held to it exactly, positions bit for bit.
 *
 * A map holds keyframes in insertion order.  A keyframe holds its pinhole intrinsics (fx, fy, cx, cy), its pose T_world_agent and one
 * RECORD per landmark, index = the caller's landmark index of the window:
 *   uv, idepth, variance (the inverse depth's), relative_baseline, flags (DSOPP_HIP_MAP_FLAG_*), type (the semantic class), rgb
 * and the bit has_image: its colours were sampled from an image.  A keyframe is LIVE while a window feeds it, then FINALISED for good.
 *
 * create: options NULL = the defaults (estimate_uncertainty 1, channels C = 1: the template parameter C of the bundle adjustment,
 *   min_relative_baseline 0.1: validForVisualization's).  `stream` NULL = a stream of the map's own.
 * add_keyframe(map, window, frame_id, pyramid or NULL), after dsopp_hip_window_push_frame of that frame: a live keyframe without records,
 *   with the intrinsics and the pose the window holds.  If the pyramid keeps an 8-bit image (dsopp_hip_pyramid_get_image's rules; the
 *   colour image if it is kept, else the grey one) the map copies it device to device, behind the pyramid's stream; the pyramid is not
 *   borrowed.  The copy is freed when the keyframe is finalised.  The window must be a whole window: a landmark shard of a
 *   dsopp_hip_window_group is DSOPP_HIP_ERR_INVALID_ARGUMENT (the group form is not built).  A frame the window does not hold:
 *   DSOPP_HIP_ERR_NOT_FOUND; an id the map holds already: DSOPP_HIP_ERR_STATE.
 * update(map, window, weights256 or NULL): ONE launch over all landmarks of all frames of the window that are live keyframes of the map,
 *   on the map's stream behind the window's; the window's next work runs behind it.  Only enqueues (it waits for the window's stream
 *   when the window's poses are newer on the device, and when a keyframe's records must grow).  A live keyframe the window no longer
 *   holds is finalised: its records and pose stay as they are.  Frames of the window the map does not know are passed over.  A keyframe
 *   takes the window's current pose estimate.  Per landmark, in this order, w_* = the window's values:
 *     1 a landmark the map has not seen gets a record: uv from the window, idepth = w_idepth, variance = DBL_MAX, relative_baseline = 0,
 *       flags = 0, type = 0, rgb = the kept image at [int(v), int(u)] (BGR -> RGB; a grey image replicated), (0, 0, 0) without an image
 *       or outside it (not 0 <= u < width and 0 <= v < height)
 *     2 w_flags & outlier: the record is an outlier                                                              (:229-231)
 *     3 not w_flags & marginalized (:232-260): |w_idepth| < 1e-8: idepth = 0, else w_idepth < 0: outlier, else idepth = w_idepth;
 *       variance = w_inv_hessian_idepth * C, or 1e-5 without estimate_uncertainty; relative_baseline = max(itself, w_relative_baseline)
 *     4 w_flags & marginalized and the record not yet marginalised: marginalize(): variance / idepth > 1e-3 or idepth < 0: outlier;
 *       then marginalised.  Such a record no longer follows the window's values (an outlier flag of the window still reaches it).
 *     5 type = semanticTypeId by the rule of dsopp_hip_window_get_semantic_types (weights256 as there); 0 while no class observation
 *       has reached the frame
 *   Call order that makes the map the reference's track: update after every solve (updateFrame runs there), once more after
 *   dsopp_hip_window_choose_marginalization(apply) — the flags it set marginalise the records, rule 4 — and before the next push_frame,
 *   which erases the marginalised frames.  A caller that updates only after the choice loses rule 3 for every landmark the choice
 *   marginalised in the same keyframe step: their records keep the idepth, variance and baseline of the update before (a landmark never
 *   updated before keeps variance DBL_MAX and becomes an outlier under rule 4), and a frame that left the window before any update has
 *   no records at all.
 * set_records: loads or replaces a FINALISED keyframe from host arrays (a new id is appended) — how a stored map comes back.  n x 2 uv,
 *   n idepth, variance, relative_baseline, flags; type and rgb (n x 3) may be NULL (zeros; has_image = rgb given).  Blocking.  A live id:
 *   DSOPP_HIP_ERR_STATE; n < 0, a NULL array with n > 0 or a flag bit other than DSOPP_HIP_MAP_FLAG_*: DSOPP_HIP_ERR_INVALID_ARGUMENT.
 * set_pose: replaces a keyframe's pose (a live keyframe's is overwritten by the next update).
 * keyframe_ids: *n = the number of keyframes; at most `capacity` ids are written, in insertion order.
 * get_records: one keyframe's raw records, blocking; every output may be NULL; state = {has_image, finalised}.
 *
 * export(map, options, n_ids, frame_ids or NULL = every keyframe in insertion order, capacity, outputs..., count, per_keyframe_counts):
 *   the records that pass, in the canonical order — keyframes in the order of frame_ids (or of insertion), then record index — packed.
 *   A record passes when
 *     idepth != 0 and relative_baseline > min_relative_baseline (the map's), and its class — OUTLIER if flagged outlier, else MARGINALIZED
 *       if flagged marginalised, else ACTIVE — is in options.classes                                   (validForVisualization)
 *     with apply_filters: variance < max_idepth_variance and relative_baseline > min_relative_baseline_filter, both strict
 *       (initializeVisiblePointsStorage, Landmark.confident; the defaults are the exporter's 5e-8 and 0.15)
 *     with frame WORLD: not |idepth| < 1e-16                                                           (point_cloud_exporter.py:99-100)
 *   xyz, binary64, every step a single IEEE operation in this order: ifx = 1 / fx, ify = 1 / fy; d = ((u - cx) ifx, (v - cy) ify, 1);
 *     KEYFRAME: (d.x / idepth, d.y / idepth, 1 / idepth)                                    (frame.cpp:152, pinhole_camera.hpp:137-139)
 *     WORLD: p_i = ((R_i0 d.x + R_i1 d.y) + R_i2) + t_i idepth; xyz_i = p_i / idepth, R from (qx, qy, qz, qw) as
 *       R00 = 1 - 2 (yy + zz), R01 = 2 (xy - zw), R02 = 2 (xz + yw), R10 = 2 (xy + zw), R11 = 1 - 2 (xx + zz), R12 = 2 (yz - xw),
 *       R20 = 2 (xz - yw), R21 = 2 (yz + xw), R22 = 1 - 2 (xx + yy)                                    (point_cloud_exporter.py:96-101)
 *   rgb by options.colours: LANDMARK_TYPE (255, 0, 0) outlier, (255, 100, 100) marginalised, (100, 255, 100) active; CONSTANT 200;
 *     SEMANTIC kSemanticColors[type % 14] (frame.cpp:19-26); IMAGE the record's rgb — DSOPP_HIP_ERR_STATE when an exported keyframe has
 *     has_image = 0.
 *   Outputs, any of which may be NULL: xyz f64 x 3, rgb u8 x 3, type u8, relative_baseline f64, idepth_variance f64, keyframe_index i32
 *   (the keyframe's position in the exported list), record_index i32; each holds `capacity` entries.  *count is always the full count
 *   and per_keyframe_counts (one per exported keyframe) the full counts; count > capacity writes the first `capacity` entries, nothing
 *   beyond, and returns DSOPP_HIP_ERR_CAPACITY.  Blocking.  Two launches whatever the number of keyframes; integer counting only: the
 *   result does not depend on the order in which workgroups run.  An id the map does not hold: DSOPP_HIP_ERR_NOT_FOUND; a class mask,
 *   frame or colour scheme out of range, n_ids or capacity < 0: DSOPP_HIP_ERR_INVALID_ARGUMENT.
 * export_device: the same into the caller's device buffers (aligned to their element; the colours to 4 bytes) on the map's stream.
 *   With count and per_keyframe_counts both NULL it only enqueues; otherwise it waits and reports as export does.
 * One thread drives a map at a time.  There is no CPU path: without a device create fails with DSOPP_HIP_ERR_HIP. */
typedef struct dsopp_hip_map dsopp_hip_map;
enum { DSOPP_HIP_MAP_FLAG_MARGINALIZED = 1, DSOPP_HIP_MAP_FLAG_OUTLIER = 2 };
enum { DSOPP_HIP_MAP_CLASS_ACTIVE = 1, DSOPP_HIP_MAP_CLASS_MARGINALIZED = 2, DSOPP_HIP_MAP_CLASS_OUTLIER = 4 };
enum { DSOPP_HIP_MAP_FRAME_KEYFRAME = 0, DSOPP_HIP_MAP_FRAME_WORLD = 1 };
enum { DSOPP_HIP_MAP_COLOURS_LANDMARK_TYPE = 0, DSOPP_HIP_MAP_COLOURS_CONSTANT = 1, DSOPP_HIP_MAP_COLOURS_SEMANTIC = 2, DSOPP_HIP_MAP_COLOURS_IMAGE = 3 };
typedef struct dsopp_hip_map_options {
  int32_t estimate_uncertainty;
  int32_t channels;
  double min_relative_baseline;
} dsopp_hip_map_options;
typedef struct dsopp_hip_map_export_options {
  int32_t classes; /* DSOPP_HIP_MAP_CLASS_* bits */
  int32_t apply_filters;
  double max_idepth_variance;
  double min_relative_baseline_filter;
  int32_t frame;   /* DSOPP_HIP_MAP_FRAME_* */
  int32_t colours; /* DSOPP_HIP_MAP_COLOURS_* */
} dsopp_hip_map_export_options;
void dsopp_hip_map_default_options(dsopp_hip_map_options *o);
/* active and marginalised records, no filters (the exporter's thresholds filled in), world frame, colours by landmark type */
void dsopp_hip_map_default_export_options(dsopp_hip_map_export_options *o);
int dsopp_hip_map_create(int device, void *stream, const dsopp_hip_map_options *options, dsopp_hip_map **out);
void dsopp_hip_map_destroy(dsopp_hip_map *m);
int dsopp_hip_map_add_keyframe(dsopp_hip_map *m, dsopp_hip_window *window, int32_t frame_id, const dsopp_hip_pyramid *pyramid);
int dsopp_hip_map_update(dsopp_hip_map *m, dsopp_hip_window *window, const uint64_t *weights256);
int dsopp_hip_map_set_records(dsopp_hip_map *m, int32_t frame_id, const double intrinsics[4], const double T_world_agent[7], int32_t n,
                              const double *uv, const double *idepth, const double *variance, const double *relative_baseline,
                              const uint8_t *flags, const uint8_t *type, const uint8_t *rgb);
int dsopp_hip_map_set_pose(dsopp_hip_map *m, int32_t frame_id, const double T_world_agent[7]);
int dsopp_hip_map_num_keyframes(dsopp_hip_map *m, int32_t *n);
int dsopp_hip_map_keyframe_ids(dsopp_hip_map *m, int32_t capacity, int32_t *ids, int32_t *n);
int dsopp_hip_map_num_records(dsopp_hip_map *m, int32_t frame_id, int32_t *n);
int dsopp_hip_map_get_records(dsopp_hip_map *m, int32_t frame_id, double *uv, double *idepth, double *variance, double *relative_baseline,
                              uint8_t *flags, uint8_t *type, uint8_t *rgb, double intrinsics[4], double T_world_agent[7], int32_t state[2]);
int dsopp_hip_map_export(dsopp_hip_map *m, const dsopp_hip_map_export_options *options, int32_t n_ids, const int32_t *frame_ids,
                         int64_t capacity, double *xyz, uint8_t *rgb, uint8_t *type, double *relative_baseline, double *idepth_variance,
                         int32_t *keyframe_index, int32_t *record_index, int64_t *count, int32_t *per_keyframe_counts);
int dsopp_hip_map_export_device(dsopp_hip_map *m, const dsopp_hip_map_export_options *options, int32_t n_ids, const int32_t *frame_ids,
                                int64_t capacity, void *xyz_dev, void *rgb_dev, void *type_dev, void *relative_baseline_dev,
                                void *idepth_variance_dev, void *keyframe_index_dev, void *record_index_dev, int64_t *count,
                                int32_t *per_keyframe_counts);

#ifdef __cplusplus
}
#endif
#endif /* DSOPP_HIP_H */
