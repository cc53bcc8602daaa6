// Self-contained driver of the camera set-up (src/sensors/sensors_builder/src/camera_fabric.cpp:142-167) over the C-ABI alone: a
// calibration text goes in (HipCameraCalibration::parse, fabric.cpp:23-113), the undistorter comes out of the camera model on the
// device, the static mask and the vignette are undistorted and taken through a HipImageTransformer (runMaskTransformers /
// runImageTransformers), and the transformers' transformCalibration is applied to the pinhole.
//   example_camera_setup [--parse | --parse-native] [calibration.txt [resize_ratio [crop_levels]]]
// Without a file the built-in TUM-FOV calibration at 160 x 120 is used; resize_ratio 0.75, crop_levels 3.  The mask and the vignette are
// integer-valued functions of the pixel, so that every caller renders the same bytes.
// --parse stops behind the parser and needs no device.  It prints the resulting calibration: its type, size and intrinsics (as bits),
// and the distorted model when there is one; --parse-native is the same with transform_to_pinhole = false (fabric.cpp:41-44,101-104).
// A refused text prints the reason and exits with 1.
// The full run prints those lines, the transformed calibration, and the transformed mask and vignette row by row in hex.
// tests/test_gpu_camera_remap.py composes the same calls through the Python binding and compares the output byte for byte.
// Exit code 0, 1 for a refused calibration, 2 without a GPU: there is no CPU fallback.
//   g++ -std=c++17 example_camera_setup.cpp -L../lib -ldsopp_hip -Wl,-rpath,$PWD/../lib -o example_camera_setup
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iterator>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
const char *kBuiltIn = "tum_fov\n160 120\n0.7 0.72 0.51 0.48\n0.93\n";

uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}

/** the static mask: valid (255) but for a rectangle and the last rows (the car's bonnet) */
uint8_t maskAt(int x, int y, int w, int h) { return (y >= h - h / 6 || (x >= w / 3 && x < w / 3 + 9 && y >= 10 && y < 21)) ? 0 : 255; }
/** the vignette: bright in the middle, falling off in integer steps */
uint8_t vignetteAt(int x, int y, int w, int h) {
  const int dx = 2 * x - w, dy = 2 * y - h;
  return static_cast<uint8_t>(255 - (dx * dx + dy * dy) * 150 / (w * w + h * h));
}

void printImage(const char *name, const std::vector<uint8_t> &image, int w, int h) {
  std::printf("%s %d %d\n", name, w, h);
  for (int y = 0; y < h; ++y) {
    for (int x = 0; x < w; ++x) std::printf("%02x", image[static_cast<size_t>(y) * w + x]);
    std::printf("\n");
  }
}
}  // namespace

int main(int argc, char **argv) {
  int arg = 1;
  const bool native = argc > arg && std::strcmp(argv[arg], "--parse-native") == 0;
  const bool parse_only = native || (argc > arg && std::strcmp(argv[arg], "--parse") == 0);
  if (parse_only) ++arg;
  std::string text = kBuiltIn;
  if (argc > arg) {
    std::ifstream file(argv[arg]);
    if (!file.is_open()) {
      std::printf("could not open calibration file %s\n", argv[arg]);
      return 1;
    }
    text.assign(std::istreambuf_iterator<char>(file), std::istreambuf_iterator<char>());
    ++arg;
  }
  const double resize_ratio = argc > arg ? std::atof(argv[arg]) : 0.75;
  const int crop_levels = argc > arg + 1 ? std::atoi(argv[arg + 1]) : 3;
  try {
    HipCameraCalibration calibration = HipCameraCalibration::parse(text, !native);
    const bool pinhole = calibration.type() == HipCameraCalibration::ModelType::kPinholeCamera;
    std::printf("calibration %s %016" PRIx64 " %016" PRIx64, pinhole ? "pinhole" : "simple_radial", bits(calibration.imageWidth()),
                bits(calibration.imageHeight()));
    for (int i = 0; i < (pinhole ? 4 : 5); ++i) std::printf(" %016" PRIx64, bits(calibration.intrinsics()[i]));
    std::printf("\n");
    if (calibration.hasUndistorter()) {
      const dsopp_hip_camera_model &m = calibration.model();
      std::printf("model %d %d %d %d", m.type, m.width, m.height, m.num_k);
      for (double v : m.params) std::printf(" %016" PRIx64, bits(v));
      for (int i = 0; i < m.num_k; ++i) std::printf(" %016" PRIx64, bits(m.k[i]));
      std::printf("\n");
    } else {
      std::printf("model none\n");
    }
    if (parse_only) return 0;

    int n_dev = 0;
    dsopp_hip_device_count(&n_dev);
    if (n_dev < 1) {
      std::printf("no GPU: the HIP backend has no CPU fallback\n");
      return 2;
    }
    const int w = static_cast<int>(calibration.imageWidth()), h = static_cast<int>(calibration.imageHeight());
    std::vector<uint8_t> mask(static_cast<size_t>(w) * h), vignette(mask.size());
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        mask[static_cast<size_t>(y) * w + x] = maskAt(x, y, w, h);
        vignette[static_cast<size_t>(y) * w + x] = vignetteAt(x, y, w, h);
      }
    // camera_fabric.cpp:157-159: the transformers change the calibration
    const HipImageTransformer transformer(w, h, resize_ratio, crop_levels);
    double image_size[2];
    const PinholeModel transformed = HipImageTransformer::transformCalibration(w, h, resize_ratio, crop_levels, calibration.pinhole(), image_size);
    std::printf("transformed %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(image_size[0]),
                bits(image_size[1]), bits(transformed.fx), bits(transformed.fy), bits(transformed.cx), bits(transformed.cy));
    // :162-167: the mask and the vignette are undistorted, then transformed
    const HipUndistorter *undistorter = calibration.undistorter();
    const std::vector<uint8_t> undistorted_mask = undistorter ? undistorter->undistort(mask.data()) : mask;
    const std::vector<uint8_t> undistorted_vignette = undistorter ? undistorter->undistort(vignette.data()) : vignette;
    printImage("mask", transformer.transformMask(undistorted_mask.data()), transformer.outWidth(), transformer.outHeight());
    printImage("vignette", transformer.transformImage(undistorted_vignette.data()), transformer.outWidth(), transformer.outHeight());
    return 0;
  } catch (const SolverError &e) {
    std::printf("refused (%d): %s\n", e.code, e.what());
    return 1;
  }
}
