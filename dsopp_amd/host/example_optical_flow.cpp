// Driver of HipOpticalFlowMatch (dsopp_hip_solvers.hpp), the Lucas-Kanade half of features::OpticalFlowMatch
// (src/feature_based_slam/features/src/optical_flow.cpp:11-42), over the C-ABI alone:
//   example_optical_flow <file>
// <file>: "width height n" in text, then the two 8-bit images (image_from, image_to; width * height bytes each) and n (x, y) float pairs,
// all binary.  Prints one line per correspondence: idx_from idx_to, the feature in image_to as the bits of its two floats, and the
// status / err pair's err bits — what a test compares with the Python binding's result.  Exit code 2 without a GPU: there is no CPU fallback.
#include <cstdio>
#include <cstring>
#include <vector>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
uint32_t bits(float v) {
  uint32_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
}  // namespace

int main(int argc, char **argv) {
  int n_dev = 0;
  dsopp_hip_device_count(&n_dev);
  if (n_dev < 1) {
    std::printf("no GPU: the HIP backend has no CPU fallback\n");
    return 2;
  }
  if (argc < 2) {
    std::printf("usage: example_optical_flow <file>\n");
    return 1;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, n = 0;
  if (!f || std::fscanf(f, "%d %d %d", &width, &height, &n) != 3 || std::fgetc(f) != '\n' || width < 2 || height < 2 || n < 0) {
    std::printf("cannot read the header of %s\n", argv[1]);
    return 1;
  }
  const size_t pixels = static_cast<size_t>(width) * static_cast<size_t>(height);
  std::vector<uint8_t> image_from(pixels), image_to(pixels);
  std::vector<std::array<float, 2>> features_from(static_cast<size_t>(n));
  const bool read = std::fread(image_from.data(), 1, pixels, f) == pixels && std::fread(image_to.data(), 1, pixels, f) == pixels &&
                    std::fread(features_from.data(), sizeof(features_from[0]), features_from.size(), f) == features_from.size();
  std::fclose(f);
  if (!read) {
    std::printf("%s is too short\n", argv[1]);
    return 1;
  }
  try {
    HipOpticalFlowMatch matcher(width, height);
    matcher.setImageFrom(image_from.data());
    const HipOpticalFlowMatch::Result r = matcher.match(features_from, image_to.data());
    std::printf("correspondences %zu of %d\n", r.correspondences.size(), n);
    for (const FlowCorrespondence &c : r.correspondences)
      std::printf("%zu %zu %08x %08x %08x\n", c.idx_from, c.idx_to, bits(r.features[c.idx_to][0]), bits(r.features[c.idx_to][1]),
                  bits(matcher.error()[c.idx_from]));
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
