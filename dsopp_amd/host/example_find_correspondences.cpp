// Driver of HipFindCorrespondences (dsopp_hip_solvers.hpp), features::findCorrespondences over features::OpticalFlowMatch
// (src/feature_based_slam/features/src/correspondences_finder.cpp:7-18, optical_flow.cpp:11-56), over the C-ABI alone, as
// MonocularInitializer::tick drives it (monocular_initializer.cpp:47-53):
//   example_find_correspondences <file>
// <file>: "width height frames number_of_features levels edge_threshold lost" in text, then `frames` 8-bit images (width * height bytes
// each), binary.  Frame 0 has no previous frame: its features are the detection.  Every later frame is matched against frame 0's features,
// the last `lost` of which are first moved off the image to (-1000 - i, -1000), so that the flow loses a known number.  Prints per
// frame "frame k features N correspondences M", a line "f" with the bits of the two floats per feature and a line "c idx_from idx_to"
// per correspondence — what a test compares with the NumPy model.  Exit code 2 without a GPU: there is no CPU fallback.
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

void print(int frame, const HipFindCorrespondences::Result &r) {
  std::printf("frame %d features %zu correspondences %zu\n", frame, r.features.size(), r.correspondences.size());
  for (const auto &f : r.features) std::printf("f %08x %08x\n", bits(f[0]), bits(f[1]));
  for (const FlowCorrespondence &c : r.correspondences) std::printf("c %zu %zu\n", c.idx_from, c.idx_to);
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
    std::printf("usage: example_find_correspondences <file>\n");
    return 1;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, frames = 0, number_of_features = 0, levels = 0, edge = 0, lost = 0;
  if (!f || std::fscanf(f, "%d %d %d %d %d %d %d", &width, &height, &frames, &number_of_features, &levels, &edge, &lost) != 7 ||
      std::fgetc(f) != '\n' || width < 2 || height < 2 || frames < 1 || number_of_features < 0 || lost < 0) {
    std::printf("cannot read the header of %s\n", argv[1]);
    return 1;
  }
  const size_t pixels = static_cast<size_t>(width) * static_cast<size_t>(height);
  std::vector<std::vector<uint8_t>> images(static_cast<size_t>(frames), std::vector<uint8_t>(pixels));
  bool read = true;
  for (auto &image : images) read = read && std::fread(image.data(), 1, pixels, f) == pixels;
  std::fclose(f);
  if (!read) {
    std::printf("%s is too short\n", argv[1]);
    return 1;
  }
  try {
    HipFindCorrespondences finder(width, height, static_cast<size_t>(number_of_features), 0, nullptr, levels, edge);
    const HipFindCorrespondences::Result first = finder.find(nullptr, images[0].data());
    print(0, first);
    finder.setImageFrom(images[0].data());
    std::vector<std::array<float, 2>> features_from = first.features;
    for (size_t i = 0; i < static_cast<size_t>(lost) && i < features_from.size(); ++i)
      features_from[features_from.size() - 1 - i] = {-1000.0f - static_cast<float>(i), -1000.0f};
    for (int k = 1; k < frames; ++k) print(k, finder.find(&features_from, images[static_cast<size_t>(k)].data()));
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
