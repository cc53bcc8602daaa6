// Driver of HipRotationStandstill (dsopp_hip_solvers.hpp), the pure-rotation RANSAC of the bootstrap's standstill test
// (src/feature_based_slam/tracker/src/estimate_so3_inlier_count.cpp:17-48), over the C-ABI alone:
//   example_rotation_ransac <file>
// <file>: "width height n iterations" in text, then binary: fx, fy, cx, cy, threshold (5 doubles), the new frame's points and the last
// keyframe's (n (x, y) double pairs each) and the sample triples (iterations x 3 int32).  iterations = -1: no triples follow, they are
// drawn from std::rand() as the reference draws them (200 of them).  Prints the counts, the rotation as the bits of its nine doubles, the
// inlier indices, and the two decisions — what a test compares with the Python binding's result.  Exit code 2 without a GPU: there is no
// CPU fallback.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
uint64_t bits(double v) {
  uint64_t b;
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
    std::printf("usage: example_rotation_ransac <file>\n");
    return 1;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, n = 0, iterations = 0;
  if (!f || std::fscanf(f, "%d %d %d %d", &width, &height, &n, &iterations) != 4 || std::fgetc(f) != '\n' || n < 0 || iterations < -1) {
    std::printf("cannot read the header of %s\n", argv[1]);
    return 1;
  }
  double camera[5];
  std::vector<Vector2> points_new(static_cast<size_t>(n)), points_keyframe(static_cast<size_t>(n));
  std::vector<int32_t> samples(iterations > 0 ? 3 * static_cast<size_t>(iterations) : 0);
  const bool read = std::fread(camera, sizeof(double), 5, f) == 5 &&
                    std::fread(points_new.data(), sizeof(Vector2), points_new.size(), f) == points_new.size() &&
                    std::fread(points_keyframe.data(), sizeof(Vector2), points_keyframe.size(), f) == points_keyframe.size() &&
                    std::fread(samples.data(), sizeof(int32_t), samples.size(), f) == samples.size();
  std::fclose(f);
  if (!read) {
    std::printf("%s is too short\n", argv[1]);
    return 1;
  }
  try {
    const PinholeModel model{camera[0], camera[1], camera[2], camera[3]};
    HipRotationStandstill standstill(width, height);
    const HipRotationStandstill::Result r = iterations < 0 ? standstill.estimate(points_new, points_keyframe, model, 200, camera[4])
                                                           : standstill.estimate(points_new, points_keyframe, model, samples, camera[4]);
    std::printf("inliers %zu of %zu, iterations %d, best %d\n", r.inliers, r.matches, r.iterations_run, r.best_iteration);
    std::printf("rotation");
    for (double v : r.rotation) std::printf(" %016" PRIx64, bits(v));
    std::printf("\nindices");
    for (int32_t i : r.inlier_indices) std::printf(" %d", i);
    const FrameStatus status = HipRotationStandstill::needNewFrame(1, r.inliers, r.matches);
    std::printf("\nneedNewFrame %s, standstill %d\n",
                status == FrameStatus::kDropFrame ? "drop" : (status == FrameStatus::kFinish ? "finish" : "keep"),
                HipRotationStandstill::isStandstill(r.inliers, r.matches) ? 1 : 0);
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
