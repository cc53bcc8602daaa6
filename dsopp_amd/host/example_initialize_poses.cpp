// Driver of HipInitializePoses (dsopp_hip_solvers.hpp): initializePoses of the feature-based bootstrap
// (src/feature_based_slam/tracker/src/initialize_poses.cpp:17-78: estimateSO3xS2, the two-view triangulatePoints, estimateSE3PnP per
// intermediate frame, optimizeTransformations, estimateSE3PnP again), over the C-ABI alone:
//   example_initialize_poses <file>
// <file>: "width height frames landmarks seed" in text, then binary as example_bootstrap_frame.cpp reads it: fx, fy, cx, cy (4 doubles);
// per frame: frame id, initialized (2 int32), t_world_agent (12 doubles: R row-major, t); per landmark: has_position, the number of
// projections (2 int32), the position (3 doubles), then per projection the frame id (int32) and the pixel (2 doubles).
// std::rand() is seeded with `seed` once, ahead of the call (every step draws its samples from it in turn).  Prints the decision, the
// two-view record and pose, the triangulated count, every PnP's record, the refinement's record, and the poses, positions and
// projection counts as the bits of their doubles — what a test compares with the Python bindings composed the same way.
// Exit code 2 without a GPU: there is no CPU fallback.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <vector>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
uint64_t bits(double v) {
  uint64_t b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
template <typename T>
bool get(std::FILE *f, T *out, size_t n) {
  return std::fread(out, sizeof(T), n, f) == n;
}
void printPnp(const char *name, const std::vector<HipEstimateSE3PnP::Result> &results) {
  for (const HipEstimateSE3PnP::Result &p : results)
    std::printf("%s: inliers %zu of %zu, best %d/%d, refined inliers %d, iterations %d, flags %d\n", name, p.inliers, p.matches, p.record.best_iteration,
                p.record.best_solution, p.record.refined_inlier_count, p.record.refine_iterations, p.record.refine_flags);
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
    std::printf("usage: example_initialize_poses <file>\n");
    return 1;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, n_frames = 0, n_landmarks = 0, seed = 0;
  if (!f || std::fscanf(f, "%d %d %d %d %d", &width, &height, &n_frames, &n_landmarks, &seed) != 5 || std::fgetc(f) != '\n' || n_frames < 2 ||
      n_landmarks < 0 || seed < 0) {
    std::printf("cannot read the header of %s\n", argv[1]);
    if (f) std::fclose(f);
    return 1;
  }
  double camera[4];
  std::deque<RefineFrame> frames(static_cast<size_t>(n_frames));
  std::vector<RefineLandmark> landmarks(static_cast<size_t>(n_landmarks));
  bool read = get(f, camera, 4);
  for (RefineFrame &frame : frames) {
    int32_t head[2] = {0, 0};
    read = read && get(f, head, 2) && get(f, frame.t_world_agent.data(), 12);
    frame.frame_id = static_cast<size_t>(head[0]);
    frame.initialized = head[1] != 0;
  }
  for (RefineLandmark &lm : landmarks) {
    int32_t head[2] = {0, 0};
    read = read && get(f, head, 2) && get(f, lm.position.data(), 3) && head[1] >= 0;
    lm.has_position = head[0] != 0;
    for (int32_t k = 0; read && k < head[1]; ++k) {
      int32_t frame_id = 0;
      Vector2 xy{};
      read = get(f, &frame_id, 1) && get(f, xy.data(), 2);
      lm.projections.emplace_back(static_cast<size_t>(frame_id), xy);
    }
  }
  std::fclose(f);
  if (!read) {
    std::printf("%s is too short\n", argv[1]);
    return 1;
  }
  try {
    const PinholeModel model{camera[0], camera[1], camera[2], camera[3]};
    HipInitializePoses initializer(width, height);
    std::srand(static_cast<unsigned>(seed));
    const HipInitializePoses::Result r = initializer.run(frames, landmarks, model);
    const dsopp_hip_two_view_ransac_result &t = r.two_view.record;
    std::printf("initialised %d: two-view inliers %zu of %zu, best %d/%d, ransac inliers %d, iterations %d %d, flags %d %d, accepted %d\n",
                r.success ? 1 : 0, r.two_view.inliers, r.two_view.matches, t.best_iteration, t.best_solution, t.ransac_inlier_count,
                t.refine_iterations[0], t.refine_iterations[1], t.refine_flags[0], t.refine_flags[1],
                HipEstimateSO3xS2::accepted(r.two_view.inliers, r.two_view.matches) ? 1 : 0);
    std::printf("two-view pose");
    for (double v : t.pose) std::printf(" %016" PRIx64, bits(v));
    std::printf("\ntriangulated %zu, pnp initialised %zu\n", r.triangulated, r.pnp_initialized);
    printPnp("pnp", r.pnp);
    printPnp("second pnp", r.second_pnp);
    std::printf("refinement: iterations %d, accepted %d, reason %d, valid %d, cost %016" PRIx64 " %016" PRIx64 "\nposes", r.refinement.iterations,
                r.refinement.accepted_steps, r.refinement.reason, r.refinement.valid_residuals, bits(r.refinement.initial_cost),
                bits(r.refinement.final_cost));
    for (const RefineFrame &fr : frames) {
      std::printf(" %d", fr.initialized ? 1 : 0);
      for (double v : fr.t_world_agent) std::printf(" %016" PRIx64, bits(v));
    }
    std::printf("\npositions");
    for (const RefineLandmark &lm : landmarks) {
      std::printf(" %d", lm.has_position ? 1 : 0);
      for (double v : lm.position) std::printf(" %016" PRIx64, bits(lm.has_position ? v : 0.0));
    }
    std::printf("\nprojections");
    for (const RefineLandmark &lm : landmarks) std::printf(" %zu", lm.projections.size());
    std::printf("\n");
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
