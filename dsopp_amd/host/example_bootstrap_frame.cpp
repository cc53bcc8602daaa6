// Driver of HipEstimateSE3PnP and HipRefineTrack (dsopp_hip_solvers.hpp): everything a bootstrap frame runs once the initialiser has
// succeeded (src/feature_based_slam/tracker/src/monocular_tracker.cpp:54-68: estimateSE3PnP, triangulatePoints, optimizeTransformations,
// removeOutliers), over the C-ABI alone:
//   example_bootstrap_frame <file>
// <file>: the format of example_refine_track.cpp: "width height frames landmarks steps" in text, then binary: fx, fy, cx, cy (4 doubles);
// per frame: frame id, initialized (2 int32), t_world_agent (12 doubles: R row-major, t); per landmark: has_position, the number of
// projections (2 int32), the position (3 doubles), then per projection the frame id (int32) and the pixel (2 doubles).  The last `steps`
// frames arrive one by one: each gets its pose from the PnP RANSAC (threshold 0.5, 256 triples from std::rand() seeded with step + 1),
// counts as initialised from then on, and the track of the frames up to it runs the three steps (4 projections to triangulate, no
// retriangulation; the last 10 frames; thresholds 1.5 and 0.5).  Prints, per step, the PnP's record and pose, the counts, the solve's
// record, and the poses and positions as the bits of their doubles — what a test compares with the Python binding composed the same
// way.  Exit code 2 without a GPU: there is no CPU fallback.
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
}  // namespace

int main(int argc, char **argv) {
  int n_dev = 0;
  dsopp_hip_device_count(&n_dev);
  if (n_dev < 1) {
    std::printf("no GPU: the HIP backend has no CPU fallback\n");
    return 2;
  }
  if (argc < 2) {
    std::printf("usage: example_bootstrap_frame <file>\n");
    return 1;
  }
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, n_frames = 0, n_landmarks = 0, steps = 0;
  if (!f || std::fscanf(f, "%d %d %d %d %d", &width, &height, &n_frames, &n_landmarks, &steps) != 5 || std::fgetc(f) != '\n' || n_frames < 0 ||
      n_landmarks < 0 || steps < 0 || steps > n_frames) {
    std::printf("cannot read the header of %s\n", argv[1]);
    if (f) std::fclose(f);
    return 1;
  }
  double camera[4];
  std::vector<RefineFrame> all_frames(static_cast<size_t>(n_frames));
  std::vector<RefineLandmark> landmarks(static_cast<size_t>(n_landmarks));
  bool read = get(f, camera, 4);
  for (RefineFrame &frame : all_frames) {
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
    HipEstimateSE3PnP pnp(width, height);
    HipRefineTrack refine(width, height);
    std::deque<RefineFrame> frames(all_frames.begin(), all_frames.end() - steps);
    for (int step = 0; step < steps; ++step) {
      frames.push_back(all_frames[static_cast<size_t>(n_frames - steps + step)]);
      RefineFrame &frame = frames.back();
      // (reseeded per step: the runtime underneath may draw from rand() too, and the triples must not depend on that)
      std::srand(static_cast<unsigned>(step + 1));
      const size_t candidates = HipEstimateSE3PnP::candidates(frame.frame_id, landmarks).size();
      const std::vector<int32_t> samples =
          candidates < 3 ? std::vector<int32_t>()
                         : HipRotationStandstill::drawSamples(candidates, static_cast<size_t>(dsopp_hip_pnp_ransac_default_iterations()));
      const HipEstimateSE3PnP::Result p = pnp.estimate(frame.frame_id, landmarks, frame, model, samples, 0.5);
      frame.initialized = true;
      std::printf("step %d: pnp inliers %zu of %zu, best %d/%d, refined inliers %d, iterations %d, flags %d, initialised %d\n", step, p.inliers,
                  p.matches, p.record.best_iteration, p.record.best_solution, p.record.refined_inlier_count, p.record.refine_iterations,
                  p.record.refine_flags, HipEstimateSE3PnP::initialised(p.inliers, p.matches) ? 1 : 0);
      std::printf("pnp pose");
      for (double v : p.record.pose) std::printf(" %016" PRIx64, bits(v));
      const size_t triangulated = refine.triangulatePoints(landmarks, frames, model, 4, false);
      const dsopp_hip_geometric_ba_result r = refine.optimizeTransformations(landmarks, frames, model, 1.5, 10);
      const size_t removed = refine.removeOutliers(landmarks, frames, model, 10, 0.5);
      std::printf("\nstep %d: triangulated %zu, iterations %d, accepted %d, reason %d, valid %d, removed %zu\n", step, triangulated, r.iterations,
                  r.accepted_steps, r.reason, r.valid_residuals, removed);
      std::printf("cost %016" PRIx64 " %016" PRIx64 "\nposes", bits(r.initial_cost), bits(r.final_cost));
      for (const RefineFrame &fr : frames)
        for (double v : fr.t_world_agent) std::printf(" %016" PRIx64, bits(v));
      std::printf("\npositions");
      for (const RefineLandmark &lm : landmarks) {
        std::printf(" %d", lm.has_position ? 1 : 0);
        for (double v : lm.position) std::printf(" %016" PRIx64, bits(lm.has_position ? v : 0.0));
      }
      std::printf("\nprojections");
      for (const RefineLandmark &lm : landmarks) std::printf(" %zu", lm.projections.size());
      std::printf("\n");
    }
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
