// Driver of HipRefineTrack (dsopp_hip_solvers.hpp), the refinement a bootstrap frame runs once the initialiser has succeeded
// (src/feature_based_slam/tracker/src/monocular_tracker.cpp:54-68: triangulatePoints, optimizeTransformations, removeOutliers), over the
// C-ABI alone:
//   example_refine_track <file> [--free-focal] [--free-center] [--simple-radial [--free-distortion]]
// <file>: "width height frames landmarks steps" in text, then binary: fx, fy, cx, cy (4 doubles); per frame: frame id, initialized
// (2 int32), t_world_agent (12 doubles: R row-major, t); per landmark: has_position, the number of projections (2 int32), the position
// (3 doubles), then per projection the frame id (int32) and the pixel (2 doubles).  The last `steps` frames arrive one by one: for each of
// them the track holds the frames up to it and runs the three steps (4 projections to triangulate, no retriangulation; the last 10 frames;
// thresholds 1.5 and 0.5).  Prints, per step, the counts, the solve's record, and the poses and positions as the bits of their doubles —
// what a test compares with the Python binding composed the same way.  With --free-focal and / or --free-center the refinement is the
// OPTIMIZE_CAMERA form: the file's pinhole intrinsics are a parameter block of which the named groups move, the steps that follow use the
// intrinsics the refinement left, and every step also prints them before and after ("intrinsics before" / "intrinsics after": the bits
// of fx, fy, cx, cy).  With --simple-radial the refinement takes the file's camera as a SimpleRadialCamera (f = fx, cx, cy, k1 = k2 = 0;
// --free-distortion frees k1 and k2) and prints its five intrinsics; triangulation and pruning, which the library has for the pinhole
// only, go on with (f, f, cx, cy).  Exit code 2 without a GPU: there is no CPU fallback.
#include <cinttypes>
#include <cstdio>
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
  HipRefineTrack::ParameterParameterization parameterization;
  bool usage = argc < 2, simple_radial = false;
  for (int k = 2; k < argc; ++k) {
    if (!std::strcmp(argv[k], "--free-focal")) {
      parameterization.fix_focal = false;
    } else if (!std::strcmp(argv[k], "--free-center")) {
      parameterization.fix_center = false;
    } else if (!std::strcmp(argv[k], "--simple-radial")) {
      simple_radial = true;
    } else if (!std::strcmp(argv[k], "--free-distortion")) {
      parameterization.fix_model_specific = false;
    } else {
      usage = true;
    }
  }
  if (usage || (!parameterization.fix_model_specific && !simple_radial)) {
    std::printf("usage: example_refine_track <file> [--free-focal] [--free-center] [--simple-radial [--free-distortion]]\n");
    return 1;
  }
  const bool optimize_camera = simple_radial || !parameterization.fix_focal || !parameterization.fix_center;
  const HipRefineTrack::CameraModel camera_model = simple_radial ? HipRefineTrack::CameraModel::kSimpleRadial : HipRefineTrack::CameraModel::kPinhole;
  std::FILE *f = std::fopen(argv[1], "rb");
  int width = 0, height = 0, n_frames = 0, n_landmarks = 0, steps = 0;
  if (!f || std::fscanf(f, "%d %d %d %d %d", &width, &height, &n_frames, &n_landmarks, &steps) != 5 || std::fgetc(f) != '\n' || n_frames < 0 ||
      n_landmarks < 0 || steps < 0 || steps > n_frames) {
    std::printf("cannot read the header of %s\n", argv[1]);
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
    std::vector<double> intrinsics(camera, camera + 4);
    if (simple_radial) intrinsics = {camera[0], camera[2], camera[3], 0.0, 0.0};
    const auto pinhole = [&] {
      return simple_radial ? PinholeModel{intrinsics[0], intrinsics[0], intrinsics[1], intrinsics[2]}
                           : PinholeModel{intrinsics[0], intrinsics[1], intrinsics[2], intrinsics[3]};
    };
    HipRefineTrack refine(width, height);
    std::deque<RefineFrame> frames(all_frames.begin(), all_frames.end() - steps);
    for (int step = 0; step < steps; ++step) {
      frames.push_back(all_frames[static_cast<size_t>(n_frames - steps + step)]);
      const PinholeModel model = pinhole();
      const size_t triangulated = refine.triangulatePoints(landmarks, frames, model, 4, false);
      dsopp_hip_geometric_ba_result r;
      if (optimize_camera) {
        std::printf("intrinsics before");
        for (double v : intrinsics) std::printf(" %016" PRIx64, bits(v));
        r = refine.optimizeTransformations(landmarks, intrinsics, camera_model, frames, parameterization, 1.5, 10);
        std::printf("\nintrinsics after");
        for (double v : intrinsics) std::printf(" %016" PRIx64, bits(v));
        std::printf(" (");
        for (size_t k = 0; k < intrinsics.size(); ++k) std::printf(k ? " %.6f" : "%.6f", intrinsics[k]);
        std::printf(")\n");
      } else {
        r = refine.optimizeTransformations(landmarks, frames, model, 1.5, 10);
      }
      const PinholeModel refined = pinhole();
      const size_t removed = refine.removeOutliers(landmarks, frames, refined, 10, 0.5);
      std::printf("step %d: triangulated %zu, iterations %d, accepted %d, reason %d, valid %d, removed %zu\n", step, triangulated, r.iterations,
                  r.accepted_steps, r.reason, r.valid_residuals, removed);
      std::printf("cost %016" PRIx64 " %016" PRIx64 "\nposes", bits(r.initial_cost), bits(r.final_cost));
      for (const RefineFrame &frame : frames)
        for (double v : frame.t_world_agent) std::printf(" %016" PRIx64, bits(v));
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
