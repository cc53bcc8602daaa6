// Self-contained driver of HipFrameMarginalizationStrategy (dsopp_hip_solvers.hpp): the tracker's marginalisation step
// (src/tracker/tracker/src/monocular_tracker.cpp:505-507) over the C-ABI alone.  Eight keyframes of an analytic scene (a textured plane at
// z = 4, the camera stepping along x, the third keyframe 2 mm from the second) enter a HipPhotometricBundleAdjustment; no solve is needed for the
// choice, which reads the poses, the flags and the connection statuses.  The sparse strategy (5, 7, 0.95) must pick the second keyframe
// — close to another one and far from the newest —, and a second window under the maximum_size strategy (6) must let its two oldest keyframes go.
//   example_marginalization [-v]
// Prints the scores, the set, the keyframes marginalised and the landmark counts; exit code 0 when both choices are the expected ones,
// 2 without a GPU: there is no CPU fallback.
//   g++ -std=c++17 example_marginalization.cpp -L../lib -ldsopp_hip -Wl,-rpath,$PWD/../lib -o example_marginalization
#include <cmath>
#include <cstdio>
#include <memory>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
constexpr int W = 64, H = 48, kFrames = 8, kLandmarks = 65;
constexpr double fx = 45, fy = 45, cx = 32, cy = 24, Z = 4.0;

std::vector<uint8_t> render(double tx) {
  std::vector<uint8_t> img(static_cast<size_t>(W) * H);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      const double X = (u - cx) / fx * Z + tx, Y = (v - cy) / fy * Z;
      const double val = 127.5 + 55 * std::sin(3.0 * X) * std::cos(2.5 * Y) + 35 * std::sin(7.0 * X + 1.0) * std::sin(6.0 * Y);
      img[static_cast<size_t>(v) * W + u] = static_cast<uint8_t>(std::lround(std::min(255.0, std::max(0.0, val))));
    }
  return img;
}

struct Window {
  std::unique_ptr<HipPhotometricBundleAdjustment> pba;
  std::vector<std::unique_ptr<DevicePyramid>> pyramids;
  std::vector<KeyframeView> frames;
  std::vector<KeyframeView *> active;
};

/** the window as pushNewKeyframe + pushFrame + updateSolver leave it: every keyframe connected with every other, all statuses kOk but
 *  every fifth landmark's towards the newest keyframe */
void fill(Window &w) {
  const TrustRegionOptions opt{7, 1e5, 1e-8, 1e-8, {1e12, 1e8}, 1e16, 20};
  w.pba = std::make_unique<HipPhotometricBundleAdjustment>(opt, true, true);
  w.frames.resize(kFrames);
  const PinholeModel model{fx, fy, cx, cy};
  for (int i = 0; i < kFrames; ++i) {
    const double tx = i == 2 ? 0.052 : 0.05 * i;
    const std::vector<uint8_t> image = render(tx);
    w.pyramids.push_back(std::make_unique<DevicePyramid>(W, H, 1));
    w.pyramids.back()->build(image.data());
    KeyframeView &f = w.frames[static_cast<size_t>(i)];
    f.keyframe_id = i;
    f.timestamp = 1000 * (i + 1);
    f.t_world_agent = {0, 0, 0, 1, tx, 0, 0};
    f.exposure_time = 1;
    f.affine_brightness = {0, 0};
    f.is_marginalized = false;
    f.pyramids = w.pyramids.back().get();
    for (int k = 0; k < kLandmarks; ++k) {
      LandmarkView lm;
      const int u = 8 + (k * 7) % (W - 16), v = 8 + (k * 5) % (H - 16);
      lm.projection = {static_cast<double>(u), static_cast<double>(v)};
      lm.idepth = 1.0 / Z;
      static const int px[8] = {0, -1, 1, -2, 0, 2, -1, 0}, py[8] = {2, 1, 1, 0, 0, 0, -1, -2};
      for (int p = 0; p < 8; ++p) lm.patch[static_cast<size_t>(p)] = image[static_cast<size_t>(v + py[p]) * W + u + px[p]];
      lm.is_marginalized = lm.is_outlier = false;
      f.active_landmarks.push_back(lm);
    }
    for (int j = 0; j < i; ++j) {
      f.reprojection_statuses[j] = std::vector<uint8_t>(kLandmarks, DSOPP_HIP_STATUS_OK);
      std::vector<uint8_t> towards_new(kLandmarks, DSOPP_HIP_STATUS_OK);
      for (int k = 0; k < kLandmarks; k += 5) towards_new[static_cast<size_t>(k)] = DSOPP_HIP_STATUS_OOB;
      w.frames[static_cast<size_t>(j)].reprojection_statuses[i] = towards_new;
    }
    w.pba->pushFrame(f, 0, model, i == 0 ? FrameParameterization::kFixed : FrameParameterization::kFree);
    for (int j = 0; j < i; ++j) w.pba->updateLocalFrame(w.frames[static_cast<size_t>(j)]);
  }
  for (KeyframeView &f : w.frames) w.active.push_back(&f);
}

int count(const KeyframeView &f, bool outliers) {
  int n = 0;
  for (const LandmarkView &lm : f.active_landmarks) n += (outliers ? lm.is_outlier : lm.is_marginalized) ? 1 : 0;
  return n;
}
}  // namespace

int main(int argc, char **) {
  int n_dev = 0;
  dsopp_hip_device_count(&n_dev);
  if (n_dev < 1) {
    std::printf("no GPU: the HIP backend has no CPU fallback\n");
    return 2;
  }
  const bool verbose = argc > 1;
  bool ok = true;
  try {
    {
      Window w;
      fill(w);
      HipFrameMarginalizationStrategy strategy(5, 7, 0.95);
      const std::vector<int32_t> gone = strategy.marginalize({w.pba.get(), w.active, {}, {}});
      const dsopp_hip_marginalization_result &r = strategy.lastResult();
      std::printf("sparse: %d active keyframes, scores", r.n_active);
      for (int i = 0; i < r.n_active; ++i) std::printf(" %.6f", r.scores[i]);
      std::printf("\nsparse: set");
      for (int i = 0; i < r.n_selected; ++i) std::printf(" %d", r.selected[i]);
      std::printf(", marginalised");
      for (int32_t id : gone) std::printf(" %d", id);
      std::printf(", %d landmarks marginalised, %d marked outlier\n", r.n_newly_marginalized, r.n_newly_outlier);
      // no optimisation was noted: a landmark that is out of boundary has no successful optimisation and becomes an outlier (13 of
      // every keyframe but the newest, all 65 of the chosen one), and ActiveKeyframe::marginalize then takes every landmark of the chosen keyframe
      ok = ok && gone == std::vector<int32_t>{1} && r.n_selected == 1 && r.selected[0] == 1;
      ok = ok && r.n_newly_marginalized == kLandmarks && r.n_newly_outlier == 6 * 13 + kLandmarks;
      for (int i = 0; i < kFrames; ++i) {
        const KeyframeView &f = w.frames[static_cast<size_t>(i)];
        if (verbose) std::printf("  keyframe %d: marginalised %d, %d landmarks marginalised, %d outlier\n", i, f.is_marginalized ? 1 : 0, count(f, false), count(f, true));
        ok = ok && f.is_marginalized == (i == 1) && count(f, false) == (i == 1 ? kLandmarks : 0);
        ok = ok && count(f, true) == (i == 1 ? kLandmarks : (i == kFrames - 1 ? 0 : 13));
      }
    }
    {
      Window w;
      fill(w);
      HipFrameMarginalizationStrategy strategy(6);
      const std::vector<int32_t> gone = strategy.marginalize({w.pba.get(), w.active, {}, {}});
      std::printf("maximum_size 6: marginalised");
      for (int32_t id : gone) std::printf(" %d", id);
      std::printf(", %d landmarks marginalised\n", strategy.lastResult().n_newly_marginalized);
      ok = ok && gone == std::vector<int32_t>{0, 1} && strategy.lastResult().n_newly_marginalized == 2 * kLandmarks;
      ok = ok && w.frames[0].is_marginalized && w.frames[1].is_marginalized && !w.frames[2].is_marginalized;
    }
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  std::printf(ok ? "ok\n" : "UNEXPECTED CHOICE\n");
  return ok ? 0 : 1;
}
