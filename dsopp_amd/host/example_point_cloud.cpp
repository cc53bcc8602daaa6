// Self-contained driver of HipMap (dsopp_hip_solvers.hpp): the track's side of a short keyframe sequence over the C-ABI alone —
//   push, solve, update, choose, update, push
// as the tracker orders them (src/tracker/tracker/src/monocular_tracker.cpp:489-514): four keyframes of an integer-valued scene (a textured
// plane at z = 4, the camera stepping 3 pixels along x per keyframe) enter a HipPhotometricBundleAdjustment and the map; the window is
// solved and the map updated; the maximum_size strategy (3) lets the oldest keyframe go and the map is updated again (its records are
// marginalised); a fifth keyframe folds the oldest out of the window, which finalises it in the map; one more solve and update.
//   example_point_cloud
// Prints the exporter's cloud (world frame, image colours, every class, no filter): per point keyframe index, record index, the bits of
// x, y, z, the colour, the type, and the bits of the relative baseline and of the inverse depth's variance.
// tests/test_gpu_point_cloud.py composes the same calls through the Python binding and compares the output byte for byte.
// Exit code 0, 2 without a GPU: there is no CPU fallback.
//   g++ -std=c++17 example_point_cloud.cpp -L../lib -ldsopp_hip -Wl,-rpath,$PWD/../lib -o example_point_cloud
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <memory>

#include "dsopp_hip_solvers.hpp"

using namespace dsopp_hip_host;

namespace {
constexpr int W = 64, H = 48, kFrames = 5, kLandmarks = 65, kStep = 3;
constexpr double fx = 45, fy = 45, cx = 32, cy = 24, Z = 4.0;

int triangle(int x, int period) {
  const int r = x % (2 * period);
  return r < period ? r : 2 * period - r;
}
/** the plane's texture at the pixel (x, y) of keyframe 0: integers only, so that every caller renders the same bytes */
int texture(int x, int y) { return 40 + 3 * triangle(x, 17) + 2 * triangle(y, 13) + 4 * triangle(x + y, 7); }

/** keyframe i sees the plane shifted by kStep * i pixels; BGR = (t, t + 10, t + 20) */
std::vector<uint8_t> render(int i) {
  std::vector<uint8_t> bgr(3 * static_cast<size_t>(W) * H);
  for (int v = 0; v < H; ++v)
    for (int u = 0; u < W; ++u) {
      const int t = texture(u + kStep * i, v);
      uint8_t *px = &bgr[3 * (static_cast<size_t>(v) * W + u)];
      px[0] = static_cast<uint8_t>(t), px[1] = static_cast<uint8_t>(t + 10), px[2] = static_cast<uint8_t>(t + 20);
    }
  return bgr;
}

uint64_t bits(double x) {
  uint64_t b;
  std::memcpy(&b, &x, sizeof(b));
  return b;
}
}  // namespace

int main() {
  int n_dev = 0;
  dsopp_hip_device_count(&n_dev);
  if (n_dev < 1) {
    std::printf("no GPU: the HIP backend has no CPU fallback\n");
    return 2;
  }
  try {
    const TrustRegionOptions opt{7, 1e5, 1e-8, 1e-8, {1e12, 1e8}, 1e16, 20};
    HipPhotometricBundleAdjustment pba(opt, true, true);
    check(dsopp_hip_window_set_deterministic(pba.handle(), 1));  // (the same bits on every run: the output is compared)
    HipMap map(true, 1, 0.05);
    const PinholeModel model{fx, fy, cx, cy};
    std::vector<std::unique_ptr<DevicePyramid>> pyramids;
    std::vector<KeyframeView> frames(kFrames);
    auto push = [&](int i) {
      const std::vector<uint8_t> bgr = render(i);
      pyramids.push_back(std::make_unique<DevicePyramid>(W, H, 1));
      pyramids.back()->buildColour(nullptr, nullptr, bgr.data(), nullptr, nullptr, true);
      KeyframeView &f = frames[static_cast<size_t>(i)];
      f.keyframe_id = i;
      f.timestamp = 1000 * (i + 1);
      f.t_world_agent = {0, 0, 0, 1, i * (kStep * (Z / fx)), 0, 0};
      f.exposure_time = 1;
      f.affine_brightness = {0, 0};
      f.is_marginalized = false;
      f.pyramids = pyramids.back().get();
      for (int k = 0; k < kLandmarks; ++k) {
        LandmarkView lm;
        const int u = 8 + (k * 7) % (W - 16), v = 8 + (k * 5) % (H - 16);
        lm.projection = {static_cast<double>(u), static_cast<double>(v)};
        lm.idepth = 1.0 / Z;
        static const int px[8] = {0, -1, 1, -2, 0, 2, -1, 0}, py[8] = {2, 1, 1, 0, 0, 0, -1, -2};
        for (int p = 0; p < 8; ++p) lm.patch[static_cast<size_t>(p)] = texture(u + px[p] + kStep * i, v + py[p]) + 10;
        lm.is_marginalized = lm.is_outlier = false;
        f.active_landmarks.push_back(lm);
      }
      for (int j = 0; j < i; ++j) {
        if (frames[static_cast<size_t>(j)].is_marginalized) continue;
        f.reprojection_statuses[j] = std::vector<uint8_t>(kLandmarks, DSOPP_HIP_STATUS_OK);
        frames[static_cast<size_t>(j)].reprojection_statuses[i] = std::vector<uint8_t>(kLandmarks, DSOPP_HIP_STATUS_OK);
      }
      pba.pushFrame(f, 0, model, i == 0 ? FrameParameterization::kFixed : FrameParameterization::kFree);
      for (int j = 0; j < i; ++j)
        if (!frames[static_cast<size_t>(j)].is_marginalized) pba.updateLocalFrame(frames[static_cast<size_t>(j)]);
      map.addKeyframe(pba, i, pyramids.back().get());
    };
    for (int i = 0; i < kFrames - 1; ++i) push(i);
    pba.solve();
    map.update(pba);
    HipFrameMarginalizationStrategy strategy(3);
    std::vector<KeyframeView *> active;
    for (int i = 0; i < kFrames - 1; ++i) active.push_back(&frames[static_cast<size_t>(i)]);
    const std::vector<int32_t> gone = strategy.marginalize({&pba, active, {}, {}});
    map.update(pba);
    push(kFrames - 1);
    pba.solve();
    map.update(pba);

    dsopp_hip_map_export_options o;
    dsopp_hip_map_default_export_options(&o);
    o.classes = DSOPP_HIP_MAP_CLASS_ACTIVE | DSOPP_HIP_MAP_CLASS_MARGINALIZED | DSOPP_HIP_MAP_CLASS_OUTLIER;
    o.colours = DSOPP_HIP_MAP_COLOURS_IMAGE;
    const PointCloud c = map.exportCloud(o);
    std::printf("marginalised");
    for (int32_t id : gone) std::printf(" %d", id);
    std::printf("; keyframes");
    for (int32_t id : map.keyframeIds()) std::printf(" %d:%d", id, map.numRecords(id));
    std::printf("; points %zu; per keyframe", c.xyz.size());
    for (int32_t n : c.per_keyframe_counts) std::printf(" %d", n);
    std::printf("\n");
    for (size_t i = 0; i < c.xyz.size(); ++i)
      std::printf("%d %d %016" PRIx64 " %016" PRIx64 " %016" PRIx64 " %d %d %d %d %016" PRIx64 " %016" PRIx64 "\n", c.keyframe_index[i], c.record_index[i],
                  bits(c.xyz[i][0]), bits(c.xyz[i][1]), bits(c.xyz[i][2]), c.rgb[i][0], c.rgb[i][1], c.rgb[i][2], c.type[i], bits(c.relative_baseline[i]),
                  bits(c.idepth_variance[i]));
    // the viewer's storage of the newest keyframe's active class holds the same points in the keyframe's own frame
    PointsStorage storage;
    map.points(kFrames - 1, PointStorageType::kActive, storage);
    std::printf("viewer: %zu active points of keyframe %d, %zu colours, %zu default colours, %zu semantic colours\n", storage.points.size(), kFrames - 1,
                storage.colors.size(), storage.default_colors.size(), storage.semantics_colors.size());
  } catch (const SolverError &e) {
    std::printf("error %d: %s\n", e.code, e.what());
    return 1;
  }
  return 0;
}
