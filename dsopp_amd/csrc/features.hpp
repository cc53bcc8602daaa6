// The tracking-feature extractor handle, shared by the Sobel extractor (features.hip) and the eigen extractor (features_eigen.hip):
// one handle type, so set_mask / extract / get_state / destroy and dsopp_hip_immature_set_create_from_features serve both kinds.
#pragma once
#include <cstdint>
#include <memory>
#include <vector>

#include "common.hpp"
#include "pyramid.hpp"

namespace dsopp_hip {

enum class ExtractorKind { Sobel, Eigen };

struct PyramidDeleter {
  void operator()(dsopp_hip_pyramid *p) const { dsopp_hip_pyramid_destroy(p); }
};

/** what the eigen extractor keeps beyond the shared members (features_eigen.hip) */
struct EigenExtractorState {
  std::unique_ptr<dsopp_hip_pyramid, PyramidDeleter> pyramid;  // the extractor's own raw pyramid (5 levels, f64, identity LUT, no vignette)
  DeviceBuffer<uint8_t> d_pattern;  // W * H random bytes (srand(3141592), (uint8_t)rand())
  DeviceBuffer<double> d_dirs;      // 16 x (cos, sin)
  DeviceBuffer<double> d_raw, d_map;  // threshold map before / after the 3 x 3 mean
  DeviceBuffer<uint16_t> d_bits;      // per pixel: possible (bits 0-4) / certain (bits 5-9) per level
  DeviceBuffer<uint16_t> d_wbits;     // per level-0 window of every top window: the OR of its pixels' bits, bit 15 = visited
  DeviceBuffer<int> d_count, d_undet, d_start;  // per top window: emissions, undetermined flag, start count
  DeviceBuffer<int> d_count2, d_split;          // per level-2 window: emissions; per top window: walked as 16 independent parts
  DeviceBuffer<int> d_result;                   // found, chained windows of the pass
  PinnedMem<int> h_result;
  // the statistics of the last extract (dsopp_hip_feature_extractor_get_eigen_stats)
  int passes = 0, potentials[2] = {0, 0}, found[2] = {0, 0}, chained = 0;
};

}  // namespace dsopp_hip

struct dsopp_hip_feature_extractor {
  dsopp_hip::StreamRef sr;
  dsopp_hip::ExtractorKind kind = dsopp_hip::ExtractorKind::Sobel;
  int width = 0, height = 0;
  double density = 0, quantile = 0;
  // the reference extractor's state (sobel_tracking_features_extractor.hpp:33-37, tracking_features_extractor.hpp:49-53); the eigen
  // extractor keeps current_potential_ in window_size and no threshold
  bool initialized = false;
  int threshold = 0;
  int window_size = 15;  // TrackingFeaturesExtractor::current_potential_ before the first call (tracking_features_extractor.hpp:51)
  int found_last = 0;
  bool has_mask = false;
  dsopp_hip::DeviceBuffer<uint8_t> d_image, d_mask, d_valid;  // u8 image | caller's mask (row pass output reuses it) | eroded mask (1 = valid)
  dsopp_hip::DeviceBuffer<int16_t> d_grad;
  dsopp_hip::DeviceBuffer<unsigned> d_hist;
  dsopp_hip::DeviceBuffer<int> d_hit, d_list, d_count, d_final;  // per-window hit | hits in window order | their count | the returned list
  dsopp_hip::DeviceBuffer<char> d_temp;                          // device select scratch
  dsopp_hip::PinnedMem<uint8_t> h_image;
  dsopp_hip::PinnedMem<int> h_count, h_list, h_final;
  dsopp_hip::PinnedMem<unsigned> h_hist;
  std::vector<int> final_list;  // the returned list as pixel indices y * W + x (host copy)
  dsopp_hip::Event final_ready;  // d_final written (recorded behind its upload)
  std::unique_ptr<dsopp_hip::EigenExtractorState> eigen;  // kind == Eigen only
};

namespace dsopp_hip {
/** dsopp_hip_feature_extractor_extract / _extract_from_pyramid for an eigen handle (features_eigen.hip): the image from the host, or,
 *  when image_host is null, the 8-bit image image_dev that the extractor's stream may read */
void eigenExtract(dsopp_hip_feature_extractor *ex, const uint8_t *image_host, const uint8_t *image_dev, int32_t capacity, double *xy, int32_t *n);
}  // namespace dsopp_hip
