// The marginalisation strategies' choice on the device (marginalization_kernels.hpp) and the landmarks' count of successful optimisations.
// The window's side — which arrays, which streams, what `apply` does with the answer — is dsopp_hip_window_choose_marginalization in pba.hip.
#include "marginalization_kernels.hpp"

#include "common.hpp"

namespace dsopp_hip {

static_assert(sizeof(MargArgs) <= 4096, "the frames' descriptors travel as kernel arguments");

void launchChooseMarginalization(const MargArgs &args, hipStream_t stream) {
  margCountAndChooseKernel<<<static_cast<unsigned>(args.n_blocks), kMargBlock, 0, stream>>>(args);
  margLandmarksKernel<<<static_cast<unsigned>(args.n_blocks), kMargBlock, 0, stream>>>(args);
  HIP_CHECK(hipGetLastError());
}

void launchNoteOptimization(const uint8_t *flags, const int32_t *n_inliers, const int32_t *to_internal, int32_t *successes, int n, hipStream_t stream) {
  if (n <= 0) return;
  margNoteOptimizationKernel<<<static_cast<unsigned>((n + kMargBlock - 1) / kMargBlock), kMargBlock, 0, stream>>>(flags, n_inliers, to_internal, successes, n);
  HIP_CHECK(hipGetLastError());
}

}  // namespace dsopp_hip

extern "C" void dsopp_hip_marginalization_default_options(dsopp_hip_marginalization_options *o) {
  if (!o) return;
  o->strategy = DSOPP_HIP_MARGINALIZATION_SPARSE;
  o->minimum_size = 5;  // test/test_data/tummono/mono.yaml
  o->maximum_size = 7;
  o->maximum_share_marginalized = 0.95;
}
