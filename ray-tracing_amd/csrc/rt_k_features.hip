// rt_k_features.hip — the first-hit feature pass's kernels (rt.h rt_render_features; rt_kernels.h render_features,
// render_features_lds), one instantiation per form of rt::plan_features: the spheres-only variant's 4-wide walk
// LDS-staged (with and without the leaf table, packed keys or key / reference pairs) and from global memory, the
// mixed resumable walk, and the recursive walk. The plain Philox key and sincos forms: nothing here was tuned.
#include "rt_kernels.h"

namespace rt {
const void* features_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    if (P.leaf_lds)
      return P.pk ? (const void*)render_features_lds<FW, true, true> : (const void*)render_features_lds<FW, true, false>;
    return P.pk ? (const void*)render_features_lds<FW, false, true> : (const void*)render_features_lds<FW, false, false>;
  }
  if (P.walk == kFeatWide)
    return P.pk ? (const void*)render_features<FW, true, false> : (const void*)render_features<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_features<FM, false, false>
                              : (const void*)render_features<FM, false, true>;
}
}  // namespace rt
