// rt_k_features_chain.hip — the specular-chain feature pass's kernels (rt.h rt_render_features_chain; rt_kernels.h
// render_features_chain, render_features_chain_lds), one instantiation per form of rt::plan_features, as
// rt_k_features.hip has them for the first-hit pass; the staged form for 3 and for 4 waves per SIMD (rt_kernels.h).
// The plain Philox key. A Metal scatter's sine and cosine through the fused sincos call (rt_device.h): the bits of
// sin and cos (tests/test_gpu_shading_fp64.py), and no polynomial constants held across the walk.
#define RT_FUSED_SINCOS 1
#include "rt_kernels.h"

namespace rt {
const void* features_chain_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    return by_waves<3, 4>(P.info.waves <= 3 ? 3 : 4, [&](auto W) {
      if (P.leaf_lds)
        return P.pk ? (const void*)render_features_chain_lds<FW, true, true, W()>
                    : (const void*)render_features_chain_lds<FW, true, false, W()>;
      return P.pk ? (const void*)render_features_chain_lds<FW, false, true, W()>
                  : (const void*)render_features_chain_lds<FW, false, false, W()>;
    });
  }
  if (P.walk == kFeatWide)
    return P.pk ? (const void*)render_features_chain<FW, true, false> : (const void*)render_features_chain<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_features_chain<FM, false, false>
                              : (const void*)render_features_chain<FM, false, true>;
}
}  // namespace rt
