// rt_k_features_chain_shard.hip — the specular-chain feature pass over a shard's slab (rt.h
// rt_render_features_shard_async with a chain; rt_kernels_shard.h render_features_chain_slab[_lds]), one instantiation
// per form of rt::plan_features exactly as rt_k_features_chain.hip has them, with that unit's fused sincos.
#define RT_FUSED_SINCOS 1
#include "rt_kernels_shard.h"

namespace rt {
const void* features_chain_shard_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    return by_waves<3, 4>(P.info.waves <= 3 ? 3 : 4, [&](auto W) {
      if (P.leaf_lds)
        return P.pk ? (const void*)render_features_chain_slab_lds<FW, true, true, W()>
                    : (const void*)render_features_chain_slab_lds<FW, true, false, W()>;
      return P.pk ? (const void*)render_features_chain_slab_lds<FW, false, true, W()>
                  : (const void*)render_features_chain_slab_lds<FW, false, false, W()>;
    });
  }
  if (P.walk == kFeatWide)
    return P.pk ? (const void*)render_features_chain_slab<FW, true, false>
                : (const void*)render_features_chain_slab<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_features_chain_slab<FM, false, false>
                              : (const void*)render_features_chain_slab<FM, false, true>;
}
}  // namespace rt
