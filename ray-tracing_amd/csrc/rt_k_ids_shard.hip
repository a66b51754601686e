// rt_k_ids_shard.hip — the material-ID pass over a shard's slab (rt.h rt_render_ids_shard_async; rt_kernels_shard.h
// render_ids_slab[_lds]), one instantiation per form of rt::plan_features exactly as rt_k_ids.hip has them, with that
// unit's fused sincos. One kernel for both modes: without a chain it runs with max_bounces = 0.
#define RT_FUSED_SINCOS 1
#include "rt_kernels_shard.h"

namespace rt {
const void* ids_shard_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    return by_waves<3, 4>(P.info.waves <= 3 ? 3 : 4, [&](auto W) {
      if (P.leaf_lds)
        return P.pk ? (const void*)render_ids_slab_lds<FW, true, true, W()> : (const void*)render_ids_slab_lds<FW, true, false, W()>;
      return P.pk ? (const void*)render_ids_slab_lds<FW, false, true, W()> : (const void*)render_ids_slab_lds<FW, false, false, W()>;
    });
  }
  if (P.walk == kFeatWide)
    return P.pk ? (const void*)render_ids_slab<FW, true, false> : (const void*)render_ids_slab<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_ids_slab<FM, false, false> : (const void*)render_ids_slab<FM, false, true>;
}
}  // namespace rt
