// rt_k_features_shard.hip — the first-hit feature pass over a shard's slab (rt.h rt_render_features_shard_async without
// a chain; rt_kernels_shard.h render_features_slab, render_features_slab_lds), one instantiation per form of
// rt::plan_features exactly as rt_k_features.hip has them, and the record merge (assemble_records).
#include "rt_kernels_shard.h"

namespace rt {
const void* features_shard_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    if (P.leaf_lds)
      return P.pk ? (const void*)render_features_slab_lds<FW, true, true> : (const void*)render_features_slab_lds<FW, true, false>;
    return P.pk ? (const void*)render_features_slab_lds<FW, false, true> : (const void*)render_features_slab_lds<FW, false, false>;
  }
  if (P.walk == kFeatWide)
    return P.pk ? (const void*)render_features_slab<FW, true, false> : (const void*)render_features_slab<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_features_slab<FM, false, false>
                              : (const void*)render_features_slab<FM, false, true>;
}

int assemble_records_launch(const rtd::SlabGeometry& G, const void* d_slabs, void* d_image, void* stream) {
  // (slab < 2^32: the callers' check; blockIdx.y strides over the shards)
  const dim3 grid((unsigned)((G.slab * 4 + kAssembleBlock - 1) / kAssembleBlock), (unsigned)std::min(G.shard_count, 65535));
  hipLaunchKernelGGL(assemble_records, grid, dim3(kAssembleBlock), 0, (hipStream_t)stream, G, (const uint4*)d_slabs,
                     (uint4*)d_image);
  return (int)hipGetLastError();
}
}  // namespace rt
