// rt_kernels_shard.h — the slab forms of the feature, chain and ID passes (rt.h rt_render_features_shard_async,
// rt_render_ids_shard_async) and the merge of their 64-byte records (rt_assemble_records_async). The kernels are
// rt_kernels.h's loops instantiated with SLAB: the same walks, folds and forms, over the blocks of one shard's slab
// (rt_layout.h slab_block) instead of the image's. Units of their own (rt_k_*_shard.hip), so that the image-order
// kernels compile to what they compile to without them.
#pragma once
#include "rt_kernels.h"

namespace {

#define RT_SLAB_SIDE(F) &stk_mem[((((F) & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + 1) * RT_BLOCK + threadIdx.x]

template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_features_slab(FeatureSlabArgs X) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  features_loop<F, PK, REC, true>(X.C.A, X.C.A.S, &stk_mem[threadIdx.x], RT_BLOCK, RT_SLAB_SIDE(F), &X.G);
}
template <unsigned F, bool LEAF_LDS, bool PK>
__global__ void __launch_bounds__(1024) render_features_slab_lds(FeatureSlabArgs X, int n_nodes, int stack_entries,
                                                                 int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(X.C.A.S, n_nodes, n_leaves, S);
  (void)stack_entries;
  features_loop<F, PK, false, true>(X.C.A, S, stk, (int)blockDim.x, stk, &X.G);
}

template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_features_chain_slab(FeatureSlabArgs X) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  features_chain_loop<F, PK, REC, true>(X.C, X.C.A.S, &stk_mem[threadIdx.x], RT_BLOCK, RT_SLAB_SIDE(F), &X.G);
}
template <unsigned F, bool LEAF_LDS, bool PK, int WAVES>
__global__ void __launch_bounds__(WAVES * 256) render_features_chain_slab_lds(FeatureSlabArgs X, int n_nodes,
                                                                              int stack_entries, int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(X.C.A.S, n_nodes, n_leaves, S);
  (void)stack_entries;
  features_chain_loop<F, PK, false, true>(X.C, S, stk, (int)blockDim.x, stk, &X.G);
}

template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_ids_slab(FeatureSlabArgs X) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  ids_loop<F, PK, REC, true>(X.C, X.C.A.S, &stk_mem[threadIdx.x], RT_BLOCK, RT_SLAB_SIDE(F), &X.G);
}
template <unsigned F, bool LEAF_LDS, bool PK, int WAVES>
__global__ void __launch_bounds__(WAVES * 256) render_ids_slab_lds(FeatureSlabArgs X, int n_nodes, int stack_entries,
                                                                   int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(X.C.A.S, n_nodes, n_leaves, S);
  (void)stack_entries;
  ids_loop<F, PK, false, true>(X.C, S, stk, (int)blockDim.x, stk, &X.G);
}

// The record merge: shard_count slabs (rank-major) -> [H][W] records, a pure byte move in slab order. A thread moves
// 16 bytes, four neighbours one record, a wave sixteen consecutive slots: contiguous loads, and stores in runs of
// 512 bytes (eight pixels of an image row). blockIdx.y strides over the shards; `G` is shard 0's geometry. A padding
// slot (slab_slot_pixel < 0) is not read.
constexpr int kAssembleBlock = 256;
__global__ void __launch_bounds__(kAssembleBlock) assemble_records(SlabGeometry G, const uint4* slabs, uint4* image) {
  const long long t = (long long)blockIdx.x * kAssembleBlock + threadIdx.x;
  if (t >= G.slab * 4) return;
  const uint32_t slot = (uint32_t)(t >> 2), quad = (uint32_t)t & 3u;
  for (int shard = (int)blockIdx.y; shard < G.shard_count; shard += (int)gridDim.y) {
    G.shard_rank = shard;
    const long long pixel = slab_slot_pixel(G, slot);
    if (pixel >= 0) image[pixel * 4 + quad] = slabs[((long long)shard * G.slab + slot) * 4 + quad];
  }
}

}  // namespace
