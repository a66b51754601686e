// rt_internal.h — host-side helpers shared by the C-ABI translation units (not installed).
#pragma once
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "rt.h"

namespace rt {

// splitmix-0.1 (System.Random.SplitMix): mix64 is the MurmurHash3 finaliser, mixGamma uses
// Stafford's variant 13 (the reverse of Java's SplittableRandom).
inline uint64_t mix64(uint64_t z) {
  z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdULL;
  z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ULL;
  return z ^ (z >> 33);
}
inline uint64_t mix64v13(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ULL;
  z = (z ^ (z >> 27)) * 0x94d049bb133111ebULL;
  return z ^ (z >> 31);
}
inline uint64_t mix_gamma(uint64_t z) {
  z = mix64v13(z) | 1ULL;
  const int n = __builtin_popcountll(z ^ (z >> 1));
  return n >= 24 ? z : (z ^ 0xaaaaaaaaaaaaaaaaULL);
}
// mkStdGen n = StdGen (mkSMGen (fromIntegral n))  (random-1.2.0; src/Random.hs:20-21)
inline void mk_smgen(uint64_t s, uint64_t out[2]) {
  out[0] = mix64(s);
  out[1] = mix_gamma(s + 0x9e3779b97f4a7c15ULL);
}
// nextWord64
inline uint64_t sm_next(uint64_t& seed, uint64_t gamma) {
  seed += gamma;
  return mix64(seed);
}
// random-1.2.0 `random :: Double` = 1 - word64 / 2^64 (src/Random.hs:23-25)
inline double word_to_draw(uint64_t w) { return 1.0 - (double)w / 18446744073709551616.0; }

void set_error(const std::string& s);
const char* last_error();

struct Box {
  double mn[3], mx[3];
};

// Traversal-stack entries a BVH node needs (rt_trace.h traverse / walk_step), given its
// children's needs. Caller's (makeBVH) nodes are walked left first, with b waiting on the stack
// while a is walked (hit BVHNode, src/Lib.hs:971-988). A rebuilt node (RT_BVH_ORDERED) enters the
// child on the ray's side of the split first, so either child can be walked above the other.
inline int bvh_stack_need(const rt_node& x, int need_a, int need_b) {
  // (either child first; an RT_BVH_MEDIA_FIRST node enters its left child first, like a reference node)
  if ((x.c & RT_BVH_ORDERED) && !(x.c & RT_BVH_MEDIA_FIRST)) return 1 + (need_a > need_b ? need_a : need_b);
  return (1 + need_a > need_b) ? 1 + need_a : need_b;
}

}  // namespace rt

// The work geometry a tier-B launch puts into its launch constants (rt_kernels.h LaunchConst), checked
// without a device: for shard p->shard_rank and a launch of `n_chunks` sample chunks from `chunk_first`
// whose last `tail_items` work-items are dealt one sample per unit, the device's decomposition (work_unit)
// of the units [first, first + n): out5[i] = {valid, px, row, s0, s1}, out_slot[i] the chunk sum's slot
// (kTailSlot + unit for a tail unit); out_totals = {work_total, items_total, tail_start, slab, chunk}.
extern "C" int rt_internal_work_units(const rt_render_params* p, int chunk_first, int n_chunks, long long tail_items,
                                      uint32_t first, int n, int32_t* out5, int64_t* out_slot, int64_t* out_totals);

// The plan of a tier-B launch (rt_launch_plan.h), decided without a device: `desc` prepared as an upload with
// `upload_flags` prepares it, on a device of `cu_count` CUs, for `span_count` chunks from `span_first` (-1: the
// whole frame) of the frame `p` describes, as the counting build (`count_build`) or an adaptive frame's launch
// (`adaptive`), under the environment's RTAMD_* knobs. *out = what rt_last_launch would report, with the blocks
// the work asks for as `grid` where the launcher bounds it by residency (no LDS staging). out_extra (may be
// null) = {n_items, entries, n_leaves, trav_stop, leaf_stop, box_first, med_batch, batch, batch_floor,
// rev_tiles, tail_items, chunks per launch, wide_packed, KernelUnit, grid, the form's WAVES}.
#define RT_PLAN_EXTRA 16
extern "C" int rt_internal_launch_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                       const rt_render_params* p, int span_first, int span_count, int count_build,
                                       int adaptive, rt_launch_info* out, int32_t* out_extra);

// The plan of a first-hit feature pass (rt_launch_plan.h plan_features), decided without a device, under the
// environment's RTAMD_LDS, RTAMD_LEAF_LDS, RTAMD_PACKED_KEYS, RTAMD_WAVES and RTAMD_WIDE: *out = what
// rt_last_feature_launch would report; out_extra (may be null) = {n_items, entries, n_leaves, wide_packed,
// leaf_stop}.
#define RT_FEATURES_PLAN_EXTRA 5
extern "C" int rt_internal_features_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                         const rt_render_params* p, rt_launch_info* out, int32_t* out_extra);

// The same for a specular-chain pass (rt_render_features_chain): RT_E_INVALID for a chain the pass rejects.
extern "C" int rt_internal_features_chain_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                               const rt_render_params* p, const rt_feature_chain* chain,
                                               rt_launch_info* out, int32_t* out_extra);

// The same for a pass over a shard's slab (rt_render_features_shard_async, rt_render_ids_shard_async): the shard is
// (p->tile, p->shard_rank, p->shard_count); `chain` != 0: the chain passes' plan (an ID pass's too). The forms are
// the image-order pass's, work_items the shard's tiles inside the image x (tile / 8)^2 (0: it owns none).
extern "C" int rt_internal_features_shard_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                               const rt_render_params* p, int chain, rt_launch_info* out,
                                               int32_t* out_extra);

// The same for a material-ID pass (rt_render_ids; `chain` may be null): the chain pass's plan, launched with
// rt_k_ids.hip's kernels. And the hipMalloc calls the ctx's last rt_render_ids*, rt_ids_matte* or rt_ids_preview*
// call made (-1: null ctx), for the tests: a repeat of one size makes none.
struct rt_ctx;
extern "C" int rt_internal_ids_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                    const rt_render_params* p, const rt_feature_chain* chain, rt_launch_info* out,
                                    int32_t* out_extra);
extern "C" int rt_internal_ids_allocs(rt_ctx* ctx);

// rt_denoise_host (rt.h) with one more output for the tests: out_variance (may be null) = V of every pixel after
// the last iteration, W*H doubles in image order, which the ABI keeps to itself.
extern "C" int rt_internal_denoise_host(const rt_denoise_params* params, const double* color, const double* se,
                                        const double* feature_sums, double* out_color, uint8_t* out_rgb8,
                                        rt_denoise_stats* stats, double* out_variance);

struct rt_builder {
  uint64_t seed, gamma;  // RandGen (SMGen)
  std::vector<rt_node> nodes;
  std::vector<rt_material> materials;
  std::vector<rt_texture> textures;
  std::vector<rt_perlin> perlins;
  std::vector<rt_image> images;
  std::vector<uint8_t> pool;
  std::map<int, rt::Box> rotate_boxes;  // Rotate's stored box (src/Lib.hs:733)
  bool failed = false;

  // randomDoubleM (src/Lib.hs:1119-1125) over random-1.2.0 / splitmix-0.1
  double draw() { return rt::word_to_draw(rt::sm_next(seed, gamma)); }
  double draw_r(double mn, double mx) { double rd = draw(); return mn + (mx - mn) * rd; }
};
