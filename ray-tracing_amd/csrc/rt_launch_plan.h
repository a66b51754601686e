// rt_launch_plan.h — the tier-B launch decision as plain data (rt_launch_plan.cpp): which kernel form a
// launch takes, its block, grid and LDS bytes, its tunables, its chunk batches and scratch needs, decided
// from the uploaded world's counts, the render parameters, the CU count and the RTAMD_* knobs. Host only,
// no HIP: rt_render.hip launches what the plan says, rt_internal_launch_plan returns it without a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt.h"
#include "rt_layout.h"

namespace rt {

// Chunk sums: [chunk][slab pixel][3] doubles, kept on the ctx and grown on demand, at most kPartialCap bytes
// (2 GiB; RTAMD_PARTIAL_CAP overrides, for tests): a frame with more chunks renders them in batches of
// consecutive chunks, one launch each (C5 at 2000 spp: 24.9 GB of chunk sums in 13 batches), and
// combine_chunks folds each batch into a running per-pixel sum in chunk order — the sum rt.h defines,
// whatever the batching.
constexpr size_t kPartialCap = 2ull << 30;
// Dynamic LDS a CU's workgroup may take: 160 KiB less the replacement loop's static per-wave work
// queues (16 waves x 8 B).
constexpr size_t kLdsBudget = 160 * 1024 - 16 * 8;

// Every RTAMD_* knob of a tier-B launch (field = the lower-case name; DESIGN.md §3 has the table), read once
// per launch by read_knobs() and never cached: callers change the environment between two renders of one
// process. Clamped there; -1 = unset where the default depends on the world (plan_launch resolves it).
struct LaunchKnobs {
  int waves = 0;           // 1..4; 0: unset or out of range
  bool waves_set = false;  // RTAMD_WAVES is set at all: no automatic 4th wave
  bool no_cold = false, packed_keys = true, lds = true, leaf_lds = true, replace = true, tile_rev = false;
  int wide = -1;           // 0 / 1; -1: rebuilt worlds
  int chunk = 0;           // 0: rt.h's rt_sample_chunk
  size_t partial_cap = kPartialCap;
  int trav_stop = -1, leaf_stop = -1, batch = 1024, batch_floor = -1, box_first = 4, med_batch = 0;
  int tail = 768;          // tail items per CU
};
LaunchKnobs read_knobs();
int chunk_knob();  // (RTAMD_CHUNK alone: LaunchKnobs::chunk)

// What the decision reads of an uploaded world (rt_prepare.h world_shape: PreparedScene's counts and kinds).
struct WorldShape {
  unsigned features = 0;
  int n_nodes = 0, n_wnodes = 0, n_leaves = 0;
  int stack_need = 0, wide_stack_need = 0;  // deepest traversal stacks the binary / 4-wide tree needs (entries)
  int frames = 1;                           // Scene::frames: instance-frame nesting, 1..RT_MAX_FRAMES
  bool has_wide = false;    // 4-wide trees: the world's (replace_ok worlds with a BVH root) or the mixed walk's
  bool has_qnodes = false;  // spheres-only worlds uploaded with RTAMD_QNODE=1: the 4-wide tree quantised
  bool rebuilt_bvh = false;
  bool mixed_wide = false;  // media / frame world with 4-wide trees over its re-bounded subtrees (F_MIXW)
  bool replace_ok = false;  // frames nest <= RT_MAX_FRAMES deep: the replacement loop applies
  bool far_boxes = false;   // a BVH box coordinate beyond 2^100: the walks take the per-axis box test
  int cu_count = 0;
};

// wide_node's packed-key form for this world's 4-wide walks (RTAMD_PACKED_KEYS=0: the key / reference pairs,
// for A/B runs): the LDS-staged kernels, the counting build of a world they render, and the closest-hits probe.
bool wide_keys_packed(const WorldShape& W, const LaunchKnobs& K);

// The translation unit that instantiates a form's kernel (rt_k_*.hip; the measured reasons are in the units):
// the variant's own table (rt_k_spheres / _cornell / _full / _full_dark), or one of the three single-form units.
enum KernelUnit : int { kUnitVariant, kUnitSpheresPacked, kUnitSpheresGlobal, kUnitCountPacked };

// One render kernel instantiation. loop 0 = one sample per lane walk, 1 = ray replacement over the binary
// tree, 2 = replacement over the 4-wide tree.
struct KernelForm {
  unsigned var = 0;       // rtd::kVar*
  int loop = 0;
  bool lds = false;       // nodes staged in LDS
  bool leaf_lds = false;  // and the 4-wide walk's leaf table (the LEAF_LDS instantiations: 2..4 waves)
  int waves = 1;          // the WAVES the instantiation is compiled with
  bool count = false;     // the counting build (F_COUNT)
  bool skip = false;      // an adaptive frame's launch (F_SKIP)
  bool pk = false;        // packed sort keys: loop 2 LDS-staged, or the packed counting kernel
  bool q = false;         // the quantised tree from global memory (F_QNODE)
  KernelUnit unit = kUnitVariant;
};

struct LaunchPlan {
  KernelForm form;
  // rt_last_launch, and the launch itself: block, dyn_lds_bytes, chunk_batches (launches), and grid: one block
  // per CU (LDS-staged), else the blocks the work asks for, which the launcher bounds by what is resident
  rt_launch_info info{};
  int n_items = 0, entries = 0, n_leaves = 0;  // the kernel's trailing int arguments (global: entries alone)
  LaunchKnobs knobs;  // the launch's knobs with trav_stop, leaf_stop and batch_floor resolved (LaunchConst's)
  float batch_per_item = 0.f;
  uint32_t rev_tiles = 0;
  long long tail_items = 0;
  int chunks_total = 0, per_batch = 0;  // the chunks of this call, and of one launch
  size_t partial_bytes = 0, acc_bytes = 0, tail_bytes = 0;  // scratch needs (acc: unless the span brings its own)
};

// The plan of one launch_philox call: `span_count` chunks from `span_first` (-1: the whole frame) of the frame
// `p` describes. Pure: no HIP call, no environment, no state; rt::set_error on RT_E_INVALID.
// `lc_bytes`: the launch constants' LDS copy (rt_kernels.h kLcBytes).
int plan_launch(const WorldShape& W, const rt_render_params& p, int span_first, int span_count, bool count_build,
                bool adaptive, const LaunchKnobs& K, size_t lc_bytes, LaunchPlan& out);

// The launch of a first-hit feature pass (rt.h rt_render_features; kernels: rt_k_features.hip). A wave takes one
// 8x8 pixel block at a time; `walk` names the closest-hit walk its lanes run, as the closest-hits probe has them.
enum FeatureWalk : int {
  kFeatWide = 2,      // spheres-only worlds with a 4-wide tree: the 4-wide walk (LDS-staged, or from global memory)
  kFeatMixed = 1,     // every other replace_ok world: the F_ALL | F_UV | F_MIXW resumable walk
  kFeatRecursive = 0  // the rest: the recursive walk
};
struct FeaturePlan {
  int walk = kFeatRecursive;
  bool lds = false, leaf_lds = false, pk = false;
  // rt_last_feature_launch: variant = the walk's feature bits, loop = `walk`, work_items = the frame's 8x8 blocks,
  // chunk = 0, chunk_batches = 1; grid: at most one block per CU (LDS-staged), else at most kFeatBlocksPerCU per CU
  rt_launch_info info{};
  int n_items = 0, entries = 0, n_leaves = 0;  // the LDS-staged kernel's trailing int arguments
  // walk_until's step schedule, /64 of the live lanes, as the render's launch of the same world resolves it
  // (scheduling only: no result depends on it). 4-wide walk: leaf steps once at most that many lanes still seek
  // their first leaf (RTAMD_LEAF_STOP, else RTAMD_TRAV_STOP, else 8, or 16 for trees over 20000 nodes); mixed
  // walk: box-only steps while more lanes than that are at BVH nodes (RTAMD_BOX_FIRST, 4).
  int leaf_stop = 0;
};
constexpr int kFeatBlocksPerCU = 8;  // global-memory forms: RT_BLOCK-thread blocks queued per CU (4 waves per SIMD)
// Pure, like plan_launch. Reads of `p` the frame size and RT_FLAG_REFERENCE_CULL; of `K` lds, leaf_lds,
// packed_keys, waves (the LDS-staged form's), wide, and leaf_stop, trav_stop and box_first (FeaturePlan::leaf_stop).
// `chain`: a specular-chain pass (rt.h rt_render_features_chain; kernels: rt_k_features_chain.hip): the same forms,
// the LDS-staged one at 3 waves per SIMD where RTAMD_WAVES does not say otherwise.
// `slab_blocks` >= 0: a pass over a shard's slab (rt.h rt_render_features_shard_async): the same forms for the same
// world, work_items and the grid from the blocks of the shard's tiles (rt_layout.h SlabGeometry::blocks; 0: the
// shard owns no tile and nothing is launched).
int plan_features(const WorldShape& W, const rt_render_params& p, const LaunchKnobs& K, FeaturePlan& out,
                  bool chain = false, long long slab_blocks = -1);

}  // namespace rt
