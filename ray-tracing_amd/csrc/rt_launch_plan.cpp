// rt_launch_plan.cpp — the tier-B launch decision (rt_launch_plan.h). Host only, no HIP.
#include "rt_launch_plan.h"

#include <algorithm>
#include <cstdlib>

#include "rt_internal.h"

using namespace rtd;

namespace rt {
namespace {
// An integer knob clamped to [lo, hi]; `unset` when the variable is not there.
int env_int(const char* name, int lo, int hi, int unset) {
  const char* e = std::getenv(name);
  return e ? std::max(lo, std::min(hi, std::atoi(e))) : unset;
}
bool env_off(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '0';
}
int invalid(const char* s) {
  set_error(s);
  return RT_E_INVALID;
}
}  // namespace

// RTAMD_CHUNK: another chunk size, for timing experiments only (it changes the summation order,
// so the image no longer follows rt.h's tier-B definition)
int chunk_knob() { return env_int("RTAMD_CHUNK", 1, 1 << 30, 0); }

LaunchKnobs read_knobs() {
  LaunchKnobs K;
  K.waves_set = std::getenv("RTAMD_WAVES") != nullptr;
  K.waves = env_int("RTAMD_WAVES", 0, 5, 0) % 5;  // (1..4, else 0)
  K.no_cold = std::getenv("RTAMD_NO_COLD") != nullptr;  // the spheres unit's global-memory 4-wide kernel
  K.packed_keys = !env_off("RTAMD_PACKED_KEYS");        // 0: the key / reference pairs
  K.lds = !env_off("RTAMD_LDS");                        // 0: no LDS-staged kernel
  K.leaf_lds = !env_off("RTAMD_LEAF_LDS");              // 0: leaves never in LDS
  K.replace = !env_off("RTAMD_REPLACE");                // 0: the per-sample loop
  if (const char* e = std::getenv("RTAMD_WIDE")) K.wide = e[0] != '0';
  K.chunk = chunk_knob();
  if (const char* e = std::getenv("RTAMD_PARTIAL_CAP")) K.partial_cap = (size_t)std::max(1ll, std::atoll(e));
  K.trav_stop = env_int("RTAMD_TRAV_STOP", 0, 63, -1);
  K.leaf_stop = env_int("RTAMD_LEAF_STOP", 0, 64, -1);
  K.batch = env_int("RTAMD_BATCH", 1, 4096, K.batch);
  K.batch_floor = env_int("RTAMD_BATCH_FLOOR", 0, 1024, -1);
  K.box_first = env_int("RTAMD_BOX_FIRST", 0, 64, K.box_first);
  K.med_batch = env_int("RTAMD_MED_BATCH", 0, 64, K.med_batch);
  K.tile_rev = std::getenv("RTAMD_TILE_REV") && !env_off("RTAMD_TILE_REV");
  K.tail = env_int("RTAMD_TAIL", 0, 1 << 16, K.tail);
  return K;
}

bool wide_keys_packed(const WorldShape& W, const LaunchKnobs& K) {
  return W.has_wide && rt_wkey_fits(W.n_wnodes, W.n_leaves) && K.packed_keys;
}

int plan_launch(const WorldShape& W, const rt_render_params& p, int span_first, int span_count, bool count_build,
                bool adaptive, const LaunchKnobs& K, size_t lc_bytes, LaunchPlan& out) {
  LaunchPlan P;
  KernelForm& f = P.form;
  rt_launch_info& I = P.info;
  const FrameGeometry g = frame_geometry(&p, K.chunk);
  I.work_items = g.slab * g.chunks, I.chunk = g.chunk;  // (the whole frame's work, whatever the span)
  // (the span: the whole frame, or a progressive frame's next chunks; its batches: kPartialCap)
  P.chunks_total = span_count < 0 ? g.chunks : span_count;
  if (span_first < 0 || P.chunks_total < 1 || span_first + P.chunks_total > g.chunks) return invalid("bad chunk span");
  const size_t per_chunk = (size_t)g.slab * 3 * sizeof(double);
  P.per_batch = (int)std::max<size_t>(1, std::min<size_t>((size_t)P.chunks_total, K.partial_cap / per_chunk));
  I.chunk_batches = (P.chunks_total + P.per_batch - 1) / P.per_batch;
  P.partial_bytes = (size_t)P.per_batch * per_chunk;
  P.acc_bytes = I.chunk_batches > 1 ? per_chunk : 0;
  const bool ref_cull = (p.flags & RT_FLAG_REFERENCE_CULL) || W.far_boxes;  // (rt_render.hip cull())
  f.var = variant_for(W.features);
  f.count = count_build, f.skip = adaptive;  // (an adaptive frame: the F_SKIP kernels, which test its mask)
  if (f.skip && f.count) return invalid("the counting build has no adaptive-frame kernels");
  // Replacement loop (RTAMD_REPLACE=0 disables) for every world whose instance frames nest at most
  // RT_MAX_FRAMES deep; worlds with media or frames walk the caller's tree in the reference's order.
  // Over the 4-wide tree when one was built (RTAMD_WIDE=0 disables; the reference-cull flag asks
  // for the binary tree's exact box test).
  const bool replace = W.replace_ok && K.replace;
  // The wide tree pays off on rebuilt (>= 16-leaf) worlds; small worlds keep the binary walk
  // (Cornell: 409 vs 262-399 Msamples/s measured), RTAMD_WIDE=1 forces it.
  const bool want_wide = K.wide >= 0 ? K.wide != 0 : W.rebuilt_bvh;
  // (the full variant has no 4-wide instantiation: its media-free worlds walk the binary tree)
  const bool wide = replace && W.has_wide && !ref_cull && want_wide && !is_full(f.var);
  f.loop = wide ? 2 : (replace ? 1 : 0);
  // The frame's tail (the full variants' replacement loop, kTail in rt_kernels.h; the per-sample loop claims
  // whole work-items): the last `tail_items` work-items of each launch are dealt one sample per unit, their
  // colours summed in sample order afterwards (tail_combine): the sums rt.h defines, whatever the dealing.
  // RTAMD_TAIL: tail items per CU (default 768, one per lane of 12 waves; 0: no tail).
  P.tail_items = (f.loop && is_full(f.var)) ? (long long)W.cu_count * K.tail : 0;
  // (work-unit indices are 32-bit on the device, and wave claims may run up to one batch per wave
  // past the end: keep 2^24 of headroom)
  if (launch_units(g.slab * P.per_batch, P.tail_items, g.chunk) >= (1ll << 32) - (1ll << 24))
    return invalid("image too large: more than 2^32 - 2^24 work units per shard and launch");
  P.tail_bytes = (size_t)std::min(g.slab * P.per_batch, P.tail_items) * (size_t)g.chunk * 3 * sizeof(double);
  // The tunables (P.knobs: K's, the unset ones resolved). Refill when at most trav_stop/64 of a wave's live
  // lanes still walk (measured: C2 flat at 2-8, -4 % at 16; the 100k-sphere C5 tree, walks ~3x longer, best at 16)
  // (the full variant's walks over the caller's tree: 16 in round 2, C4 1496 vs 1567 ms at 200 spp; with
  // the mixed walk (round 3) 8: C4 at 100 spp 323.7 vs 326.0 ms, 24: 334.0)
  P.knobs = K;
  if (K.trav_stop < 0) P.knobs.trav_stop = W.n_nodes > 20000 ? 16 : 8;
  // leaf steps once <= that many lanes still seek their first leaf (measured: C2 212.6 ms at 6-8/64
  // vs 219.7 at 0 and 232 without postponement; C5 (16 spp) 219.9 ms at 16/64 vs 326 at 0)
  if (K.leaf_stop < 0) P.knobs.leaf_stop = P.knobs.trav_stop;
  // Work-items a wave claims per atomic: one claim per batch instead of one per acquisition round
  // (RTAMD_BATCH; 1 = the lanes' exact need every time). The batch tapers as the frame runs out: a
  // wave claims at most rem / (16 * waves) items when about `rem` remain, so the waves' unstarted
  // claims together never exceed 1/16 of what is left.
  P.batch_per_item = (float)(1.0 / (16.0 * ((double)W.cu_count * 4 * 4)));  // at most 4 waves per SIMD
  // ... but never below one item per lane of the claiming wave (RTAMD_BATCH_FLOOR): near the end of
  // a frame the taper otherwise shrinks claims to the lanes' exact need, one contended atomic per
  // few items; 64 items are consumed by the wave's lanes in parallel, so they hoard nothing (C2
  // per shard at N = 8: 21.05 -> 19.95 ms, 0.83 -> 0.88 of ideal; N = 1 140.7 -> 139.3 ms; 256:
  // 21.2 ms, 512: 26 ms). Not for the full variant, whose items are long and uneven (C4 at 100
  // spp with 128: 286 -> 293 ms): 0 there.
  if (K.batch_floor < 0) P.knobs.batch_floor = is_full(f.var) ? 0 : 64;
  // binary walks of the full variant (media / frame worlds, C4): box-only steps while more than
  // box_first/64 of the live lanes are at BVH nodes (4-wide nodes count; measured on C4 at 100 spp, round
  // 2: 64 (never) 430 ms, 48 416, 32 406, 16 398, 8 413; round 5, hoisted media and one 4-wide tree, with
  // trav_stop 8: 0 189.6, 2 178.6, 4 174.6, 8 176.3, 16 182.3, 32 185.3; C3's Cornell kernel does not
  // take it): knobs.box_first.
  // lanes at a medium wait for med_batch of them (round 4, C4 at 100 spp: 0 249.0 ms, 4 245.3, 8 245.9,
  // 16 295). Since round 5 a world's own media are hoisted (RT_BVH_MEDIA_FIRST, taken where walks start):
  // only media inside instance frames still wait here, none in C4 (0 174.6 ms vs 4 176.3): knobs.med_batch 0.
  // work order only (the chunk sums do not depend on it): the slab's tiles last to first
  P.rev_tiles = K.tile_rev ? (uint32_t)g.per_shard : 0u;

  // waves per SIMD (measured): spheres 4 when the LDS-staged kernel fits at 4 (C2 158.4 ms vs
  // 166.6 at 3, 203.2 at 2), else 3 (C5 186.7 ms vs 228.5 at 4, -15 % at 2); Cornell-like on the
  // replacement loop 3 (C3 359.6 ms vs 374.3 at 4, 453.3 at 2), 1 on the per-sample loop; full
  // variant on the replacement loop 3 (C4 at 100 spp: 90.9 vs 87.5 Msamples/s at 2), on the
  // per-sample loop 2 despite 784 B/lane of scratch (C4 35.2 vs 23.4 at 1 wave, 9.1 at 3)
  int waves = K.waves ? K.waves : ((f.var == kVarSpheres || f.loop) ? 3 : (is_full(f.var) ? 2 : 1));
  // Per lane after the walk stack: Side slots, then the 4 lane ints philox_loop2 keeps in LDS (RT_LANE_LDS).
  // The stack: this world's bound (wide_node writes 3 slots)
  const int side_ints = side_ints_of(f.var, W.frames, f.loop) + (lane_lds_of(f.var, f.loop) ? 4 : 0);
  P.entries = wide ? W.wide_stack_need + 3 : W.stack_need + 2;
  const bool pk = wide && wide_keys_packed(W, K);
  // LDS-staged kernel when the traversal's node array plus the stacks fit one CU's 160 KiB
  // (RTAMD_LDS=0 disables it for A/B runs).
  // (the counting build walks from global memory; it only learns here whether the timed launch of this world
  // takes the packed 4-wide kernels, whose walk it then counts)
  if (K.lds && (!is_full(f.var) || f.loop)) {
    const int items = wide ? W.n_wnodes : W.n_nodes;
    const size_t rec = wide ? sizeof(rt_wnode) : sizeof(rt_node);
    const bool leaf_lds = wide && K.leaf_lds;
    // LDS bytes at `w` waves per SIMD: the launch constants, the nodes, the lane stacks, and the wide
    // walk's leaf table when it fits as well
    auto lds_bytes = [&](int w, int& n_leaves) {
      const size_t b = lc_bytes + (size_t)items * rec + (size_t)(P.entries + side_ints) * (w * 256) * sizeof(int);
      n_leaves = leaf_lds && b + (size_t)W.n_leaves * sizeof(rt_node) <= kLdsBudget ? W.n_leaves : 0;
      return b + (size_t)n_leaves * sizeof(rt_node);
    };
    int n_leaves = 0;
    // (and only when there is work for the 4th wave: C1's 20 000 items fill less than 3 waves)
    if (f.var == kVarSpheres && !K.waves_set && lds_bytes(4, n_leaves) <= kLdsBudget && (!leaf_lds || n_leaves > 0) &&
        I.work_items >= (long long)W.cu_count * 1024)
      waves = 4;
    // (the full variants' LDS-staged kernels exist at 2 and 3 waves)
    const int w = is_full(f.var) ? std::max(2, std::min(3, waves)) : waves;
    const size_t bytes = lds_bytes(w, n_leaves);
    if (bytes <= kLdsBudget && f.count) {
      f.pk = pk;
    } else if (bytes <= kLdsBudget) {
      f.lds = true;
      f.waves = w;
      f.leaf_lds = n_leaves > 0 && w >= 2;  // (1 wave: the leaves are read from global memory)
      f.pk = pk;
      I.block = w * 256, I.dyn_lds_bytes = (int)bytes, I.grid = W.cu_count;
      P.n_items = items, P.n_leaves = n_leaves;
    }
  }
  if (!f.lds) {
    // instantiated: the counting build at 1 wave; the full variants at 2..4 on the replacement loop
    // (4: RTAMD_WAVES=4, A/B only) and at 1 or 2 on the per-sample loop; every other kernel at 1..4
    f.waves = f.count ? 1 : !is_full(f.var) ? waves : f.loop ? std::max(2, waves) : std::min(2, waves);
    // (spheres-only worlds uploaded with RTAMD_QNODE=1 read the 4-wide tree from global memory in its
    // 64-byte quantised form: A/B only, measured slower)
    f.q = f.loop == 2 && W.has_qnodes;
    // replacement loops: lane stacks (+ Side slots) in dynamic LDS behind the launch constants, sized for
    // this world's stack bound; the per-sample loop keeps both in static LDS
    I.block = RT_BLOCK;
    I.dyn_lds_bytes = f.loop ? (int)(lc_bytes + (size_t)(P.entries + side_ints) * RT_BLOCK * sizeof(int)) : 0;
    I.grid = (int)std::max<long long>(1, (I.work_items + RT_BLOCK - 1) / RT_BLOCK);
  }
  // (the 4-wide tree from global memory, 128-byte nodes, has a unit of its own: rt_k_spheres_global.hip)
  if (f.count && f.pk) f.unit = kUnitCountPacked;
  else if (f.var == kVarSpheres && f.loop == 2 && f.lds && f.pk) f.unit = kUnitSpheresPacked;
  else if (f.var == kVarSpheres && f.loop == 2 && !f.lds && !f.count && !f.q && !K.no_cold) f.unit = kUnitSpheresGlobal;
  I.variant = f.var | (f.loop == 2 ? F_WIDE : 0u) | (f.count ? F_COUNT : 0u) | (f.skip ? F_SKIP : 0u);
  I.loop = f.loop, I.lds_staged = f.lds, I.leaf_lds = P.n_leaves > 0, I.waves = f.waves;
  I.wide_nodes = (f.loop == 2 || (f.loop == 1 && W.mixed_wide)) ? W.n_wnodes : 0;
  out = P;
  return RT_OK;
}

int plan_features(const WorldShape& W, const rt_render_params& p, const LaunchKnobs& K, FeaturePlan& out, bool chain,
                  long long slab_blocks) {
  FeaturePlan P;
  rt_launch_info& I = P.info;
  // (8x8 pixel blocks, one per wave: the image's, or the blocks of a shard's tiles for a slab pass)
  const long long blocks = slab_blocks >= 0 ? slab_blocks : (long long)((p.width + 7) / 8) * ((p.height + 7) / 8);
  if ((long long)p.width * p.height >= (1ll << 32)) return invalid("image too large for 32-bit pixel ids");
  const bool ref_cull = (p.flags & RT_FLAG_REFERENCE_CULL) || W.far_boxes;
  // The 4-wide walk for the worlds the spheres variant renders over a 4-wide tree (the reference-cull flag asks
  // for the binary tree's exact box test, RTAMD_WIDE=0 for the binary walk); any other world whose frames nest
  // at most RT_MAX_FRAMES deep takes the mixed resumable walk, the rest the recursive one.
  if (variant_for(W.features) == kVarSpheres && W.has_wide && W.replace_ok && !ref_cull && K.wide != 0) P.walk = kFeatWide;
  else P.walk = W.replace_ok ? kFeatMixed : kFeatRecursive;
  I.variant = P.walk == kFeatWide ? (kVarSpheres | F_WIDE) : (F_ALL | F_UV | F_MIXW);
  I.loop = P.walk;
  I.work_items = blocks, I.chunk = 0, I.chunk_batches = 1;
  I.wide_nodes = (P.walk == kFeatWide || (P.walk == kFeatMixed && W.mixed_wide)) ? W.n_wnodes : 0;
  I.block = RT_BLOCK, I.waves = 1, I.dyn_lds_bytes = 0;
  I.grid = (int)std::max<long long>(1, std::min<long long>((blocks + RT_BLOCK / 64 - 1) / (RT_BLOCK / 64),
                                                           (long long)W.cu_count * kFeatBlocksPerCU));
  P.leaf_stop = P.walk == kFeatMixed ? K.box_first : 0;
  if (P.walk == kFeatWide) {
    P.leaf_stop = K.leaf_stop >= 0 ? K.leaf_stop : K.trav_stop >= 0 ? K.trav_stop : W.n_nodes > 20000 ? 16 : 8;
    P.pk = wide_keys_packed(W, K);
    P.entries = W.wide_stack_need + 3;  // (wide_node writes 3 slots)
    // LDS-staged like the render's 4-wide kernels: the wide nodes, the leaf table when it fits as well, and the
    // lane stacks of one workgroup per CU, at the most waves per SIMD (4, a chain pass 3, or RTAMD_WAVES) that fit kLdsBudget
    // with the leaves, else with the nodes alone.
    if (K.lds) {
      auto lds_bytes = [&](int w, bool leaves) {
        return (size_t)W.n_wnodes * sizeof(rt_wnode) + (leaves ? (size_t)W.n_leaves * sizeof(rt_node) : 0) +
               (size_t)P.entries * (w * 256) * sizeof(int);
      };
      // (a chain pass: 3, the most at which its staged kernels hold the chain's state in registers; rt_kernels.h)
      const int w = K.waves ? K.waves : chain ? 3 : 4;
      const bool leaves = K.leaf_lds && W.n_leaves > 0 && lds_bytes(w, true) <= kLdsBudget;
      if (lds_bytes(w, leaves) <= kLdsBudget) {
        P.lds = true, P.leaf_lds = leaves;
        P.n_items = W.n_wnodes, P.n_leaves = leaves ? W.n_leaves : 0;
        I.waves = w, I.block = w * 256, I.dyn_lds_bytes = (int)lds_bytes(w, leaves);
        // (one workgroup per CU, fewer when the frame has no block for every wave)
        I.grid = (int)std::max<long long>(1, std::min<long long>(W.cu_count, (blocks + w * 4 - 1) / (w * 4)));
      }
    }
  }
  I.lds_staged = P.lds, I.leaf_lds = P.leaf_lds;
  out = P;
  return RT_OK;
}

}  // namespace rt
