// rt_layout.h — the device copy of a scene as the host prepares it and the kernels read it: node-id
// tags, stack bounds, kernel feature flags and variants, the device material record, the record slab's
// block map. Plain C++ in a CPU build (the host-only scene preparation, rt_prepare.cpp, and the stand-alone
// checks are also built under ASan/UBSan); under hipcc it includes the HIP runtime header, in every unit
// alike, so that the few helpers the kernels call (RT_HD) are host and device functions everywhere.
#pragma once
#include <stdint.h>
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include "rt.h"
#include "rt_wide.h"

#ifndef RT_BLOCK
#define RT_BLOCK 128 /* threads per workgroup (2 waves) */
#endif
#ifndef RT_STACK
#define RT_STACK 32 /* traversal stack entries per lane (LDS) */
#endif
#ifndef RT_WSTACK
#define RT_WSTACK 48 /* the same for the 4-wide walk (up to 3 siblings stacked per level) */
#endif
#define RT_LIGHT_DEPTH 2  /* max BVH depth of the lights tree (host-validated) */
#define RT_MAX_FRAMES 4   /* max nesting of instance frames on the replacement loop (host-validated) */
#define RT_FRAME 0x40000000 /* stack-entry tag: instance frame marker */
#define RT_WNODE 0x10000000 /* node-id tag (mixed walks, F_MIXW): a 4-wide node of a re-bounded subtree */
#define RT_ISBOX 0x08000000 /* node-id tag: a BVH node (set by the upload on the device copy's BVH children
                               and on the roots), so that a walk schedules box steps without a load */
#define RT_WROOT 0x20000000 /* rt_node.c flag of an RT_BVH_ORDERED node whose subtree has a 4-wide tree, */
#define RT_WROOT_MASK 0x3ffffff /* whose root index is (c >> 2) & RT_WROOT_MASK (mixed walks) */
#define RT_ISMED 0x04000000 /* node-id tag: a ConstantMedium (set like RT_ISBOX), so that a walk can hold the
                               lanes at media back without a load (node ids stay below 2^26) */
#define RT_IDTAGS (RT_ISBOX | RT_ISMED) /* the kind tags every walk masks off a node id */
#define RT_SAMEBOX RT_IDTAGS /* both tags (a BVH node is no medium): the left child of a reference-order BVH node
                                whose box is bit-identical to its parent's, entered right after the parent's
                                passing test under the same bound: its own test would pass too */
#define RT_SUB 0x20000000   /* node-id tag (walks in the reference's order): inside a re-bounded,
                               media-free subtree (below an RT_BVH_ORDERED node) */
#define RT_CHAIN_PRIM 0x100 /* device node type flag: Translate/Rotate chain ending in a primitive */
/* Leaf-table copies of instance frames (mixed walks): the frame chain opened from this leaf is described by
   the copy itself, so the walk opens it without loading the chain's records. FUSED: one frame (this node),
   whose child `a` is not an instance frame opened with it; FUSED2: two frames, this one and its child `a`, a
   Rotate (sin f[3], cos f[4], axis (type >> RT_FRAME_AX2_SHIFT) & 3). Either way (int)f[5] is where the walk
   goes on inside: the innermost child, or RT_WNODE | the 4-wide tree of that child when it has one (its
   children's fp32 boxes cull what its own exact box test would). */
#define RT_FRAME_FUSED 0x200
#define RT_FRAME_FUSED2 0x400
#define RT_FRAME_AX2_SHIFT 11
#define RT_TYPE_MASK 0xff

namespace rtd {

// Scene features a kernel variant is compiled for (host picks the variant per scene).
enum : unsigned {
  F_RECT = 1u,    // Rect / Cuboid nodes
  F_MOVING = 2u,  // MovingSphere
  F_INST = 4u,    // Translate / Rotate
  F_MEDIA = 8u,   // ConstantMedium (+ Isotropic)
  F_LIGHTS = 16u, // a lights tree (Lambertian light sampling / pdf)
  F_TEX = 32u,    // Checker / Perlin / Image textures (and sphere u, v)
  F_FRAMES = 512u,  // instance frames (Translate/Rotate over a BVH) in the resumable walk
  F_ALL = 63u | 512u,
  F_UV = 64u,     // always compute sphere (u, v) (debug queries)
  F_COUNT = 128u, // counting build: per-lane work counters (DESIGN.md "Roofline")
  F_WIDE = 256u,  // resumable walk over the 4-wide fp32-box tree (rt_wide.h) instead of the binary one
  F_MIXW = 1024u, // the mixed walk (media / frame worlds) enters 4-wide fp32-box trees built over the
                  // re-bounded subtrees (RT_WROOT nodes) instead of walking them node by node
  F_SLIBM = 2048u, // tier A with RT_FLAG_SHARED_LIBM: sin / cos / log / atan / asin from include/rt_libm.h
                   // (the oracle's too) instead of OCML
  F_QNODE = 4096u, // (spheres-only F_WIDE kernels reading the tree from global memory) the quantised 4-wide
                   // nodes (rt_qnode) and the leaves' sphere quadruples instead of the 128 / 64-byte records
  // (8192 and 16384 stay unused: kernel symbol names carry the flag word)
  F_SKIP = 32768u, // an adaptive progressive frame's launches: work_item tests the frame's skip bitmask
                   // (LaunchConst::skip). Its own instantiations, so that every other launch runs the
                   // kernels without the test
};

// Kernel variants: spheres-only (configs 1, 2, 5), Cornell-like (rects, instances, lights), full.
constexpr unsigned kVarSpheres = 0u;
constexpr unsigned kVarCornell = F_RECT | F_INST | F_LIGHTS;
// the full variant without light sampling (lights Unhittable: next_week_final, the textured
// scenes), whose Lambertian scatter needs no lights-tree code
constexpr unsigned kVarFullDark = (F_ALL & ~F_LIGHTS) | F_MIXW;
// the full variant with light sampling
constexpr unsigned kVarFull = F_ALL | F_MIXW;
inline unsigned variant_for(unsigned f) {
  if ((f & ~kVarSpheres) == 0) return kVarSpheres;
  if ((f & ~kVarCornell) == 0) return kVarCornell;
  return (f & F_LIGHTS) ? kVarFull : kVarFullDark;
}
inline bool is_full(unsigned var) { return (var & F_FRAMES) != 0; }

// Side ints per lane for frames nesting `frames` deep: the world ray (14), then the open frames and the
// frames around the best hit. The host sizes the dynamic LDS per scene: C4's two-deep frames take 8 ints
// per lane fewer than RT_MAX_FRAMES would. (The world ray's reciprocals stored as well, 6 more ints, would
// spare prep's divisions when the last frame closes, but take C4's kernel past six blocks per CU: 243.8
// -> 250.1 ms at 100 spp.)
constexpr int side_ints_for(int frames) { return 14 + 2 * frames; }
// The replacement loop's per-lane LDS ints after the walk stack (philox_loop2's layout, plan_launch's
// sizing — one definition for both): Side slots for the frame kernels on the binary / mixed walk (loop
// 1), then, with RT_LANE_LDS, the 4 lane ints (pixel, row, chunk end, depth) of the
// reference-order kernels (RT_LANE_LDS 1) or of every replacement-loop kernel (2).
#ifndef RT_LANE_LDS
#define RT_LANE_LDS 1
#endif
constexpr int side_ints_of(unsigned var, int frames, int loop) {
  return ((var & F_FRAMES) && loop == 1) ? side_ints_for(frames) : 0;
}
constexpr bool lane_lds_of(unsigned var, int loop) {
  return loop >= 1 && (RT_LANE_LDS >= 2 || (RT_LANE_LDS == 1 && (var & (F_MEDIA | F_FRAMES)) != 0));
}

// Tile edge when the caller leaves it 0 (round 5: 8, was 16; work order and shard dealing only, the
// image does not depend on it: C2 136.0-136.2 -> 135.5 ms, its 8-shard probe 19.1 -> 18.9 ms slowest
// shard, C3 320.0 -> 318.7, C4 at 100 spp 153.3 -> 148.6, C5 at 64 spp 653.0 -> 651.8)
constexpr int kDefaultTile = 8;
// The work geometry of a tier-B frame: its tiles, its shard's slab, its sample chunks (`chunk_knob`:
// LaunchKnobs::chunk, 0 = rt.h's rt_sample_chunk) ...
struct FrameGeometry {
  int tile, tiles_x;
  long long tiles_total, per_shard, slab;
  int chunk, chunks;
};
inline FrameGeometry frame_geometry(const rt_render_params* p, int chunk_knob = 0) {
  FrameGeometry g{};
  g.tile = p->tile ? p->tile : kDefaultTile;
  const int shards = p->shard_count > 0 ? p->shard_count : 1;
  g.tiles_x = (p->width + g.tile - 1) / g.tile;
  const int tiles_y = (p->height + g.tile - 1) / g.tile;
  g.tiles_total = (long long)g.tiles_x * tiles_y;
  g.per_shard = (g.tiles_total + shards - 1) / shards;
  g.slab = g.per_shard * g.tile * g.tile;
  g.chunk = rt_sample_chunk((int64_t)p->width * p->height, p->spp);
  if (chunk_knob > 0) g.chunk = chunk_knob < p->spp ? chunk_knob : p->spp;
  g.chunks = (p->spp + g.chunk - 1) / g.chunk;
  return g;
}
// ... and the claimable units of one launch over `items` work-items whose last `tail_items` are dealt one
// sample per unit.
inline long long launch_units(long long items, long long tail_items, int chunk) {
  return items + (items < tail_items ? items : tail_items) * (chunk - 1);
}

// The inline helpers below that kernels call: host and device in every unit hipcc compiles (the HIP runtime
// header is included above for it), plain inline functions in a CPU build. (Undefined at the end of this header.)
#if defined(__HIPCC__)
#define RT_HD __host__ __device__ __forceinline__
#else
#define RT_HD inline
#endif

// Unsigned 32-bit division by an invariant divisor d >= 1 (Granlund & Montgomery): with
// l = ceil(log2 d) and m = floor(2^32 (2^l - d) / d) + 1, n / d = (t + ((n - t) >> s1)) >> s2 for
// every 32-bit n, t = umulhi(m, n), s1 = min(l, 1), s2 = max(l - 1, 0). One multiply and a few
// shifts instead of the software division a `/` on the device becomes.
struct UDiv {
  uint32_t m;
  int s1, s2;
};
inline UDiv make_udiv(uint32_t d) {
  int l = 0;
  while ((1ull << l) < d) ++l;
  const uint64_t m = ((1ull << 32) * ((1ull << l) - d)) / d + 1;
  return UDiv{(uint32_t)m, l < 1 ? l : 1, l > 1 ? l - 1 : 0};
}
RT_HD uint32_t udiv(uint32_t n, UDiv d) {
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t t = __umulhi(d.m, n);
#else  // (the host evaluates the work decomposition for the launch-geometry check)
  const uint32_t t = (uint32_t)(((uint64_t)d.m * n) >> 32);
#endif
  return (t + ((n - t) >> d.s1)) >> d.s2;
}

// The record slab of shard (tile, shard_rank, shard_count) of a frame (rt.h rt_render_features_shard_async): one
// 64-byte record per slab pixel, in the slot rt_kernels.h's assemble reads,
//   slot = lt * tile^2 + (by * bpr + bx) * 64 + (row & 7) * 8 + (px & 7),
// lt the shard's lt-th tile (image tile shard_rank + lt * shard_count), (bx, by) the pixel's 8x8 block inside the
// tile, bpr = tile / 8. So slot >> 6 numbers the slab's 8x8 blocks, tile-major and row-major inside a tile, and
// slot & 63 is the pixel's place in its block: block b is what one wave of a slab pass folds, lane l its pixel
// (l & 7, l >> 3), stored at slot b * 64 + l. A shard's tiles inside the image are its first `owned_tiles`, so its
// first `blocks` blocks are the ones with image tiles; the slab's other blocks are padding.
struct SlabGeometry {
  int W, H, tile, tiles_x, bpr;
  int shard_rank, shard_count;
  long long tiles_total, slab;      // (FrameGeometry's: image tiles, slab pixels of every shard)
  long long owned_tiles, blocks;    // this shard's tiles inside the image, and their 8x8 blocks
  UDiv div_bpt, div_bpr, div_tiles_x;  // by bpr * bpr, bpr, tiles_x
};
// What a record slab's callers reject of the frame and shard fields (null: fine): what rt_shard_geometry rejects of
// width, height, tile, shard_rank and shard_count, and a slab of 2^32 slots or more (block and slot ids are 32-bit).
inline const char* slab_params_error(const rt_render_params* p) {
  if (p->width <= 0 || p->height <= 0) return "width and height must be positive";
  if ((long long)p->width * p->height >= (1ll << 32)) return "a frame of 2^32 pixels or more";
  const int tile = p->tile ? p->tile : kDefaultTile;
  if (tile <= 0 || tile % 8 || tile > 256) return "tile must be a multiple of 8 in [8, 256]";
  if (p->shard_count < 0 || (p->shard_count > 0 && (p->shard_rank < 0 || p->shard_rank >= p->shard_count)) ||
      (p->shard_count <= 1 && p->shard_rank != 0))
    return "bad shard_rank/shard_count";
  const long long tx = (p->width + tile - 1) / tile, ty = (p->height + tile - 1) / tile;
  const long long shards = p->shard_count > 0 ? p->shard_count : 1;
  if ((tx * ty + shards - 1) / shards * tile * tile >= (1ll << 32)) return "a slab of 2^32 slots or more";
  return nullptr;
}
inline SlabGeometry slab_geometry(const rt_render_params* p) {
  const FrameGeometry g = frame_geometry(p);
  SlabGeometry G{};
  G.W = p->width, G.H = p->height, G.tile = g.tile, G.tiles_x = g.tiles_x, G.bpr = g.tile >> 3;
  G.shard_count = p->shard_count > 0 ? p->shard_count : 1;
  G.shard_rank = p->shard_rank;
  G.tiles_total = g.tiles_total, G.slab = g.slab;
  G.owned_tiles = G.shard_rank < g.tiles_total ? (g.tiles_total - G.shard_rank + G.shard_count - 1) / G.shard_count : 0;
  G.blocks = G.owned_tiles * G.bpr * G.bpr;
  G.div_bpt = make_udiv((uint32_t)(G.bpr * G.bpr)), G.div_bpr = make_udiv((uint32_t)G.bpr);
  G.div_tiles_x = make_udiv((uint32_t)G.tiles_x);
  return G;
}
// (The third statement of the slab map: rt_kernels.h's work_pixel is the same map per slab pixel with the render's
// launch constants, its `assemble` the inverse. The render kernels keep theirs; a change to one is a change to all.)
// Block b (< 2^32 / 64) of the slab -> the image pixel of its lane 0; false: a block of a tile past the image's
// last. Lane l's pixel is (px0 + (l & 7), row0 + (l >> 3)), in the image where px < W and row < H.
RT_HD bool slab_block(const SlabGeometry& G, uint32_t b, int& px0, int& row0) {
  const uint32_t lt = udiv(b, G.div_bpt), blk = b - lt * (uint32_t)(G.bpr * G.bpr);
  const long long gt = (long long)G.shard_rank + (long long)lt * G.shard_count;
  if (gt >= G.tiles_total) return false;
  const uint32_t ty = udiv((uint32_t)gt, G.div_tiles_x), tx = (uint32_t)gt - ty * (uint32_t)G.tiles_x;
  const uint32_t by = udiv(blk, G.div_bpr), bx = blk - by * (uint32_t)G.bpr;
  px0 = (int)(tx * (uint32_t)G.tile + bx * 8u);
  row0 = (int)(ty * (uint32_t)G.tile + by * 8u);
  return true;
}
// Slab slot -> image pixel index row * W + px, or -1 for a padding slot.
RT_HD long long slab_slot_pixel(const SlabGeometry& G, uint32_t slot) {
  int px0, row0;
  if (!slab_block(G, slot >> 6, px0, row0)) return -1;
  const int px = px0 + (int)(slot & 7u), row = row0 + (int)((slot >> 3) & 7u);
  return px < G.W && row < G.H ? (long long)row * G.W + px : -1;
}
// Image pixels the shard owns (host: a loop over its tiles).
inline long long slab_owned_pixels(const SlabGeometry& G) {
  long long n = 0;
  for (long long lt = 0; lt < G.owned_tiles; ++lt) {
    const long long gt = G.shard_rank + lt * G.shard_count;
    const long long x0 = (gt % G.tiles_x) * G.tile, y0 = (gt / G.tiles_x) * G.tile;
    const long long w = G.W - x0 < G.tile ? G.W - x0 : G.tile, h = G.H - y0 < G.tile ? G.H - y0 : G.tile;
    n += w * h;
  }
  return n;
}

// Device material: the rt_material record plus whether its texture tree reads (u, v).
struct DMat {
  int type;
  int tex;
  double param;
  int needs_uv;
  int _pad;
};

#undef RT_HD

}  // namespace rtd
