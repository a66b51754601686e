// rt_kernels.h — the render kernels as templates (device code), shared by the kernel translation
// units: rt_k_spheres.hip, rt_k_cornell.hip and rt_k_full.hip each instantiate one scene
// variant's render kernels (so the variants compile in parallel), rt_render.hip the small kernels
// and the host half of the C ABI. Kernel design: DESIGN.md §3.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "rt.h"
#include "rt_device.h"
#include "rt_error.h"
#include "rt_ids.h"
#include "rt_internal.h"
#include "rt_launch_plan.h"
#include "rt_trace.h"

using namespace rtd;

namespace {

// (UDiv, make_udiv, udiv: rt_layout.h, with the record slab's block map that divides with them)

// The launch's constants: everything a launch passes to its kernels. The small kernels (combine_chunks,
// tail_combine) and tier A take it by value, and so do a progressive frame's frame_* helpers, which read the frame
// geometry, acc, chunk, spp and out_rgb / out_lin. The tier-B render kernels get a device copy (RenderArgs::lc,
// written by launch_setup ahead of the launch) and stage it in LDS once per workgroup: the persistent loops read
// the camera, the table pointers, the work geometry and the claim parameters from there where they use them,
// instead of holding them in scalar registers (and their spill lanes) across the walk. DESIGN.md §3.1.
struct LaunchConst {
  Scene S;
  rt_camera cam;
  int W, H, spp, max_depth;
  uint32_t flags;
  int tile, tiles_x, tiles_total, shard_rank, shard_count;
  long long work_total;  // claimable units of this launch (< 2^32): work-items before tail_start, then one
                         // unit per sample of each work-item from tail_start on (kTail kernels)
  long long slab;        // slab pixels of this shard
  int chunk, chunks;     // tier B: samples per chunk (rt_sample_chunk) and chunks per pixel in this launch
  int chunk_base;        // the launch's first chunk (a frame may render its chunks in batches)
  int combine;           // combine_chunks: 1 = add to the running sums in `acc`, 2 = the last batch (store)
  double* acc;           // running per-pixel sums between chunk batches, [slab pixel][3]
  UDiv div_tp, div_tile, div_tiles_x, div_bpr;  // by tile*tile, tile*tile*chunks, tiles_x, tile/8
  double* partial;       // tier B: chunk sums, [chunk][slab pixel][3]
  uint64_t seed;
  unsigned long long* counter;
  unsigned long long* work;  // counting build: [segments, box, prim, other, light, blocks, samples]
  unsigned long long* prof;  // counting build, optional: the walk's step profile (Cnt::prof)
  int trav_stop;             // replacement loop: keep stepping while > trav_stop/64 of live lanes walk
  int batch;                 // replacement loop: most work-items a wave claims per atomic
  float batch_per_item;      // ...tapering to rem * batch_per_item as `rem` items remain (>= need)
  int batch_floor;           // ...but never below this many (RTAMD_BATCH_FLOOR; 0: the lanes' need)
  int leaf_stop;             // 4-wide walk: leaf step once <= leaf_stop/64 of live lanes seek a leaf
  int box_first;             // binary walk: box-only steps while > box_first/64 of live lanes are at BVH
                             // nodes (64: never)
  uint32_t rev_tiles;        // RTAMD_TILE_REV: the slab's tiles run last to first (this count; 0: in order)
  uint8_t* out_rgb;  // tier B: slab; tier A: image
  double* out_lin;
  uint64_t* gens;  // tier A: per-column (seed, gamma), updated in place
  int med_batch;   // binary walk of media worlds: lanes at a medium wait until this many are there (or
                   // nothing else walks); 0: never wait
  double* trace;   // tier A, rt_debug_exact_trace: column trace_col's path segments (10 doubles each)
  int* trace_n;
  int trace_col, trace_cap;
  // (last, so that the fields before keep their kernel-argument offsets in the kernels that do not read
  // these: moved in the middle, they cost the spheres and Cornell kernels 0.7 %)
  long long items_total; // work-items of this launch: slab pixels x sample chunks
  long long tail_start;  // the work-items from here on are dealt one sample per unit (kTail: the frame's
                         // tail, so that no lane starts a whole chunk of long paths as the GPU runs dry),
                         // their colours stored in tail_buf and summed in sample order by tail_combine
  double* tail_buf;      // [unit][3]
  UDiv div_chunk;        // by chunk
  // (last again: an adaptive progressive frame's skip bitmask, one 64-bit word per 64 consecutive slab
  // pixels, bit set = the pixel is stopped (rt.h); null: nothing is skipped. Read by the F_SKIP kernels
  // only, which such a frame's launches select. Device memory: the host's calls of work_item / work_unit
  // are the instantiations without the test.)
  const unsigned long long* skip;
};
// (its LDS copy sits at the start of the workgroup's lane-stack memory, 16-byte aligned)
constexpr int kLcBytes = (int)((sizeof(LaunchConst) + 15) & ~(size_t)15);

// Kernel arguments of the tier-B render kernels: what a walk step touches, and the launch constants'
// device copy. Of S the walks read the node tables, `world`, `ref_walk` and `frames`; shading reads the
// scene through the LDS copy.
struct RenderArgs {
  Scene S;
  const LaunchConst* lc;
  uint64_t seed;  // (scalar: the Philox round keys are derived from it where a block is computed)
  uint32_t flags;
  int trav_stop, leaf_stop, box_first, med_batch;  // (as in LaunchConst)
  unsigned long long* prof;
};

// Copies the launch constants to `lds` (kLcBytes, 16-byte aligned); the caller's barrier publishes them.
__device__ __forceinline__ const LaunchConst& stage_const(const RenderArgs& A, void* lds) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(A.lc);
  uint32_t* dst = reinterpret_cast<uint32_t*>(lds);
  for (int i = threadIdx.x; i < (int)(sizeof(LaunchConst) / 4); i += blockDim.x) dst[i] = src[i];
  return *reinterpret_cast<const LaunchConst*>(lds);
}

// Writes a launch's constants to their device copy and resets the work counter (one block, ahead of
// the render kernel on its stream; the struct travels as a kernel argument, copied at launch).
__global__ void __launch_bounds__(64) launch_setup(LaunchConst L, LaunchConst* dst) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(&L);
  uint32_t* d = reinterpret_cast<uint32_t*>(dst);
  for (int i = threadIdx.x; i < (int)(sizeof(LaunchConst) / 4); i += 64) d[i] = src[i];
  if (threadIdx.x == 0) *L.counter = 0ull;
}

// Slab pixel index -> image pixel (tile-major, 8x8 blocks inside a tile). Slab indices are < 2^32
// (plan_launch checks). The same map is stated twice more: `assemble` below is its inverse (image pixel -> slot),
// and rt_layout.h's slab_block is this function per 8x8 block for the record slabs of the feature and ID passes
// (tests/c/shard_block_check.cpp holds slab_block to assemble's formula). A change to one is a change to all.
__host__ __device__ __forceinline__ bool work_pixel(const LaunchConst& A, uint32_t w, int& px, int& row) {
  const uint32_t tp = (uint32_t)(A.tile * A.tile);
  const uint32_t lt = udiv(w, A.div_tp);
  const uint32_t within = w - lt * tp;
  const long long gt = (long long)A.shard_rank + (long long)lt * A.shard_count;
  if (gt >= A.tiles_total) return false;
  const uint32_t ty = udiv((uint32_t)gt, A.div_tiles_x), tx = (uint32_t)gt - ty * (uint32_t)A.tiles_x;
  const uint32_t blk = within >> 6, l = within & 63;
  const uint32_t by = udiv(blk, A.div_bpr), bx = blk - by * (uint32_t)(A.tile >> 3);
  px = (int)(tx * A.tile + bx * 8 + (l & 7));
  row = (int)(ty * A.tile + by * 8 + (l >> 3));
  return px < A.W && row < A.H;
}

// A slab pixel's bit in a skip bitmask (LaunchConst::skip; null: never set).
__host__ __device__ __forceinline__ bool skip_bit(const unsigned long long* skip, uint32_t idx) {
  return skip && ((skip[idx >> 6] >> (idx & 63u)) & 1ull);
}

// Tier-B work-item -> (slab pixel, sample chunk). Items run tile by tile, chunk by chunk inside a
// tile, so a wave's 64 consecutive items are one 8x8 pixel block at one chunk (coherent rays).
// Returns false for pixels outside the image and, under SKIP (the F_SKIP kernels), for the stopped pixels
// of an adaptive frame (A.skip): such a pixel takes the path a pixel outside the image takes. Else the
// sample range [s0, s1) and the chunk sum's slot in `partial`.
template <bool SKIP = false>
__host__ __device__ __forceinline__ bool work_item(const LaunchConst& A, uint32_t wi, int& px, int& row, int& s0,
                                                   int& s1, long long& slot) {
  const uint32_t tp = (uint32_t)(A.tile * A.tile);
  const uint32_t lw = udiv(wi, A.div_tile);  // by tp * chunks
  const uint32_t rem = wi - lw * tp * (uint32_t)A.chunks;
  const uint32_t lt = A.rev_tiles ? A.rev_tiles - 1 - lw : lw;
  const uint32_t k = udiv(rem, A.div_tp);
  const uint32_t idx = lt * tp + (rem - k * tp);
  if (!work_pixel(A, idx, px, row)) return false;
  if constexpr (SKIP) {
    if (skip_bit(A.skip, idx)) return false;
  }
  s0 = (A.chunk_base + (int)k) * A.chunk;
  s1 = A.spp < s0 + A.chunk ? A.spp : s0 + A.chunk;
  slot = (long long)k * A.slab + idx;
  return s0 < s1;
}
__device__ __forceinline__ void store_partial_at(double* base, long long slot, V3 sum) {
  double* q = base + slot * 3;
  q[0] = sum.x;
  q[1] = sum.y;
  q[2] = sum.z;
}
__device__ __forceinline__ void store_partial(const LaunchConst& A, long long slot, V3 sum) {
  store_partial_at(A.partial, slot, sum);
}
// Sample-granular tails: in the full variants' kernels only (media / frame worlds, C4), whose work-items
// (8 samples of paths up to 50 segments through fog) are long and uneven — a frame's last claims left
// C4 a ~19 ms tail per launch. (In the spheres kernel the extra state cost more than its ~2 ms tail:
// DESIGN.md §3.1.)
template <unsigned F>
constexpr bool kTail = (F & F_FRAMES) != 0;
// A claimable unit: a work-item, or (from tail_start on) one sample of one. A tail unit's slot is
// kTailSlot + its index (its colour goes to tail_buf); false for pixels outside the image and for units
// past the work-item's last sample.
constexpr long long kTailSlot = 1ll << 40;
template <bool SKIP = false>
__host__ __device__ __forceinline__ bool work_unit(const LaunchConst& A, uint32_t wi, int& px, int& row, int& s0,
                                                   int& s1, long long& slot) {
  if ((long long)wi < A.tail_start) return work_item<SKIP>(A, wi, px, row, s0, s1, slot);
  const uint32_t u = wi - (uint32_t)A.tail_start;
  const uint32_t q = udiv(u, A.div_chunk);
  const uint32_t k = u - q * (uint32_t)A.chunk;
  if (!work_item<SKIP>(A, (uint32_t)A.tail_start + q, px, row, s0, s1, slot)) return false;
  s0 += (int)k;
  if (s0 >= s1) return false;
  s1 = s0 + 1;
  slot = kTailSlot + u;
  return true;
}

// getRay (Lib.hs:1253-1267): the disk and time draws always happen.
template <class R>
__device__ __forceinline__ Ray get_ray(const rt_camera& k, double s, double t, R& g) {
  const V3 rd = scale(k.lens_radius, random_in_unit_disk(g));
  const V3 offset = scale(rd.x, vload(k.u)) + scale(rd.y, vload(k.v));
  g.reserve(1);
  const double tm = draw_r(g, k.t0, k.t1);
  Ray r;
  r.o = vload(k.origin) + offset;
  r.d = (((vload(k.llc) + scale(s, vload(k.horiz))) + scale(t, vload(k.vert))) - vload(k.origin)) - offset;
  r.tm = tm;
  return r;
}

// scaleColor (Lib.hs:287-288): NaN -> 0, +inf -> 255.
__device__ __forceinline__ uint8_t scale_color(double x) {
  const double s = sqrt(x);
  const double cl = s < 0.0 ? 0.0 : (s > 0.999 ? 0.999 : s);
  const double f = floor(256 * cl);
  return f == f ? (uint8_t)(int)f : (uint8_t)0;
}

// RT_FLAG_NAN_ZERO (parity diagnostic, rt.h): a NaN channel of a sample's colour adds 0
__device__ __forceinline__ V3 nan_zero(V3 a) {
  return v3(a.x != a.x ? 0.0 : a.x, a.y != a.y ? 0.0 : a.y, a.z != a.z ? 0.0 : a.z);
}

__device__ __forceinline__ void store_pixel(const LaunchConst& A, long long idx, V3 avg) {
  A.out_rgb[idx * 3 + 0] = scale_color(avg.x);
  A.out_rgb[idx * 3 + 1] = scale_color(avg.y);
  A.out_rgb[idx * 3 + 2] = scale_color(avg.z);
  if (A.out_lin) {
    A.out_lin[idx * 3 + 0] = avg.x;
    A.out_lin[idx * 3 + 1] = avg.y;
    A.out_lin[idx * 3 + 2] = avg.z;
  }
}

// The rest of a segment once its closest hit is known (rayColor, Lib.hs:1309-1333): background,
// emission, or a scatter. Returns true when the path ends (contribution in `contrib`).
template <unsigned F, class R>
__device__ __forceinline__ bool shade_hit(const Scene& S, bool got, const Hit& h, Ray& ray, V3& thr, int& depth, R& g,
                                          V3& contrib, Cnt& cnt) {
  if (!got) {
    contrib = vmul(thr, v3(S.bg[0], S.bg[1], S.bg[2]));
    return true;
  }
  const DMat m = S.mats[h.mat];
  const V3 tx = hit_texture<F>(S, m, h);  // (the kernel's one copy of the texture code)
  if (m.type == RT_MAT_DIFFUSE_LIGHT) {
    contrib = vmul(thr, h.ff ? v3(0, 0, 0) : mat_texture<F>(S, m, h, tx));
    return true;
  }
  Scatter s;
  if constexpr ((F & F_COUNT) != 0) cnt.light += (m.type == RT_MAT_LAMBERTIAN && S.lights >= 0);
  scatter<F>(S, m, ray, h, g, s, tx);
  if (s.specular) {
    thr = vmul(thr, s.att);
  } else {
    const double c = dot(h.n, s.ray.d);
    const double spdf = c < 0 ? 0 : c / kPi;
    const double k = spdf / s.pdf;
    thr = vmul(thr, scale(k, s.att));
  }
  ray = s.ray;
  --depth;
  return false;
}

// One path segment: closest hit, then emission/background or a scatter. Returns true when the
// path ends, with its contribution in `contrib` (rayColor, Lib.hs:1298-1333).
// (S: the walk's scene, its node tables possibly in LDS; SC: the scene shading reads)
template <unsigned F, class R, class AT>
__device__ __forceinline__ bool segment(const AT& A, const Scene& S, const Scene& SC, Ray& ray, V3& thr, int& depth,
                                        R& g, int* stk, V3& contrib, Cnt& cnt, int stride = RT_BLOCK,
                                        unsigned long long* t_trav = nullptr) {
  if (depth <= 0) {  // d <= 0 -> black
    contrib = vmul(thr, v3(0.0, 0.0, 0.0));
    return true;
  }
  Hit h;
  // (worlds walked in the reference's order: the recursive walk takes the caller's tree as is)
  const bool got = traverse<F>(S, S.ref_walk ? S.world_ref : S.world, ray, kEps, INFINITY, h, g, stk,
                               !(A.flags & RT_FLAG_REFERENCE_CULL), cnt, stride);
  if constexpr ((F & F_COUNT) != 0) *t_trav = stamp();
  return shade_hit<F>(SC, got, h, ray, thr, depth, g, contrib, cnt);
}

// ---------------------------------------------------------------- tier B: Philox per (pixel, sample)
// Wave-reduce a per-lane counter and add it once per wave.
__device__ __forceinline__ void wave_add(unsigned long long* dst, unsigned long long v) {
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  if ((threadIdx.x & 63) == 0) atomicAdd(dst, v);
}

// The persistent tier-B loop, shared by the global-memory and LDS-staged kernels.
template <unsigned F>
__device__ __forceinline__ void philox_loop(const RenderArgs& A, const LaunchConst& L, const Scene& S, int* stk,
                                            int stride) {
  const int lane = threadIdx.x & 63;
  const unsigned long long lanes_below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));

  long long w = -1;  // the current chunk's slot in A.partial
  bool done = false, path = false;
  int px = 0, row = 0, s = 0, s_end = 0, depth = 0;
  Ray ray;
  V3 thr = v3(0, 0, 0), sum = v3(0, 0, 0);
  RngPhilox g;
  g.init(A.seed, 0, 0);
  Cnt cnt{};
  unsigned long long segs = 0, blocks = 0, samples = 0;
  unsigned long long ph_acq = 0, ph_trav = 0, ph_shade = 0, s0 = 0, s1 = 0, s2 = 0;

  for (;;) {
    if constexpr ((F & F_COUNT) != 0) s0 = stamp();
    // acquire pixels for idle lanes: one atomic per wave per round
    for (;;) {
      const bool need = (w < 0) && !done;
      const unsigned long long mask = __ballot(need);
      if (!mask) break;
      const int leader = __ffsll((long long)mask) - 1;
      unsigned long long base = 0;
      if (lane == leader) base = atomicAdd(L.counter, (unsigned long long)__popcll(mask));
      base = __shfl(base, leader);
      if (need) {
        const long long wi = (long long)(base + __popcll(mask & lanes_below));
        if (wi >= L.work_total) {
          done = true;
        } else if (work_item<(F & F_SKIP) != 0>(L, (uint32_t)wi, px, row, s, s_end, w)) {
          sum = v3(0, 0, 0);
          path = false;
        } else {
          w = -1;
        }
      }
    }
    if (w < 0) break;  // no pixel left for this lane (done); the others keep going
    if (!path) {  // start sample s: uniformRandomUVs' pair, then getRay
      const uint32_t pid = (uint32_t)((long long)row * L.W + px);
      g.init(A.seed, pid, (uint32_t)s);
      g.reserve(3);  // the UV pair and the first disk try
      const double ru = g.draw(), rv = g.draw();
      const int y = L.H - 1 - row;
      const double u = ((double)px + ru) / (double)L.W;
      const double v = ((double)y + rv) / (double)L.H;
      ray = get_ray(L.cam, u, v, g);
      thr = v3(1.0, 1.0, 1.0);
      depth = L.max_depth;
      path = true;
    }
    V3 contrib;
    if constexpr ((F & F_COUNT) != 0) {
      segs += depth > 0;
      s1 = stamp();
      s2 = s1;
    }
    bool ended = segment<F>(A, S, L.S, ray, thr, depth, g, stk, contrib, cnt, stride, &s2);
    // the dead-path cut (philox_loop2 has the reasoning): a throughput that is NaN in all three channels
    // decides the sample's colour, thr * 0 as at depth 0. Here, after segment(), not in it: tier A
    // (render_exact) shares segment() and shade_hit() and must trace every path to its end.
    if (!ended && thr.x != thr.x && thr.y != thr.y && thr.z != thr.z) {
      contrib = vmul(thr, v3(0.0, 0.0, 0.0));
      ended = true;
    }
    if constexpr ((F & F_COUNT) != 0) {
      const unsigned long long s3 = stamp();
      ph_acq += s1 - s0;
      ph_trav += s2 - s1;
      ph_shade += s3 - s2;
    }
    if (ended) {
      if constexpr ((F & F_COUNT) != 0) {
        blocks += g.pair;
        ++samples;
      }
      if (A.flags & RT_FLAG_NAN_ZERO) contrib = nan_zero(contrib);
      sum = sum + contrib;
      path = false;
      ++s;
      const bool all_nan = (A.flags & RT_FLAG_NAN_CULL) && sum.x != sum.x && sum.y != sum.y && sum.z != sum.z;
      if (s == s_end || all_nan) {
        store_partial(L, w, sum);
        w = -1;
      }
    }
  }
  if constexpr ((F & F_COUNT) != 0) {  // lanes re-converge after the loop: one add per wave
    wave_add(&L.work[0], segs);
    wave_add(&L.work[1], cnt.box);
    wave_add(&L.work[2], cnt.prim);
    wave_add(&L.work[3], cnt.other);
    wave_add(&L.work[4], cnt.light);
    wave_add(&L.work[5], blocks);
    wave_add(&L.work[6], samples);
    if ((threadIdx.x & 63) == 0) {  // wave-uniform phase times (s_memtime ticks)
      atomicAdd(&L.work[8], ph_acq);
      atomicAdd(&L.work[9], ph_trav);
      atomicAdd(&L.work[10], ph_shade);
    }
  }
}

template <unsigned F, int WAVES>
__global__ void __launch_bounds__(RT_BLOCK, WAVES) render_philox(RenderArgs A) {
  // (the launch constants ahead of the stacks, in one array: stack stores may alias them, so their reads
  // stay where the loop uses them)
  __shared__ __attribute__((aligned(16))) int stk_mem[kLcBytes / 4 + RT_STACK * RT_BLOCK];
  const LaunchConst& L = stage_const(A, stk_mem);
  __syncthreads();
  philox_loop<F>(A, L, A.S, &stk_mem[kLcBytes / 4 + threadIdx.x], RT_BLOCK);
}

// LDS-staged variant: one workgroup of WAVES*4 waves per CU; the whole node array is copied
// into LDS once, ahead of the traversal stack, so every node fetch of the traversal's
// dependent chain is an LDS read (~64 cycles) instead of an L2 hit (~200-500 cycles).
template <unsigned F, int WAVES>
__global__ void __launch_bounds__(WAVES * 256, WAVES) render_philox_lds(RenderArgs A, int n_nodes, int stack_entries) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  // (the launch constants first, kLcBytes, then the nodes, then the stacks)
  const LaunchConst& L = stage_const(A, lds);
  rt_node* nodes = reinterpret_cast<rt_node*>(lds + kLcBytes);
  {
    const uint4* src = reinterpret_cast<const uint4*>(A.S.nodes);
    uint4* dst = reinterpret_cast<uint4*>(lds + kLcBytes);
    const int n16 = n_nodes * (int)(sizeof(rt_node) / 16);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
  }
  __syncthreads();
  Scene S = A.S;
  S.nodes = nodes;
  int* stk = reinterpret_cast<int*>(lds + kLcBytes + (size_t)n_nodes * sizeof(rt_node)) + threadIdx.x;
  (void)stack_entries;
  philox_loop<F>(A, L, S, stk, WAVES * 256);
}

// Tier-B loop with ray replacement (media-free worlds without instance frames): traversal state
// persists in registers across iterations; each iteration first shades the lanes whose walk has
// ended and starts their next segment (or sample, or pixel), then steps every walking lane one
// node at a time until at most trav_stop/64 of the live lanes are still walking. Lanes never
// wait for the slowest walk of their wave, and shading runs for many lanes at once.
// PK: the 4-wide walk sorts a node's children as packed keys (wide_node<F, true>; worlds within rt_wkey_fits).
template <unsigned F, bool PK = false>
__device__ __forceinline__ void philox_loop2(const RenderArgs& A, const LaunchConst& L, const Scene& S, int* stk,
                                             int stride, int* side_p, volatile uint32_t* wq) {
  const int lane = threadIdx.x & 63;
  const unsigned long long lanes_below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  const bool joint = !(A.flags & RT_FLAG_REFERENCE_CULL);

  long long w = -1;  // the current chunk's slot in A.partial
  bool done = false, walking = false, ready = false;
  // wq[0..1]: the wave's claimed, not yet handed out work-items [next, end), in LDS (lanes that
  // are walking skip the acquisition code, so a per-lane copy would go stale); indices are < 2^32
  // (plan_launch checks)
  if (lane == 0) {
    wq[0] = 0u;
    wq[1] = 0u;
  }
  // (the ints only acquisition and shading touch — pixel, row, the chunk's end sample, the path depth —
  // live in LDS after the stacks and Side slots, out of the walk loop's VGPRs; RT_LANE_LDS: 1 the
  // reference-order kernels, 2 every replacement-loop kernel)
  constexpr int kLoop = (F & F_WIDE) ? 2 : 1;
  constexpr bool kLaneLds = lane_lds_of(F, kLoop);
  int l_px = 0, l_row = 0, l_s_end = 0, l_depth = 0;
  int* ex = side_p + side_ints_of(F, S.frames, kLoop) * stride;  // (the host sizes the LDS with the same helpers)
  int& px = kLaneLds ? ex[0] : l_px;
  int& row = kLaneLds ? ex[stride] : l_row;
  int& s_end = kLaneLds ? ex[2 * stride] : l_s_end;
  int& depth = kLaneLds ? ex[3 * stride] : l_depth;
  px = 0, row = 0, s_end = 0, depth = 0;
  int s = 0;
  V3 thr = v3(0, 0, 0), sum = v3(0, 0, 0);  // the segment's throughput, the chunk's sum
  RngPhilox g;
  g.init(A.seed, 0, 0);
  Trav t;  // the segment's ray lives only here between segments (no second copy is carried)
  Side side{side_p, stride, S.frames};
  Cnt cnt{};
  if constexpr ((F & F_COUNT) != 0) cnt.prof = A.prof;
  unsigned long long segs = 0, blocks = 0, samples = 0, ph_setup = 0, ph_trav = 0, ph_shade = 0;

  // sample s is over: add its colour; the chunk is done after its last sample
  auto end_sample = [&](V3 contrib) __attribute__((always_inline)) {
    if constexpr ((F & F_COUNT) != 0) {
      blocks += g.pair;
      ++samples;
    }
    if (A.flags & RT_FLAG_NAN_ZERO) contrib = nan_zero(contrib);
    const V3 sm = sum + contrib;
    sum = sm;
    ++s;
    const bool all_nan = (A.flags & RT_FLAG_NAN_CULL) && sm.x != sm.x && sm.y != sm.y && sm.z != sm.z;
    if (s == s_end || all_nan) {
      // (a tail unit: its one sample's colour, summed in order with its chunk's others by tail_combine)
      if (kTail<F> && w >= kTailSlot) store_partial_at(L.tail_buf, w - kTailSlot, contrib);
      else store_partial(L, w, sm);
      w = -1;
    }
  };
  // (by reference: by value the compiler promotes `thr` to registers before inlining and numbers the loop's
  // values in another order — the same code with the registers permuted, and a kernel that was not timed)
  auto all_nan3 = [](const V3& a) __attribute__((always_inline)) { return a.x != a.x && a.y != a.y && a.z != a.z; };

  for (;;) {
    unsigned long long s0 = 0;
    if constexpr ((F & F_COUNT) != 0) {
      s0 = stamp();
      ++cnt.oslot;
    }
    // ---- shade finished walks, then set up the next walk for every lane that is not walking
    // exact tie, or a NaN-t rect hit in a re-bounded subtree (trav_take: `lite` in a first walk): redo
    // this walk as the reference does (once). (NaN-t hits come from the Lambertian quirk's +x ray in a
    // box top's plane, whose pdf is 0 / 0: DESIGN.md §4.3. A walking path's throughput is never NaN in
    // every channel: such a path ends where it is shaded, below.)
    if (ready && (((t.tie || (kRefMixed<F> && t.lite)) && !t.redo) || redo_again<F>(t))) {
      if constexpr ((F & F_COUNT) != 0) ++cnt.ties;
      trav_redo<F>(t, L.S.world_ref, INFINITY);
      // (the redo's binary box tests need 1/d: recomputed here, the same values, so that the 4-wide
      // walk need not carry Trav::ray.inv)
      if constexpr ((F & F_WIDE) != 0) t.ray = prep(plain(t.ray));
      if constexpr (kLeanWalk<F, PK>) {
        // The redo runs to its end here, a divergent loop over the flagged lanes, and the lane is shaded below
        // in this same iteration (`ready` stays set; t.redo keeps it from being redone): the 4-wide step loop then
        // holds no binary step and no lane in a redo. Ties are rare (C2 none); only test worlds have many.
        do {
          while (trav_step<F, true>(S, t, kEps, stk, stride, joint, cnt, g, side)) {
          }
        } while (redo_again<F>(t) && (trav_redo<F>(t, L.S.world_ref, INFINITY), true));
        t.node = kNone;  // (with pend = -1: the walk is over, in walk_until's terms too)
      } else {
        ready = false;
        walking = true;
      }
    }
    // the next walk's ray: a scattered ray (next segment) or a camera ray (next sample), parked in
    // t.ray (free once the walk's hit is recorded); both kinds of lane start their walk together
    // below, so the walk set-up runs once per wave
    bool start = false;
    if (ready) {
      ready = false;
      Hit h;
      Ray ray = plain(t.ray);  // (every frame has closed: the world ray again)
      const bool got = trav_finish<F>(L.S, t, ray, kEps, h, side);
      V3 contrib;
      V3 th = thr;
      if (shade_hit<F>(L.S, got, h, ray, th, depth, g, contrib, cnt)) {
        end_sample(contrib);
      } else if (depth <= 0 || all_nan3(th)) {
        // rayColor's d <= 0 -> black (thr * 0 keeps a NaN throughput NaN) — and the dead-path cut: once
        // the throughput is NaN in all three channels (the Lambertian quirk's 0 / 0), every
        // way the path can end gives (NaN, NaN, NaN): thr * background, thr * emitted, thr * 0 at depth 0.
        // A tier-B sample draws from its own (pixel, sample) stream, so the draws the rest of the path
        // would make reach no other sample: the sample ends here with the same thr * 0. Exactly "all
        // three": a zero throughput is not decided (a later 0 * NaN factor turns it into NaN), and with
        // one or two NaN channels the others still carry colour. Tier B only, and so not in segment() or
        // shade_hit(), which render_exact shares: tier A's column stream runs through every draw of
        // every sample, so tier A traces every path to its end.
        end_sample(vmul(th, v3(0.0, 0.0, 0.0)));
      } else {  // next segment of the same path
        thr = th;
        t.ray.o = ray.o;
        t.ray.d = ray.d;
        t.ray.tm = ray.tm;
        start = true;
        if constexpr ((F & F_COUNT) != 0) ++segs;
      }
    }
    unsigned long long s0b = 0;
    if constexpr ((F & F_COUNT) != 0) s0b = stamp();
    while (!walking && !start) {
      // acquire work-items for idle lanes: from the wave's claimed range first; when it runs short,
      // one atomic claims a batch of L.batch more (exactly the lanes' need once the counter is near
      // the end, so that no wave hoards the frame's last items)
      for (;;) {
        const bool need = (w < 0) && !done;
        const unsigned long long mask = __ballot(need);
        if (!mask) break;
        const uint32_t n_need = (uint32_t)__popcll(mask);
        const uint32_t q_next = wq[0], q_end = wq[1];
        const uint32_t avail = q_end - q_next;
        uint32_t base2 = q_next, end2 = q_end;  // items past `avail` come from a new claim
        if (avail < n_need) {
          const int leader = __ffsll((long long)mask) - 1;
          unsigned long long claim = 0;
          if (lane == leader) {
            // batch: L.batch items, fewer as the frame runs out (the wave's last claim end tells it
            // roughly how many remain), so that no wave hoards the tail; never less than the need
            const uint32_t want = n_need - avail;
            const long long rem = L.work_total - (long long)q_end;
            const uint32_t b = rem <= 0 ? 0u : max((uint32_t)L.batch_floor,
                                                   (uint32_t)fminf((float)L.batch, (float)rem * L.batch_per_item));
            const uint32_t got = want < b ? b : want;
            const unsigned long long c0 = atomicAdd(L.counter, (unsigned long long)got);
            // (claims past 2^32 only happen once every item is handed out: clamp, the lanes see
            // `done`); the claim and its size travel together in one broadcast
            claim = (c0 < 0xffff0000ull ? c0 : 0xffff0000ull) | ((unsigned long long)got << 32);
          }
          const unsigned long long c1 = __shfl(claim, leader);
          base2 = (uint32_t)c1;
          end2 = base2 + (uint32_t)(c1 >> 32);
        }
        const uint32_t rank = (uint32_t)__popcll(mask & lanes_below);
        if (need) {
          const long long wi = (long long)(rank < avail ? q_next + rank : base2 + (rank - avail));
          if (wi >= L.work_total) {
            done = true;
          } else if (kTail<F> ? work_unit<(F & F_SKIP) != 0>(L, (uint32_t)wi, px, row, s, s_end, w)
                              : work_item<(F & F_SKIP) != 0>(L, (uint32_t)wi, px, row, s, s_end, w)) {
            sum = v3(0, 0, 0);
          } else {
            w = -1;
          }
        }
        const int leader = __ffsll((long long)mask) - 1;
        if (lane == leader) {
          wq[0] = avail < n_need ? base2 + (n_need - avail) : q_next + n_need;
          wq[1] = end2;
        }
      }
      if (w < 0) break;  // no work left for this lane
      // start sample s: uniformRandomUVs' pair, then getRay
      const uint32_t pid = (uint32_t)((long long)row * L.W + px);
      g.init(A.seed, pid, (uint32_t)s);
      g.reserve(3);  // the UV pair and the first disk try
      const double ru = g.draw(), rv = g.draw();
      const int y = L.H - 1 - row;
      const double u = ((double)px + ru) / (double)L.W;
      const double v = ((double)y + rv) / (double)L.H;
      const Ray cray = get_ray(L.cam, u, v, g);
      t.ray.o = cray.o;
      t.ray.d = cray.d;
      t.ray.tm = cray.tm;
      thr = v3(1.0, 1.0, 1.0);
      depth = L.max_depth;
      if (depth <= 0) {
        end_sample(vmul(v3(1.0, 1.0, 1.0), v3(0.0, 0.0, 0.0)));
        continue;
      }
      start = true;
      if constexpr ((F & F_COUNT) != 0) ++segs;
    }
    if (start) {
      trav_begin<F>(t, plain(t.ray), S.world, kEps, INFINITY);
      // worlds with media or frames: the reference's order over the re-bounded skeleton
      if (S.ref_walk) trav_restart_ref(t, S.world, INFINITY);
      trav_media_first<F>(S, t, kEps, cnt, g, side);  // (hoisted media: RT_BVH_MEDIA_FIRST)
      walking = true;
    }
    if (!walking) break;  // this lane is finished; the rest of the wave carries on without it
    unsigned long long s1 = 0;
    if constexpr ((F & F_COUNT) != 0) s1 = stamp();
    // ---- walk until few lanes are still walking
    const int live = __popcll(__ballot(true));
    const int stop = (live * A.trav_stop) >> 6;
    const int ls = (F & F_WIDE) ? A.leaf_stop : A.box_first;
    walk_until<F, PK>(S, t, walking, kEps, stk, stride, joint, stop, (live * ls) >> 6, cnt, g, side, A.med_batch);
    ready = !walking;
    if constexpr ((F & F_COUNT) != 0) {
      const unsigned long long s2 = stamp();
      ph_shade += s0b - s0;
      ph_setup += s1 - s0b;
      ph_trav += s2 - s1;
    }
  }
  if constexpr ((F & F_COUNT) != 0) {
    wave_add(&L.work[0], segs);
    wave_add(&L.work[1], cnt.box);
    wave_add(&L.work[2], cnt.prim);
    wave_add(&L.work[3], cnt.other);
    wave_add(&L.work[4], cnt.light);
    wave_add(&L.work[5], blocks);
    wave_add(&L.work[6], samples);
    wave_add(&L.work[7], cnt.wide);
    wave_add(&L.work[11], cnt.islot);
    wave_add(&L.work[12], cnt.lslot);
    wave_add(&L.work[13], cnt.oslot);
    wave_add(&L.work[14], cnt.phit);
    wave_add(&L.work[15], cnt.ties);
    if ((threadIdx.x & 63) == 0) {
      atomicAdd(&L.work[8], ph_setup);
      atomicAdd(&L.work[9], ph_trav);
      atomicAdd(&L.work[10], ph_shade);
    }
  }
}

// LDS ints per lane of a kernel: the traversal stack, then (instance frames possible) Side slots
template <unsigned F>
constexpr int lane_ints() {
  return ((F & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + ((F & F_FRAMES) ? kSideInts : 0);
}

// Global-memory replacement loop: the lane stacks (and Side slots) in dynamic LDS sized by the host
// for the world's stack bound (`stack_entries` per lane), not for the RT_STACK / RT_WSTACK maxima:
// the LDS per workgroup then does not cap the occupancy (C4: 54 -> 40 ints per lane, 2.5 -> 3 waves
// per SIMD).
template <unsigned F, int WAVES>
__global__ void __launch_bounds__(RT_BLOCK, WAVES) render_philox2(RenderArgs A, int stack_entries) {
  extern __shared__ __attribute__((aligned(16))) int stk_mem[];  // (the launch constants, kLcBytes, first)
  __shared__ uint32_t wave_q[RT_BLOCK / 64][2];
  const LaunchConst& L = stage_const(A, stk_mem);
  __syncthreads();
  int* lane0 = &stk_mem[kLcBytes / 4 + threadIdx.x];
  philox_loop2<F>(A, L, A.S, lane0, RT_BLOCK, lane0 + stack_entries * RT_BLOCK,
                  wave_q[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}

// The counting build of a 4-wide world whose timed launch takes the packed form (plan_launch): the same
// global-memory loop with wide_node<F, true> and the stack cull, so that the work counters describe the walk the
// timed kernel does. A kernel of its own (rt_k_count_packed.hip), so that no timed kernel's name or unit changes.
template <unsigned F>
__global__ void __launch_bounds__(RT_BLOCK, 1) render_philox2_count_packed(RenderArgs A, int stack_entries) {
  static_assert((F & F_WIDE) != 0 && (F & F_COUNT) != 0, "the 4-wide counting build only");
  extern __shared__ __attribute__((aligned(16))) int stk_mem[];  // (as render_philox2)
  __shared__ uint32_t wave_q[RT_BLOCK / 64][2];
  const LaunchConst& L = stage_const(A, stk_mem);
  __syncthreads();
  int* lane0 = &stk_mem[kLcBytes / 4 + threadIdx.x];
  philox_loop2<F, true>(A, L, A.S, lane0, RT_BLOCK, lane0 + stack_entries * RT_BLOCK,
                        wave_q[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}

// LDS-staged replacement loop: the traversal's node array (the wide records for F_WIDE, else the
// flat nodes) and the per-lane stacks live in the CU's LDS; leaves are read from global memory
// under F_WIDE.
// LEAF_LDS: the 4-wide walk's leaf table is staged too (n_leaves > 0); as its own instantiation,
// so that the leaf reads compile to ds_read (a pointer that is LDS or global at run time would
// make them flat loads, which wait on both the vector-memory and LDS counters).
// PK: packed sort keys in the 4-wide walk (its own instantiation as well, not a flag bit: the flag word is
// what rt_launch_info reports, and the form changes no result).
template <unsigned F, int WAVES, bool LEAF_LDS = false, bool PK = false>
__global__ void __launch_bounds__(WAVES * 256, WAVES)
    render_philox2_lds(RenderArgs A, int n_nodes, int stack_entries, int n_leaves) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds0[];
  __shared__ uint32_t wave_q[WAVES * 4][2];  // (static: kStaticLds bytes ahead of the dynamic LDS)
  constexpr int rec = (F & F_WIDE) ? (int)sizeof(rt_wnode) : (int)sizeof(rt_node);
  constexpr int lrec = (int)sizeof(rt_node);
  // (dynamic LDS: the launch constants, kLcBytes, then the nodes, the leaf table, the lanes' stacks and slots)
  const LaunchConst& L = stage_const(A, lds0);
  unsigned char* lds = lds0 + kLcBytes;
  {
    const uint4* src = (F & F_WIDE) ? reinterpret_cast<const uint4*>(A.S.wnodes)
                                    : reinterpret_cast<const uint4*>(A.S.nodes);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    const int n16 = n_nodes * (rec / 16);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    // F_WIDE: the leaf table too, when it fits (n_leaves > 0)
    const uint4* lsrc = reinterpret_cast<const uint4*>(A.S.leaves);
    uint4* ldst = reinterpret_cast<uint4*>(lds + (size_t)n_nodes * rec);
    const int l16 = n_leaves * (lrec / 16);
    for (int i = threadIdx.x; i < l16; i += blockDim.x) ldst[i] = lsrc[i];
  }
  __syncthreads();
  Scene S = A.S;
  if constexpr ((F & F_WIDE) != 0) S.wnodes = reinterpret_cast<const rt_wnode*>(lds);
  else S.nodes = reinterpret_cast<const rt_node*>(lds);
  if constexpr (LEAF_LDS) S.leaves = reinterpret_cast<const rt_node*>(lds + (size_t)n_nodes * rec);
  else n_leaves = 0;
  constexpr int lanes = WAVES * 256;
  unsigned char* lane_base = lds + (size_t)n_nodes * rec + (size_t)n_leaves * lrec;
  int* stk = reinterpret_cast<int*>(lane_base) + threadIdx.x;
  // (per lane: stack_entries stack entries, then side_ints_of Side slots, then lane_lds_of's 4 lane ints —
  // plan_launch sizes the dynamic LDS with the same helpers)
  int* side_p = reinterpret_cast<int*>(lane_base + (size_t)stack_entries * lanes * sizeof(int)) + threadIdx.x;
  philox_loop2<F, PK>(A, L, S, stk, lanes, side_p, wave_q[__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)]);
}

// The tail's work-items (work_unit): each chunk's sample colours added in sample order from 0, as the
// lane that renders a whole chunk adds them (end_sample), into the chunk's slot.
template <bool SKIP>
__device__ __forceinline__ void tail_body(const LaunchConst& A) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j >= A.items_total - A.tail_start) return;
  int px, row, s0, s1;
  long long slot;
  if (!work_item<SKIP>(A, (uint32_t)(A.tail_start + j), px, row, s0, s1, slot)) return;
  const double* q = A.tail_buf + j * A.chunk * 3;
  V3 sum = v3(0, 0, 0);
  for (int k = 0; k < s1 - s0; ++k) sum = sum + v3(q[3 * k], q[3 * k + 1], q[3 * k + 2]);
  store_partial(A, slot, sum);
}
__global__ void __launch_bounds__(256) tail_combine(LaunchConst A) { tail_body<false>(A); }
__global__ void __launch_bounds__(256) tail_combine_skip(LaunchConst A) { tail_body<true>(A); }

// Tier B: a slab pixel's chunk sums added in chunk order, then averaged and stored (rt.h); with chunk
// batches, each batch's chunks are added to the running sum of the batches before it.
// MOMENTS (a tracked progressive frame, RT_FRAME_MOMENTS): the same additions to the sums, and the chunks'
// (S_k * S_k) / n_k added in chunk order to the pixel's second moments Q (`moments`, [slab pixel][3]; rt.h),
// n_k the sample count of the frame's chunk chunk_base + k.
// SKIP (an adaptive frame's launches): a stopped pixel's sums and moments stay as they are; its chunk sums
// were never written.
template <bool MOMENTS, bool SKIP = false>
__device__ __forceinline__ void combine_body(const LaunchConst& A, double* moments) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= A.slab) return;
  int px, row;
  if (!work_pixel(A, (uint32_t)idx, px, row)) return;  // outside the image: never assembled
  if constexpr (SKIP) {
    if (skip_bit(A.skip, (uint32_t)idx)) return;
  }
  V3 acc = (A.combine & 1) ? vload(A.acc + idx * 3) : v3(0, 0, 0);
  V3 mom = v3(0, 0, 0);
  if constexpr (MOMENTS) {
    if (A.combine & 1) mom = vload(moments + idx * 3);
  }
  for (int k = 0; k < A.chunks; ++k) {
    const double* q = A.partial + ((long long)k * A.slab + idx) * 3;
    acc = acc + v3(q[0], q[1], q[2]);
    if constexpr (MOMENTS) {
      const int s0 = (A.chunk_base + k) * A.chunk;
      const double n = (double)(A.spp - s0 < A.chunk ? A.spp - s0 : A.chunk);
      mom = mom + v3((q[0] * q[0]) / n, (q[1] * q[1]) / n, (q[2] * q[2]) / n);
    }
  }
  if constexpr (MOMENTS) {
    moments[idx * 3 + 0] = mom.x;
    moments[idx * 3 + 1] = mom.y;
    moments[idx * 3 + 2] = mom.z;
  }
  if (A.combine & 2) {
    store_pixel(A, idx, divide(acc, (double)A.spp));
  } else {  // a batch of chunks before the last: keep the running sum
    A.acc[idx * 3 + 0] = acc.x;
    A.acc[idx * 3 + 1] = acc.y;
    A.acc[idx * 3 + 2] = acc.z;
  }
}
__global__ void __launch_bounds__(256) combine_chunks(LaunchConst A) { combine_body<false>(A, nullptr); }
__global__ void __launch_bounds__(256) combine_chunks_moments(LaunchConst A, double* moments) {
  combine_body<true>(A, moments);
}
__global__ void __launch_bounds__(256) combine_chunks_skip(LaunchConst A) { combine_body<false, true>(A, nullptr); }
__global__ void __launch_bounds__(256) combine_chunks_moments_skip(LaunchConst A, double* moments) {
  combine_body<true, true>(A, moments);
}

// ---------------------------------------------------------------- tier A: the reference's stream
// One lane per image column; rows top to bottom; each pixel draws its 2*ns UVs first and uses
// them in reverse draw order (uniformRandomUVs' foldr, Lib.hs:1358-1371) — the UV pairs are
// recomputed from the pixel's starting state (SplitMix is seed + k*gamma), no list is stored.
// Columns per wave of the tier-A kernel (lanes 0..k-1 of each wave; 64: every lane).
#ifndef RT_EXACT_COLS_PER_WAVE
#define RT_EXACT_COLS_PER_WAVE 1
#endif
constexpr int kExactColsPerWave = RT_EXACT_COLS_PER_WAVE;
// LDS (round 5): the whole node array staged in the block's LDS when it fits (n_nodes records; the
// launch sizes the dynamic LDS). Tier A runs one lane per column, so few waves hold the GPU and each
// dependent node read's latency is the lane's own time: from L2 it cost the Cornell box ~10x the
// 16-thread CPU oracle's time.
template <unsigned F, bool LDS = false>
__global__ void __launch_bounds__(RT_BLOCK) render_exact(LaunchConst A, int n_nodes) {
  __shared__ int stk_mem[RT_STACK * RT_BLOCK];
  int* stk = &stk_mem[threadIdx.x];
  // Tier A reproduces the reference's stream exactly, exact ties included: walk the caller's tree.
  Scene S = A.S;
  S.world = S.world_ref;
  if constexpr (LDS) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_nodes[];
    const uint4* src = reinterpret_cast<const uint4*>(A.S.nodes);
    uint4* dst = reinterpret_cast<uint4*>(lds_nodes);
    const int n16 = n_nodes * (int)(sizeof(rt_node) / 16);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
    S.nodes = reinterpret_cast<const rt_node*>(lds_nodes);
  }
  // One column per wave, on its lane 0: a column is one serial chain of draws (the stream threads every
  // row, sample and bounce), so a wave of 64 columns ran every sample at its slowest lane's path length
  // and through every lane's branches; alone, a lane runs only its own (RT_EXACT_COLS_PER_WAVE).
  const int x = blockIdx.x * (RT_BLOCK / 64) * kExactColsPerWave + (int)(threadIdx.x >> 6) * kExactColsPerWave +
                (int)(threadIdx.x & 63);
  if ((int)(threadIdx.x & 63) >= kExactColsPerWave || x >= A.W) return;
  RngExactT<kSL<F>> g{A.gens[2 * x], A.gens[2 * x + 1]};
  const bool traced = A.trace && x == A.trace_col;
  int tn = 0;
  const int ns = A.spp;
  for (int row = 0; row < A.H; ++row) {
    const int y = A.H - 1 - row;
    const uint64_t seed0 = g.seed;
    g.seed += (uint64_t)(2 * (long long)ns) * g.gamma;
    V3 sum = v3(0, 0, 0);
    for (int j = 0; j < ns; ++j) {
      const int i = ns - 1 - j;
      const double ru = word_to_draw(mix64(seed0 + (uint64_t)(2 * i + 1) * g.gamma));
      const double rv = word_to_draw(mix64(seed0 + (uint64_t)(2 * i + 2) * g.gamma));
      const double u = ((double)x + ru) / (double)A.W;
      const double v = ((double)y + rv) / (double)A.H;
      Ray ray = get_ray(A.cam, u, v, g);
      V3 thr = v3(1.0, 1.0, 1.0), contrib;
      int depth = A.max_depth;
      Cnt cnt{};
      for (int seg = 0;; ++seg) {
        const bool end = segment<F>(A, S, S, ray, thr, depth, g, stk, contrib, cnt);
        if (traced && tn < A.trace_cap) {  // (rt_debug_exact_trace: the oracle's oracle_exact_trace layout)
          double* o = A.trace + 10 * (long long)tn++;
          o[0] = row, o[1] = j, o[2] = end ? -(seg + 1) : seg;
          o[3] = ray.o.x, o[4] = ray.o.y, o[5] = ray.o.z, o[6] = ray.d.x, o[7] = ray.d.y, o[8] = ray.d.z;
          o[9] = __longlong_as_double((long long)g.seed);
        }
        if (end) break;
      }
      if (A.flags & RT_FLAG_NAN_ZERO) contrib = nan_zero(contrib);
      sum = sum + contrib;
    }
    store_pixel(A, (long long)row * A.W + x, divide(sum, (double)ns));
  }
  A.gens[2 * x] = g.seed;
  if (traced) *A.trace_n = tn;
}

// ---------------------------------------------------------------- slab -> image
template <class T>
__global__ void assemble(const T* slabs, T* image, int W, int H, int tile, int tiles_x, int shards,
                         long long slab_pixels) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long long)W * H) return;
  const int row = (int)(i / W), px = (int)(i % W);
  const int gt = (row / tile) * tiles_x + (px / tile);
  const int shard = gt % shards;
  const long long lt = gt / shards;
  const int bpr = tile >> 3;
  const int bx = (px % tile) >> 3, by = (row % tile) >> 3;
  const int within = (by * bpr + bx) * 64 + (row & 7) * 8 + (px & 7);
  const long long src = (long long)shard * slab_pixels + lt * tile * tile + within;
  image[i * 3 + 0] = slabs[src * 3 + 0];
  image[i * 3 + 1] = slabs[src * 3 + 1];
  image[i * 3 + 2] = slabs[src * 3 + 2];
}

// ---------------------------------------------------------------- progressive frames (rt_frame_*)
// The helper kernels of a progressive frame, one set for both traversal orders (SLAB). An unsharded frame
// (SLAB = false) keeps its previews, its error map and its copy of K_p in image order and runs one thread
// per image pixel. A shard frame (SLAB = true, rt.h) is a frame over the slab of (tile, shard_rank,
// shard_count): it keeps all of them in slab order and runs one thread per slab pixel, so its reads and
// writes are contiguous in the slab. Sums, moments and kp are in slab order in both. A carries the frame's
// geometry (fill_frame_geometry with the frame's own shard; an unsharded frame is shard 0 of 1), its sums
// (A.acc) and what a stopped pixel's N_p needs (A.chunk, A.spp). `kp` is an adaptive frame's K_p per slab
// pixel (0 = active); null: no stop call yet, every pixel is active. frame_resolve and frame_error read it
// under ADAPT only, the instantiation a frame takes once it has a kp: as a run-time test in the one kernel it
// cost a C2 frame's rt_frame_error 1.4 us of 119.

// Image pixel -> its slot in an unsharded slab (assemble's map at shards = 1).
__device__ __forceinline__ long long frame_slot(long long i, int W, int tile, int tiles_x) {
  const int row = (int)(i / W), px = (int)(i % W);
  const long long lt = (long long)(row / tile) * tiles_x + (px / tile);
  const int bpr = tile >> 3;
  const int bx = (px % tile) >> 3, by = (row % tile) >> 3;
  return lt * tile * tile + (by * bpr + bx) * 64 + (row & 7) * 8 + (px & 7);
}

// Thread t's pixel. False: it has none (past the image; in slab order also a padding slot, outside the
// image or of a tile past the image's last when there are more shards than tiles: never read, never
// written, never counted). Else `slot` is where the pixel's sums, moments and kp live and `img` is
// row * W + px. A kernel's own outputs (preview, se, K_p copy) and the previous preview are at index t in
// both orders.
template <bool SLAB>
__device__ __forceinline__ bool frame_pixel(const LaunchConst& A, long long t, long long& slot, long long& img) {
  if constexpr (SLAB) {
    int px, row;
    if (t >= A.slab || !work_pixel(A, (uint32_t)t, px, row)) return false;
    slot = t;
    img = (long long)row * A.W + px;
  } else {
    if (t >= (long long)A.W * A.H) return false;
    slot = frame_slot(t, A.W, A.tile, A.tiles_x);
    img = t;
  }
  return true;
}

// A stopped pixel of an adaptive frame (kp[slot] = K_p != 0) is averaged and estimated at its own K_p chunks
// and N_p = min(spp, K_p * CH) samples; an active pixel keeps the frame's `chunks` and `samples`.
__device__ __forceinline__ void pixel_counts(const LaunchConst& A, const int* kp, long long slot, int& chunks,
                                             int& samples) {
  const int k = kp ? kp[slot] : 0;
  if (!k) return;
  const long long n = (long long)k * A.chunk;
  chunks = k;
  samples = n < A.spp ? (int)n : A.spp;
}

// Two per-wave counts (a wave's ballots, already popcounted) summed over the block's 4 waves through LDS;
// they leave the block as at most one atomic per counter.
__device__ __forceinline__ void block_add2(unsigned a, unsigned b, unsigned long long* counts) {
  __shared__ unsigned wave_a[4], wave_b[4];
  if ((threadIdx.x & 63) == 0) {
    wave_a[threadIdx.x >> 6] = a;
    wave_b[threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned ba = wave_a[0] + wave_a[1] + wave_a[2] + wave_a[3];
    const unsigned bb = wave_b[0] + wave_b[1] + wave_b[2] + wave_b[3];
    if (ba) atomicAdd(&counts[0], (unsigned long long)ba);
    if (bb) atomicAdd(&counts[1], (unsigned long long)bb);
  }
}

// A frame's preview: the running sums (A.acc) over `samples` samples (a stopped pixel: over its own N_p),
// averaged and stored as combine_chunks' last batch stores them (divide, store_pixel) in the frame's order:
// A.out_rgb / A.out_lin are its H*W*3 image buffers, or a shard frame's slab*3 buffers (out_lin may be
// null). A.out_rgb still holds the previous preview: counts[0] += pixels whose sum has a NaN channel,
// counts[1] += bytes that change (block_add2). The per-pixel arithmetic does not depend on the order, so the
// assembled slabs of all shards are the unsharded preview bit for bit and their counts add up to its counts.
template <bool SLAB, bool ADAPT>
__global__ void __launch_bounds__(256) frame_resolve(LaunchConst A, int samples, unsigned long long* counts,
                                                     const int* kp) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool nan = false, c0 = false, c1 = false, c2 = false;
  long long slot, img;
  if (frame_pixel<SLAB>(A, t, slot, img)) {
    const V3 sum = vload(A.acc + slot * 3);
    nan = sum.x != sum.x || sum.y != sum.y || sum.z != sum.z;
    if constexpr (ADAPT) {
      int chunks = 0;
      pixel_counts(A, kp, slot, chunks, samples);
    }
    const V3 avg = divide(sum, (double)samples);
    const uint8_t p0 = A.out_rgb[t * 3 + 0], p1 = A.out_rgb[t * 3 + 1], p2 = A.out_rgb[t * 3 + 2];
    store_pixel(A, t, avg);
    c0 = scale_color(avg.x) != p0;
    c1 = scale_color(avg.y) != p1;
    c2 = scale_color(avg.z) != p2;
  }
  const unsigned n_nan = (unsigned)__popcll(__ballot(nan));
  const unsigned n_chg = (unsigned)(__popcll(__ballot(c0)) + __popcll(__ballot(c1)) + __popcll(__ballot(c2)));
  block_add2(n_nan, n_chg, counts);
}

// Saved sums or moments (image order, the whole image) into a frame's slab-order buffer: every pixel of the
// frame's slab fetches its image pixel (rt_frame_restore*). Unsharded, this is assemble<double>'s inverse at
// shards = 1; a shard frame takes the pixels it owns and leaves the other shards' alone.
template <bool SLAB>
__global__ void __launch_bounds__(256) frame_scatter(LaunchConst A, const double* image, double* sums) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long slot, img;
  if (!frame_pixel<SLAB>(A, t, slot, img)) return;
  sums[slot * 3 + 0] = image[img * 3 + 0];
  sums[slot * 3 + 1] = image[img * 3 + 1];
  sums[slot * 3 + 2] = image[img * 3 + 2];
}

// A tracked frame's error map and summary (rt.h): a thread reads its pixel's sums (A.acc) and `moments`,
// computes se[3] (rt::pixel_error, the host's text) at the frame's `chunks` >= 2 and `samples`, or at a
// stopped pixel's own (K_p, N_p): with K_p < 2 that pixel is non-finite, its se channels NaN. `out_se`, when
// given, gets se in the frame's order (device memory; a shard frame's padding slots are left alone).
// acc[0] += non-finite pixels, acc[1] += finite unconverged pixels (block_add2); acc[2] = max se over the
// finite pixels' channels, as the value's bit pattern (non-negative finite doubles order as unsigned
// integers: a lane-shuffle max per wave, LDS, one atomicMax per block); and the block's sum of those se in a
// fixed order (a pixel's channels in order, a wave's lanes by halving shuffles, the waves in wave order) to
// block_sums[blockIdx.x]: frame_error_sum adds them, so the total has no floating-point atomic in it and
// repeats.
template <bool SLAB, bool ADAPT>
__global__ void __launch_bounds__(256) frame_error(LaunchConst A, const double* moments, double* out_se, int chunks,
                                                   int samples, double abs_tol, double rel_tol,
                                                   unsigned long long* acc, double* block_sums, const int* kp) {
  __shared__ unsigned long long wave_max[4];
  __shared__ double wave_sum[4];
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  bool bad = false, open = false;
  double sum = 0.0;
  unsigned long long top = 0ull;
  long long slot, img;
  if (frame_pixel<SLAB>(A, t, slot, img)) {
    const double s[3] = {A.acc[slot * 3], A.acc[slot * 3 + 1], A.acc[slot * 3 + 2]};
    const double q[3] = {moments[slot * 3], moments[slot * 3 + 1], moments[slot * 3 + 2]};
    double se[3];
    if constexpr (ADAPT) pixel_counts(A, kp, slot, chunks, samples);
    int cls = rt::kPixelNonFinite;
    if (!ADAPT || chunks >= 2) {
      cls = rt::pixel_error(s, q, chunks, samples, abs_tol, rel_tol, se);
    } else {
      se[0] = se[1] = se[2] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (out_se) {
      out_se[t * 3 + 0] = se[0];
      out_se[t * 3 + 1] = se[1];
      out_se[t * 3 + 2] = se[2];
    }
    bad = cls == rt::kPixelNonFinite;
    open = cls == rt::kPixelUnconverged;
    if (!bad) {
      sum = (se[0] + se[1]) + se[2];
      const double m = fmax(fmax(se[0], se[1]), se[2]);
      top = (unsigned long long)__double_as_longlong(m);
    }
  }
  const unsigned n_bad = (unsigned)__popcll(__ballot(bad)), n_open = (unsigned)__popcll(__ballot(open));
  for (int off = 32; off > 0; off >>= 1) {
    sum = sum + __shfl_down(sum, off, 64);
    const unsigned long long other = __shfl_down(top, off, 64);
    top = other > top ? other : top;
  }
  if ((threadIdx.x & 63) == 0) {
    wave_max[threadIdx.x >> 6] = top;
    wave_sum[threadIdx.x >> 6] = sum;
  }
  block_add2(n_bad, n_open, acc);  // (its barrier publishes wave_max and wave_sum too)
  if (threadIdx.x == 0) {
    unsigned long long m = wave_max[0];
    for (int w = 1; w < 4; ++w) m = wave_max[w] > m ? wave_max[w] : m;
    if (m) atomicMax(&acc[2], m);
    block_sums[blockIdx.x] = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
  }
}

// frame_error's block sums added in a fixed order by one block: thread t adds blocks t, t + 256, ... in
// block order, then the threads' sums fold as a block's do (lanes by halving shuffles, waves in wave order).
__global__ void __launch_bounds__(256) frame_error_sum(const double* block_sums, int blocks, double* out) {
  __shared__ double wave_sum[4];
  double sum = 0.0;
  for (int b = threadIdx.x; b < blocks; b += 256) sum = sum + block_sums[b];
  for (int off = 32; off > 0; off >>= 1) sum = sum + __shfl_down(sum, off, 64);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) *out = ((wave_sum[0] + wave_sum[1]) + wave_sum[2]) + wave_sum[3];
}

// K_p in the frame's order (rt_frame_chunk_counts, rt_frame_shard_state): a stopped pixel's kp, else the
// frame's K.
template <bool SLAB>
__global__ void __launch_bounds__(256) frame_chunk_counts(LaunchConst A, const int* kp, int* out, int K) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  long long slot, img;
  if (!frame_pixel<SLAB>(A, t, slot, img)) return;
  const int k = kp ? kp[slot] : 0;
  out[t] = k ? k : K;
}

// Adaptive frames (rt.h): stops active pixels, by the rule (RULE: rt::adapt_pixel, the host's text, at the
// frame's K chunks and N samples) or by the caller's image-order byte mask. One thread per slab pixel in
// both kinds of frame, so that a wave is one word of the skip bitmask (64 consecutive slab pixels, one 8x8
// block; work_pixel is frame_slot's inverse): a newly stopped pixel gets kp = K, and the wave's lane 0
// writes the word from one ballot of "stopped before or now" (padding pixels outside the image: never set,
// never counted). counts[0] += pixels stopped by this call, counts[1] += those of them whose sum has a NaN
// channel (block_add2).
template <bool RULE>
__device__ __forceinline__ void adapt_body(const LaunchConst& A, const double* moments, int* kp,
                                           unsigned long long* skip, const uint8_t* mask, int K, int N,
                                           rt_adapt_rule rule, unsigned long long* counts) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  bool stopped = false, now = false, now_nan = false;
  long long slot, img;
  if (frame_pixel<true>(A, idx, slot, img)) {
    stopped = kp[idx] != 0;
    if (!stopped) {
      const double s[3] = {A.acc[idx * 3], A.acc[idx * 3 + 1], A.acc[idx * 3 + 2]};
      if constexpr (RULE) {
        double q[3] = {0.0, 0.0, 0.0};
        if (moments) q[0] = moments[idx * 3], q[1] = moments[idx * 3 + 1], q[2] = moments[idx * 3 + 2];
        now = rt::adapt_pixel(s, q, K, N, rule.flags, rule.abs_tol, rule.rel_tol, rule.min_chunks) != rt::kAdaptKeep;
      } else {
        now = mask[img] != 0;
      }
      if (now) {
        kp[idx] = K;
        now_nan = s[0] != s[0] || s[1] != s[1] || s[2] != s[2];
      }
    }
  }
  const unsigned long long word = __ballot(stopped || now);
  const unsigned n_now = (unsigned)__popcll(__ballot(now)), n_nan = (unsigned)__popcll(__ballot(now_nan));
  // (the slab is whole 8x8 blocks: a wave is inside it or past it)
  if ((threadIdx.x & 63) == 0 && idx < A.slab) skip[idx >> 6] = word;
  block_add2(n_now, n_nan, counts);
}
__global__ void __launch_bounds__(256) frame_adapt(LaunchConst A, const double* moments, int* kp,
                                                   unsigned long long* skip, int K, int N, rt_adapt_rule rule,
                                                   unsigned long long* counts) {
  adapt_body<true>(A, moments, kp, skip, nullptr, K, N, rule, counts);
}
__global__ void __launch_bounds__(256) frame_stop_mask(LaunchConst A, int* kp, unsigned long long* skip,
                                                       const uint8_t* mask, int K, unsigned long long* counts) {
  adapt_body<false>(A, nullptr, kp, skip, mask, K, 0, rt_adapt_rule{}, counts);
}

// An adaptive frame's stops put back from a checkpoint (rt_frame_resume*): one thread per slab pixel in both
// kinds of frame, as adapt_body, so that a wave is one word of the skip bitmask. A thread reads its pixel's
// saved K_p (`stops`: the whole image, image order, 0 = active) into kp, and the wave's lane 0 writes the word
// from one ballot of "stopped". The sums (A.acc) have been scattered before: counts[0] += stopped pixels,
// counts[1] += those of them whose sum has a NaN channel (block_add2). Padding slots: never set, never counted
// (kp is zeroed beforehand).
__global__ void __launch_bounds__(256) frame_restore_stops(LaunchConst A, const int* stops, int* kp,
                                                           unsigned long long* skip, unsigned long long* counts) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  bool stopped = false, nan = false;
  long long slot, img;
  if (frame_pixel<true>(A, idx, slot, img)) {
    const int k = stops[img];
    kp[idx] = k;
    stopped = k != 0;
    if (stopped) {
      const double s[3] = {A.acc[idx * 3], A.acc[idx * 3 + 1], A.acc[idx * 3 + 2]};
      nan = s[0] != s[0] || s[1] != s[1] || s[2] != s[2];
    }
  }
  const unsigned long long word = __ballot(stopped);
  const unsigned n_stopped = (unsigned)__popcll(word), n_nan = (unsigned)__popcll(__ballot(nan));
  // (the slab is whole 8x8 blocks: a wave is inside it or past it)
  if ((threadIdx.x & 63) == 0 && idx < A.slab) skip[idx >> 6] = word;
  block_add2(n_stopped, n_nan, counts);
}

// ---------------------------------------------------------------- debug: closest hits
template <unsigned F, bool PK = false>
__global__ void __launch_bounds__(RT_BLOCK) closest_hits(Scene S, const double* rays, int n, double tmin,
                                                         double tmax, uint64_t seed, int joint, int walk, double* out) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  int* stk = &stk_mem[threadIdx.x];
  Side side{&stk_mem[(((F & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + 1) * RT_BLOCK + threadIdx.x], RT_BLOCK};
  const int i = blockIdx.x * RT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double* q = rays + 7 * (long long)i;
  const Ray r{v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), q[6]};
  RngPhilox g;
  g.init(seed, (uint32_t)i, 0);
  Hit h;
  double* o = out + 12 * (long long)i;
  Cnt cnt{};
  bool got;
  if (walk == 0) {
    got = traverse<F>(S, S.ref_walk ? S.world_ref : S.world, r, tmin, tmax, h, g, stk, joint != 0, cnt);
  } else {  // the render loop's resumable walk (binary, or 4-wide under F_WIDE)
    Trav t;
    trav_begin<F>(t, r, S.world, tmin, tmax);
    if (S.ref_walk) trav_restart_ref(t, S.world, tmax);  // (the re-bounded skeleton, mixed walk)
    trav_media_first<F>(S, t, tmin, cnt, g, side);        // (hoisted media as the render loop takes them)
    bool walking = true;
    walk_until<F, PK>(S, t, walking, tmin, stk, RT_BLOCK, joint != 0, 0, 0, cnt, g, side);
    if (t.tie || (kRefMixed<F> && t.lite)) {
      trav_redo<F>(t, S.world_ref, tmax);
      if constexpr (kNoInv<F>) t.ray = prep(plain(t.ray));  // (the redo's binary box tests need 1/d)
      do {
        while (trav_step<F>(S, t, tmin, stk, RT_BLOCK, joint != 0, cnt, g, side)) {
        }
      } while (redo_again<F>(t) && (trav_redo<F>(t, S.world_ref, tmax), true));
    }
    got = trav_finish<F>(S, t, r, tmin, h, side);
  }
  if (got) {
    o[0] = 1; o[1] = h.t;
    o[2] = h.p.x; o[3] = h.p.y; o[4] = h.p.z;
    o[5] = h.n.x; o[6] = h.n.y; o[7] = h.n.z;
    o[8] = h.u; o[9] = h.v; o[10] = h.ff; o[11] = h.mat;
  } else {
    for (int k = 0; k < 12; ++k) o[k] = 0;
  }
}

// ---------------------------------------------------------------- first-hit feature buffers (rt.h rt_render_features)
// Kernel arguments of a feature pass. Passed by value: the pass has no launch constants of its own to stage.
struct FeatureArgs {
  Scene S;
  rt_camera cam;
  int W, H;
  uint32_t flags;  // (RT_FLAG_REFERENCE_CULL)
  uint64_t seed;
  int first, count;  // samples first .. first + count - 1 (first + count <= INT32_MAX)
  int accumulate;    // the fold starts from `sums` instead of 0
  int leaf_stop;     // walk_until's leaf_stop, /64 of the live lanes (FeaturePlan::leaf_stop: scheduling only)
  int blocks_x;      // 8x8 pixel blocks per row of blocks, and in the frame
  unsigned long long blocks_total;
  unsigned long long* counter;  // the next unclaimed block (0 at launch)
  double* sums;                 // [H][W][RT_FEATURE_DOUBLES], image order
};

// The first segment's closest hit in [kEps, +inf), by the sequence the closest_hits probe runs: the resumable
// walk to its end (stop 0, so the wave's lanes step in lockstep until the last one is done), then the tie redo;
// REC: the recursive walk. `g` is the sample's own stream after getRay, so a medium's keyed draw sees the
// position the render's first segment sees.
template <unsigned F, bool PK, bool REC>
__device__ __forceinline__ bool first_hit(const Scene& S, const Ray& r, RngPhilox& g, int* stk, int stride, Side& side,
                                          bool joint, int leaf_stop, Hit& h) {
  Cnt cnt{};
  if constexpr (REC) {
    return traverse<F>(S, S.ref_walk ? S.world_ref : S.world, r, kEps, INFINITY, h, g, stk, joint, cnt, stride);
  } else {
    Trav t;
    trav_begin<F>(t, r, S.world, kEps, INFINITY);
    if (S.ref_walk) trav_restart_ref(t, S.world, INFINITY);
    trav_media_first<F>(S, t, kEps, cnt, g, side);
    bool walking = true;
    const int live = __popcll(__ballot(true));
    walk_until<F, PK>(S, t, walking, kEps, stk, stride, joint, 0, (live * leaf_stop) >> 6, cnt, g, side);
    if (t.tie || (kRefMixed<F> && t.lite)) {
      trav_redo<F>(t, S.world_ref, INFINITY);
      if constexpr (kNoInv<F>) t.ray = prep(plain(t.ray));  // (the redo's binary box tests need 1/d)
      do {
        while (trav_step<F>(S, t, kEps, stk, stride, joint, cnt, g, side)) {
        }
      } while (redo_again<F>(t) && (trav_redo<F>(t, S.world_ref, INFINITY), true));
    }
    return trav_finish<F>(S, t, r, kEps, h, side);
  }
}

// A wave is one 8x8 pixel block, a lane one pixel: the lane folds the feature vectors of its samples, in sample
// order, into eight accumulators and stores them once (64 contiguous bytes). Blocks are claimed from the pass's
// counter, one atomic per wave and block; which wave folds a pixel does not show in its sums. Lanes outside the
// image idle through the block.
// SLAB (rt_kernels_shard.h's kernels): the pass over a shard's record slab. A claimed block is block b of the slab
// (rt_layout.h slab_block gives its pixels, `G` the shard's geometry) and the lane's record lives at slot b * 64 +
// lane instead of the pixel's place in the image: a wave's 64 stores are one contiguous 4 KB run.
template <unsigned F, bool PK, bool REC, bool SLAB = false>
__device__ __forceinline__ void features_loop(const FeatureArgs& A, const Scene& S, int* stk, int stride, int* side_p,
                                              const SlabGeometry* G = nullptr) {
  const int lane = threadIdx.x & 63;
  const bool joint = !(A.flags & RT_FLAG_REFERENCE_CULL);
  Side side{side_p, stride};
  for (;;) {
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(A.counter, 1ull);
    b = __shfl(b, 0);
    if (b >= A.blocks_total) break;
    int px, row;
    if constexpr (SLAB) {
      int px0 = A.W, row0 = A.H;  // (a block of a tile past the image's last, which the host never hands out: idles)
      slab_block(*G, (uint32_t)b, px0, row0);
      px = px0 + (lane & 7), row = row0 + (lane >> 3);
    } else {
      const uint32_t by = (uint32_t)b / (uint32_t)A.blocks_x, bx = (uint32_t)b - by * (uint32_t)A.blocks_x;
      px = (int)(bx * 8u) + (lane & 7), row = (int)(by * 8u) + (lane >> 3);
    }
    if (px >= A.W || row >= A.H) continue;  // (idles until the wave's next claim)
    const uint32_t pid = (uint32_t)((long long)row * A.W + px);
    double* q = A.sums + (SLAB ? (size_t)b * 64 + (size_t)lane : (size_t)pid) * RT_FEATURE_DOUBLES;
    double acc[RT_FEATURE_DOUBLES];
#pragma unroll
    for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) acc[k] = A.accumulate ? q[k] : 0.0;
    const int s_end = A.first + A.count;
    for (int s = A.first; s < s_end; ++s) {
      RngPhilox g;
      g.init(A.seed, pid, (uint32_t)s);
      g.reserve(3);  // the UV pair and the first disk try
      const double ru = g.draw(), rv = g.draw();
      const int y = A.H - 1 - row;
      const double u = ((double)px + ru) / (double)A.W;
      const double v = ((double)y + rv) / (double)A.H;
      const Ray ray = get_ray(A.cam, u, v, g);
      Hit h;
      double f[RT_FEATURE_DOUBLES] = {A.S.bg[0], A.S.bg[1], A.S.bg[2], 0.0, 0.0, 0.0, 0.0, 0.0};
      if (first_hit<F, PK, REC>(S, ray, g, stk, stride, side, joint, A.leaf_stop, h)) {
        // textureValue for every material that has a texture, a DiffuseLight's front face included (so not
        // hit_texture, which leaves that one out); the kernel's one copy of the texture code
        const DMat m = S.mats[h.mat];
        const V3 a = m.type == RT_MAT_DIELECTRIC ? v3(1.0, 1.0, 1.0) : texture_value<F>(S, m.tex, h.u, h.v, h.p);
        f[RT_FEAT_ALBEDO] = a.x, f[RT_FEAT_ALBEDO + 1] = a.y, f[RT_FEAT_ALBEDO + 2] = a.z;
        f[RT_FEAT_NORMAL] = h.n.x, f[RT_FEAT_NORMAL + 1] = h.n.y, f[RT_FEAT_NORMAL + 2] = h.n.z;
        f[RT_FEAT_DEPTH] = h.t * sqrt(dot(ray.d, ray.d));
        f[RT_FEAT_HITS] = 1.0;
      }
#pragma unroll
      for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) acc[k] = acc[k] + f[k];
    }
#pragma unroll
    for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) q[k] = acc[k];
  }
}

// From global memory: the lane stacks (and Side slots) in static LDS at their maxima, as the closest_hits probe.
template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_features(FeatureArgs A) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  features_loop<F, PK, REC>(A, A.S, &stk_mem[threadIdx.x],  RT_BLOCK,
                            &stk_mem[(((F & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + 1) * RT_BLOCK + threadIdx.x]);
}

// The staged 4-wide kernels' prologue: the wide nodes, and with LEAF_LDS the leaf table, copied into the dynamic LDS
// by the whole workgroup, a barrier, and the scene that reads them there; returns this lane's stack behind them.
template <bool LEAF_LDS>
__device__ __forceinline__ int* stage_wide_lds(const Scene& in, int n_nodes, int n_leaves, Scene& S) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  constexpr int rec = (int)sizeof(rt_wnode), lrec = (int)sizeof(rt_node);
  {
    const uint4* src = reinterpret_cast<const uint4*>(in.wnodes);
    uint4* dst = reinterpret_cast<uint4*>(lds);
    const int n16 = n_nodes * (rec / 16);
    for (int i = threadIdx.x; i < n16; i += blockDim.x) dst[i] = src[i];
    if constexpr (LEAF_LDS) {
      const uint4* lsrc = reinterpret_cast<const uint4*>(in.leaves);
      uint4* ldst = reinterpret_cast<uint4*>(lds + (size_t)n_nodes * rec);
      const int l16 = n_leaves * (lrec / 16);
      for (int i = threadIdx.x; i < l16; i += blockDim.x) ldst[i] = lsrc[i];
    }
  }
  __syncthreads();
  S = in;
  S.wnodes = reinterpret_cast<const rt_wnode*>(lds);
  if constexpr (LEAF_LDS) S.leaves = reinterpret_cast<const rt_node*>(lds + (size_t)n_nodes * rec);
  else n_leaves = 0;
  return reinterpret_cast<int*>(lds + (size_t)n_nodes * rec + (size_t)n_leaves * lrec) + threadIdx.x;
}

// LDS-staged 4-wide walk (spheres-only worlds): the wide nodes, the leaf table (LEAF_LDS, its own instantiation
// as in render_philox2_lds) and the lane stacks, `stack_entries` per lane, copied once per workgroup of up to 16
// waves; the block size is the launch's (1 to 4 waves per SIMD).
template <unsigned F, bool LEAF_LDS, bool PK>
__global__ void __launch_bounds__(1024) render_features_lds(FeatureArgs A, int n_nodes, int stack_entries, int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(A.S, n_nodes, n_leaves, S);
  (void)stack_entries;  // (the host sizes the LDS with it: plan_features)
  features_loop<F, PK, false>(A, S, stk, (int)blockDim.x, stk);  // (no frames: the Side slots are never touched)
}

// ---------------------------------------------------------------- specular-chain feature buffers (rt.h rt_render_features_chain)
// A first-hit pass's arguments and the chain's. Kernels and a loop of their own, siblings of the first-hit ones,
// which compile to what they compiled to before.
struct FeatureChainArgs {
  FeatureArgs A;
  int max_bounces;       // 0..RT_CHAIN_MAX_BOUNCES
  uint32_t chain_flags;  // RT_CHAIN_*
  double max_fuzz;
  unsigned long long* counts;  // {ended_miss, ended_cap, bounces}, 0 at launch
};

// features_loop with the chain of rt.h per sample: first_hit, then the sample ends or the lane scatters and runs
// first_hit again. The chain loop relies on reconvergence: a lane whose chain has ended leaves the loop and is masked
// off until the wave's last chain ends, so walk_until's ballots (its `stop` of 0 walks until no active lane walks)
// and first_hit's live count, which scales leaf_stop, see the lanes still in a chain and nothing else; no lane
// carries a `walking = false` through a walk it takes no part in. Counts: three integers per lane over all the
// blocks the wave folds, reduced and added once per wave after the last block (wave_add, as the render loops do).
// Not once per block: an `if (lane == 0) atomicAdd` at the bottom of the block loop sits next to the claim's
// `if (lane == 0)` at its top, the compiler threads the one branch into the other, and the wave's lanes no longer
// meet at the claim's __shfl: the lanes that skipped both read a stale block id and never leave the loop.
template <unsigned F, bool PK, bool REC, bool SLAB = false>  // (SLAB: as features_loop)
__device__ __forceinline__ void features_chain_loop(const FeatureChainArgs& C, const Scene& S, int* stk, int stride,
                                                    int* side_p, const SlabGeometry* G = nullptr) {
  const FeatureArgs& A = C.A;
  const int lane = threadIdx.x & 63;
  const bool joint = !(A.flags & RT_FLAG_REFERENCE_CULL);
  Side side{side_p, stride};
  unsigned long long n_miss = 0, n_cap = 0, n_bounce = 0;
  for (;;) {
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(A.counter, 1ull);
    b = __shfl(b, 0);
    if (b >= A.blocks_total) break;
    int px, row;
    if constexpr (SLAB) {
      int px0 = A.W, row0 = A.H;
      slab_block(*G, (uint32_t)b, px0, row0);
      px = px0 + (lane & 7), row = row0 + (lane >> 3);
    } else {
      const uint32_t by = (uint32_t)b / (uint32_t)A.blocks_x, bx = (uint32_t)b - by * (uint32_t)A.blocks_x;
      px = (int)(bx * 8u) + (lane & 7), row = (int)(by * 8u) + (lane >> 3);
    }
    if (px < A.W && row < A.H) {  // (a lane outside the image idles until the wave's next claim)
      const uint32_t pid = (uint32_t)((long long)row * A.W + px);
      double* q = A.sums + (SLAB ? (size_t)b * 64 + (size_t)lane : (size_t)pid) * RT_FEATURE_DOUBLES;
      double acc[RT_FEATURE_DOUBLES];
#pragma unroll
      for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) acc[k] = A.accumulate ? q[k] : 0.0;
      const int s_end = A.first + A.count;
      for (int s = A.first; s < s_end; ++s) {
        RngPhilox g;
        g.init(A.seed, pid, (uint32_t)s);
        g.reserve(3);  // the UV pair and the first disk try
        const double ru = g.draw(), rv = g.draw();
        const int y = A.H - 1 - row;
        const double u = ((double)px + ru) / (double)A.W;
        const double v = ((double)y + rv) / (double)A.H;
        Ray ray = get_ray(A.cam, u, v, g);
        V3 thr = v3(1.0, 1.0, 1.0);
        double len = 0.0;
        int nb = 0;
        for (;;) {
          Hit h;
          if (!first_hit<F, PK, REC>(S, ray, g, stk, stride, side, joint, A.leaf_stop, h)) {
            const V3 c = vmul(thr, v3(A.S.bg[0], A.S.bg[1], A.S.bg[2]));
            acc[RT_FEAT_ALBEDO] = acc[RT_FEAT_ALBEDO] + c.x;
            acc[RT_FEAT_ALBEDO + 1] = acc[RT_FEAT_ALBEDO + 1] + c.y;
            acc[RT_FEAT_ALBEDO + 2] = acc[RT_FEAT_ALBEDO + 2] + c.z;
#pragma unroll
            for (int k = RT_FEAT_NORMAL; k < RT_FEATURE_DOUBLES; ++k) acc[k] = acc[k] + 0.0;  // (-0.0 + 0.0 is +0.0)
            ++n_miss;
            break;
          }
          len = len + h.t * sqrt(dot(ray.d, ray.d));
          const DMat m = S.mats[h.mat];
          const bool diel = m.type == RT_MAT_DIELECTRIC, metal = m.type == RT_MAT_METAL;
          const bool follows = diel ? (C.chain_flags & RT_CHAIN_DIELECTRIC) != 0
                                    : metal && (C.chain_flags & RT_CHAIN_METAL) != 0 && m.param <= C.max_fuzz;
          // The first-hit rule's albedo, which is also scatter's attenuation of the two followed materials
          // (Dielectric (1,1,1), Metal its texture): the kernel's one copy of the texture code.
          const V3 a = diel ? v3(1.0, 1.0, 1.0) : texture_value<F>(S, m.tex, h.u, h.v, h.p);
          if (!follows || nb >= C.max_bounces) {
            const V3 c = vmul(thr, a);
            acc[RT_FEAT_ALBEDO] = acc[RT_FEAT_ALBEDO] + c.x;
            acc[RT_FEAT_ALBEDO + 1] = acc[RT_FEAT_ALBEDO + 1] + c.y;
            acc[RT_FEAT_ALBEDO + 2] = acc[RT_FEAT_ALBEDO + 2] + c.z;
            acc[RT_FEAT_NORMAL] = acc[RT_FEAT_NORMAL] + h.n.x;
            acc[RT_FEAT_NORMAL + 1] = acc[RT_FEAT_NORMAL + 1] + h.n.y;
            acc[RT_FEAT_NORMAL + 2] = acc[RT_FEAT_NORMAL + 2] + h.n.z;
            acc[RT_FEAT_DEPTH] = acc[RT_FEAT_DEPTH] + len;
            acc[RT_FEAT_HITS] = acc[RT_FEAT_HITS] + 1.0;
            n_cap += follows;
            break;
          }
          g.rewind();  // (the words buffered before the walk were not carried through it)
          const V3 d = scatter_specular(m, metal, ray, h, g);
          ray.o = h.p, ray.d = d;  // (the time stays the sample's)
          thr = vmul(thr, a);
          ++nb;
        }
        n_bounce += (unsigned)nb;
      }
#pragma unroll
      for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) q[k] = acc[k];
    }
  }
  wave_add(&C.counts[0], n_miss);
  wave_add(&C.counts[1], n_cap);
  wave_add(&C.counts[2], n_bounce);
}

template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_features_chain(FeatureChainArgs C) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  features_chain_loop<F, PK, REC>(C, C.A.S, &stk_mem[threadIdx.x], RT_BLOCK,
                                  &stk_mem[(((F & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + 1) * RT_BLOCK + threadIdx.x]);
}

// render_features_lds's staging. WAVES: the most waves per SIMD the kernel is launched with (blocks of up to
// WAVES * 256 threads), which sets its register budget: 3 leaves the chain's state in registers, 4 spills it.
template <unsigned F, bool LEAF_LDS, bool PK, int WAVES>
__global__ void __launch_bounds__(WAVES * 256) render_features_chain_lds(FeatureChainArgs C, int n_nodes, int stack_entries,
                                                                  int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(C.A.S, n_nodes, n_leaves, S);
  (void)stack_entries;
  features_chain_loop<F, PK, false>(C, S, stk, (int)blockDim.x, stk);
}

// ---------------------------------------------------------------- material-ID coverage buffers (rt.h rt_render_ids)
// A chain pass's arguments: A.sums is the pass's rt_id_record array (64 bytes per pixel, as a feature vector), a
// pass without a chain has max_bounces = 0, and `counts` may be null (then nothing is counted).
using IdArgs = FeatureChainArgs;
// A slab pass's arguments (rt_kernels_shard.h's kernels), for all three passes: the chain pass's (a first-hit pass
// reads C.A alone, an ID pass without a chain has max_bounces = 0 and null counts) and the shard's geometry.
struct FeatureSlabArgs {
  FeatureChainArgs C;
  SlabGeometry G;
};

// features_chain_loop's nest (its comment says why it has this shape: ended lanes leave the chain loop and
// reconverge, first_hit's ballot sees the lanes still in a chain, the counts go through wave_add after the block
// loop) with a sample's id where that loop takes its features: the material of the chain's terminal vertex, or
// RT_ID_MISS, folded into the lane's record by rt_ids.h's ids_fold_one, whose slots are compared and updated under
// predicates and so stay in registers. No throughput, no path length, no albedo: the kernel has no texture code.
// One loop for both modes: a pass without a chain runs it with max_bounces = 0, where no material is followed.
template <unsigned F, bool PK, bool REC, bool SLAB = false>  // (SLAB: as features_loop)
__device__ __forceinline__ void ids_loop(const IdArgs& C, const Scene& S, int* stk, int stride, int* side_p,
                                         const SlabGeometry* G = nullptr) {
  const FeatureArgs& A = C.A;
  const int lane = threadIdx.x & 63;
  const bool joint = !(A.flags & RT_FLAG_REFERENCE_CULL);
  Side side{side_p, stride};
  unsigned long long n_miss = 0, n_cap = 0, n_bounce = 0;
  for (;;) {
    unsigned long long b = 0;
    if (lane == 0) b = atomicAdd(A.counter, 1ull);
    b = __shfl(b, 0);
    if (b >= A.blocks_total) break;
    int px, row;
    if constexpr (SLAB) {
      int px0 = A.W, row0 = A.H;
      slab_block(*G, (uint32_t)b, px0, row0);
      px = px0 + (lane & 7), row = row0 + (lane >> 3);
    } else {
      const uint32_t by = (uint32_t)b / (uint32_t)A.blocks_x, bx = (uint32_t)b - by * (uint32_t)A.blocks_x;
      px = (int)(bx * 8u) + (lane & 7), row = (int)(by * 8u) + (lane >> 3);
    }
    if (px < A.W && row < A.H) {  // (a lane outside the image idles until the wave's next claim)
      const uint32_t pid = (uint32_t)((long long)row * A.W + px);
      // (hipMalloc'd: 16-byte aligned records)
      uint4* q = reinterpret_cast<uint4*>(A.sums) + (SLAB ? (size_t)b * 64 + (size_t)lane : (size_t)pid) * 4;
      static_assert(sizeof(rt_id_record) == 64 && sizeof(rt_id_record) == sizeof(double) * RT_FEATURE_DOUBLES, "rt.h");
      // the record, field by field in rt.h's order: id[7], count[7], other, samples
      const uint4 z = make_uint4(0u, 0u, 0u, 0u);
      const uint4 w0 = A.accumulate ? q[0] : z, w1 = A.accumulate ? q[1] : z, w2 = A.accumulate ? q[2] : z,
                  w3 = A.accumulate ? q[3] : z;
      rt_id_record r;
      r.id[0] = w0.x, r.id[1] = w0.y, r.id[2] = w0.z, r.id[3] = w0.w, r.id[4] = w1.x, r.id[5] = w1.y, r.id[6] = w1.z;
      r.count[0] = w1.w, r.count[1] = w2.x, r.count[2] = w2.y, r.count[3] = w2.z, r.count[4] = w2.w;
      r.count[5] = w3.x, r.count[6] = w3.y, r.other = w3.z, r.samples = w3.w;
      const int s_end = A.first + A.count;
      for (int s = A.first; s < s_end; ++s) {
        RngPhilox g;
        g.init(A.seed, pid, (uint32_t)s);
        g.reserve(3);  // the UV pair and the first disk try
        const double ru = g.draw(), rv = g.draw();
        const int y = A.H - 1 - row;
        const double u = ((double)px + ru) / (double)A.W;
        const double v = ((double)y + rv) / (double)A.H;
        Ray ray = get_ray(A.cam, u, v, g);
        int nb = 0;
        uint32_t id = RT_ID_MISS;
        for (;;) {
          Hit h;
          if (!first_hit<F, PK, REC>(S, ray, g, stk, stride, side, joint, A.leaf_stop, h)) {
            ++n_miss;
            break;
          }
          const DMat m = S.mats[h.mat];
          const bool diel = m.type == RT_MAT_DIELECTRIC, metal = m.type == RT_MAT_METAL;
          const bool follows = diel ? (C.chain_flags & RT_CHAIN_DIELECTRIC) != 0
                                    : metal && (C.chain_flags & RT_CHAIN_METAL) != 0 && m.param <= C.max_fuzz;
          if (!follows || nb >= C.max_bounces) {
            id = (uint32_t)h.mat;
            n_cap += follows;
            break;
          }
          g.rewind();  // (the words buffered before the walk were not carried through it)
          const V3 d = scatter_specular(m, metal, ray, h, g);
          ray.o = h.p, ray.d = d;  // (the time stays the sample's)
          ++nb;
        }
        n_bounce += (unsigned)nb;
        rt::ids_fold_one(r, id);
      }
      q[0] = make_uint4(r.id[0], r.id[1], r.id[2], r.id[3]);
      q[1] = make_uint4(r.id[4], r.id[5], r.id[6], r.count[0]);
      q[2] = make_uint4(r.count[1], r.count[2], r.count[3], r.count[4]);
      q[3] = make_uint4(r.count[5], r.count[6], r.other, r.samples);
    }
  }
  if (C.counts) {  // (uniform: a kernel argument)
    wave_add(&C.counts[0], n_miss);
    wave_add(&C.counts[1], n_cap);
    wave_add(&C.counts[2], n_bounce);
  }
}

template <unsigned F, bool PK, bool REC>
__global__ void __launch_bounds__(RT_BLOCK) render_ids(IdArgs C) {
  __shared__ int stk_mem[(lane_ints<F>() + 1) * RT_BLOCK];
  ids_loop<F, PK, REC>(C, C.A.S, &stk_mem[threadIdx.x], RT_BLOCK,
                       &stk_mem[(((F & (F_WIDE | F_MIXW)) ? RT_WSTACK : RT_STACK) + 1) * RT_BLOCK + threadIdx.x]);
}

// render_features_chain_lds's staging and WAVES.
template <unsigned F, bool LEAF_LDS, bool PK, int WAVES>
__global__ void __launch_bounds__(WAVES * 256) render_ids_lds(IdArgs C, int n_nodes, int stack_entries, int n_leaves) {
  static_assert((F & F_WIDE) != 0 && (F & F_FRAMES) == 0, "the spheres-only 4-wide walk");
  Scene S;
  int* stk = stage_wide_lds<LEAF_LDS>(C.A.S, n_nodes, n_leaves, S);
  (void)stack_entries;
  ids_loop<F, PK, false>(C, S, stk, (int)blockDim.x, stk);
}

// ---------------------------------------------------------------- debug: per-function probes
// The hot-path functions one at a time on device inputs (rt_debug_probe; layouts in rt.h and
// oracle/oracle.c oracle_probe): record i draws from its own tier-B Philox stream (key = seed, pid = i,
// sample 0), so the oracle's golden vectors consume the same numbers.
constexpr int kProbeIn[6] = {18, 3, 6, 6, 2, 14}, kProbeOut[6] = {14, 4, 2, 3, 8, 3};
template <unsigned F>
__global__ void __launch_bounds__(RT_BLOCK) fn_probe(Scene S, rt_camera cam, int op, const double* in, int n,
                                                    uint64_t seed, double* out) {
  const int i = blockIdx.x * RT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const double* q = in + (long long)kProbeIn[op] * i;
  double* o = out + (long long)kProbeOut[op] * i;
  for (int k = 0; k < kProbeOut[op]; ++k) o[k] = 0.0;
  RngPhilox g;
  g.init(seed, (uint32_t)i, 0);
  if (op == 0) {  // scatter (or emitted for DiffuseLight), as shade_hit runs it
    const Ray r{v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), q[6]};
    Hit h;
    h.t = q[7];
    h.p = v3(q[8], q[9], q[10]);
    h.n = v3(q[11], q[12], q[13]);
    h.u = q[14];
    h.v = q[15];
    h.ff = (int)q[16];
    h.mat = (int)q[17];
    const DMat m = S.mats[h.mat];
    const V3 tx = hit_texture<F>(S, m, h);
    if (m.type == RT_MAT_DIFFUSE_LIGHT) {
      const V3 e = h.ff ? v3(0, 0, 0) : mat_texture<F>(S, m, h, tx);
      o[8] = e.x, o[9] = e.y, o[10] = e.z;
    } else {
      Scatter sc;
      scatter<F>(S, m, r, h, g, sc, tx);
      o[0] = 1;
      o[1] = sc.ray.o.x, o[2] = sc.ray.o.y, o[3] = sc.ray.o.z;
      o[4] = sc.ray.d.x, o[5] = sc.ray.d.y, o[6] = sc.ray.d.z, o[7] = sc.ray.tm;
      o[8] = sc.att.x, o[9] = sc.att.y, o[10] = sc.att.z;
      o[11] = sc.pdf;
      o[12] = sc.specular;
    }
    o[13] = g.consumed();
  } else if (op == 1) {  // htblRandom on the lights tree
    const V3 d = htbl_random(S, S.lights, v3(q[0], q[1], q[2]), g);
    o[0] = d.x, o[1] = d.y, o[2] = d.z;
    o[3] = g.consumed();
  } else if (op == 2) {  // htblPdfValue on the lights tree
    const V3 org = v3(q[0], q[1], q[2]), v = v3(q[3], q[4], q[5]);
    o[0] = S.lights < 0 ? 0.0 : htbl_pdf_value<F, RT_LIGHT_DEPTH>(S, S.lights, org, v, prep(Ray{org, v, 0.0}));
    o[1] = g.consumed();
  } else if (op == 3) {  // textureValue
    const V3 a = texture_value<F>(S, (int)q[0], q[1], q[2], v3(q[3], q[4], q[5]));
    o[0] = a.x, o[1] = a.y, o[2] = a.z;
  } else if (op == 5) {  // the box test: division-free (the walks'), with divisions, the reference's per-axis
    const RayX r = prep(Ray{v3(q[6], q[7], q[8]), v3(q[9], q[10], q[11]), 0.0});
    o[0] = box_hit(q, r, q[12], q[13], true);
    o[1] = box_hit_exact(q, r, q[12], q[13], true);
    o[2] = box_hit_exact(q, r, q[12], q[13], false);
  } else {  // getRay
    const Ray r = get_ray(cam, q[0], q[1], g);
    o[0] = r.o.x, o[1] = r.o.y, o[2] = r.o.z;
    o[3] = r.d.x, o[4] = r.d.y, o[5] = r.d.z, o[6] = r.tm;
    o[7] = g.consumed();
  }
}

// ---------------------------------------------------------------- debug: numerics probe
__global__ void math_probe(int op, const double* x, const double* y, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double a = x[i], b = y[i];
  double r;
  switch (op) {
    case 0: r = a / b; break;
    case 1: r = div_exact(a, b, 1.0 / b); break;
    case 2: r = sqrt(a); break;
    case 3: r = sin(a); break;
    case 4: r = cos(a); break;
    case 5: r = atan(a); break;
    case 6: r = asin(a); break;
    case 7: r = log(a); break;
    case 8: r = pow(a, b); break;
    case 9: r = ghc_atan2(a, b); break;
    case 11: r = pow5(a); break;
    // the shared portable functions (include/rt_libm.h; RT_FLAG_SHARED_LIBM)
    case 12: r = rtlm_sin(a); break;
    case 13: r = rtlm_cos(a); break;
    case 14: r = rtlm_atan(a); break;
    case 15: r = rtlm_asin(a); break;
    case 16: r = rtlm_log(a); break;
    case 17: r = ghc_atan2<true>(a, b); break;
    default: r = tan(a); break;
  }
  out[i] = r;
}
// Ops 18 and 19: the sine and the cosine of the shading code's fused sincos (RT_FUSED_SINCOS), through the call
// the kernels make. A kernel of its own, and a template: only the unit that launches it (rt_render.hip) emits it,
// and the render units that leave the form off compile to the device code they had before.
template <int = 0>
__global__ void math_probe_sincos(int op, const double* x, int n, double* out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double2 sc = sincos_call(x[i]);
  out[i] = op == 18 ? sc.x : sc.y;
}

// The kernel instantiation of a KernelForm (rt_launch_plan.h; plan_launch makes only forms that exist).
// `V` carries the variant with F_WIDE and F_SKIP; the F_SKIP instantiations are the same kernels for an
// adaptive frame's launches (there is no counting build of those).
// by_waves<Ws...>(w, k): k(std::integral_constant<int, w>) for the w among Ws, the WAVES values the kernel
// is instantiated with; nullptr for any other.
template <int... Ws, class K>
const void* by_waves(int w, K k) {
  const void* fn = nullptr;
  (void)((w == Ws && (fn = k(std::integral_constant<int, Ws>{}), true)) || ...);
  return fn;
}
// The LDS-staged 4-wide kernels that sort packed keys (worlds within rt_wkey_fits: wide_keys_packed).
template <unsigned V>
const void* pick_packed(const rt::KernelForm& f) {
  static_assert((V & F_WIDE) != 0, "4-wide kernels only");
  // (1 wave: the leaves are read from global memory)
  if (f.leaf_lds)
    return by_waves<2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2_lds<V, W(), true, true>; });
  return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2_lds<V, W(), false, true>; });
}
template <unsigned V>
const void* pick_w(const rt::KernelForm& f) {
  if constexpr ((V & ~F_SKIP) == (kVarSpheres | F_WIDE)) {
    if (!f.lds && f.q)  // (the quantised tree and sphere quadruples from global memory)
      return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2<V | F_QNODE, W()>; });
  }
  // (the spheres-only variant's packed kernels are instantiated in a unit of their own, rt_k_spheres_packed.hip)
  if constexpr ((V & F_WIDE) != 0 && (V & ~F_SKIP) != (kVarSpheres | F_WIDE)) {
    if (f.lds && f.pk) return pick_packed<V>(f);
  }
  if constexpr ((V & F_WIDE) != 0) {
    if (f.lds && f.leaf_lds)
      return by_waves<2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2_lds<V, W(), true>; });
  }
  if (f.lds) return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2_lds<V, W()>; });
  return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2<V, W()>; });
}
template <unsigned V>
const void* pick(const rt::KernelForm& f) {
  if constexpr ((V & F_SKIP) == 0) {
    if (f.skip) return f.count ? nullptr : pick<V | F_SKIP>(f);
    if (f.count) {
      if constexpr (V == kVarSpheres) {
        if (f.loop == 2 && f.q) return (const void*)render_philox2<V | F_WIDE | F_COUNT | F_QNODE, 1>;
      }
      if (f.loop == 2) return (const void*)render_philox2<V | F_WIDE | F_COUNT, 1>;
      return f.loop ? (const void*)render_philox2<V | F_COUNT, 1> : (const void*)render_philox<V | F_COUNT, 1>;
    }
  }
  if (f.loop == 2) return pick_w<V | F_WIDE>(f);
  if (f.loop == 1) return pick_w<V>(f);
  if (f.lds) return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox_lds<V, W()>; });
  return by_waves<1, 2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox<V, W()>; });
}
// full variants (media, frames, textures, motion): ray replacement over the caller's tree in the
// reference's order (loop 1), or the per-sample loop (loop 0)
template <unsigned V>
const void* pick_full(const rt::KernelForm& f) {
  if constexpr ((V & F_SKIP) == 0) {
    if (f.skip) return f.count ? nullptr : pick_full<V | F_SKIP>(f);
    if (f.count)
      return f.loop ? (const void*)render_philox2<V | F_COUNT, 1> : (const void*)render_philox<V | F_COUNT, 1>;
  }
  if (f.loop) {
    if (f.lds) return by_waves<2, 3>(f.waves, [](auto W) { return (const void*)render_philox2_lds<V, W()>; });
    // (4: RTAMD_WAVES=4, A/B only)
    return by_waves<2, 3, 4>(f.waves, [](auto W) { return (const void*)render_philox2<V, W()>; });
  }
  return by_waves<1, 2>(f.waves, [](auto W) { return (const void*)render_philox<V, W()>; });
}

}  // namespace

// Render-kernel tables, one per kernel translation unit (KernelForm::unit and, for kUnitVariant, ::var).
namespace rt {
const void* philox_kernel_spheres(const KernelForm& f);
const void* philox_kernel_spheres_global(const KernelForm& f);  // rt_k_spheres_global.hip
const void* philox_kernel_spheres_packed(const KernelForm& f);  // rt_k_spheres_packed.hip
const void* philox_kernel_count_packed(const KernelForm& f);    // rt_k_count_packed.hip (kVarSpheres or kVarCornell)
const void* philox_kernel_cornell(const KernelForm& f);
const void* philox_kernel_full(const KernelForm& f);
const void* philox_kernel_full_dark(const KernelForm& f);
const void* features_kernel(const FeaturePlan& P);  // rt_k_features.hip (render_features / render_features_lds)
const void* features_chain_kernel(const FeaturePlan& P);  // rt_k_features_chain.hip (the same forms, with a chain)
const void* ids_kernel(const FeaturePlan& P);  // rt_k_ids.hip (the same forms: render_ids / render_ids_lds)
// The slab forms (rt_kernels_shard.h), one unit per pass: the same form table, the kernels taking FeatureSlabArgs.
const void* features_shard_kernel(const FeaturePlan& P);        // rt_k_features_shard.hip
const void* features_chain_shard_kernel(const FeaturePlan& P);  // rt_k_features_chain_shard.hip
const void* ids_shard_kernel(const FeaturePlan& P);             // rt_k_ids_shard.hip
// rt_k_features_shard.hip: the record merge queued on `stream` (G: shard 0's geometry); a hipError_t as int.
int assemble_records_launch(const rtd::SlabGeometry& G, const void* d_slabs, void* d_image, void* stream);
}  // namespace rt
