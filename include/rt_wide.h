// rt_wide.h — the device's 4-wide BVH record (internal; shared by the host builder in rt_bvh.cpp
// and the traversal in rt_trace.h). Not part of the C ABI: rt_upload_scene derives it from the
// flattened world tree when the world holds no ConstantMedium and no instance frames.
//
// One record is 128 bytes = one LDS/L2 line pair: four child boxes as single-precision rows
// (lo[axis][child], hi[axis][child]), rounded OUTWARD from the fp64 boxes so that each box
// contains the double-precision one, then four child references. The fp32 test over these boxes
// only culls (it accepts every ray the fp64 slab test over the same boxes accepts, see
// wide_keys2 in rt_trace.h); every leaf is still hit-tested in fp64 exactly as the reference.
#pragma once
#include <stdint.h>

#define RT_WIDE 4

typedef struct rt_wnode {
  float lo[3][RT_WIDE];
  float hi[3][RT_WIDE];
  int32_t child[RT_WIDE];  // >= 0: wide node id; < 0: leaf, ~child = flat rt_node id (an unused
                           // slot: empty box lo = +inf, hi = -inf over a leaf of this node)
  int32_t pad[RT_WIDE];
} rt_wnode;

// The same node with its child boxes quantised to 8 bits per plane against a per-node grid (64 bytes:
// half an L2 line; the kernels that read the tree from global memory, where the 100k-sphere world's
// nodes and leaves do not fit an XCD's L2). Per axis a, plane q of child k is origin[a] + q * scale[a]
// exactly in fp32: scale is a power of two and origin an integer multiple of it below 2^23 * scale, so
// the decoded boxes are fp32 planes containing the node's fp32 boxes (lo rounded down, hi up to the grid)
// and the fp32 test over them culls conservatively, as over rt_wnode's. qlo[a] / qhi[a] hold child k's
// lower / upper plane in byte k. An unused slot has qlo 255 and qhi 0 on every axis (an empty box) and
// refers to a leaf of this node, as in rt_wnode.
typedef struct rt_qnode {
  float origin[3];
  float scale[3];
  uint32_t qlo[3];
  uint32_t qhi[3];
  int32_t child[RT_WIDE];
} rt_qnode;

// ---- packed sort keys (the 4-wide walk's wide_node<F, true>, rt_trace.h)
// A child's sort key and its reference in one 32-bit word: the fp32 key's top 32 - RT_WKEY_BITS bits (sign,
// 8 exponent and 9 mantissa bits) over the reference's low RT_WKEY_BITS bits, so that four words sort with
// integer min / max alone and no child id travels beside its key. The words are compared as SIGNED ints: an
// accepted key is a non-negative float below +inf (its bit pattern orders as an integer; -0.0, which only the
// rays the fp32 test cannot describe produce, is the most negative word and sorts first, as the zero it is), a
// rejected key is +inf exactly, whose word 0x7f800000 | ref lies above every accepted one. The truncation
// only changes the order among children whose entry distances agree to 2^-9 relative; equal truncated keys
// fall back to the reference's bits, which is deterministic. The walk's result does not depend on the order.
// A reference is a wide node id >= 0 or ~leaf slot < 0: both survive the sign-extending unpack while
// -2^(BITS-1) <= ref < 2^(BITS-1), i.e. for trees of at most RT_WKEY_MAX_IDS wide nodes and as many leaf slots
// (rt_wkey_fits; the host takes the unpacked form otherwise). An LDS-staged tree always fits: 160 KiB hold
// fewer than 1280 wide nodes of 128 bytes, and a tree of n wide nodes has at most 4 n leaf slots (< 5120).
#define RT_WKEY_BITS 14
#define RT_WKEY_MASK ((1u << RT_WKEY_BITS) - 1u)
#define RT_WKEY_MAX_IDS (1 << (RT_WKEY_BITS - 1))
#define RT_WKEY_REJECTED 0x7f800000u  /* +inf: the key of a child whose box the ray misses */

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RT_WKEY_FN __host__ __device__ static inline
#else
#define RT_WKEY_FN static inline
#endif

RT_WKEY_FN int rt_wkey_fits(long long n_wide_nodes, long long n_leaf_slots) {
  return n_wide_nodes <= RT_WKEY_MAX_IDS && n_leaf_slots <= RT_WKEY_MAX_IDS;
}
// (key_bits: the fp32 key's bit pattern)
RT_WKEY_FN int32_t rt_wkey_pack(uint32_t key_bits, int32_t ref) {
  return (int32_t)((key_bits & ~RT_WKEY_MASK) | ((uint32_t)ref & RT_WKEY_MASK));
}
RT_WKEY_FN int32_t rt_wkey_ref(int32_t word) {
  const uint32_t low = (uint32_t)word & RT_WKEY_MASK;  // sign-extend the low RT_WKEY_BITS bits
  return (int32_t)(low ^ (1u << (RT_WKEY_BITS - 1))) - (1 << (RT_WKEY_BITS - 1));
}

// ---- the stack cull (the packed form's stack holds the sorted words, not the unpacked references: rt_trace.h,
// wide_node<F, true> pushes them, trav_pop<true> unpacks one, wide_leaf<F, true> culls)
// A stacked child was accepted under the bound that held when its node was visited. Once a leaf is hit the
// bound (Trav::tmax32) shrinks, and an entry whose box the ray enters beyond the new bound can be dropped from
// the stack before it costs a wide step or an fp64 leaf test. The word's key is bits(word & ~RT_WKEY_MASK)
// read as a float; the entry is beyond the bound exactly when
//     key * (1 - 2^-21) > fma(tmax32, 1 + 2^-21, slack)
// — wide_keys2's acceptance (rt_trace.h) with near = key and far = tmax32, negated, the same expression with
// the same roundings. No new proof is needed:
//   - the truncated key is <= the true near distance n the word was packed from (truncating the low mantissa
//     bits of a non-negative float lowers it or leaves it; the accepted key min(n, 3.0e38) is <= n; -0.0 stays);
//   - fp32 multiplication by a positive constant and the fma (in its first argument, under a positive factor)
//     are monotone, roundings included;
//   - a re-test of the child now would use far = min(far planes, tmax32) <= tmax32;
//   - so "beyond" implies n * (1 - 2^-21) > fma(far, 1 + 2^-21, slack): wide_keys2 itself would reject that
//     child under the current bound;
//   - and a box wide_keys2 rejects holds no hit in [tmin, closest_up], a tie at `closest` included, since
//     tmax32 = f32_upper(closest) >= closest_up.
// Special cases: tmax32 = +inf (no hit yet) never culls (the right side is +inf, or NaN with slack = -inf);
// slack = +inf (the rays the fp32 test cannot describe, the only ones with -0.0 keys) never culls (the right
// side is +inf); the -0.0 word is beyond no bound of tmax32 >= 0 and slack >= 0 either; slack = -inf (NaN rays)
// has nothing stacked, every child being rejected; tmax32 = 0 after a rect hit at t = NaN leaves `slack` alone
// as the bound and culls as the box test would, which rejects the same children. A NaN bound culls nothing.
RT_WKEY_FN int rt_wkey_beyond(int32_t word, float tmax32, float slack) {
  const uint32_t kb = (uint32_t)word & ~RT_WKEY_MASK;
  float key;
  __builtin_memcpy(&key, &kb, sizeof key);  // (the bit pattern as a float, in C and on the device alike)
  return key * (1.0f - 0x1p-21f) > __builtin_fmaf(tmax32, 1.0f + 0x1p-21f, slack);
}

// ---- the lean step loop's lane state (the sphere-only packed kernels' walk_until and wide_leaf, rt_trace.h)
// A lane of the 4-wide walk with one postponed leaf is described by Trav's node, pend and sp alone, and the step
// loop reads its predicates off those registers where it uses them instead of carrying a flag per lane:
//   walking: the walk is not over — a node is left to visit, or a parked leaf to test;
//   seeking: the slot is free and the lane is at a wide node — it needs wide steps before it can test a leaf;
//   holding: a leaf is parked — a leaf step tests it.
// The loop makes progress because every walking lane is seeking or holding: the pops never leave a lane at a leaf
// with the slot free (trav_postpone parks it), where neither kind of step would move it and its wave would spin.
// tests/c/walk_step_check.c proves that over every state a step can leave.
#define RT_WNONE ((int32_t)0x80000000) /* Trav::node once nothing is left to visit (kNone, rt_trace.h) */

RT_WKEY_FN int rt_wlane_walking(int32_t node, int32_t pend) { return (node != RT_WNONE) | (pend >= 0); }
RT_WKEY_FN int rt_wlane_seeking(int32_t node, int32_t pend) { return (pend < 0) & (node >= 0); }
RT_WKEY_FN int rt_wlane_holding(int32_t pend) { return pend >= 0; }

typedef struct rt_wstep {
  int32_t node, pend, sp;  // the lane's Trav::node, Trav::pend (a leaf slot, or -1: free) and Trav::sp
} rt_wstep;

// The slot of the lane's stack that holds its top entry, or slot 0 of an empty stack (always allocated; what it
// holds is then ignored): a top-of-stack read needs no branch on sp, and its address is formed from the live
// stack base (written as stk[(sp - 1) * stride] under `sp != 0`, the compiler hoists the loop-invariant
// stk - stride out of the walk loop and spills it).
RT_WKEY_FN int32_t rt_wstep_slot(int32_t sp) { return sp > 0 ? sp - 1 : 0; }

// trav_postpone (rt_trace.h) as selects, for the end of a leaf step: a lane at a leaf with the slot free parks the
// leaf and goes on with the top entry (`word`, read from slot rt_wstep_slot(sp) by every lane), or with RT_WNONE
// from an empty stack. The entry taken stays the node whatever it is: the slot is busy now.
RT_WKEY_FN rt_wstep rt_wstep_postpone(int32_t node, int32_t pend, int32_t sp, int32_t word) {
  const int park = (node < 0) & (node != RT_WNONE) & (pend < 0);
  const int has = sp > 0;
  rt_wstep s;
  s.node = park ? (has ? rt_wkey_ref(word) : RT_WNONE) : node;
  s.pend = park ? ~node : pend;
  s.sp = sp - (park & has);
  return s;
}

#ifdef __cplusplus
static_assert(sizeof(rt_wnode) == 128, "rt_wnode is 128 bytes");
static_assert(sizeof(rt_qnode) == 64, "rt_qnode is 64 bytes");
#endif
