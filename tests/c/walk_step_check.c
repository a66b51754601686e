/* The lean step loop of the packed 4-wide walk (walk_until / wide_leaf of the sphere-only packed kernels, rt_trace.h)
 * rests on host-and-device inlines of include/rt_wide.h: the lane predicates rt_wlane_walking / _seeking / _holding,
 * the branch-free top-of-stack slot rt_wstep_slot and the leaf step's postpone as selects, rt_wstep_postpone. A
 * stand-alone check of them against the walk's steps, which are restated here from rt_trace.h (wide_node's three
 * stores and its sp and node update, trav_pop, trav_postpone, the stack cull's sweep):
 *
 *   1. The progress invariant, exhaustively: after a wide step from every input (0..4 accepted children, every
 *      leaf / wide pattern of the four sorted references, the slot free and busy, sp 0..3, stacked entries of both
 *      kinds below sp) and after a leaf step's postpone from every state, a lane that rt_wlane_walking reports is
 *      rt_wlane_seeking or rt_wlane_holding. The loop steps only such lanes: a walking lane that is neither would
 *      never advance and its wave would spin, so this is proved here and not found on a GPU. A lane that is not
 *      walking is neither (it is never stepped again), and no lane is both.
 *   2. rt_wstep_postpone leaves the lane state trav_postpone leaves (node, pend, sp; the stack is not written),
 *      exhaustively over the same states, reading its word from slot rt_wstep_slot(sp), which is always a slot of
 *      the lane's stack.
 *   3. The sweep in its branch-free form (top word read from rt_wstep_slot(sp) before sp is tested) stops at the
 *      same sp as `while (sp && rt_wkey_beyond(stk[sp - 1], ...)) --sp`, over random stacks and bounds.
 *   4. Random walks: long chains of wide and leaf steps with deeper stacks, the select forms against the branch
 *      forms after every step, the invariant after every step, and the walk over exactly when the loop's exit
 *      test says so. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rt_wide.h"

#define DEPTH 64

static long failures = 0;
static void fail(const char* what, int a, int b, int c, int d) {
  if (failures < 10) printf("FAIL %s (%d %d %d %d)\n", what, a, b, c, d);
  ++failures;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void) { /* xorshift64* */
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}

static uint32_t fbits(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}
static float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

typedef struct lane {
  int32_t node, pend, sp;
  int32_t stk[DEPTH + 3];
} lane;

/* ---- the walk's steps as rt_trace.h has them (wide_inner<F, true>, trav_pop<true>, trav_postpone<true>) */
static int32_t pop(lane* t) { return t->sp ? rt_wkey_ref(t->stk[--t->sp]) : RT_WNONE; }
static void postpone(lane* t) {
  if (t->node < 0 && t->node != RT_WNONE && t->pend < 0) {
    t->pend = ~t->node;
    t->node = pop(t);
  }
}
static void wide_step(lane* t, int n_hit, const int32_t p[4]) {
  const int32_t e0 = n_hit > 3 ? p[3] : (n_hit > 2 ? p[2] : p[1]);
  const int32_t e1 = n_hit > 3 ? p[2] : p[1];
  t->stk[t->sp] = e0;
  t->stk[t->sp + 1] = e1;
  t->stk[t->sp + 2] = p[1];
  t->sp += n_hit > 1 ? n_hit - 1 : 0;
  t->node = rt_wkey_ref(p[0]);
  if (n_hit == 0) t->node = pop(t);
  postpone(t);
}
static void sweep(lane* t, float tmax32, float slack) {
  while (t->sp && rt_wkey_beyond(t->stk[t->sp - 1], tmax32, slack)) --t->sp;
}

/* ---- the lean kernels' forms (wide_leaf<F, true> under kLeanWalk) */
static int32_t slot_checked(int32_t sp) {
  const int32_t s = rt_wstep_slot(sp);
  if (s < 0 || s >= DEPTH + 3 || (sp > 0 && s != sp - 1) || (sp <= 0 && s != 0)) fail("slot", sp, s, 0, 0);
  return s;
}
static void lean_postpone(lane* t) {
  const rt_wstep s = rt_wstep_postpone(t->node, t->pend, t->sp, t->stk[slot_checked(t->sp)]);
  t->node = s.node;
  t->pend = s.pend;
  t->sp = s.sp;
}
static void lean_sweep(lane* t, float tmax32, float slack) {
  for (;;) {
    const int32_t top = slot_checked(t->sp);
    const int32_t word = t->stk[top];
    if (!((t->sp > 0) & (rt_wkey_beyond(word, tmax32, slack) != 0))) break;
    t->sp = top;
  }
}

static int same_lane(const lane* a, const lane* b) {
  if (a->node != b->node || a->pend != b->pend || a->sp != b->sp) return 0;
  for (int i = 0; i < a->sp; ++i)
    if (a->stk[i] != b->stk[i]) return 0;
  return 1;
}
/* the invariant the step loop rests on */
static int lane_ok(const lane* t) {
  const int walking = rt_wlane_walking(t->node, t->pend);
  const int seeking = rt_wlane_seeking(t->node, t->pend), holding = rt_wlane_holding(t->pend);
  if (seeking && holding) return 0;
  if (walking) return seeking || holding;
  return !seeking && !holding;
}

/* the four sorted words of a node: accepted keys ascending, rejected ones +inf; bit i of `kinds`: child i a leaf */
static void make_words(int n_hit, int kinds, int base, int32_t p[4]) {
  for (int i = 0; i < 4; ++i) {
    const int32_t ref = (kinds >> i & 1) ? ~(int32_t)(base + 20 + i) : (int32_t)(base + 10 + i);
    const float key = i < n_hit ? 1.0f + 0.25f * (float)i : INFINITY;
    p[i] = rt_wkey_pack(fbits(key), ref);
  }
  for (int i = 0; i + 1 < n_hit; ++i) /* (the accepted ones in the network's order: signed words ascending) */
    if (p[i] > p[i + 1]) fail("test words unsorted", n_hit, kinds, i, 0);
}
static void fill_below(lane* t, int sp, int below) { /* bit i of `below`: entry i a leaf */
  for (int i = 0; i < DEPTH + 3; ++i) t->stk[i] = rt_wkey_pack(fbits(9.0f), 4000 + i); /* dead slots */
  for (int i = 0; i < sp; ++i)
    t->stk[i] = rt_wkey_pack(fbits(0.5f + (float)i), (below >> i & 1) ? ~(int32_t)(300 + i) : 200 + i);
  t->sp = sp;
}

static long steps = 0, stuck_candidates = 0;

static void exhaustive(void) {
  for (int n_hit = 0; n_hit <= 4; ++n_hit)
    for (int kinds = 0; kinds < 16; ++kinds)
      for (int busy = 0; busy < 2; ++busy)
        for (int sp = 0; sp <= 3; ++sp)
          for (int below = 0; below < (1 << sp); ++below) {
            lane a;
            memset(&a, 0, sizeof a);
            fill_below(&a, sp, below);
            a.pend = busy ? 77 : -1;
            a.node = 5; /* the wide node being visited */
            if (!lane_ok(&a)) fail("a lane at a wide node is not steppable", busy, sp, 0, 0);
            int32_t p[4];
            make_words(n_hit, kinds, 100, p);
            wide_step(&a, n_hit, p);
            ++steps;
            if (!lane_ok(&a)) fail("wide step leaves a stuck lane", n_hit, kinds, busy, sp * 16 + below);
            /* (the step did meet the case the invariant is about: a leaf became the node while the slot was free) */
            stuck_candidates += a.pend >= 0 && !busy;
          }
  /* the leaf step's end: node wide / leaf / none, slot free / busy, sp 0..3, both kinds below */
  for (int kind = 0; kind < 3; ++kind)
    for (int busy = 0; busy < 2; ++busy)
      for (int sp = 0; sp <= 3; ++sp)
        for (int below = 0; below < (1 << sp); ++below) {
          lane a;
          memset(&a, 0, sizeof a);
          fill_below(&a, sp, below);
          a.pend = busy ? 77 : -1;
          a.node = kind == 0 ? 5 : (kind == 1 ? ~(int32_t)6 : RT_WNONE);
          lane b = a;
          postpone(&a);
          lean_postpone(&b);
          ++steps;
          if (!same_lane(&a, &b)) fail("postpone differs", kind, busy, sp, below);
          /* (a leaf step frees the slot before the postpone: a leaf as the node with the slot busy is a state
           * before a leaf step, steppable as holding, and the postpone leaves it alone) */
          if (!lane_ok(&b)) fail("postpone leaves a stuck lane", kind, busy, sp, below);
        }
}

static void sweeps(void) {
  for (long i = 0; i < 400000; ++i) {
    lane a;
    memset(&a, 0, sizeof a);
    const int sp = (int)(rnd() % 9u);
    const float base = float_of(rnd() & 0x7fffffffu);
    for (int k = 0; k < sp; ++k) {
      float key = (rnd() & 1u) ? float_of(rnd() & 0x7f7fffffu) : base * (0.5f + 0.25f * (float)(rnd() % 5u));
      if (!(key == key)) key = 1.0f;
      a.stk[k] = rt_wkey_pack(fbits(key), (int32_t)(rnd() % 8000u) - 4000);
    }
    a.sp = sp;
    lane b = a;
    float tmax32 = (rnd() & 3u) ? base : float_of(rnd() & 0x7fffffffu);
    if (rnd() % 16u == 0) tmax32 = INFINITY;
    const float slack = (rnd() % 16u == 0) ? INFINITY : ((rnd() & 1u) ? 0.0f : base * 0x1p-20f);
    sweep(&a, tmax32, slack);
    lean_sweep(&b, tmax32, slack);
    ++steps;
    if (a.sp != b.sp) fail("sweep differs", sp, a.sp, b.sp, 0);
  }
}

static void random_walks(void) {
  for (int walk = 0; walk < 20000; ++walk) {
    lane a;
    memset(&a, 0, sizeof a);
    a.node = 0, a.pend = -1, a.sp = 0; /* trav_begin */
    lane b = a;
    int step = 0;
    for (; step < 400; ++step) {
      if (!same_lane(&a, &b)) {
        fail("random walk diverged", walk, step, a.node, b.node);
        break;
      }
      if (!lane_ok(&b)) {
        fail("random walk stuck", walk, step, b.node, b.pend);
        break;
      }
      if (!rt_wlane_walking(b.node, b.pend)) break; /* over: the loop's exit test */
      const int can_wide = b.node >= 0, can_leaf = rt_wlane_holding(b.pend);
      if (can_wide && (!can_leaf || (rnd() & 3u))) { /* (a wide step runs every lane at a wide node) */
        int n_hit = (int)(rnd() % 5u);
        if (b.sp + 3 > DEPTH) n_hit = 0;
        int32_t p[4];
        make_words(n_hit, (int)(rnd() & 15u), 100 + 8 * (step & 255), p);
        wide_step(&a, n_hit, p);
        wide_step(&b, n_hit, p);
      } else { /* a leaf step: the parked leaf is tested, the cull may drop entries, then the postpone */
        a.pend = b.pend = -1;
        if (rnd() % 4u == 0) {
          const float tmax32 = 0.25f * (float)(rnd() % 12u);
          sweep(&a, tmax32, 0.0f);
          lean_sweep(&b, tmax32, 0.0f);
        }
        postpone(&a);
        lean_postpone(&b);
      }
      ++steps;
    }
    if (step == 400 && b.sp == 0 && b.node == RT_WNONE && b.pend < 0 && rt_wlane_walking(b.node, b.pend))
      fail("a finished walk still walks", walk, 0, 0, 0);
  }
}

int main(void) {
  exhaustive();
  sweeps();
  random_walks();
  if (stuck_candidates == 0) ++failures; /* (the parking case is exercised) */
  printf("walk_step_check: %ld steps, %ld of them parked a leaf\n", steps, stuck_candidates);
  printf("walk_step_check: %s (%ld failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
