/* The stack cull of the 4-wide walk's packed form (rt_wkey_beyond, include/rt_wide.h): a stand-alone check that the
 * cull never drops an entry the box test would still accept.
 *   - whenever rt_wkey_beyond(rt_wkey_pack(bits(n), ref), tmax32, slack) is true, a restatement of wide_keys2's
 *     acceptance (rt_trace.h) with near = n and far = min(f, tmax32) rejects, for every far-plane distance f;
 *   - beyond is false for tmax32 = +inf, for slack = +inf and for the -0.0 word.
 * n ranges over what a stacked key can be: a non-negative float (wide_keys2 clamps an accepted key to 3.0e38; the
 * unclamped n is tried as well) or -0.0. A negative n only arises with tmin32 <= 0, which set_ray32 answers with
 * slack = +inf: those are tried under that slack alone. Built without FMA contraction (ISO C mode), so that
 * the roundings are the device's (-ffp-contract=off there). */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "rt_wide.h"

static uint32_t bits_of(float f) {
  uint32_t u;
  memcpy(&u, &f, sizeof u);
  return u;
}
static float float_of(uint32_t u) {
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(void) {  /* xorshift64* */
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return (uint32_t)((rng_state * 0x2545f4914f6cdd1dull) >> 32);
}
static int32_t rnd_ref(void) { return (int32_t)(rnd() % (2u * RT_WKEY_MAX_IDS)) - RT_WKEY_MAX_IDS; }
static float rnd_nonneg(void) {  /* any non-negative float, +inf included, no NaN */
  for (;;) {
    const float f = float_of(rnd() & 0x7fffffffu);
    if (f == f) return f;
  }
}
/* a few ulps, or a few units of the truncated field, either way from x (x >= 0 stays >= 0, no NaN) */
static float nudge(float x) {
  const uint32_t b = bits_of(x);
  const uint32_t step = (rnd() & 1u) ? rnd() % 5u : (rnd() % 5u) << RT_WKEY_BITS;
  const uint32_t c = (rnd() & 1u) ? b + step : (b >= step ? b - step : 0u);
  const float y = float_of(c & 0x7fffffffu);
  return y == y ? y : x;
}

/* wide_keys2's acceptance of one child: near n, far planes' minimum f, the walk's bound and slack */
static int box_accepts(float n, float f, float tmax32, float slack) {
  const float far = fminf(f, tmax32);
  return n * (1.0f - 0x1p-21f) <= fmaf(far, 1.0f + 0x1p-21f, slack);
}

static long failures = 0, culled = 0, rejected = 0, tried = 0;

static void check(float n, float f, float tmax32, float slack) {
  const int32_t ref = rnd_ref();
  const float keys[2] = {n, fminf(n, 3.0e38f)};
  for (int k = 0; k < 2; ++k) {
    const int32_t w = rt_wkey_pack(bits_of(keys[k]), ref);
    const int beyond = rt_wkey_beyond(w, tmax32, slack);
    const int accepts = box_accepts(n, f, tmax32, slack);
    ++tried;
    culled += beyond;
    rejected += !accepts;
    if (beyond && accepts) {
      if (failures < 10) printf("culled an accepted child: n %a f %a tmax32 %a slack %a\n", n, f, tmax32, slack);
      ++failures;
    }
    if (beyond && (tmax32 == INFINITY || slack == INFINITY)) {
      if (failures < 10) printf("culled under an infinite bound: n %a tmax32 %a slack %a\n", n, tmax32, slack);
      ++failures;
    }
    if (rt_wkey_ref(w) != ref) ++failures;
  }
}

int main(void) {
  /* adversarial values: zeros, subnormals, the smallest normal, values the truncation changes (low mantissa bits
   * set) next to ones it keeps, the clamp, the largest float, +inf */
  const float pos[] = {0.0f, 1.4e-45f, 3.0e-42f, 1.1754942e-38f, 1.17549435e-38f, 1.0e-30f, 1.0e-4f, 0.9999999f,
                       1.0f, 1.0000001f, 1.0009765625f, 1.0019531f, 1.001953125f, 1.9999999f, 2.0f, 7.25f, 1000.5f,
                       1.0e30f, 3.0e38f, 3.4028235e38f, INFINITY};
  const int np = (int)(sizeof pos / sizeof pos[0]);
  const float slacks[] = {0.0f, 1.4e-45f, 1.0e-12f, 9.5e-7f, 1.0e-3f, 1.0f, 1.0e30f, INFINITY, -INFINITY};
  const int ns = (int)(sizeof slacks / sizeof slacks[0]);
  for (int i = 0; i < np; ++i)      /* n (and -0.0 below) */
    for (int j = 0; j < 2 * np + 1; ++j) {  /* f: both signs, and NaN (fminf drops it) */
      const float f = j == 2 * np ? NAN : (j < np ? pos[j] : -pos[j - np]);
      for (int k = 0; k < 2 * np; ++k) {  /* tmax32: both signs (a caller's bound may be anything) */
        const float tmax32 = k < np ? pos[k] : -pos[k - np];
        for (int s = 0; s < ns; ++s) {
          check(pos[i], f, tmax32, slacks[s]);
          if (i == 0) check(-0.0f, f, tmax32, slacks[s]);
        }
      }
    }
  /* random tuples; half of them with f, tmax32 and slack within ulps (or units of the truncated field) of n */
  for (long i = 0; i < 3000000; ++i) {
    const float n = (i % 64 == 0) ? pos[rnd() % (uint32_t)np] : rnd_nonneg();
    float f = rnd_nonneg(), tmax32 = rnd_nonneg(), slack = rnd_nonneg();
    if (i & 1) {
      f = (rnd() & 3u) ? nudge(n) : f;
      tmax32 = (rnd() & 3u) ? nudge(n) : tmax32;
      slack = (rnd() & 1u) ? nudge(n) * 0x1p-20f : ((rnd() & 1u) ? 0.0f : slack);
    }
    if (rnd() % 16u == 0) f = -f;
    if (rnd() % 64u == 0) slack = (rnd() & 1u) ? INFINITY : -INFINITY;
    if (rnd() % 64u == 0) tmax32 = INFINITY;
    check(n, f, tmax32, slack);
  }
  /* never beyond: no hit yet, an undescribed ray, the -0.0 word (under any bound a walk can hold: tmax32 >= 0,
   * slack >= 0 or +inf), and a negative key, which only undescribed rays (slack = +inf) can stack */
  for (long i = 0; i < 1000000; ++i) {
    const float n = rnd_nonneg(), tmax32 = rnd_nonneg(), slack = rnd_nonneg();
    const int32_t ref = rnd_ref();
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(n), ref), INFINITY, slack)) ++failures;
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(n), ref), INFINITY, -INFINITY)) ++failures;
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(n), ref), tmax32, INFINITY)) ++failures;
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(-n), ref), tmax32, INFINITY)) ++failures;
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(-0.0f), ref), tmax32, slack)) ++failures;
    if (rt_wkey_beyond(rt_wkey_pack(bits_of(-0.0f), ref), 0.0f, 0.0f)) ++failures;
  }
  /* the cull does cull: a key well beyond a finite bound, and one the truncation brings down to the bound */
  if (!rt_wkey_beyond(rt_wkey_pack(bits_of(2.0f), 5), 1.0f, 1.0e-6f)) ++failures;
  if (!rt_wkey_beyond(rt_wkey_pack(bits_of(1.0e-3f), ~7), 0.0f, 0.0f)) ++failures;
  if (rt_wkey_beyond(rt_wkey_pack(bits_of(1.0019f), 5), 1.001f, 0.0f)) ++failures; /* (truncated to 1.0: kept) */
  if (culled == 0 || rejected <= culled) ++failures;  /* (the cull is exercised, and is the weaker test) */
  printf("pop_cull_check: %ld tuples, %ld rejected by the box test, %ld of them culled from the stack\n", tried, rejected,
         culled);
  printf("pop_cull_check: %s (%ld failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
