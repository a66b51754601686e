/* The packed sort keys of the 4-wide walk (include/rt_wide.h): a stand-alone check of the pack / unpack
 * helpers the device code shares with the host.
 *   - every child reference of the admitted range survives pack -> unpack under every key;
 *   - words of keys a < b never order b before a once the reference bits are cleared, and order a strictly
 *     first whenever the truncated keys differ, whatever the references;
 *   - a rejected child's word (+inf) lies above every accepted one; -0.0 sorts first.
 * Words are compared as signed ints, as the walk's min / max do. */
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
/* an accepted key: a non-negative float up to wide_keys2's clamp 3.0e38f, any exponent */
static float rnd_key(void) {
  for (;;) {
    const float f = float_of(rnd() & 0x7fffffffu);
    if (f == f && f <= 3.0e38f) return f;
  }
}

int main(void) {
  long failures = 0;
  const int32_t lo = -RT_WKEY_MAX_IDS, hi = RT_WKEY_MAX_IDS - 1;
  /* the key patterns every reference is packed under: zeros, the smallest subnormal and normal, 1, the clamp,
   * all ones in the kept bits, +inf (a rejected child) */
  const float keys[] = {0.0f, -0.0f, 1.4e-45f, 1.17549435e-38f, 1.0f, 1.0009765625f, 3.0e38f, INFINITY};
  for (size_t k = 0; k < sizeof keys / sizeof keys[0]; ++k) {
    for (int32_t ref = lo; ref <= hi; ++ref) {
      const int32_t w = rt_wkey_pack(bits_of(keys[k]), ref);
      if (rt_wkey_ref(w) != ref) ++failures;
      if (((uint32_t)w & ~RT_WKEY_MASK) != (bits_of(keys[k]) & ~RT_WKEY_MASK)) ++failures;
    }
  }
  /* a wide node id is at most RT_WKEY_MAX_IDS - 1 and a leaf ~slot at least -RT_WKEY_MAX_IDS */
  if (!rt_wkey_fits(RT_WKEY_MAX_IDS, RT_WKEY_MAX_IDS) || rt_wkey_fits(RT_WKEY_MAX_IDS + 1, 1) ||
      rt_wkey_fits(1, RT_WKEY_MAX_IDS + 1))
    ++failures;
  if (rt_wkey_ref(rt_wkey_pack(bits_of(1.0f), ~(RT_WKEY_MAX_IDS - 1))) != ~(RT_WKEY_MAX_IDS - 1)) ++failures;

  const int32_t rej_min = rt_wkey_pack(RT_WKEY_REJECTED, 0) & (int32_t)~RT_WKEY_MASK;  /* the lowest rejected word */
  for (long i = 0; i < 2000000; ++i) {
    float a = rnd_key(), b = rnd_key();
    if (i % 4 == 0) b = float_of(bits_of(a) + (rnd() % (4u << RT_WKEY_BITS)));  /* near-equal keys */
    if (!(b == b) || b > 3.0e38f) continue;
    if (b < a) {
      const float t = a;
      a = b;
      b = t;
    }
    const int32_t ra = rnd_ref(), rb = rnd_ref();
    const int32_t wa = rt_wkey_pack(bits_of(a), ra), wb = rt_wkey_pack(bits_of(b), rb);
    const int32_t ta = wa & (int32_t)~RT_WKEY_MASK, tb = wb & (int32_t)~RT_WKEY_MASK;
    if (a < b && tb < ta) ++failures;             /* never b before a */
    if (ta != tb && !(wa < wb)) ++failures;       /* distinct truncated keys: the references do not matter */
    if (ta == tb && ra != rb && wa == wb) ++failures;  /* equal truncated keys: the references break the tie */
    if (!(wa < rej_min) || !(wb < rej_min)) ++failures;
    if (!(wa < rt_wkey_pack(RT_WKEY_REJECTED, rnd_ref()))) ++failures;
    /* -0.0 (only rays the fp32 test cannot describe produce it) is accepted and sorts ahead of everything */
    if (!(rt_wkey_pack(bits_of(-0.0f), ra) < wb) && bits_of(b) != bits_of(-0.0f)) ++failures;
  }
  printf("packed_keys_check: %s (%ld failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
