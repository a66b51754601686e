// features_plan_check.cpp — the host-only launch decision of a feature pass (rt_launch_plan.cpp plan_features, with
// and without a specular chain) as a stand-alone program, for a CPU build under AddressSanitizer + UBSan
// (tests/test_features_chain_sanitize.py compiles and runs it). No HIP, no GPU: hand-made world shapes over every
// walk form, every knob the decision reads, frame sizes from 1x1 to the 32-bit pixel-id bound.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "rt_launch_plan.h"
#include "rt_layout.h"

static int failures = 0;
#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);        \
      ++failures;                                                     \
    }                                                                 \
  } while (0)

static rt_render_params params(int w, int h, unsigned flags = 0) {
  rt_render_params p;
  std::memset(&p, 0, sizeof p);
  p.width = w, p.height = h, p.spp = 1, p.max_depth = 1, p.rng_mode = RT_RNG_PHILOX, p.flags = flags;
  return p;
}

int main() {
  using namespace rt;
  WorldShape spheres;  // a spheres-only world with a 4-wide tree (the book-one cover's counts)
  spheres.features = 0, spheres.n_nodes = 971, spheres.n_wnodes = 213, spheres.n_leaves = 486;
  spheres.stack_need = 12, spheres.wide_stack_need = 17, spheres.has_wide = true, spheres.rebuilt_bvh = true;
  spheres.replace_ok = true, spheres.cu_count = 256;
  WorldShape mixed = spheres;  // frames and media: the mixed walk
  mixed.features = rtd::F_ALL, mixed.mixed_wide = true;
  WorldShape deep = mixed;  // frames nested too deep: the recursive walk
  deep.replace_ok = false, deep.has_wide = false, deep.mixed_wide = false;
  const int sizes[][2] = {{1, 1}, {37, 21}, {1200, 800}, {65535, 65536}};
  for (const WorldShape* W : {&spheres, &mixed, &deep}) {
    for (const auto& wh : sizes) {
      for (int waves = 0; waves <= 4; ++waves) {
        for (int mask = 0; mask < 16; ++mask) {
          LaunchKnobs K;
          K.waves = waves, K.waves_set = waves != 0;
          K.lds = mask & 1, K.leaf_lds = (mask & 2) != 0, K.packed_keys = (mask & 4) != 0, K.wide = (mask & 8) ? 0 : -1;
          for (unsigned flags : {0u, (unsigned)RT_FLAG_REFERENCE_CULL}) {
            const rt_render_params p = params(wh[0], wh[1], flags);
            FeaturePlan a, b;
            CHECK(plan_features(*W, p, K, a, false) == RT_OK);
            CHECK(plan_features(*W, p, K, b, true) == RT_OK);
            // a chain pass takes the first-hit pass's form; staged and unforced it runs at 3 waves instead of 4
            CHECK(a.walk == b.walk && a.pk == b.pk && a.leaf_stop == b.leaf_stop && a.entries == b.entries);
            CHECK(a.info.work_items == b.info.work_items && a.info.variant == b.info.variant);
            if (b.lds && waves == 0) {
              CHECK(b.info.waves == 3 && b.info.block == 768 && (!a.lds || a.info.waves == 4));
            } else if (a.lds == b.lds) {
              CHECK(std::memcmp(&a.info, &b.info, sizeof a.info) == 0);
            }
            CHECK(b.info.dyn_lds_bytes >= 0 && (size_t)b.info.dyn_lds_bytes <= kLdsBudget);
            CHECK(b.info.grid >= 1 && b.info.block >= 64 && b.info.block <= 1024);
            if (b.lds) {
              const size_t want = (size_t)W->n_wnodes * sizeof(rt_wnode) + (size_t)b.n_leaves * sizeof(rt_node) +
                                  (size_t)b.entries * b.info.block * sizeof(int);
              CHECK((size_t)b.info.dyn_lds_bytes == want);
            }
          }
        }
      }
    }
  }
  FeaturePlan P;
  CHECK(plan_features(spheres, params(65536, 65536), LaunchKnobs{}, P, true) == RT_E_INVALID);
  std::printf("features_plan_check: %s (%d failures)\n", failures ? "FAILED" : "clean", failures);
  return failures != 0;
}
