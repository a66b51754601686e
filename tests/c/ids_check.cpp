// ids_check.cpp — the host half of the material-ID coverage buffers (rt_ids.h's shared fold, matte and preview text
// through rt_ids.cpp's entry points, and the launch decision an id pass shares with a chain pass) as a stand-alone
// program, for a CPU build under AddressSanitizer + UBSan (tests/test_ids_sanitize.py compiles and runs it). No
// HIP, no GPU: streams of ids from a small generator, arrays sized exactly to what each call may touch.
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt.h"
#include "rt_ids.h"
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

static uint32_t lcg(uint32_t& s) { return s = s * 1664525u + 1013904223u; }

// rt.h's fold, restated the plain way
static void fold_plain(rt_id_record& r, uint32_t x) {
  if (r.samples == 0xFFFFFFFFu) return;
  ++r.samples;
  for (int k = 0; k < RT_ID_SLOTS; ++k)
    if (r.count[k] && r.id[k] == x) {
      ++r.count[k];
      return;
    }
  for (int k = 0; k < RT_ID_SLOTS; ++k)
    if (!r.count[k]) {
      r.id[k] = x, r.count[k] = 1;
      return;
    }
  ++r.other;
}

int main() {
  static_assert(sizeof(rt_id_record) == 64, "rt.h");
  uint32_t seed = 12345u;
  const int pixels = 777;
  std::vector<rt_id_record> recs(pixels);
  std::memset(recs.data(), 0, sizeof(rt_id_record) * pixels);
  for (int i = 0; i < pixels; ++i) {
    const int distinct = 1 + (int)(lcg(seed) >> 16) % 12, n = (int)(lcg(seed) >> 16) % 90;
    std::vector<uint32_t> ids(n);
    for (int k = 0; k < n; ++k) {
      const uint32_t v = (lcg(seed) >> 16) % (uint32_t)distinct;
      ids[k] = v == 0 ? RT_ID_MISS : v * 37u;
    }
    rt_id_record want;
    std::memset(&want, 0, sizeof want);
    for (uint32_t x : ids) fold_plain(want, x);
    const int cut = n ? (int)(lcg(seed) >> 16) % (n + 1) : 0;  // in two parts: the record carries the state
    CHECK(rt_ids_fold_host(&recs[i], ids.data(), cut) == RT_OK);
    CHECK(rt_ids_fold_host(&recs[i], ids.data() + cut, n - cut) == RT_OK);
    CHECK(std::memcmp(&recs[i], &want, sizeof want) == 0);
  }
  rt_id_record full;
  std::memset(&full, 0, sizeof full);
  full.id[0] = 5, full.count[0] = 0xFFFFFFFEu, full.samples = 0xFFFFFFFEu;
  const uint32_t three[3] = {5, 6, 7};
  CHECK(rt_ids_fold_host(&full, three, 3) == RT_OK);
  CHECK(full.count[0] == 0xFFFFFFFFu && full.samples == 0xFFFFFFFFu && full.count[1] == 0 && full.other == 0);
  CHECK(rt_ids_fold_host(nullptr, three, 3) == RT_E_INVALID && rt_ids_fold_host(&full, nullptr, 1) == RT_E_INVALID);

  // resolve: exactly sized outputs, each alone and together
  std::vector<uint32_t> rank_ids((size_t)pixels * RT_ID_SLOTS);
  std::vector<double> rank_cov((size_t)pixels * RT_ID_SLOTS), other_cov(pixels);
  CHECK(rt_ids_resolve(recs.data(), pixels, rank_ids.data(), rank_cov.data(), other_cov.data()) == RT_OK);
  CHECK(rt_ids_resolve(recs.data(), pixels, rank_ids.data(), nullptr, nullptr) == RT_OK);
  CHECK(rt_ids_resolve(recs.data(), pixels, nullptr, rank_cov.data(), nullptr) == RT_OK);
  CHECK(rt_ids_resolve(recs.data(), pixels, nullptr, nullptr, other_cov.data()) == RT_OK);
  CHECK(rt_ids_resolve(recs.data(), 0, nullptr, nullptr, nullptr) == RT_E_INVALID);
  for (int i = 0; i < pixels; ++i) {
    double sum = other_cov[i];
    for (int k = 0; k < RT_ID_SLOTS; ++k) {
      sum += rank_cov[(size_t)i * RT_ID_SLOTS + k];
      if (k) CHECK(rank_cov[(size_t)i * RT_ID_SLOTS + k] <= rank_cov[(size_t)i * RT_ID_SLOTS + k - 1]);
    }
    CHECK(recs[i].samples ? (sum > 1.0 - 1e-12 && sum < 1.0 + 1e-12) : sum == 0.0);
  }

  // mattes: lists of 1, 3 and RT_ID_MATTE_MAX ids, the last one's end at the array's end
  std::vector<double> cov(pixels);
  std::vector<uint8_t> u8(pixels);
  std::vector<uint32_t> list(RT_ID_MATTE_MAX);
  for (int k = 0; k < RT_ID_MATTE_MAX; ++k) list[k] = (uint32_t)k * 37u;
  list[RT_ID_MATTE_MAX - 1] = RT_ID_MISS;
  for (int n_ids : {1, 3, RT_ID_MATTE_MAX}) {
    const uint32_t* l = list.data() + (RT_ID_MATTE_MAX - n_ids);
    CHECK(rt_ids_matte_host(recs.data(), pixels, l, n_ids, cov.data(), u8.data()) == RT_OK);
    CHECK(rt_ids_matte_host(recs.data(), pixels, l, n_ids, nullptr, u8.data()) == RT_OK);
    CHECK(rt_ids_matte_host(recs.data(), pixels, l, n_ids, cov.data(), nullptr) == RT_OK);
    for (int i = 0; i < pixels; ++i) {
      CHECK(cov[i] >= 0.0 && cov[i] <= 1.0 && u8[i] == (uint8_t)(cov[i] * 255.0 + 0.5));
      if (n_ids == RT_ID_MATTE_MAX && recs[i].samples) CHECK(cov[i] + other_cov[i] > 1.0 - 1e-12);  // (every id is listed)
    }
  }
  CHECK(rt_ids_matte_host(recs.data(), pixels, list.data(), 0, cov.data(), u8.data()) == RT_E_INVALID);
  CHECK(rt_ids_matte_host(recs.data(), pixels, list.data(), RT_ID_MATTE_MAX + 1, cov.data(), u8.data()) == RT_E_INVALID);
  const uint32_t unsorted[3] = {4, 4, 9};
  CHECK(rt_ids_matte_host(recs.data(), pixels, unsorted, 3, cov.data(), u8.data()) == RT_E_INVALID);
  CHECK(rt_ids_matte_host(recs.data(), pixels, list.data(), 1, nullptr, nullptr) == RT_E_INVALID);

  // preview: 3 bytes per pixel; the per-pixel text once more directly, on the saturated record too
  std::vector<uint8_t> rgb((size_t)pixels * 3);
  CHECK(rt_ids_preview_host(recs.data(), pixels, rgb.data()) == RT_OK);
  for (int i = 0; i < pixels; ++i) {
    uint8_t px[3];
    rt::ids_preview_px(recs[i], px);
    CHECK(std::memcmp(px, &rgb[(size_t)i * 3], 3) == 0);
  }
  uint8_t px[3];
  rt::ids_preview_px(full, px);
  CHECK(rt::ids_fmix32(0u) == 0u && rt::ids_fmix32(1u) == 0x514E28B7u);
  CHECK(rt::ids_byte(0.0) == 0 && rt::ids_byte(1.0) == 255 && rt::ids_byte(1e300) == 255);

  // the plan: an id pass launches with the chain pass's plan (rt_launch_plan.cpp plan_features, chain = true)
  using namespace rt;
  WorldShape spheres;
  spheres.features = 0, spheres.n_nodes = 971, spheres.n_wnodes = 213, spheres.n_leaves = 486;
  spheres.stack_need = 12, spheres.wide_stack_need = 17, spheres.has_wide = true, spheres.rebuilt_bvh = true;
  spheres.replace_ok = true, spheres.cu_count = 256;
  WorldShape mixed = spheres;
  mixed.features = rtd::F_ALL, mixed.mixed_wide = true;
  for (const WorldShape* W : {&spheres, &mixed}) {
    for (int waves = 0; waves <= 4; ++waves) {
      rt_render_params p;
      std::memset(&p, 0, sizeof p);
      p.width = 37, p.height = 21, p.spp = 1, p.max_depth = 1, p.rng_mode = RT_RNG_PHILOX;
      LaunchKnobs K;
      K.waves = waves, K.waves_set = waves != 0;
      FeaturePlan P;
      CHECK(plan_features(*W, p, K, P, true) == RT_OK);
      CHECK(P.info.work_items == 5 * 3 && P.info.block <= 1024 && (size_t)P.info.dyn_lds_bytes <= kLdsBudget);
      if (W == &spheres && P.lds) CHECK(P.info.waves == (waves ? waves : 3));
    }
  }
  std::printf("ids_check: %s (%d failures)\n", failures ? "FAILED" : "clean", failures);
  return failures != 0;
}
