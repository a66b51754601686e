// rt_ids.cpp — the host half of the material-ID coverage buffers (include/rt.h): the fold over a list of sample
// ids, the rank resolve, and the host matte and preview, all over rt_ids.h's shared text. No HIP, no device: it
// builds for the CPU as is.
#include <algorithm>
#include <string>

#include "rt.h"
#include "rt_ids.h"
#include "rt_internal.h"

namespace {
int invalid(const char* what, const char* why) {
  rt::set_error(std::string(what) + ": " + why);
  return RT_E_INVALID;
}
}  // namespace

extern "C" int rt_ids_fold_host(rt_id_record* rec, const uint32_t* ids, int64_t n) {
  if (!rec || n < 0 || (n > 0 && !ids)) return invalid("rt_ids_fold_host", "needs a record, n >= 0 and n ids");
  rt_id_record r = *rec;
  for (int64_t i = 0; i < n; ++i) rt::ids_fold_one(r, ids[i]);
  *rec = r;
  return RT_OK;
}

extern "C" int rt_ids_resolve(const rt_id_record* recs, int64_t pixels, uint32_t* out_rank_ids, double* out_rank_cov,
                              double* out_other_cov) {
  if (!recs || pixels < 1) return invalid("rt_ids_resolve", "needs records and pixels >= 1");
  for (int64_t i = 0; i < pixels; ++i) {
    const rt_id_record& r = recs[i];
    int order[RT_ID_SLOTS];
    for (int k = 0; k < RT_ID_SLOTS; ++k) order[k] = k;
    // count descending, then id ascending; free slots (count 0) last, where their order does not show
    std::sort(order, order + RT_ID_SLOTS, [&](int a, int b) {
      return r.count[a] != r.count[b] ? r.count[a] > r.count[b] : r.id[a] < r.id[b];
    });
    const double n = (double)r.samples;
    for (int k = 0; k < RT_ID_SLOTS; ++k) {
      const int s = order[k];
      if (out_rank_ids) out_rank_ids[RT_ID_SLOTS * i + k] = r.count[s] ? r.id[s] : RT_ID_MISS;
      if (out_rank_cov) out_rank_cov[RT_ID_SLOTS * i + k] = r.samples ? (double)r.count[s] / n : 0.0;
    }
    if (out_other_cov) out_other_cov[i] = r.samples ? (double)r.other / n : 0.0;
  }
  return RT_OK;
}

extern "C" int rt_ids_matte_host(const rt_id_record* recs, int64_t pixels, const uint32_t* ids, int n_ids,
                                 double* out_cov, uint8_t* out_u8) {
  if (const char* bad = rt::ids_list_error(ids, n_ids)) return invalid("rt_ids_matte_host", bad);
  if (!recs || pixels < 1 || (!out_cov && !out_u8))
    return invalid("rt_ids_matte_host", "needs records, pixels >= 1 and an output");
  for (int64_t i = 0; i < pixels; ++i) {
    const double cov = rt::ids_matte_cov(recs[i], ids, n_ids);
    if (out_cov) out_cov[i] = cov;
    if (out_u8) out_u8[i] = rt::ids_byte(cov);
  }
  return RT_OK;
}

extern "C" int rt_ids_preview_host(const rt_id_record* recs, int64_t pixels, uint8_t* out_rgb8) {
  if (!recs || pixels < 1 || !out_rgb8) return invalid("rt_ids_preview_host", "needs records, pixels >= 1 and an output");
  for (int64_t i = 0; i < pixels; ++i) rt::ids_preview_px(recs[i], out_rgb8 + 3 * i);
  return RT_OK;
}
