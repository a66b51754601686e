// rt_ids.h — the material-ID coverage buffers' per-sample and per-pixel text (include/rt.h, rt_render_ids and
// rt_ids_*): the fold of one sample id into a record, the matte coverage, the preview colour and the byte of a
// coverage, written once for the device (rt_kernels.h ids_loop, rt_k_ids.hip) and the host (rt_ids.cpp), so that
// both give the same bits. No HIP includes: it builds for the CPU as is.
#pragma once
#include <stdint.h>

#include "rt.h"

#ifdef __HIPCC__
#define RT_IDS_HD __host__ __device__
#define RT_IDS_UNROLL _Pragma("unroll")
#else
#define RT_IDS_HD
#define RT_IDS_UNROLL
#endif

namespace rt {

// One sample id folded into a record by rt.h's rule. Every slot is compared and updated under a predicate, the
// loops unroll, and no slot is addressed by a run-time index: on the device the record stays in 16 registers.
// `open`: the saturation guard (a record at UINT32_MAX samples is left as it is).
RT_IDS_HD inline void ids_fold_one(rt_id_record& r, uint32_t x) {
  const bool open = r.samples != 0xFFFFFFFFu;
  bool placed = !open;
  RT_IDS_UNROLL
  for (int k = 0; k < RT_ID_SLOTS; ++k) {  // a used slot that holds the id
    const bool m = !placed && r.count[k] != 0u && r.id[k] == x;
    r.count[k] += m ? 1u : 0u;
    placed |= m;
  }
  RT_IDS_UNROLL
  for (int k = 0; k < RT_ID_SLOTS; ++k) {  // else the first free slot
    const bool t = !placed && r.count[k] == 0u;
    r.id[k] = t ? x : r.id[k];
    r.count[k] = t ? 1u : r.count[k];
    placed |= t;
  }
  r.other += placed ? 0u : 1u;
  r.samples += open ? 1u : 0u;
}

// MurmurHash3's 32-bit finaliser (Appleby, public domain)
RT_IDS_HD inline uint32_t ids_fmix32(uint32_t h) {
  h ^= h >> 16;
  h *= 0x85ebca6bu;
  h ^= h >> 13;
  h *= 0xc2b2ae35u;
  h ^= h >> 16;
  return h;
}

// Channel c of an id's preview colour
RT_IDS_HD inline double ids_colour(uint32_t id, int c) {
  return id == RT_ID_MISS ? 0.0 : (double)((ids_fmix32(id) >> (8 * c)) & 255u) / 255.0;
}

// The byte of a coverage or of a preview channel: (uint8_t)(v * 255.0 + 0.5). (The bound only keeps the conversion
// defined for a record whose counts exceed its samples; a folded record never reaches it.)
RT_IDS_HD inline uint8_t ids_byte(double v) {
  const double b = v * 255.0 + 0.5;
  return (uint8_t)(int)(b < 255.5 ? b : 255.5);
}

// Is x in the strictly ascending list ids[0..n)? (bisection)
RT_IDS_HD inline bool ids_listed(const uint32_t* ids, int n, uint32_t x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && ids[lo] == x;
}

// A pixel's matte coverage: the counts of the used slots whose id is listed, summed as integers, over samples.
RT_IDS_HD inline double ids_matte_cov(const rt_id_record& r, const uint32_t* ids, int n) {
  uint64_t sum = 0;
  RT_IDS_UNROLL
  for (int k = 0; k < RT_ID_SLOTS; ++k)
    if (r.count[k] != 0u && ids_listed(ids, n, r.id[k])) sum += r.count[k];
  return r.samples ? (double)sum / (double)r.samples : 0.0;
}

// A pixel's preview bytes
RT_IDS_HD inline void ids_preview_px(const rt_id_record& r, uint8_t out[3]) {
  double acc[3] = {0.0, 0.0, 0.0};
  RT_IDS_UNROLL
  for (int k = 0; k < RT_ID_SLOTS; ++k) {
    const double cov = r.samples ? (double)r.count[k] / (double)r.samples : 0.0;
    for (int c = 0; c < 3; ++c) acc[c] = acc[c] + cov * ids_colour(r.id[k], c);
  }
  for (int c = 0; c < 3; ++c) out[c] = ids_byte(acc[c]);
}

// A matte's id list, checked as rt.h states: the message of what is wrong, or null.
inline const char* ids_list_error(const uint32_t* ids, int n_ids) {
  if (!ids) return "null id list";
  if (n_ids < 1 || n_ids > RT_ID_MATTE_MAX) return "n_ids must be in 1..RT_ID_MATTE_MAX";
  for (int i = 1; i < n_ids; ++i)
    if (ids[i - 1] >= ids[i]) return "the id list must be strictly ascending";
  return nullptr;
}

// rt_k_ids.hip: the matte and the preview kernels over device pointers on `stream` (a hipStream_t), one thread per
// pixel; d_ids: the list on the device. Either matte output may be null. Return the hipError_t of the launch.
int ids_matte_launch(const rt_id_record* d_recs, long long pixels, const uint32_t* d_ids, int n_ids, double* d_out_cov,
                     uint8_t* d_out_u8, void* stream);
int ids_preview_launch(const rt_id_record* d_recs, long long pixels, uint8_t* d_out_rgb8, void* stream);

}  // namespace rt
