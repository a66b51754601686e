// rt_features.cpp — the host half of the first-hit feature buffers (include/rt.h): the guide images from a
// feature pass's sums, and the merge of the shards' record slabs. No HIP, no device: it builds for the CPU as is.
#include <cmath>
#include <limits>

#include "rt.h"
#include "rt_denoise.h"  // (scale_color8: scaleColor, shared with the denoiser's outputs)
#include "rt_internal.h"
#include "rt_layout.h"  // (the record slab's block map: rt_assemble_records_host)

// The record merge on the host (rt.h): every slot of every shard's slab through the slab's block map, the padding
// slots never touched.
extern "C" int rt_assemble_records_host(const rt_render_params* p, const void* slabs, void* image) {
  if (!p || !slabs || !image) {
    rt::set_error("rt_assemble_records_host: null argument");
    return RT_E_INVALID;
  }
  if (const char* bad = rtd::slab_params_error(p)) {
    rt::set_error(std::string("rt_assemble_records_host: ") + bad);
    return RT_E_INVALID;
  }
  rtd::SlabGeometry G = rtd::slab_geometry(p);
  struct Rec {
    unsigned char b[64];
  };
  const Rec* src = static_cast<const Rec*>(slabs);
  Rec* dst = static_cast<Rec*>(image);
  for (int shard = 0; shard < G.shard_count; ++shard) {
    G.shard_rank = shard;
    for (long long slot = 0; slot < G.slab; ++slot) {
      const long long pixel = rtd::slab_slot_pixel(G, (uint32_t)slot);
      if (pixel >= 0) dst[pixel] = src[(long long)shard * G.slab + slot];
    }
  }
  return RT_OK;
}

extern "C" int rt_features_resolve(const double* sums, int64_t pixels, int n_samples, double* out_albedo,
                                   double* out_normal, double* out_depth, double* out_coverage,
                                   uint8_t* out_albedo_rgb8) {
  if (!sums || pixels < 1 || n_samples < 1) {
    rt::set_error("rt_features_resolve: needs sums, pixels >= 1 and n_samples >= 1");
    return RT_E_INVALID;
  }
  const double n = (double)n_samples;
  for (int64_t i = 0; i < pixels; ++i) {
    const double* s = sums + RT_FEATURE_DOUBLES * i;
    for (int c = 0; c < 3; ++c) {
      const double a = s[RT_FEAT_ALBEDO + c] / n;
      if (out_albedo) out_albedo[3 * i + c] = a;
      if (out_albedo_rgb8) out_albedo_rgb8[3 * i + c] = rt::scale_color8(a);
      if (out_normal) out_normal[3 * i + c] = s[RT_FEAT_NORMAL + c] / n;
    }
    const double hits = s[RT_FEAT_HITS];
    if (out_depth) out_depth[i] = hits == 0.0 ? std::numeric_limits<double>::infinity() : s[RT_FEAT_DEPTH] / hits;
    if (out_coverage) out_coverage[i] = hits / n;
  }
  return RT_OK;
}
