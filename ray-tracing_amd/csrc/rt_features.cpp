// rt_features.cpp — the host half of the first-hit feature buffers (include/rt.h): the guide images from a
// feature pass's sums. No HIP, no device: it builds for the CPU as is.
#include <cmath>
#include <limits>

#include "rt.h"
#include "rt_denoise.h"  // (scale_color8: scaleColor, shared with the denoiser's outputs)
#include "rt_internal.h"

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
