// rt_features.cpp — the host half of the first-hit feature buffers (include/rt.h): the guide images from a
// feature pass's sums. No HIP, no device: it builds for the CPU as is.
#include <cmath>
#include <limits>

#include "rt.h"
#include "rt_internal.h"

namespace {
// scaleColor (Lib.hs:287-288) as the device's scale_color (rt_kernels.h): NaN -> 0, +inf -> 255.
uint8_t scale_color(double x) {
  const double s = std::sqrt(x);
  const double cl = s < 0.0 ? 0.0 : (s > 0.999 ? 0.999 : s);
  const double f = std::floor(256 * cl);
  return f == f ? (uint8_t)(int)f : (uint8_t)0;
}
}  // namespace

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
      if (out_albedo_rgb8) out_albedo_rgb8[3 * i + c] = scale_color(a);
      if (out_normal) out_normal[3 * i + c] = s[RT_FEAT_NORMAL + c] / n;
    }
    const double hits = s[RT_FEAT_HITS];
    if (out_depth) out_depth[i] = hits == 0.0 ? std::numeric_limits<double>::infinity() : s[RT_FEAT_DEPTH] / hits;
    if (out_coverage) out_coverage[i] = hits / n;
  }
  return RT_OK;
}
