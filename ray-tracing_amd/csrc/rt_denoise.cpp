// rt_denoise.cpp — the host half of the feature-guided denoiser (include/rt.h): rt_denoise_host, the definition
// the device path is compared with and the offline filter of a checkpoint's preview, by the per-pixel text the
// kernels compile (rt_denoise.h). No HIP, no device: it builds for the CPU as is.
#include <string>
#include <vector>

#include "rt.h"
#include "rt_denoise.h"
#include "rt_internal.h"

extern "C" int rt_internal_denoise_host(const rt_denoise_params* params, const double* color, const double* se,
                                        const double* feature_sums, double* out_color, uint8_t* out_rgb8,
                                        rt_denoise_stats* stats, double* out_variance) {
  const char* bad = rt::denoise_params_error(params);
  if (!bad && (!color || !feature_sums || !out_color)) bad = "null color, feature_sums or out_color";
  if (bad) {
    rt::set_error(std::string("rt_denoise_host: ") + bad);
    return RT_E_INVALID;
  }
  const rt::DenoiseConst K = rt::denoise_const(*params);
  const int W = K.W, H = K.H;
  const size_t npx = (size_t)W * (size_t)H;
  std::vector<double> guide(4 * npx), a(4 * npx), b(4 * npx);
  for (size_t i = 0; i < npx; ++i)
    rt::denoise_prepare(K, color + 3 * i, se ? se + 3 * i : nullptr, feature_sums + RT_FEATURE_DOUBLES * i,
                        &guide[4 * i], &a[4 * i]);
  double *src = a.data(), *dst = b.data();
  for (int it = 0; it < params->iterations; ++it) {
    const long long s = 1ll << it;
    for (int y = 0; y < H; ++y)
      for (int x = 0; x < W; ++x) {
        const size_t i = (size_t)y * W + x;
        auto tap = [&](int dx, int dy, double gq[4], double cq[4]) {
          const long long qx = x + s * dx, qy = y + s * dy;
          if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
          const size_t q = (size_t)qy * W + (size_t)qx;
          for (int c = 0; c < 4; ++c) gq[c] = guide[4 * q + c], cq[c] = src[4 * q + c];
          return true;
        };
        rt::denoise_iterate(K, &guide[4 * i], src + 4 * i, tap, dst + 4 * i);
      }
    std::swap(src, dst);
  }
  rt_denoise_stats st{};
  st.pixels = (int64_t)npx;
  for (size_t i = 0; i < npx; ++i) {
    const bool was = rt::denoise_valid(color + 3 * i);
    double o[3];
    rt::denoise_finish(K, src + 4 * i, feature_sums + RT_FEATURE_DOUBLES * i, o);
    for (int c = 0; c < 3; ++c) {
      out_color[3 * i + c] = o[c];
      if (out_rgb8) out_rgb8[3 * i + c] = rt::scale_color8(o[c]);
    }
    if (out_variance) out_variance[i] = src[4 * i + 3];
    const bool is = rt::denoise_valid(o);
    st.invalid_in += !was;
    st.invalid_out += !is;
    st.filled += !was && is;
  }
  if (stats) *stats = st;
  return RT_OK;
}

extern "C" int rt_denoise_host(const rt_denoise_params* params, const double* color, const double* se,
                               const double* feature_sums, double* out_color, uint8_t* out_rgb8,
                               rt_denoise_stats* stats) {
  return rt_internal_denoise_host(params, color, se, feature_sums, out_color, out_rgb8, stats, nullptr);
}
