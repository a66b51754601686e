// rt_denoise.h — the feature-guided denoiser's per-pixel text (include/rt.h, rt_denoise*): the guide set-up, the
// tap weight, one iteration of a pixel and the finish, written once for the device (rt_denoise_kernels.h) and the
// host (rt_denoise_host, rt_denoise.cpp), so that both give the same bits; and scaleColor for both. No HIP
// includes: it builds for the CPU as is.
#pragma once
#include <math.h>

#include <initializer_list>

#include "rt.h"
#include "rt_error.h"

#ifdef __HIPCC__
#define RT_DENOISE_HD __host__ __device__
#define RT_DENOISE_UNROLL _Pragma("unroll")
#else
#define RT_DENOISE_HD
#define RT_DENOISE_UNROLL
#endif

namespace rt {

// scaleColor (Lib.hs:287-288) of a linear channel: NaN -> 0, +inf -> 255. The bytes of rt_features_resolve's albedo
// and of a denoised image, on the host and on the device.
RT_DENOISE_HD inline uint8_t scale_color8(double x) {
  const double s = sqrt(x);
  const double cl = s < 0.0 ? 0.0 : (s > 0.999 ? 0.999 : s);
  const double f = floor(256 * cl);
  return f == f ? (uint8_t)(int)f : (uint8_t)0;
}

// What an iteration reads of a call's parameters: the flags, the sigmas and rn = 1 / (sigma_normal * sigma_normal),
// which the host computes once (denoise_const) and hands to the device as a value.
struct DenoiseConst {
  unsigned flags;
  int W, H;
  double n;  // (double)feature_samples
  double sigma_color, color_floor, sigma_depth, rn;
};

// A pixel's records: guide g = {N_x, N_y, N_z, Z}, and cv = {r, g, b, V}, 4 doubles each.
enum { kDenoiseRec = 4 };

RT_DENOISE_HD inline bool denoise_valid(const double* c) {
  return error_finite(c[0]) && error_finite(c[1]) && error_finite(c[2]);
}
RT_DENOISE_HD inline double denoise_luma(const double* c) { return (0.2126 * c[0] + 0.7152 * c[1]) + 0.0722 * c[2]; }
RT_DENOISE_HD inline double denoise_falloff(double x) { return x < 1.0 ? (1.0 - x) * (1.0 - x) : 0.0; }
// The B3 spline's taps k[|d|]
RT_DENOISE_HD inline double denoise_b3(int d) { return d == 0 ? 0.375 : (d == 1 || d == -1) ? 0.25 : 0.0625; }
// a_c of rt.h: the albedo a colour is divided by and multiplied back with
RT_DENOISE_HD inline double denoise_albedo(double sum, double n) {
  const double a = sum / n;
  return a > 1e-3 ? (a < 1.0 ? a : 1.0) : 1e-3;
}

// The guide record and the first (colour, V) record of a pixel from its colour, its se (may be null) and its
// feature sums f[8].
RT_DENOISE_HD inline void denoise_prepare(const DenoiseConst& K, const double* color, const double* se, const double* f,
                                          double g[4], double cv[4]) {
  for (int c = 0; c < 3; ++c) g[c] = f[RT_FEAT_NORMAL + c] / K.n;
  const double hits = f[RT_FEAT_HITS];
  g[3] = hits == 0.0 ? 0.0 : f[RT_FEAT_DEPTH] / hits;
  const bool demod = (K.flags & RT_DENOISE_DEMODULATE) && denoise_valid(color);
  double a[3] = {1.0, 1.0, 1.0};
  if (demod)
    for (int c = 0; c < 3; ++c) a[c] = denoise_albedo(f[RT_FEAT_ALBEDO + c], K.n);
  for (int c = 0; c < 3; ++c) cv[c] = demod ? color[c] / a[c] : color[c];
  double v = 0.0;
  if (se && error_finite(se[0]) && error_finite(se[1]) && error_finite(se[2])) {
    // (the standard errors of what the filter sees: of the demodulated channels when it demodulates)
    const double e0 = demod ? se[0] / a[0] : se[0], e1 = demod ? se[1] / a[1] : se[1], e2 = demod ? se[2] / a[2] : se[2];
    const double t0 = 0.2126 * e0, t1 = 0.7152 * e1, t2 = 0.0722 * e2;
    v = (t0 * t0 + t1 * t1) + t2 * t2;
    if (!error_finite(v)) v = 0.0;
  }
  cv[3] = v;
}

// One iteration of the pixel whose records are gp and cp: out[4] = its next (colour, V). tap(dx, dy, gq, cq) fills
// the records of the tap at (dx, dy) strides from the centre and returns false when it lies outside the image; the
// taps are asked for in rt.h's order, which is the order of the sums.
template <class Tap>
RT_DENOISE_HD inline void denoise_iterate(const DenoiseConst& K, const double gp[4], const double cp[4], Tap&& tap,
                                          double out[4]) {
  for (int c = 0; c < 4; ++c) out[c] = cp[c];
  const bool valid = denoise_valid(cp);
  if (!valid && !(K.flags & RT_DENOISE_FILL)) return;
  const bool use_c = valid && !(K.flags & RT_DENOISE_GUIDES_ONLY);
  const double rz = 1.0 / (K.sigma_depth * gp[3] + 1e-12);
  const double rc = use_c ? 1.0 / (K.sigma_color * sqrt(cp[3]) + K.color_floor) : 0.0;
  const double lp = use_c ? denoise_luma(cp) : 0.0;
  double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, wsum = 0.0, vacc = 0.0;
  RT_DENOISE_UNROLL
  for (int dy = -2; dy <= 2; ++dy) {
    RT_DENOISE_UNROLL
    for (int dx = -2; dx <= 2; ++dx) {
      double gq[4], cq[4];
      if (!tap(dx, dy, gq, cq) || !denoise_valid(cq)) continue;
      const double h = denoise_b3(dx) * denoise_b3(dy);
      const double ex = gp[0] - gq[0], ey = gp[1] - gq[1], ez = gp[2] - gq[2];
      const double wn = denoise_falloff(((ex * ex + ey * ey) + ez * ez) * K.rn);
      const double wz = denoise_falloff(fabs(gp[3] - gq[3]) * rz);
      const double wc = use_c ? denoise_falloff(fabs(lp - denoise_luma(cq)) * rc) : 1.0;
      const double w = ((h * wn) * wz) * wc;
      acc0 += w * cq[0];
      acc1 += w * cq[1];
      acc2 += w * cq[2];
      wsum += w;
      vacc += (w * w) * cq[3];
    }
  }
  if (!(wsum > 0.0)) return;
  out[0] = acc0 / wsum;
  out[1] = acc1 / wsum;
  out[2] = acc2 / wsum;
  out[3] = vacc / (wsum * wsum);
}

// The output colour of a pixel from its last (colour, V) record and its feature sums: a valid pixel's albedo is
// multiplied back under RT_DENOISE_DEMODULATE, every other pixel is copied.
RT_DENOISE_HD inline void denoise_finish(const DenoiseConst& K, const double cv[4], const double* f, double out[3]) {
  const bool remod = (K.flags & RT_DENOISE_DEMODULATE) && denoise_valid(cv);
  for (int c = 0; c < 3; ++c) out[c] = remod ? cv[c] * denoise_albedo(f[RT_FEAT_ALBEDO + c], K.n) : cv[c];
}

// A caller's parameters, checked as rt.h states (null: invalid): the message of what is wrong, or null.
inline const char* denoise_params_error(const rt_denoise_params* p) {
  if (!p) return "null params";
  if (p->width < 1 || p->height < 1) return "width and height must be positive";
  if ((long long)p->width * p->height >= (1ll << 31)) return "an image of 2^31 pixels or more";
  if (p->iterations < 1 || p->iterations > RT_DENOISE_MAX_ITERATIONS) return "iterations must be in 1..8";
  if (p->feature_samples < 1) return "feature_samples must be >= 1";
  if (p->flags & ~(RT_DENOISE_DEMODULATE | RT_DENOISE_GUIDES_ONLY | RT_DENOISE_FILL)) return "unknown flag bits";
  for (double s : {p->sigma_color, p->color_floor, p->sigma_normal, p->sigma_depth})
    if (!(s > 0.0) || !error_finite(s)) return "sigma_color, color_floor, sigma_normal and sigma_depth must be > 0 and finite";
  return nullptr;
}

// The iteration kernel's tile (rt_denoise_kernels.h): a workgroup owns kDenoiseTileW x kDenoiseTileH pixels of one
// residue class and stages their taps' eight values in LDS planes of (kDenoiseTileH + 4) rows, kDenoisePitch apart.
enum {
  kDenoiseTileW = 32,
  kDenoiseTileH = 8,
  kDenoisePitch = kDenoiseTileW + 4,
  kDenoiseLdsBytes = 8 * kDenoisePitch * (kDenoiseTileH + 4) * 8
};

// The device buffers a denoise call works in, all for W*H pixels: the guide records and the two (colour, V)
// buffers, 32 bytes per pixel each, and three 64-bit counts {invalid_in, invalid_out, filled}.
struct DenoiseBuffers {
  void* guide;
  void* a;
  void* b;
  unsigned long long* counts;
};

// rt_k_denoise.hip: zeroes the counts and queues prepare, `iterations` iteration launches and finish on `stream`
// (a hipStream_t) over device pointers in image order (d_se and d_out_rgb8 may be null). Returns the hipError_t of
// the first call that failed (0: all queued) and the kernels queued in *launches.
int denoise_launch(const DenoiseConst& K, int iterations, const double* d_color, const double* d_se,
                   const double* d_feature_sums, const DenoiseBuffers& B, double* d_out_color, uint8_t* d_out_rgb8,
                   void* stream, int* launches);

inline DenoiseConst denoise_const(const rt_denoise_params& p) {
  DenoiseConst K{};
  K.flags = p.flags;
  K.W = p.width, K.H = p.height;
  K.n = (double)p.feature_samples;
  K.sigma_color = p.sigma_color, K.color_floor = p.color_floor, K.sigma_depth = p.sigma_depth;
  K.rn = 1.0 / (p.sigma_normal * p.sigma_normal);
  return K;
}

}  // namespace rt
