// rt_error.h — a pixel's error estimate from its running sums S and second moments Q (include/rt.h,
// RT_FRAME_MOMENTS): one text for the device (frame_error, rt_kernels.h) and the host
// (rt_error_estimate, rt_frame_error.cpp), so that both give the same bits; and the stop rule of adaptive
// frames over them (adapt_pixel: frame_adapt on the device, rt_adapt_decide on the host). No HIP includes:
// it builds for the CPU as is.
#pragma once
#include <math.h>

#include "rt.h"

#ifdef __HIPCC__
#define RT_ERROR_HD __host__ __device__
#else
#define RT_ERROR_HD
#endif

namespace rt {

// What pixel_error says of a pixel.
enum { kPixelConverged = 0, kPixelUnconverged = 1, kPixelNonFinite = 2 };

// (neither NaN nor infinite; a comparison, so that no fast-math setting can fold it)
RT_ERROR_HD inline bool error_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

// se[c] = sqrt(((Q_c - S_c^2 / N) / (K - 1)) / N) in rt.h's operation order, K = chunks >= 2, N = samples;
// the pixel's class under (abs_tol, rel_tol).
RT_ERROR_HD inline int pixel_error(const double* s, const double* q, int chunks, int samples, double abs_tol,
                                   double rel_tol, double se[3]) {
  const double n = (double)samples, k1 = (double)(chunks - 1);
  bool finite = true, converged = true;
  for (int c = 0; c < 3; ++c) {
    const double t = (s[c] * s[c]) / n;
    double d = q[c] - t;
    if (d < 0.0) d = 0.0;
    se[c] = sqrt((d / k1) / n);
    finite = finite && error_finite(se[c]);
    converged = converged && se[c] <= abs_tol + rel_tol * fabs(s[c] / n);
  }
  return !finite ? kPixelNonFinite : converged ? kPixelConverged : kPixelUnconverged;
}

// What adapt_pixel says of an active pixel (include/rt.h, adaptive frames).
enum { kAdaptKeep = 0, kAdaptStopNan = 1, kAdaptStopConverged = 2 };

// The stop rule of rt_frame_adapt and rt_adapt_decide for one active pixel after `chunks` chunks and
// `samples` samples: with RT_ADAPT_NAN a running sum with a NaN channel stops; otherwise, with
// RT_ADAPT_CONVERGED and chunks >= max(2, min_chunks), a pixel that pixel_error calls converged stops (NaN
// and infinite sums are non-finite there, so they never stop by this branch). `q` is read only under
// RT_ADAPT_CONVERGED.
RT_ERROR_HD inline int adapt_pixel(const double* s, const double* q, int chunks, int samples, unsigned flags,
                                   double abs_tol, double rel_tol, int min_chunks) {
  if ((flags & RT_ADAPT_NAN) && (s[0] != s[0] || s[1] != s[1] || s[2] != s[2])) return kAdaptStopNan;
  if ((flags & RT_ADAPT_CONVERGED) && chunks >= 2 && chunks >= min_chunks) {
    double se[3];
    if (pixel_error(s, q, chunks, samples, abs_tol, rel_tol, se) == kPixelConverged) return kAdaptStopConverged;
  }
  return kAdaptKeep;
}

// A caller's rule, checked as rt.h states: flags 0 or unknown bits, a negative or NaN tolerance, and
// min_chunks < 2 under RT_ADAPT_CONVERGED are invalid.
inline bool adapt_rule_ok(const rt_adapt_rule* r) {
  if (!r || r->flags == 0u || (r->flags & ~(RT_ADAPT_NAN | RT_ADAPT_CONVERGED))) return false;
  if (!(r->abs_tol >= 0.0) || !(r->rel_tol >= 0.0)) return false;
  return !(r->flags & RT_ADAPT_CONVERGED) || r->min_chunks >= 2;
}

// A caller's tolerance (NULL: {0, 0}) as two values; false when one is negative or NaN.
inline bool error_tol(const rt_error_tol* tol, double& abs_tol, double& rel_tol) {
  abs_tol = tol ? tol->abs_tol : 0.0;
  rel_tol = tol ? tol->rel_tol : 0.0;
  return abs_tol >= 0.0 && rel_tol >= 0.0;
}

}  // namespace rt
