// rt_error.h — a pixel's error estimate from its running sums S and second moments Q (include/rt.h,
// RT_FRAME_MOMENTS): one text for the device (frame_error, rt_kernels.h) and the host
// (rt_error_estimate, rt_frame_error.cpp), so that both give the same bits. No HIP includes: it builds
// for the CPU as is.
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

// A caller's tolerance (NULL: {0, 0}) as two values; false when one is negative or NaN.
inline bool error_tol(const rt_error_tol* tol, double& abs_tol, double& rel_tol) {
  abs_tol = tol ? tol->abs_tol : 0.0;
  rel_tol = tol ? tol->rel_tol : 0.0;
  return abs_tol >= 0.0 && rel_tol >= 0.0;
}

}  // namespace rt
