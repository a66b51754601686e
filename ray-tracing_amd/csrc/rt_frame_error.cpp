// rt_frame_error.cpp — the host half of a progressive frame's error estimate (include/rt.h): the error
// map and its summary from image-order sums and moments, by the per-pixel function the device runs
// (rt_error.h). No HIP, no device: it builds for the CPU as is (tests/c/error_estimate_check.c drives
// it under the sanitizers).
#include <string>

#include "rt.h"
#include "rt_error.h"
#include "rt_internal.h"

extern "C" {

int rt_error_estimate(const double* sums, const double* moments, int64_t pixels, int chunks_done, int samples_done,
                      const rt_error_tol* tol, double* out_se, rt_error_stats* out) {
  double abs_tol, rel_tol;
  if (!sums || !moments || pixels <= 0 || chunks_done < 2 || samples_done < chunks_done) {
    rt::set_error("rt_error_estimate: needs sums, moments, pixels >= 1 and samples_done >= chunks_done >= 2");
    return RT_E_INVALID;
  }
  if (!rt::error_tol(tol, abs_tol, rel_tol)) {
    rt::set_error("rt_error_estimate: abs_tol and rel_tol must be >= 0 and not NaN");
    return RT_E_INVALID;
  }
  rt_error_stats st{};
  st.chunks_done = chunks_done;
  st.samples_done = samples_done;
  st.pixels = pixels;
  double total = 0.0;  // (over the finite pixels' channels, in pixel and channel order)
  for (int64_t i = 0; i < pixels; ++i) {
    double se[3];
    const int cls = rt::pixel_error(sums + 3 * i, moments + 3 * i, chunks_done, samples_done, abs_tol, rel_tol, se);
    if (out_se)
      for (int c = 0; c < 3; ++c) out_se[3 * i + c] = se[c];
    if (cls == rt::kPixelNonFinite) {
      ++st.nonfinite_pixels;
      continue;
    }
    if (cls == rt::kPixelUnconverged) ++st.unconverged_pixels;
    for (int c = 0; c < 3; ++c) {
      total += se[c];
      if (se[c] > st.max_se) st.max_se = se[c];
    }
  }
  const int64_t finite = pixels - st.nonfinite_pixels;
  st.mean_se = finite ? total / (double)(3 * finite) : 0.0;
  if (out) *out = st;
  return RT_OK;
}

}  // extern "C"
