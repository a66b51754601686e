// rt_frame_error.cpp — the host half of a progressive frame's error estimate (include/rt.h): the error
// map and its summary from image-order sums and moments, by the per-pixel function the device runs
// (rt_error.h), and an adaptive frame's stop rule over the same arrays (rt_adapt_decide). No HIP, no
// device: it builds for the CPU as is (tests/c/error_estimate_check.c and tests/c/adapt_decide_check.c
// drive it under the sanitizers).
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

int rt_adapt_decide(const double* sums, const double* moments, const int32_t* chunks_in, int64_t pixels,
                    int chunks_done, int chunk, int spp, const rt_adapt_rule* rule, int32_t* chunks_out,
                    rt_adapt_stats* out) {
  if (!sums || !rule || (!chunks_out && !out) || pixels <= 0 || chunks_done < 1 || chunk < 1 || spp < 1 ||
      (int64_t)(chunks_done - 1) * chunk >= spp) {
    rt::set_error("rt_adapt_decide: needs sums, a rule, an output, pixels >= 1 and 1 <= chunks_done <= ceil(spp / chunk)");
    return RT_E_INVALID;
  }
  if (!rt::adapt_rule_ok(rule)) {
    rt::set_error("rt_adapt_decide: bad rule (flags, a negative or NaN tolerance, or min_chunks < 2 with RT_ADAPT_CONVERGED)");
    return RT_E_INVALID;
  }
  if ((rule->flags & RT_ADAPT_CONVERGED) && !moments) {
    rt::set_error("rt_adapt_decide: RT_ADAPT_CONVERGED needs the moments");
    return RT_E_INVALID;
  }
  if (chunks_in)
    for (int64_t i = 0; i < pixels; ++i)
      if (chunks_in[i] < 0 || chunks_in[i] > chunks_done) {
        rt::set_error("rt_adapt_decide: chunks_in holds a count outside [0, chunks_done]");
        return RT_E_INVALID;
      }
  const int64_t n64 = (int64_t)chunks_done * chunk;
  const int samples = (int)(n64 < spp ? n64 : spp);
  rt_adapt_stats st{};
  st.chunks_done = chunks_done;
  st.pixels = pixels;
  for (int64_t i = 0; i < pixels; ++i) {
    const double* s = sums + 3 * i;
    int32_t k = chunks_in ? chunks_in[i] : 0;
    if (k == 0 && rt::adapt_pixel(s, moments ? moments + 3 * i : nullptr, chunks_done, samples, rule->flags,
                                  rule->abs_tol, rule->rel_tol, rule->min_chunks) != rt::kAdaptKeep) {
      k = chunks_done;
      ++st.stopped_now;
    }
    if (k) ++((s[0] != s[0] || s[1] != s[1] || s[2] != s[2]) ? st.stopped_nan : st.stopped_converged_or_masked);
    if (chunks_out) chunks_out[i] = k;
  }
  st.active_pixels = pixels - st.stopped_nan - st.stopped_converged_or_masked;
  if (out) *out = st;
  return RT_OK;
}

int rt_error_stats_merge(const rt_error_stats* parts, int n, rt_error_stats* out) {
  if (!parts || !out || n < 1) {
    rt::set_error("rt_error_stats_merge: needs parts, n >= 1 and an output");
    return RT_E_INVALID;
  }
  rt_error_stats st{};
  st.chunks_done = parts[0].chunks_done;
  st.samples_done = parts[0].samples_done;
  double total = 0.0;  // (the parts' mean * finite pixels, in part order)
  int64_t finite = 0;
  for (int r = 0; r < n; ++r) {
    const rt_error_stats& p = parts[r];
    if (p.chunks_done != st.chunks_done || p.samples_done != st.samples_done) {
      rt::set_error("rt_error_stats_merge: the parts disagree in chunks_done or samples_done");
      return RT_E_INVALID;
    }
    if (p.pixels < 0 || p.nonfinite_pixels < 0 || p.nonfinite_pixels > p.pixels) {
      rt::set_error("rt_error_stats_merge: a part's pixel counts are out of range");
      return RT_E_INVALID;
    }
    st.pixels += p.pixels;
    st.nonfinite_pixels += p.nonfinite_pixels;
    st.unconverged_pixels += p.unconverged_pixels;
    if (p.max_se > st.max_se) st.max_se = p.max_se;
    const int64_t fin = p.pixels - p.nonfinite_pixels;
    if (fin) total += p.mean_se * (double)fin;
    finite += fin;
  }
  st.mean_se = finite ? total / (double)finite : 0.0;
  *out = st;
  return RT_OK;
}

}  // extern "C"
