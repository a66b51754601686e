// rt_k_denoise.hip — the feature-guided denoiser's kernels (rt.h rt_denoise*; rt_denoise_kernels.h) and their
// launch sequence: prepare, one iteration launch per stride, finish, all on the caller's stream.
#include "rt_denoise_kernels.h"

namespace rt {

int denoise_launch(const DenoiseConst& K, int iterations, const double* d_color, const double* d_se,
                   const double* d_feature_sums, const DenoiseBuffers& B, double* d_out_color, uint8_t* d_out_rgb8,
                   void* stream, int* launches) {
  hipStream_t st = (hipStream_t)stream;
  const long long npx = (long long)K.W * K.H;
  const dim3 pixel_grid((unsigned)((npx + 255) / 256));
  double4 *guide = (double4*)B.guide, *src = (double4*)B.a, *dst = (double4*)B.b;
  *launches = 0;
  hipError_t e = hipMemsetAsync(B.counts, 0, 3 * sizeof(unsigned long long), st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(rtdn::denoise_prepare, pixel_grid, dim3(256), 0, st, K, d_color, d_se, d_feature_sums, guide, src,
                     B.counts);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ++*launches;
  for (int it = 0; it < iterations; ++it) {
    // classes that hold a pixel: min(s, W) x min(s, H); tiles over the largest class, ceil(W / s) x ceil(H / s)
    const long long s = 1ll << it;
    const int nrx = (int)(s < K.W ? s : K.W), nry = (int)(s < K.H ? s : K.H);
    const int tiles_x = (int)(((K.W + s - 1) / s + kDenoiseTileW - 1) / kDenoiseTileW);
    const int tiles_y = (int)(((K.H + s - 1) / s + kDenoiseTileH - 1) / kDenoiseTileH);
    const long long blocks = (long long)nrx * tiles_x * nry * tiles_y;  // (< 2^31: fewer than pixels / 4 + 2^16)
    hipLaunchKernelGGL(rtdn::denoise_iteration, dim3((unsigned)blocks), dim3(kDenoiseTileW * kDenoiseTileH), 0, st, K,
                       (const double4*)guide, (const double4*)src, dst, it, nrx, tiles_x, tiles_y);
    if ((e = hipGetLastError()) != hipSuccess) return (int)e;
    ++*launches;
    double4* t = src;
    src = dst;
    dst = t;
  }
  hipLaunchKernelGGL(rtdn::denoise_finish, pixel_grid, dim3(256), 0, st, K, (const double4*)src, d_feature_sums, d_color,
                     d_out_color, d_out_rgb8, B.counts);
  if ((e = hipGetLastError()) != hipSuccess) return (int)e;
  ++*launches;
  return 0;
}

}  // namespace rt
