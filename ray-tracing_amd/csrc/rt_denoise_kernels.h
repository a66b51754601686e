// rt_denoise_kernels.h — the feature-guided denoiser's kernels (include/rt.h rt_denoise*; instantiated in
// rt_k_denoise.hip): prepare, one launch per a-trous iteration, finish. The per-pixel arithmetic is rt_denoise.h's,
// the text rt_denoise_host compiles, so the device's image is the host's bit for bit; the kernels only decide
// which lane computes which pixel and where its taps come from. DESIGN.md §3.9.
#pragma once
#include <hip/hip_runtime.h>

#include "rt_denoise.h"

namespace rtdn {

using rt::DenoiseConst;

// Exact per-block counts: each wave's ballot leaves as one integer atomic.
__device__ __forceinline__ void wave_count(bool flag, unsigned long long* counter) {
  const unsigned n = (unsigned)__popcll(__ballot(flag));
  if (n && (threadIdx.x & 63) == 0) atomicAdd(counter, (unsigned long long)n);
}

// Pixel i's guide record (N, Z) and first (colour, V) record, 32 bytes each, from the call's inputs in image order;
// counts[0] += pixels of `color` that are invalid.
__global__ void __launch_bounds__(256) denoise_prepare(DenoiseConst K, const double* __restrict__ color,
                                                       const double* __restrict__ se, const double* __restrict__ feat,
                                                       double4* __restrict__ guide, double4* __restrict__ cv,
                                                       unsigned long long* counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool invalid = false;
  if (i < (long long)K.W * K.H) {
    double c[3], e[3], f[RT_FEATURE_DOUBLES], g[4], v[4];
    for (int k = 0; k < 3; ++k) c[k] = color[3 * i + k];
    for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) f[k] = feat[RT_FEATURE_DOUBLES * i + k];
    if (se) {  // (two inlined calls: a pointer chosen at run time would put e[] in scratch)
      for (int k = 0; k < 3; ++k) e[k] = se[3 * i + k];
      rt::denoise_prepare(K, c, e, f, g, v);
    } else {
      rt::denoise_prepare(K, c, nullptr, f, g, v);
    }
    guide[i] = make_double4(g[0], g[1], g[2], g[3]);
    cv[i] = make_double4(v[0], v[1], v[2], v[3]);
    invalid = !rt::denoise_valid(c);
  }
  wave_count(invalid, &counts[0]);
}

// One iteration at stride s = 1 << shift. The pixels of one residue class mod s in both axes, (s X + rx, s Y + ry),
// form a sub-image in which the stencil has stride 1, so a workgroup owns a kTileW x kTileH block of one class and
// stages the (kTileW + 4) x (kTileH + 4) lattice of its taps in LDS once: the same LDS, the same code and the same
// reuse (1.7 records staged per pixel) at every stride. Blocks: class-major, nrx = min(s, W) classes of tiles_x
// tiles across, nry x tiles_y down; a class's last tiles may lie partly or wholly outside the image.
// LDS holds eight planes (N_x N_y N_z Z r g b V) of doubles, row pitch kPitch: a wave is two rows of 32 lanes, so
// each half-wave of a ds_read_b64 reads 256 contiguous bytes, one bank row, whatever the tap offset: no conflicts.
// A tap outside the image is staged with a NaN colour: rt.h skips invalid taps and taps outside alike.
__global__ void __launch_bounds__(rt::kDenoiseTileW * rt::kDenoiseTileH)
denoise_iteration(DenoiseConst K, const double4* __restrict__ guide, const double4* __restrict__ src,
                  double4* __restrict__ dst, int shift, int nrx, int tiles_x, int tiles_y) {
  constexpr int TW = rt::kDenoiseTileW, TH = rt::kDenoiseTileH, PW = rt::kDenoisePitch, PH = TH + 4;
  constexpr int kPlane = PW * PH;
  __shared__ double lds[8 * kPlane];
  static_assert(sizeof(lds) == rt::kDenoiseLdsBytes, "rt_last_denoise reports the iteration kernel's LDS");
  const long long s = 1ll << shift;
  const int bx = (int)(blockIdx.x % (unsigned)(nrx * tiles_x)), by = (int)(blockIdx.x / (unsigned)(nrx * tiles_x));
  const int rx = bx / tiles_x, tx = bx % tiles_x, ry = by / tiles_y, ty = by % tiles_y;
  for (int idx = threadIdx.x; idx < kPlane; idx += TW * TH) {
    const int hx = idx % PW, hy = idx / PW;
    const long long X = (long long)tx * TW + hx - 2, Y = (long long)ty * TH + hy - 2;
    const long long x = X * s + rx, y = Y * s + ry;
    double4 g = make_double4(0.0, 0.0, 0.0, 0.0);
    double4 c = make_double4(__builtin_nan(""), 0.0, 0.0, 0.0);
    if (X >= 0 && Y >= 0 && x < K.W && y < K.H) {
      const long long q = y * K.W + x;
      g = guide[q];
      c = src[q];
    }
    lds[0 * kPlane + idx] = g.x, lds[1 * kPlane + idx] = g.y, lds[2 * kPlane + idx] = g.z, lds[3 * kPlane + idx] = g.w;
    lds[4 * kPlane + idx] = c.x, lds[5 * kPlane + idx] = c.y, lds[6 * kPlane + idx] = c.z, lds[7 * kPlane + idx] = c.w;
  }
  __syncthreads();
  const int lx = threadIdx.x % TW, ly = threadIdx.x / TW;
  const long long x = ((long long)tx * TW + lx) * s + rx, y = ((long long)ty * TH + ly) * s + ry;
  if (x >= K.W || y >= K.H) return;
  const int centre = (ly + 2) * PW + lx + 2;
  auto record = [&](int at, double g[4], double c[4]) {
    for (int k = 0; k < 4; ++k) g[k] = lds[k * kPlane + at], c[k] = lds[(4 + k) * kPlane + at];
  };
  double gp[4], cp[4], out[4];
  record(centre, gp, cp);
  rt::denoise_iterate(
      K, gp, cp,
      [&](int dx, int dy, double gq[4], double cq[4]) {
        record(centre + dy * PW + dx, gq, cq);
        return true;  // (outside the image: staged invalid)
      },
      out);
  dst[y * K.W + x] = make_double4(out[0], out[1], out[2], out[3]);
}

// The output colour and bytes of pixel i from its last record; counts[1] += invalid outputs, counts[2] += pixels
// invalid in `color` and valid in the output.
__global__ void __launch_bounds__(256) denoise_finish(DenoiseConst K, const double4* __restrict__ cv,
                                                      const double* __restrict__ feat, const double* color,
                                                      double* out_color, uint8_t* out_rgb8, unsigned long long* counts) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  bool invalid = false, filled = false;
  if (i < (long long)K.W * K.H) {
    const double4 r = cv[i];
    const double v[4] = {r.x, r.y, r.z, r.w};
    double c[3], f[RT_FEATURE_DOUBLES], o[3];
    for (int k = 0; k < 3; ++k) c[k] = color[3 * i + k];
    for (int k = 0; k < RT_FEATURE_DOUBLES; ++k) f[k] = feat[RT_FEATURE_DOUBLES * i + k];
    rt::denoise_finish(K, v, f, o);
    for (int k = 0; k < 3; ++k) {
      out_color[3 * i + k] = o[k];
      if (out_rgb8) out_rgb8[3 * i + k] = rt::scale_color8(o[k]);
    }
    invalid = !rt::denoise_valid(o);
    filled = !invalid && !rt::denoise_valid(c);
  }
  wave_count(invalid, &counts[1]);
  wave_count(filled, &counts[2]);
}

}  // namespace rtdn
