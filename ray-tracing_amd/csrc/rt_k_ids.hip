// rt_k_ids.hip — the material-ID coverage buffers' kernels (rt.h rt_render_ids, rt_ids_matte*, rt_ids_preview*).
// The pass: rt_kernels.h render_ids / render_ids_lds, one instantiation per form of rt::plan_features as
// rt_k_features_chain.hip has them, and no first-hit twins: a pass without a chain runs the same kernel with
// max_bounces = 0. The resolve kernels: one thread per pixel over rt_ids.h's per-pixel text.
// The plain Philox key; a Metal scatter's sine and cosine through the fused sincos call, as the chain pass.
#define RT_FUSED_SINCOS 1
#include "rt_kernels.h"

namespace rt {
const void* ids_kernel(const FeaturePlan& P) {
  constexpr unsigned FW = kVarSpheres | F_WIDE, FM = F_ALL | F_UV | F_MIXW;
  if (P.walk == kFeatWide && P.lds) {
    return by_waves<3, 4>(P.info.waves <= 3 ? 3 : 4, [&](auto W) {
      if (P.leaf_lds)
        return P.pk ? (const void*)render_ids_lds<FW, true, true, W()> : (const void*)render_ids_lds<FW, true, false, W()>;
      return P.pk ? (const void*)render_ids_lds<FW, false, true, W()> : (const void*)render_ids_lds<FW, false, false, W()>;
    });
  }
  if (P.walk == kFeatWide) return P.pk ? (const void*)render_ids<FW, true, false> : (const void*)render_ids<FW, false, false>;
  return P.walk == kFeatMixed ? (const void*)render_ids<FM, false, false> : (const void*)render_ids<FM, false, true>;
}
}  // namespace rt

namespace {
constexpr int kIdsBlock = 256;

__device__ __forceinline__ rt_id_record load_record(const rt_id_record* recs, long long i) {
  const uint4* q = reinterpret_cast<const uint4*>(recs + i);  // (64-byte records in a hipMalloc'd array)
  const uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  rt_id_record r;
  r.id[0] = w0.x, r.id[1] = w0.y, r.id[2] = w0.z, r.id[3] = w0.w, r.id[4] = w1.x, r.id[5] = w1.y, r.id[6] = w1.z;
  r.count[0] = w1.w, r.count[1] = w2.x, r.count[2] = w2.y, r.count[3] = w2.z, r.count[4] = w2.w;
  r.count[5] = w3.x, r.count[6] = w3.y, r.other = w3.z, r.samples = w3.w;
  return r;
}

// The id list staged in LDS by the workgroup, then one pixel per thread: the list is searched by bisection
// (rt_ids.h ids_listed) once per used slot.
__global__ void __launch_bounds__(kIdsBlock) ids_matte(const rt_id_record* recs, long long pixels, const uint32_t* ids,
                                                       int n_ids, double* out_cov, uint8_t* out_u8) {
  __shared__ uint32_t list[RT_ID_MATTE_MAX];
  for (int k = threadIdx.x; k < n_ids; k += kIdsBlock) list[k] = ids[k];  // (n_ids <= RT_ID_MATTE_MAX: the host's check)
  __syncthreads();
  const long long i = (long long)blockIdx.x * kIdsBlock + threadIdx.x;
  if (i >= pixels) return;
  const double cov = rt::ids_matte_cov(load_record(recs, i), list, n_ids);
  if (out_cov) out_cov[i] = cov;
  if (out_u8) out_u8[i] = rt::ids_byte(cov);
}

__global__ void __launch_bounds__(kIdsBlock) ids_preview(const rt_id_record* recs, long long pixels, uint8_t* out_rgb8) {
  const long long i = (long long)blockIdx.x * kIdsBlock + threadIdx.x;
  if (i >= pixels) return;
  uint8_t px[3];
  rt::ids_preview_px(load_record(recs, i), px);
  out_rgb8[3 * i] = px[0], out_rgb8[3 * i + 1] = px[1], out_rgb8[3 * i + 2] = px[2];
}
}  // namespace

namespace rt {
int ids_matte_launch(const rt_id_record* d_recs, long long pixels, const uint32_t* d_ids, int n_ids, double* d_out_cov,
                     uint8_t* d_out_u8, void* stream) {
  const dim3 grid((unsigned)((pixels + kIdsBlock - 1) / kIdsBlock));  // (pixels < 2^32: the callers' check)
  hipLaunchKernelGGL(ids_matte, grid, dim3(kIdsBlock), 0, (hipStream_t)stream, d_recs, pixels, d_ids, n_ids, d_out_cov,
                     d_out_u8);
  return (int)hipGetLastError();
}

int ids_preview_launch(const rt_id_record* d_recs, long long pixels, uint8_t* d_out_rgb8, void* stream) {
  const dim3 grid((unsigned)((pixels + kIdsBlock - 1) / kIdsBlock));
  hipLaunchKernelGGL(ids_preview, grid, dim3(kIdsBlock), 0, (hipStream_t)stream, d_recs, pixels, d_out_rgb8);
  return (int)hipGetLastError();
}
}  // namespace rt
