// rt_render.hip — the device half of the C ABI (include/rt.h): scene upload, launches, assembly,
// debug probes. The render kernels are templates in rt_kernels.h, instantiated per scene variant in
// rt_k_spheres.hip / rt_k_cornell.hip / rt_k_full.hip / rt_k_full_dark.hip; the first-hit feature pass's
// (rt_render_features) in rt_k_features.hip; the denoiser's (rt_denoise*) with their launch sequence in
// rt_k_denoise.hip.
//
// Kernel design:
//  * tier B work-items are (pixel, chunk of up to 32 samples): a lane sums its chunk in sample
//    order and stores the sum; `combine_chunks` adds a pixel's chunk sums in chunk order (rt.h);
//  * persistent waves with ray replacement (`philox_loop2`): the closest-hit walk is resumable;
//    each iteration shades the lanes whose walk ended and starts their next segment, sample or
//    work-item (one wave-aggregated atomicAdd on a work counter), then steps the walking lanes
//    until few still walk — a wave never waits for its slowest walk;
//  * the 4-wide fp32-box walk postpones leaves so wide-node steps and fp64 leaf tests do not
//    share a divergent step; worlds with media or instance frames walk the caller's tree in the
//    reference's own order (media draws);
//  * forward throughput (thr *= att * (spdf / pdf)) instead of the reference's continuation;
//    colour never feeds control flow or the RNG, so this changes rounding only;
//  * traversal stacks live in LDS, [entry][lane] so consecutive lanes hit consecutive banks;
//  * a launch's constants (camera, table pointers, work geometry, claim parameters: LaunchConst) reach
//    the tier-B kernels through a device copy that each workgroup stages in LDS ahead of its stacks;
//    only what a walk step reads travels as kernel arguments (RenderArgs);
//  * tier B (Philox per (pixel, sample)) shards by tiles with no data-path collective before the
//    final framebuffer gather; tier A (the reference's per-column SplitMix stream) runs one lane per
//    column;
//  * a multi-device ctx (rt_create_multi) renders one tile shard per GPU from one host thread and
//    gathers the RGB8 slabs to its first device with RCCL (grouped ncclGather), which assembles.
#include <rccl/rccl.h>

#include <numeric>
#include <vector>

#include "rt_denoise.h"
#include "rt_frame_blob.h"
#include "rt_kernels.h"
#include "rt_prepare.h"

// =================================================================== host side
struct rt_ctx {
  int device = 0;
  int cu_count = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  // Recorded after every tier-B launch: the next launch (on any stream) waits on it before it
  // resets the shared work counter and reuses the chunk-sum buffer.
  hipEvent_t ev_done = nullptr;
  hipStream_t last_stream = nullptr;  // the stream of the last tier-B launch (ev_done's)
  // device scene
  rt_node* d_nodes = nullptr;
  DMat* d_mats = nullptr;
  rt_texture* d_texs = nullptr;
  rt_perlin* d_perlins = nullptr;
  rt_image* d_images = nullptr;
  uint8_t* d_pool = nullptr;
  Scene scene{};
  rt::WorldShape shape;  // the uploaded world's counts and kinds (what the launch decision reads)
  int n_materials = 0, n_textures = 0;  // (rt_debug_probe checks record ids against them)
  rt_wnode* d_wnodes = nullptr;  // 4-wide world tree (replace_ok worlds with a BVH root)
  rt_node* d_leaves = nullptr;   // its leaf table (Scene::leaves)
  rt_qnode* d_qnodes = nullptr;  // spheres-only worlds: the 4-wide tree quantised (Scene::qnodes)
  double* d_sleaves = nullptr;   // and the leaf table's spheres (Scene::sleaves)
  bool has_scene = false;
  unsigned long long* d_counter = nullptr;
  double last_ms = 0.0;
  rt_launch_info last_launch{};  // rt_last_launch
  int last_wide_packed = 0;      // the last 4-wide walk sorted packed keys (rt_debug_wide_keys)
  rt_launch_info last_feature{}; // rt_last_feature_launch
  // The last chain pass (rt_last_feature_chain): an event of the ctx's own recorded after it (created by the first
  // chain pass; not ev_done, which later launches record again, and not the caller's stream, which may be gone by
  // then), pixels * samples, and the device counts {ended_miss, ended_cap, bounces} (fc_counts, below)
  bool fc_made = false;
  hipEvent_t ev_fc = nullptr;
  int64_t fc_samples = 0;
  // rt_render's frame events: after the render launches (gather start), after the gather, after assembly
  hipEvent_t ev_gather = nullptr, ev_gathered = nullptr, ev_asm = nullptr;
  rt_frame_timing last_frame{};  // rt_last_frame_timing
  // Multi-device ctx (rt_create_multi): this ctx is the first device's (RCCL rank 0, the gather root);
  // peers[r - 1] is device r's, comms[r] its communicator (ncclCommInitAll, ranks in list order).
  std::vector<rt_ctx*> peers;
  std::vector<ncclComm_t> comms;
  // rt_render's own device buffers, kept between calls and grown on demand (every rt_render returns after
  // its stream is drained, so the next call may reuse them): the slab (RGB8, fp64) this device renders
  // into, and on a multi-device ctx's first device the gathered slabs and the assembled image; tier A's
  // column generators. Repeated frames of one size allocate nothing.
  struct FrameBuf {
    void* p = nullptr;
    size_t bytes = 0;
  };
  FrameBuf fb_slab, fb_slab_lin, fb_gather, fb_gather_lin, fb_img, fb_img_lin, fb_gens;
  // tier-B scratch, grown on demand: a launch's chunk sums (at most rt::kPartialCap), its tail units' sample
  // colours (LaunchConst::tail_buf), the running per-pixel sums of a frame rendered in chunk batches
  FrameBuf fb_partial, fb_tail, fb_acc;
  int allocs = 0;  // hipMalloc calls made on this device by the current rt_render (rt_frame_timing)
  // The denoiser's buffers (rt.h rt_denoise*), kept and grown like the frame buffers: the guide records and the two
  // (colour, V) buffers, its counts; the device copies of a blocking call's inputs and outputs (rt_frame_denoise:
  // the frame's preview and error map), and the scratch counts of that preview's frame_resolve launch
  FrameBuf dn_guide, dn_a, dn_b, dn_counts, dn_color, dn_se, dn_feat, dn_out, dn_rgb, dn_fcounts;
  FrameBuf fc_counts;
  // Material-ID buffers (rt_render_ids, rt_ids_matte*, rt_ids_preview*): a matte's id list on the device, the device
  // copies of a blocking call's records and outputs, and the hipMalloc calls the last of those calls made
  FrameBuf id_list, id_recs, id_cov, id_u8;
  int id_allocs = 0;
  hipEvent_t ev_dn0 = nullptr, ev_dn1 = nullptr;  // around a blocking denoise call's kernels (kernel_ms)
  rt_denoise_info last_denoise{};                 // rt_last_denoise
  // Progressive frames open on this ctx (rt_frame_*), and what a saved frame records of the scene: the
  // fingerprint of the caller's descriptor and the upload flags (rt_frame_blob.cpp)
  std::vector<rt_frame*> frames;
  uint64_t fingerprint = 0;
  uint32_t upload_flags = 0;
};

// A progressive frame (rt.h): the running per-pixel sums of the chunks rendered so far, in the slab order
// of its shard's launch (`p`'s shard fields; an unsharded frame is shard 0 of 1), and the buffers of its
// previews in the frame's own order: image order, or a shard frame's slab order. One set of helper kernels
// (rt_kernels.h frame_*<SLAB>, launched through FRAME_KERNEL* with frame_const's constants) and one *_run
// function per call serve both kinds. All its work is queued on the ctx's stream.
struct rt_frame {
  rt_ctx* ctx = nullptr;
  bool valid = true;  // false once the ctx's scene was replaced
  rt_camera cam{};
  rt_render_params p{};
  int chunk = 0, chunks_total = 0, chunks_done = 0;
  long long slab = 0, npx = 0;
  // A shard frame (rt_frame_open_shard, rt_frame_restore_shard): `p` keeps its shard fields, the slab is
  // that shard's, and the previews and the error map stay in slab order (d_rgb, d_lin: slab*3). `owned` =
  // the image pixels in the frame's slab (an unsharded frame: npx).
  bool shard = false;
  long long owned = 0;
  double* d_sum = nullptr;   // [slab pixel][3]
  uint8_t* d_rgb = nullptr;  // the last preview's bytes (zero before the first), H*W*3 (shard frame: slab*3)
  double* d_lin = nullptr;   // the last linear preview, H*W*3 (shard frame: slab*3)
  double* d_stage = nullptr; // unsharded: save's and restore's image-order copy of the sums, H*W*3, on first use
  unsigned long long* d_counts = nullptr;  // frame_resolve's {nan_pixels, bytes_changed}
  // RT_FRAME_MOMENTS: the second moments Q of the chunk sums, [slab pixel][3] like d_sum (else null);
  // frame_error's image-order map, H*W*3, and its {non-finite, unconverged, max bits, sum} followed by one
  // partial sum per block, both on first use
  double* d_q = nullptr;
  double* d_se = nullptr;
  unsigned long long* d_err = nullptr;
  // Adaptive frames (rt.h), all allocated by the first stop call: K_p per slab pixel (0 = active), the skip
  // bitmask the render kernels read (one 64-bit word per 64 consecutive slab pixels), frame_adapt's
  // {stopped now, of them NaN}, and on first use the image-order staging of a caller's mask / of K_p
  int* d_kp = nullptr;
  unsigned long long* d_skip = nullptr;
  unsigned long long* d_adapt = nullptr;
  uint8_t* d_mask = nullptr;
  int* d_kimg = nullptr;
  long long stopped_nan = 0, stopped_other = 0;  // stopped pixels by their sums (rt_adapt_stats)
  rt_frame_stats last{};     // the last resolve's counts (a poll with nothing new rendered repeats them)
  // one event pair per advance since the last resolve (kernel_ms); `used` of them are pending
  std::vector<std::pair<hipEvent_t, hipEvent_t>> events;
  size_t used = 0;
};

// The chunks one launch_philox call renders. Default: the whole frame, folded through the ctx's fb_acc
// into the stored image. A progressive frame renders `count` chunks from `first` and keeps the running
// sums in its own buffer.
struct ChunkSpan {
  int first = 0;
  int count = -1;           // -1: every chunk of the frame
  double* acc = nullptr;    // running sums between launches; nullptr: the ctx's fb_acc, grown on demand
  bool keep = false;        // keep the running sums in `acc` after the last chunk (no image is stored)
  double* moments = nullptr;  // a tracked frame's second moments, folded with the sums (combine_chunks_moments)
  hipEvent_t ev_begin = nullptr, ev_end = nullptr;  // around the render launches; nullptr: the ctx's ev0 / ev1
  const unsigned long long* skip = nullptr;  // an adaptive frame's skip bitmask (LaunchConst::skip)
};

namespace {

int hip_fail(hipError_t e, const char* what) {
  rt::set_error(std::string(what) + ": " + hipGetErrorString(e));
  return RT_E_HIP;
}
int hip_ok(hipError_t e, const char* what) { return e == hipSuccess ? RT_OK : hip_fail(e, what); }
#define HIPCHK(x)                                  \
  do {                                             \
    hipError_t _e = (x);                           \
    if (_e != hipSuccess) return hip_fail(_e, #x); \
  } while (0)

int nccl_fail(ncclResult_t r, const char* what) {
  rt::set_error(std::string(what) + ": " + ncclGetErrorString(r));
  return RT_E_COMM;
}
#define NCCLCHK(x)                                    \
  do {                                                \
    ncclResult_t _r = (x);                            \
    if (_r != ncclSuccess) return nccl_fail(_r, #x);  \
  } while (0)

// Device allocation released when it goes out of scope (every return path of the blocking calls).
struct DevBuf {
  void* p = nullptr;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() {
    if (p) (void)hipFree(p);
  }
};

// Selects a ctx's device for the duration of a C-ABI call and restores the caller's current device
// on every return path (a process driving several GPUs from one thread keeps its own selection).
struct DeviceGuard {
  int prev = -1;
  hipError_t err = hipSuccess;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    err = hipSetDevice(dev);
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard&) = delete;
  DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define DEVICE_SCOPE(dev)                                  \
  DeviceGuard _dg(dev);                                    \
  if (_dg.err != hipSuccess) return hip_fail(_dg.err, "hipSetDevice")

// A frame buffer of the ctx with at least `need` bytes on the current device (the caller selects the
// ctx's device): reused as is when large enough, else freed and allocated again (counted in c->allocs).
int grow(rt_ctx* c, rt_ctx::FrameBuf& b, size_t need) {
  if (need <= b.bytes) return RT_OK;
  (void)hipFree(b.p);
  b.p = nullptr;
  b.bytes = 0;
  ++c->allocs;
  HIPCHK(hipMalloc(&b.p, need));
  b.bytes = need;
  return RT_OK;
}
void free_frame_bufs(rt_ctx* c) {
  for (rt_ctx::FrameBuf* b : {&c->fb_slab, &c->fb_slab_lin, &c->fb_gather, &c->fb_gather_lin, &c->fb_img,
                              &c->fb_img_lin, &c->fb_gens, &c->fb_partial, &c->fb_tail, &c->fb_acc, &c->dn_guide,
                              &c->dn_a, &c->dn_b, &c->dn_counts, &c->dn_color, &c->dn_se, &c->dn_feat, &c->dn_out,
                              &c->dn_rgb, &c->dn_fcounts, &c->fc_counts, &c->id_list, &c->id_recs, &c->id_cov, &c->id_u8}) {
    (void)hipFree(b->p);
    b->p = nullptr;
    b->bytes = 0;
  }
}

int invalid(const std::string& s) {
  rt::set_error(s);
  return RT_E_INVALID;
}
int unsupported(const std::string& s) {
  rt::set_error(s);
  return RT_E_UNSUPPORTED;
}

void free_scene(rt_ctx* c) {
  for (void** p : {(void**)&c->d_nodes, (void**)&c->d_mats, (void**)&c->d_texs, (void**)&c->d_perlins,
                   (void**)&c->d_images, (void**)&c->d_pool, (void**)&c->d_wnodes, (void**)&c->d_leaves,
                   (void**)&c->d_qnodes, (void**)&c->d_sleaves}) {
    (void)hipFree(*p);
    *p = nullptr;
  }
  c->shape = rt::WorldShape{};
  c->has_scene = false;
}

template <class T>
int upload(T** dst, const T* src, size_t count) {
  if (count == 0 || !src) return RT_OK;
  HIPCHK(hipMalloc((void**)dst, sizeof(T) * count));
  HIPCHK(hipMemcpy(*dst, src, sizeof(T) * count, hipMemcpyHostToDevice));
  return RT_OK;
}

int check_params(const rt_render_params* p) {
  if (!p) return invalid("null params");
  if (p->width <= 0 || p->height <= 0 || p->spp <= 0 || p->max_depth < 0)
    return invalid("width/height/spp must be positive and max_depth >= 0");
  if (p->rng_mode != RT_RNG_EXACT && p->rng_mode != RT_RNG_PHILOX) return invalid("unknown rng_mode");
  if ((p->flags & RT_FLAG_SHARED_LIBM) && p->rng_mode != RT_RNG_EXACT)
    return invalid("RT_FLAG_SHARED_LIBM is a tier-A (RT_RNG_EXACT) flag");
  const int tile = p->tile ? p->tile : kDefaultTile;
  if (tile <= 0 || tile % 8 || tile > 256) return invalid("tile must be a multiple of 8 in [8, 256]");
  if (p->shard_count < 0 || (p->shard_count > 0 && (p->shard_rank < 0 || p->shard_rank >= p->shard_count)) ||
      (p->shard_count <= 1 && p->shard_rank != 0))
    return invalid("bad shard_rank/shard_count");
  if ((long long)p->width * p->height >= (1ll << 32)) return invalid("image too large for 32-bit pixel ids");
  return RT_OK;
}

// The ctx's work-counter allocation: the counter's 256 bytes, then the device copy of the launch
// constants (LaunchConst) that the tier-B kernels stage in LDS.
constexpr size_t kCounterBytes = 256;

// The render kernel of a form (the kernels live in one translation unit per variant or form: rt_k_*.hip).
const void* philox_kernel(const rt::KernelForm& f) {
  if (f.unit == rt::kUnitSpheresPacked) return rt::philox_kernel_spheres_packed(f);
  if (f.unit == rt::kUnitSpheresGlobal) return rt::philox_kernel_spheres_global(f);
  if (f.unit == rt::kUnitCountPacked) return rt::philox_kernel_count_packed(f);
  if (f.var == kVarSpheres) return rt::philox_kernel_spheres(f);
  if (f.var == kVarCornell) return rt::philox_kernel_cornell(f);
  return f.var == kVarFullDark ? rt::philox_kernel_full_dark(f) : rt::philox_kernel_full(f);
}
// The largest 4-wide tree an LDS-staged launch can be given: its 128-byte nodes alone within the budget
// (whatever the waves, stacks and leaf table take comes off that).
constexpr int kLdsMaxWideNodes = (int)((rt::kLdsBudget - kLcBytes) / sizeof(rt_wnode));
// Every LDS-staged tree is within the packed sort keys' id bound (include/rt_wide.h), with its at most 4
// leaf slots per node; rt::wide_keys_packed still checks the uploaded world's own counts.
static_assert(4 * kLdsMaxWideNodes <= RT_WKEY_MAX_IDS, "an LDS-staged 4-wide tree fits the packed keys");
template <bool LDS>
const void* exact_variant_l(unsigned f, bool shared_libm) {
  switch (variant_for(f)) {
    case kVarSpheres:
      return shared_libm ? (const void*)render_exact<kVarSpheres | F_SLIBM, LDS> : (const void*)render_exact<kVarSpheres, LDS>;
    case kVarCornell:
      return shared_libm ? (const void*)render_exact<kVarCornell | F_SLIBM, LDS> : (const void*)render_exact<kVarCornell, LDS>;
    default: return shared_libm ? (const void*)render_exact<F_ALL | F_SLIBM, LDS> : (const void*)render_exact<F_ALL, LDS>;
  }
}
// Blocks of the tier-A kernel: kExactColsPerWave columns per wave, RT_BLOCK / 64 waves per block.
unsigned exact_blocks(int width) {
  const int per_block = (RT_BLOCK / 64) * kExactColsPerWave;
  return (unsigned)((width + per_block - 1) / per_block);
}
// The tier-A kernel for the ctx's scene and its dynamic LDS bytes: the node array staged in LDS when it
// fits beside the static lane stacks (RTAMD_EXACT_LDS=0: never).
int exact_launch(rt_ctx* c, bool shared_libm, const void** fn, size_t* bytes) {
  const size_t need = (size_t)c->shape.n_nodes * sizeof(rt_node);
  const size_t budget = 160 * 1024 - (size_t)RT_STACK * RT_BLOCK * sizeof(int);
  const char* e = std::getenv("RTAMD_EXACT_LDS");
  if (need <= budget && !(e && e[0] == '0')) {
    *fn = exact_variant_l<true>(c->shape.features, shared_libm);
    *bytes = need;
    HIPCHK(hipFuncSetAttribute(*fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
  } else {
    *fn = exact_variant_l<false>(c->shape.features, shared_libm);
    *bytes = 0;
  }
  return RT_OK;
}

int launch_combine(rt_ctx* c, const LaunchConst& A, hipStream_t st, double* moments) {
  LaunchConst B = A;
  void* args[] = {&B, &moments};  // (combine_chunks takes the first alone)
  // (an adaptive frame's launch, A.skip: the bodies that leave stopped pixels alone)
  const void* fn = A.skip ? (moments ? (const void*)combine_chunks_moments_skip : (const void*)combine_chunks_skip)
                          : (moments ? (const void*)combine_chunks_moments : (const void*)combine_chunks);
  HIPCHK(hipLaunchKernel(fn, dim3((unsigned)((A.slab + 255) / 256)), dim3(256), args, 0, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_done, st));
  return RT_OK;
}

// The launch's culling flags: the caller's, with the per-axis test alone for far-box worlds (WorldShape::far_boxes).
uint32_t cull(const rt_ctx* c, uint32_t flags) { return flags | (c->shape.far_boxes ? RT_FLAG_REFERENCE_CULL : 0u); }

// The work geometry of a tier-B launch in its constants: the frame's part (p's shard, an unsharded frame being
// shard 0 of 1; the tiles, the sample chunks and their divisors; `chunk_knob`: LaunchKnobs::chunk) ...
void fill_frame_geometry(LaunchConst& A, const rt_render_params* p, int chunk_knob) {
  const FrameGeometry g = frame_geometry(p, chunk_knob);
  A.W = p->width, A.H = p->height, A.spp = p->spp;
  A.tile = g.tile, A.tiles_x = g.tiles_x, A.tiles_total = (int)g.tiles_total;
  A.shard_rank = p->shard_rank, A.shard_count = p->shard_count > 0 ? p->shard_count : 1;
  A.slab = g.slab, A.chunk = g.chunk, A.chunks = g.chunks;
  A.work_total = g.slab * g.chunks;  // (the whole frame's; each chunk batch's launch sets its own)
  A.items_total = A.work_total;
  A.tail_start = A.work_total;
  A.div_tp = make_udiv((uint32_t)(A.tile * A.tile));
  A.div_tiles_x = make_udiv((uint32_t)A.tiles_x);
  A.div_bpr = make_udiv((uint32_t)(A.tile >> 3));
  A.div_chunk = make_udiv((uint32_t)A.chunk);
}
// ... and one launch's: `nk` chunks from the frame's chunk `k0`, the last `tail_items` work-items dealt
// one sample per unit.
void fill_batch_geometry(LaunchConst& A, int k0, int nk, long long tail_items) {
  A.chunk_base = k0;
  A.chunks = nk;
  A.items_total = A.slab * nk;
  A.tail_start = A.items_total - std::min(A.items_total, tail_items);
  A.work_total = launch_units(A.items_total, tail_items, A.chunk);
  A.div_tile = make_udiv((uint32_t)(A.tile * A.tile * nk));
}

// A launch's constants (the caller has set its outputs: out_rgb, out_lin, work, prof), and the render kernel's
// own arguments: what a walk step reads, and the constants' device copy, which lives behind the ctx's work
// counter (kCounterBytes) and is rewritten by launch_setup ahead of every launch, in stream order after the
// launch before.
void fill_launch_const(LaunchConst& A, RenderArgs& R, const rt_ctx* c, const rt_camera* cam, const rt_render_params* p,
                       const ChunkSpan& span, const rt::LaunchPlan& P) {
  const rt::LaunchKnobs& K = P.knobs;
  A.S = c->scene;
  A.cam = *cam;
  A.max_depth = p->max_depth, A.seed = p->seed;
  A.flags = cull(c, p->flags);
  fill_frame_geometry(A, p, K.chunk);
  A.counter = c->d_counter;
  A.skip = span.skip;
  A.partial = (double*)c->fb_partial.p;
  A.acc = span.acc ? span.acc : (double*)c->fb_acc.p;
  A.tail_buf = (double*)c->fb_tail.p;
  A.batch = K.batch, A.batch_per_item = P.batch_per_item, A.batch_floor = K.batch_floor;
  A.trav_stop = K.trav_stop, A.leaf_stop = K.leaf_stop, A.box_first = K.box_first, A.med_batch = K.med_batch;
  A.rev_tiles = P.rev_tiles;
  const LaunchConst* d_lc = reinterpret_cast<LaunchConst*>(reinterpret_cast<unsigned char*>(c->d_counter) + kCounterBytes);
  R = RenderArgs{A.S, d_lc, A.seed, A.flags, A.trav_stop, A.leaf_stop, A.box_first, A.med_batch, A.prof};
}

// One launch per chunk batch of the plan (stream-ordered; the span's events around all the render launches):
// the constants' device copy, the render kernel, the tail's sums, the fold into the running sums.
int run_batches(rt_ctx* c, LaunchConst& A, const LaunchConst* d_lc, const rt::LaunchPlan& P, const ChunkSpan& span,
                const void* fn, int grid, void** args, hipStream_t st) {
  hipEvent_t ev_begin = span.ev_begin ? span.ev_begin : c->ev0, ev_end = span.ev_end ? span.ev_end : c->ev1;
  for (int b0 = 0; b0 < P.chunks_total; b0 += P.per_batch) {
    const int nk = std::min(P.per_batch, P.chunks_total - b0);
    const int k0 = span.first + b0;  // the launch's first chunk of the frame
    fill_batch_geometry(A, k0, nk, P.tail_items);
    const bool last = b0 + nk == P.chunks_total;
    A.combine = (k0 > 0 ? 1 : 0) | (last && !span.keep ? 2 : 0);
    LaunchConst B = A;  // (arguments are copied at launch)
    void* sargs[] = {&B, &d_lc};  // the constants' device copy, and the work counter back to 0
    HIPCHK(hipLaunchKernel((const void*)launch_setup, dim3(1), dim3(64), sargs, 0, st));
    HIPCHK(hipGetLastError());
    if (b0 == 0) HIPCHK(hipEventRecord(ev_begin, st));
    HIPCHK(hipLaunchKernel(fn, dim3(grid), dim3(P.info.block), args, (size_t)P.info.dyn_lds_bytes, st));
    HIPCHK(hipGetLastError());
    if (A.tail_start < A.items_total) {
      void* targs[] = {&B};
      HIPCHK(hipLaunchKernel(A.skip ? (const void*)tail_combine_skip : (const void*)tail_combine,
                             dim3((unsigned)((A.items_total - A.tail_start + 255) / 256)), dim3(256), targs, 0, st));
      HIPCHK(hipGetLastError());
    }
    if (last) HIPCHK(hipEventRecord(ev_end, st));
    const int rc = launch_combine(c, A, st, span.moments);
    if (rc) return rc;
  }
  return RT_OK;
}

// One tier-B render of p's shard of the ctx's scene on `st`: plan (rt_launch_plan.h), scratch, constants, run.
int launch_philox(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, uint8_t* d_rgb, double* d_lin,
                  hipStream_t st, unsigned long long* d_work = nullptr, unsigned long long* d_prof = nullptr,
                  const ChunkSpan& span = ChunkSpan{}) {
  rt::LaunchPlan P;
  int rc = rt::plan_launch(c->shape, *p, span.first, span.count, d_work != nullptr, span.skip != nullptr,
                           rt::read_knobs(), kLcBytes, P);
  if (rc) return rc;
  const void* fn = philox_kernel(P.form);
  if (!fn) return unsupported("no render kernel is built for this launch's form");
  // The work counter and the scratch buffers are the ctx's: order this launch after the previous
  // one, whichever stream that was on (on the same stream, stream order already does).
  if (st != c->last_stream) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
  c->last_stream = st;
  const size_t need_acc = span.acc ? 0 : P.acc_bytes;
  if (P.partial_bytes > c->fb_partial.bytes || need_acc > c->fb_acc.bytes || P.tail_bytes > c->fb_tail.bytes) {
    HIPCHK(hipEventSynchronize(c->ev_done));
    if ((rc = grow(c, c->fb_partial, P.partial_bytes)) || (rc = grow(c, c->fb_acc, need_acc)) ||
        (rc = grow(c, c->fb_tail, P.tail_bytes)))
      return rc;
  }
  LaunchConst A{};
  RenderArgs R{};
  A.out_rgb = d_rgb, A.out_lin = d_lin, A.work = d_work, A.prof = d_prof;
  fill_launch_const(A, R, c, cam, p, span, P);
  const int lds = P.info.dyn_lds_bytes;
  if (lds) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int grid = P.info.grid, n_items = P.n_items, entries = P.entries, n_leaves = P.n_leaves;
  if (!P.form.lds) {  // (at most the blocks that are resident at once)
    int bpc = 1;
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&bpc, fn, P.info.block, (size_t)lds));
    grid = (int)std::min<long long>(grid, (long long)c->cu_count * std::max(1, bpc));
  }
  c->last_launch = P.info;
  c->last_launch.grid = grid;
  c->last_wide_packed = P.form.pk;
  void* staged_args[] = {&R, &n_items, &entries, &n_leaves};
  void* global_args[] = {&R, &entries};
  return run_batches(c, A, R.lc, P, span, fn, grid, P.form.lds ? staged_args : global_args, st);
}

// rt_render, tier B, on a multi-device ctx (rt_create_multi): shard r of N = the ctx's r-th device. Every
// device renders its tiles into a slab on its own stream (the launches are queued from this thread and
// run concurrently); the slabs are gathered to device 0 by RCCL (one ncclGather per communicator, grouped,
// each on its device's stream after that device's render), which assembles the image.
// Not in place: device 0 renders into its own slab too, so the gather moves bytes even at N = 1.
int render_multi(rt_ctx* c, const rt_camera* cam, rt_render_params p, uint8_t* out_rgb, double* out_lin) {
  const int n = 1 + (int)c->peers.size();
  p.shard_count = n;
  const long long slab = frame_geometry(&p).slab;
  auto dev_ctx = [&](int r) { return r == 0 ? c : c->peers[r - 1]; };
  const long long npx = (long long)p.width * p.height;
  // the send slabs on every device, the gathered slabs and the image on device 0: the ctx's frame buffers,
  // grown on demand (rt_ctx::FrameBuf), so that repeated frames allocate nothing
  int rc = RT_OK;
  for (int r = 0; r < n && !rc; ++r) {
    rt_ctx* d = dev_ctx(r);
    DEVICE_SCOPE(d->device);
    if ((rc = grow(d, d->fb_slab, (size_t)slab * 3))) break;
    if (out_lin && (rc = grow(d, d->fb_slab_lin, sizeof(double) * (size_t)slab * 3))) break;
  }
  {
    DEVICE_SCOPE(c->device);
    if (!rc) rc = grow(c, c->fb_gather, (size_t)n * slab * 3);
    if (!rc && out_lin) rc = grow(c, c->fb_gather_lin, sizeof(double) * (size_t)n * slab * 3);
    if (!rc) rc = grow(c, c->fb_img, (size_t)npx * 3);
    if (!rc && out_lin) rc = grow(c, c->fb_img_lin, sizeof(double) * (size_t)npx * 3);
  }
  if (rc) return rc;
  void* gathered = c->fb_gather.p;
  void* gathered_lin = c->fb_gather_lin.p;
  void* img = c->fb_img.p;
  void* img_lin = c->fb_img_lin.p;
  // the shards' renders, one per device, queued back to back
  for (int r = 0; r < n; ++r) {
    rt_ctx* d = dev_ctx(r);
    DEVICE_SCOPE(d->device);
    rt_render_params pr = p;
    pr.shard_rank = r;
    if ((rc = launch_philox(d, cam, &pr, (uint8_t*)d->fb_slab.p, out_lin ? (double*)d->fb_slab_lin.p : nullptr,
                            d->stream)))
      return rc;
    if (r == 0) HIPCHK(hipEventRecord(c->ev_gather, c->stream));
  }
  // the RCCL gather of the slabs to device 0 (rank 0), in the ranks' stream order after their renders
  {
    DeviceGuard _dg(c->device);
    NCCLCHK(ncclGroupStart());
    for (int r = 0; r < n; ++r) {
      rt_ctx* d = dev_ctx(r);
      const ncclResult_t g = ncclGather(d->fb_slab.p, r == 0 ? gathered : nullptr, (size_t)slab * 3, ncclUint8, 0,
                                        c->comms[r], d->stream);
      const ncclResult_t gl = g == ncclSuccess && out_lin
                                  ? ncclGather(d->fb_slab_lin.p, r == 0 ? gathered_lin : nullptr, (size_t)slab * 3,
                                               ncclFloat64, 0, c->comms[r], d->stream)
                                  : g;
      if (gl != ncclSuccess) {
        (void)ncclGroupEnd();
        return nccl_fail(gl, "ncclGather");
      }
    }
    NCCLCHK(ncclGroupEnd());
  }
  {
    DEVICE_SCOPE(c->device);
    HIPCHK(hipEventRecord(c->ev_gathered, c->stream));
    if ((rc = rt_assemble_async(c, &p, (const uint8_t*)gathered, (uint8_t*)img, c->stream))) return rc;
    if (out_lin && (rc = rt_assemble_linear_async(c, &p, (const double*)gathered_lin, (double*)img_lin, c->stream)))
      return rc;
    HIPCHK(hipEventRecord(c->ev_asm, c->stream));
  }
  for (int r = 0; r < n; ++r) {  // (the peers' streams too: the next frame reuses their slabs)
    rt_ctx* d = dev_ctx(r);
    DEVICE_SCOPE(d->device);
    HIPCHK(hipStreamSynchronize(d->stream));
  }
  DEVICE_SCOPE(c->device);
  HIPCHK(hipMemcpy(out_rgb, img, (size_t)npx * 3, hipMemcpyDeviceToHost));
  if (out_lin) HIPCHK(hipMemcpy(out_lin, img_lin, sizeof(double) * (size_t)npx * 3, hipMemcpyDeviceToHost));
  rt_frame_timing ft{};
  ft.n_devices = n;
  for (int r = 0; r < n; ++r) ft.device_allocs += dev_ctx(r)->allocs;
  float ms = 0;
  for (int r = 0; r < n; ++r) {
    rt_ctx* d = dev_ctx(r);
    HIPCHK(hipEventElapsedTime(&ms, d->ev0, d->ev1));
    d->last_ms = ms;
    ft.kernel_ms[r] = ms;
  }
  HIPCHK(hipEventElapsedTime(&ms, c->ev_gather, c->ev_gathered));
  ft.gather_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->ev_gathered, c->ev_asm));
  ft.assemble_ms = ms;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev_asm));
  ft.frame_ms = ms;
  c->last_frame = ft;
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_device_count(int* out) {
  if (!out) return invalid("null out");
  HIPCHK(hipGetDeviceCount(out));
  return RT_OK;
}

int rt_create(int device, rt_ctx** out) {
  if (!out) return invalid("null out");
  *out = nullptr;
  int n = 0;
  HIPCHK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return invalid("device index out of range");
  DEVICE_SCOPE(device);
  rt_ctx* c = new rt_ctx();
  c->device = device;
  auto init = [c]() -> int {
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, c->device));
    c->cu_count = prop.multiProcessorCount;
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipEventCreate(&c->ev0));
    HIPCHK(hipEventCreate(&c->ev1));
    HIPCHK(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
    HIPCHK(hipEventCreate(&c->ev_gather));
    HIPCHK(hipEventCreate(&c->ev_gathered));
    HIPCHK(hipEventCreate(&c->ev_asm));
    HIPCHK(hipEventCreate(&c->ev_dn0));
    HIPCHK(hipEventCreate(&c->ev_dn1));
    HIPCHK(hipMalloc((void**)&c->d_counter, kCounterBytes + sizeof(LaunchConst)));
    return RT_OK;
  };
  const int rc = init();
  if (rc) {
    rt_destroy(c);
    return rc;
  }
  *out = c;
  return RT_OK;
}

int rt_create_multi(int n, const int* devices, rt_ctx** out) {
  if (!out) return invalid("null out");
  *out = nullptr;
  if (n < 1 || n > RT_MAX_DEVICES) return invalid("n_devices must be in [1, RT_MAX_DEVICES]");
  int avail = 0;
  HIPCHK(hipGetDeviceCount(&avail));
  std::vector<int> list(n);
  if (devices) std::copy(devices, devices + n, list.begin());
  else std::iota(list.begin(), list.end(), 0);
  for (int i = 0; i < n; ++i) {
    if (list[i] < 0 || list[i] >= avail) return invalid("device index out of range");
    for (int j = 0; j < i; ++j)
      if (list[j] == list[i]) return invalid("device listed twice (one RCCL rank per GPU)");
  }
  rt_ctx* c = nullptr;
  int rc = rt_create(list[0], &c);
  if (rc) return rc;
  for (int i = 1; i < n && !rc; ++i) {
    rt_ctx* p = nullptr;
    rc = rt_create(list[i], &p);
    if (!rc) c->peers.push_back(p);
  }
  if (!rc) {
    DeviceGuard _dg(list[0]);  // (ncclCommInitAll selects each device in turn; the caller's is restored)
    c->comms.assign(n, nullptr);
    const ncclResult_t r = ncclCommInitAll(c->comms.data(), n, list.data());
    if (r != ncclSuccess) {
      c->comms.clear();
      rc = nccl_fail(r, "ncclCommInitAll");
    }
  }
  if (rc) {
    rt_destroy(c);
    return rc;
  }
  *out = c;
  return RT_OK;
}

int rt_ctx_devices(const rt_ctx* c, int* out_n, int* out_devices, int cap) {
  if (!c || !out_n || cap < 0) return invalid("null argument");
  *out_n = 1 + (int)c->peers.size();
  for (int r = 0; out_devices && r < *out_n && r < cap; ++r)
    out_devices[r] = r == 0 ? c->device : c->peers[r - 1]->device;
  return RT_OK;
}

int rt_last_frame_timing(rt_ctx* c, rt_frame_timing* out) {
  if (!c || !out) return invalid("null argument");
  *out = c->last_frame;
  return RT_OK;
}

void rt_destroy(rt_ctx* c) {
  if (!c) return;
  while (!c->frames.empty()) rt_frame_close(c->frames.back());  // (each close removes its frame)
  for (size_t r = 0; r < c->comms.size(); ++r) {
    if (!c->comms[r]) continue;
    DeviceGuard _dr(r == 0 ? c->device : c->peers[r - 1]->device);
    (void)ncclCommDestroy(c->comms[r]);
  }
  c->comms.clear();
  for (rt_ctx* p : c->peers) rt_destroy(p);
  c->peers.clear();
  DeviceGuard _dg(c->device);
  free_scene(c);
  free_frame_bufs(c);
  (void)hipFree(c->d_counter);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  if (c->ev_fc) (void)hipEventDestroy(c->ev_fc);
  if (c->ev_gather) (void)hipEventDestroy(c->ev_gather);
  if (c->ev_gathered) (void)hipEventDestroy(c->ev_gathered);
  if (c->ev_asm) (void)hipEventDestroy(c->ev_asm);
  if (c->ev_dn0) (void)hipEventDestroy(c->ev_dn0);
  if (c->ev_dn1) (void)hipEventDestroy(c->ev_dn1);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

int rt_upload_scene(rt_ctx* c, const rt_scene_desc* d) { return rt_upload_scene_ex(c, d, 0u); }

}  // extern "C"

namespace {
// Copies a prepared scene to c's device (replacing its scene).
int upload_prepared(rt_ctx* c, const rt::PreparedScene& P, const rt_scene_desc* din) {
  int rc = RT_OK;
  DEVICE_SCOPE(c->device);
  free_scene(c);
  if ((rc = upload(&c->d_nodes, P.nodes.data(), P.nodes.size())) ||
      (rc = upload(&c->d_mats, P.mats.data(), P.mats.size())) ||
      (rc = upload(&c->d_texs, din->textures, (size_t)din->n_textures)) ||
      (rc = upload(&c->d_perlins, din->perlins, (size_t)din->n_perlins)) ||
      (rc = upload(&c->d_images, din->images, (size_t)din->n_images)) ||
      (rc = upload(&c->d_pool, din->image_pool, (size_t)din->image_pool_bytes)) ||
      (rc = upload(&c->d_wnodes, P.wnodes.data(), P.wnodes.size())) ||
      (rc = upload(&c->d_leaves, P.leaves.data(), P.leaves.size())) ||
      (rc = upload(&c->d_qnodes, P.qnodes.data(), P.qnodes.size())) ||
      (rc = upload(&c->d_sleaves, P.sleaves.data(), P.sleaves.size()))) {
    free_scene(c);
    return rc;
  }
  Scene& S = c->scene;
  S.nodes = c->d_nodes;
  S.mats = c->d_mats;
  S.texs = c->d_texs;
  S.perlins = c->d_perlins;
  S.images = c->d_images;
  S.pool = c->d_pool;
  S.wnodes = c->d_wnodes;
  S.leaves = c->d_leaves;
  S.qnodes = c->d_qnodes;
  S.sleaves = c->d_sleaves;
  S.world = P.world;
  S.world_ref = P.world_ref;
  S.lights = P.lights;
  S.ref_walk = P.ref_walk;
  c->shape = rt::world_shape(P, c->cu_count);
  S.frames = c->shape.frames;
  for (int i = 0; i < 3; ++i) S.bg[i] = din->background[i];
  c->n_materials = din->n_materials;
  c->n_textures = din->n_textures;
  c->has_scene = true;
  return RT_OK;
}
}  // namespace

extern "C" {

int rt_upload_scene_ex(rt_ctx* c, const rt_scene_desc* din, uint32_t flags) {
  if (!c || !din) return invalid("null argument");
  // the host half (rt_prepare.cpp): validation, the walk's trees, the tagged device copy — once, then
  // the copy goes to every device of the ctx (a malformed descriptor leaves every device's scene as it was)
  rt::PreparedScene P;
  int rc = rt::prepare_scene(din, flags, P);
  if (rc) return rc;
  // the scene is replaced from here on: the ctx's open progressive frames are over (their queued work is
  // drained first, it reads the scene about to be freed)
  if (!c->frames.empty()) {
    DEVICE_SCOPE(c->device);
    HIPCHK(hipStreamSynchronize(c->stream));
    for (rt_frame* f : c->frames) f->valid = false;
  }
  c->fingerprint = rt::scene_fingerprint(din);
  c->upload_flags = flags;
  rc = upload_prepared(c, P, din);
  for (size_t r = 0; r < c->peers.size() && !rc; ++r) rc = upload_prepared(c->peers[r], P, din);
  if (rc) {  // (a device failed: no device keeps a scene, so a multi-device render cannot mix two)
    for (rt_ctx* p : c->peers) {
      DeviceGuard _dg(p->device);
      free_scene(p);
    }
    DeviceGuard _dg(c->device);
    free_scene(c);
  }
  return rc;
}

int rt_shard_geometry(const rt_render_params* p, int64_t* tiles_total, int64_t* tiles_per_shard,
                      int64_t* slab_pixels) {
  int rc = check_params(p);
  if (rc) return rc;
  const FrameGeometry g = frame_geometry(p);
  if (tiles_total) *tiles_total = g.tiles_total;
  if (tiles_per_shard) *tiles_per_shard = g.per_shard;
  if (slab_pixels) *slab_pixels = g.slab;
  return RT_OK;
}

// Internal (rt_internal.h; no device needed): the launch constants' work geometry as launch_philox fills
// it for shard p->shard_rank and a launch of `n_chunks` chunks from `chunk_first`, and the device's own
// decomposition (work_unit) of the units [first, first + n) evaluated on the host.
int rt_internal_work_units(const rt_render_params* p, int chunk_first, int n_chunks, long long tail_items,
                           uint32_t first, int n, int32_t* out5, int64_t* out_slot, int64_t* out_totals) {
  int rc = check_params(p);
  if (rc) return rc;
  if (n < 0 || (n > 0 && (!out5 || !out_slot))) return invalid("null output");
  LaunchConst A{};
  fill_frame_geometry(A, p, rt::chunk_knob());
  if (chunk_first < 0 || n_chunks < 1 || chunk_first + n_chunks > A.chunks || tail_items < 0)
    return invalid("bad chunk span");
  fill_batch_geometry(A, chunk_first, n_chunks, tail_items);
  if (out_totals) {
    out_totals[0] = A.work_total;
    out_totals[1] = A.items_total;
    out_totals[2] = A.tail_start;
    out_totals[3] = A.slab;
    out_totals[4] = A.chunk;
  }
  for (int i = 0; i < n; ++i) {
    int px = -1, row = -1, s0 = 0, s1 = 0;
    long long slot = -1;
    const bool ok = work_unit(A, first + (uint32_t)i, px, row, s0, s1, slot);
    int32_t* o = out5 + 5 * (size_t)i;
    o[0] = ok, o[1] = px, o[2] = row, o[3] = s0, o[4] = s1;
    out_slot[i] = slot;
  }
  return RT_OK;
}

// Internal (rt_internal.h; no device needed): the launch plan launch_philox would make for `desc` uploaded
// with `upload_flags` on a device of `cu_count` CUs, under the environment's knobs.
int rt_internal_launch_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count, const rt_render_params* p,
                            int span_first, int span_count, int count_build, int adaptive, rt_launch_info* out,
                            int32_t* out_extra) {
  if (!desc || !out || cu_count < 1) return invalid("null argument");
  int rc = check_params(p);
  if (rc) return rc;
  rt::PreparedScene S;
  if ((rc = rt::prepare_scene(desc, upload_flags, S))) return rc;
  rt::LaunchPlan P;
  rc = rt::plan_launch(rt::world_shape(S, cu_count), *p, span_first, span_count, count_build != 0, adaptive != 0,
                       rt::read_knobs(), kLcBytes, P);
  if (rc) return rc;
  *out = P.info;
  if (out_extra) {
    const rt::LaunchKnobs& K = P.knobs;
    const int32_t extra[RT_PLAN_EXTRA] = {
        P.n_items,     P.entries,           P.n_leaves,           K.trav_stop, K.leaf_stop, K.box_first, K.med_batch, K.batch,
        K.batch_floor, (int32_t)P.rev_tiles, (int32_t)P.tail_items, P.per_batch, P.form.pk,   P.form.unit, P.info.grid, P.form.waves};
    std::copy(extra, extra + RT_PLAN_EXTRA, out_extra);
  }
  return RT_OK;
}

namespace {
// rt_render_features_chain's own argument checks (rt.h), before any HIP call and before features_check's.
int chain_check(const rt_feature_chain* ch) {
  if (!ch) return invalid("rt_render_features_chain: null argument");
  if (ch->max_bounces < 0 || ch->max_bounces > RT_CHAIN_MAX_BOUNCES)
    return invalid("rt_render_features_chain: max_bounces must be in 0..64");
  if (ch->flags & ~(RT_CHAIN_DIELECTRIC | RT_CHAIN_METAL)) return invalid("rt_render_features_chain: unknown flag bits");
  if (!(ch->max_fuzz >= 0.0) || ch->max_fuzz == INFINITY)
    return invalid("rt_render_features_chain: max_fuzz must be finite and >= 0");
  return RT_OK;
}

int features_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count, const rt_render_params* p, bool chain,
                  rt_launch_info* out, int32_t* out_extra, long long slab_blocks = -1) {
  if (!desc || !p || !out || cu_count < 1) return invalid("null argument");
  if (p->width <= 0 || p->height <= 0) return invalid("width and height must be positive");
  rt::PreparedScene S;
  int rc = rt::prepare_scene(desc, upload_flags, S);
  if (rc) return rc;
  rt::FeaturePlan P;
  if ((rc = rt::plan_features(rt::world_shape(S, cu_count), *p, rt::read_knobs(), P, chain, slab_blocks))) return rc;
  *out = P.info;
  if (out_extra) {
    const int32_t extra[RT_FEATURES_PLAN_EXTRA] = {P.n_items, P.entries, P.n_leaves, P.pk, P.leaf_stop};
    std::copy(extra, extra + RT_FEATURES_PLAN_EXTRA, out_extra);
  }
  return RT_OK;
}
}  // namespace

// Internal (rt_internal.h; no device needed): the plan launch_features would make, like rt_internal_launch_plan.
int rt_internal_features_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count, const rt_render_params* p,
                              rt_launch_info* out, int32_t* out_extra) {
  return features_plan(desc, upload_flags, cu_count, p, false, out, out_extra);
}
int rt_internal_features_chain_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count,
                                    const rt_render_params* p, const rt_feature_chain* chain, rt_launch_info* out,
                                    int32_t* out_extra) {
  const int rc = chain_check(chain);
  return rc ? rc : features_plan(desc, upload_flags, cu_count, p, true, out, out_extra);
}

int rt_render_shard_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, uint8_t* d_rgb, double* d_lin,
                          void* stream) {
  if (!c || !cam || !d_rgb) return invalid("null argument");
  int rc = check_params(p);
  if (rc) return rc;
  if (!c->has_scene) {
    rt::set_error("rt_render_shard_async: no scene uploaded");
    return RT_E_STATE;
  }
  if (p->rng_mode != RT_RNG_PHILOX) return invalid("sharded rendering needs RT_RNG_PHILOX (tier B)");
  DEVICE_SCOPE(c->device);
  return launch_philox(c, cam, p, d_rgb, d_lin, (hipStream_t)stream);
}

int rt_assemble_async(rt_ctx* c, const rt_render_params* p, const uint8_t* d_slabs, uint8_t* d_image, void* stream) {
  if (!c || !d_slabs || !d_image) return invalid("null argument");
  int rc = check_params(p);
  if (rc) return rc;
  const FrameGeometry g = frame_geometry(p);
  const long long n = (long long)p->width * p->height;
  DEVICE_SCOPE(c->device);  // (the caller's current device may be another ctx's)
  hipLaunchKernelGGL(assemble<uint8_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_slabs,
                     d_image, p->width, p->height, g.tile, g.tiles_x, p->shard_count > 0 ? p->shard_count : 1, g.slab);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int rt_assemble_linear_async(rt_ctx* c, const rt_render_params* p, const double* d_slabs, double* d_image,
                             void* stream) {
  if (!c || !d_slabs || !d_image) return invalid("null argument");
  int rc = check_params(p);
  if (rc) return rc;
  const FrameGeometry g = frame_geometry(p);
  const long long n = (long long)p->width * p->height;
  DEVICE_SCOPE(c->device);
  hipLaunchKernelGGL(assemble<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, d_slabs,
                     d_image, p->width, p->height, g.tile, g.tiles_x, p->shard_count > 0 ? p->shard_count : 1, g.slab);
  HIPCHK(hipGetLastError());
  return RT_OK;
}

int rt_render(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, const uint64_t* col_gens, uint8_t* out_rgb,
              double* out_lin, uint64_t* out_gens) {
  if (!c || !cam || !pin || !out_rgb) return invalid("null argument");
  rt_render_params p = *pin;  // whole image: the shard fields are ignored
  p.shard_rank = 0;
  p.shard_count = 1;
  int rc = check_params(&p);
  if (rc) return rc;
  if (!c->has_scene) {
    rt::set_error("rt_render: no scene uploaded");
    return RT_E_STATE;
  }
  if (p.rng_mode == RT_RNG_EXACT && !col_gens) return invalid("rt_render: tier A needs col_gens (2*width words)");
  for (rt_ctx* q : c->peers)
    if (!q->has_scene) {
      rt::set_error("rt_render: no scene uploaded on every device");
      return RT_E_STATE;
    }
  c->allocs = 0;
  for (rt_ctx* q : c->peers) q->allocs = 0;
  if (p.rng_mode == RT_RNG_PHILOX && !c->comms.empty()) return render_multi(c, cam, p, out_rgb, out_lin);
  DEVICE_SCOPE(c->device);
  const long long npx = (long long)p.width * p.height;
  hipStream_t st = c->stream;
  // (the ctx's frame buffers, grown on demand: repeated frames allocate nothing)
  if ((rc = grow(c, c->fb_img, (size_t)npx * 3))) return rc;
  if (out_lin && (rc = grow(c, c->fb_img_lin, sizeof(double) * (size_t)npx * 3))) return rc;
  uint8_t* d_img = (uint8_t*)c->fb_img.p;
  double* d_img_lin = out_lin ? (double*)c->fb_img_lin.p : nullptr;
  rt_frame_timing ft{};
  ft.n_devices = 1;
  if (p.rng_mode == RT_RNG_PHILOX) {
    const long long slab = frame_geometry(&p).slab;
    if ((rc = grow(c, c->fb_slab, (size_t)slab * 3))) return rc;
    if (out_lin && (rc = grow(c, c->fb_slab_lin, sizeof(double) * (size_t)slab * 3))) return rc;
    const uint8_t* slab_rgb = (const uint8_t*)c->fb_slab.p;
    const double* slab_lin = out_lin ? (const double*)c->fb_slab_lin.p : nullptr;
    rc = launch_philox(c, cam, &p, (uint8_t*)slab_rgb, (double*)slab_lin, st);
    if (!rc) rc = hip_ok(hipEventRecord(c->ev_gather, st), "hipEventRecord");
    if (!rc) rc = rt_assemble_async(c, &p, slab_rgb, d_img, st);
    if (!rc && out_lin) rc = rt_assemble_linear_async(c, &p, slab_lin, d_img_lin, st);
    if (!rc) rc = hip_ok(hipEventRecord(c->ev_asm, st), "hipEventRecord");
    HIPCHK(hipStreamSynchronize(st));
    if (rc) return rc;
    float a = 0, f = 0;
    HIPCHK(hipEventElapsedTime(&a, c->ev_gather, c->ev_asm));
    HIPCHK(hipEventElapsedTime(&f, c->ev0, c->ev_asm));
    ft.assemble_ms = a;
    ft.frame_ms = f;
  } else {
    if ((rc = grow(c, c->fb_gens, sizeof(uint64_t) * 2 * (size_t)p.width))) return rc;
    uint64_t* d_gens = (uint64_t*)c->fb_gens.p;
    HIPCHK(hipMemcpyAsync(d_gens, col_gens, sizeof(uint64_t) * 2 * (size_t)p.width, hipMemcpyHostToDevice, st));
    LaunchConst A{};
    A.S = c->scene;
    A.cam = *cam;
    A.W = p.width;
    A.H = p.height;
    A.spp = p.spp;
    A.max_depth = p.max_depth;
    A.flags = cull(c, p.flags);  // (RT_FLAG_REFERENCE_CULL)
    A.gens = d_gens;
    A.out_rgb = d_img;
    A.out_lin = d_img_lin;
    const void* fn = nullptr;
    size_t lds = 0;
    if (int rc = exact_launch(c, (p.flags & RT_FLAG_SHARED_LIBM) != 0, &fn, &lds)) return rc;
    int n_nodes = c->shape.n_nodes;
    HIPCHK(hipEventRecord(c->ev0, st));
    void* args[] = {&A, &n_nodes};
    HIPCHK(hipLaunchKernel(fn, dim3(exact_blocks(p.width)), dim3(RT_BLOCK), args, lds, st));
    HIPCHK(hipEventRecord(c->ev1, st));
    if (out_gens)
      HIPCHK(hipMemcpyAsync(out_gens, d_gens, sizeof(uint64_t) * 2 * (size_t)p.width, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
  }
  HIPCHK(hipMemcpy(out_rgb, d_img, (size_t)npx * 3, hipMemcpyDeviceToHost));
  if (out_lin) HIPCHK(hipMemcpy(out_lin, d_img_lin, sizeof(double) * (size_t)npx * 3, hipMemcpyDeviceToHost));
  float ms = 0;
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_ms = ms;
  ft.kernel_ms[0] = ms;
  if (p.rng_mode == RT_RNG_EXACT) ft.frame_ms = ms;
  ft.device_allocs = c->allocs;
  c->last_frame = ft;
  return RT_OK;
}

namespace {
int render_counting(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, uint64_t* out_work, uint64_t* out_prof) {
  if (!c || !cam || !pin || !out_work) return invalid("null argument");
  int rc = check_params(pin);
  if (rc) return rc;
  if (!c->has_scene) {
    rt::set_error("rt_render_work: no scene uploaded");
    return RT_E_STATE;
  }
  if (pin->rng_mode != RT_RNG_PHILOX) return invalid("rt_render_work: tier B only");
  DEVICE_SCOPE(c->device);
  rt_render_params p = *pin;
  const long long slab = frame_geometry(&p).slab;
  DevBuf slab_buf, work;
  HIPCHK(hipMalloc(&slab_buf.p, (size_t)slab * 3));
  HIPCHK(hipMalloc(&work.p, sizeof(unsigned long long) * (16 + 64)));
  unsigned long long* d_work = (unsigned long long*)work.p;
  HIPCHK(hipMemsetAsync(d_work, 0, sizeof(unsigned long long) * (16 + 64), c->stream));
  rc = launch_philox(c, cam, &p, (uint8_t*)slab_buf.p, nullptr, c->stream, d_work,
                     out_prof ? d_work + 16 : nullptr);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  unsigned long long w[16 + 64];
  HIPCHK(hipMemcpy(w, d_work, sizeof w, hipMemcpyDeviceToHost));
  for (int i = 0; i < 16; ++i) out_work[i] = w[i];
  if (out_prof)
    for (int i = 0; i < 64; ++i) out_prof[i] = w[16 + i];
  return RT_OK;
}
}  // namespace

int rt_render_work(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, uint64_t out_work[16]) {
  return render_counting(c, cam, pin, out_work, nullptr);
}

int rt_render_step_profile(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, uint64_t out_work[16],
                           uint64_t out_prof[64]) {
  if (!out_prof) return invalid("null argument");
  return render_counting(c, cam, pin, out_work, out_prof);
}

int rt_last_kernel_ms(rt_ctx* c, double* out_ms) {
  if (!c || !out_ms) return invalid("null argument");
  float ms = 0;
  HIPCHK(hipEventSynchronize(c->ev1));
  HIPCHK(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  c->last_ms = ms;
  *out_ms = ms;
  return RT_OK;
}

int rt_last_launch(rt_ctx* c, rt_launch_info* out) {
  if (!c || !out) return invalid("null argument");
  *out = c->last_launch;
  return RT_OK;
}

namespace {
// rt_render_features' argument checks (rt.h), before any HIP call; the ctx last, so that every other case can be
// checked without a device.
int features_check(const rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int first, int n, const double* sums) {
  if (!cam || !p || !sums) return invalid("rt_render_features: null argument");
  if (p->width <= 0 || p->height <= 0) return invalid("rt_render_features: width and height must be positive");
  if ((long long)p->width * p->height >= (1ll << 32)) return invalid("rt_render_features: a frame of 2^32 pixels or more");
  if (p->rng_mode != RT_RNG_PHILOX) return invalid("rt_render_features: tier B only (RT_RNG_PHILOX)");
  if (p->flags & RT_FLAG_SHARED_LIBM) return invalid("rt_render_features: RT_FLAG_SHARED_LIBM is a tier-A flag");
  if (p->shard_count > 1) return invalid("rt_render_features: shard_count > 1 (a feature pass covers the whole image)");
  if (first < 0 || n < 1 || (long long)first + n > INT32_MAX)
    return invalid("rt_render_features: needs first_sample >= 0, n_samples >= 1 and first_sample + n_samples <= INT32_MAX");
  if (!c) return invalid("rt_render_features: null ctx");
  if (!c->has_scene) {
    rt::set_error("rt_render_features: no scene uploaded");
    return RT_E_STATE;
  }
  return RT_OK;
}

// One feature pass over the whole image on `st`: plan (rt_launch_plan.h plan_features), the block counter back
// to 0, the kernel. The counter is the ctx's work counter, so the pass takes its place in the ctx's launch
// order: after the previous tier-B launch (ev_done), and the next one waits for it. `ch`: a chain pass (the same
// plan, rt_k_features_chain.hip's kernels, its counts zeroed in the ctx's buffer); null: a first-hit pass.
// `G`: the pass over a shard's slab (rt_render_features_shard_async): the slab forms of the same kernels
// (rt_kernels_shard.h), d_sums the slab; a shard that owns no tile queues everything but the kernel.
int launch_features(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int first, int n, int accumulate,
                    double* d_sums, hipStream_t st, const rt_feature_chain* ch = nullptr, const SlabGeometry* G = nullptr) {
  rt::FeaturePlan P;
  int rc = rt::plan_features(c->shape, *p, rt::read_knobs(), P, ch != nullptr, G ? G->blocks : -1);
  if (rc) return rc;
  const void* fn = G    ? (ch ? rt::features_chain_shard_kernel(P) : rt::features_shard_kernel(P))
                   : ch ? rt::features_chain_kernel(P)
                        : rt::features_kernel(P);
  if (ch && (rc = grow(c, c->fc_counts, 3 * sizeof(unsigned long long)))) return rc;
  if (ch && !c->ev_fc) HIPCHK(hipEventCreateWithFlags(&c->ev_fc, hipEventDisableTiming));
  if (st != c->last_stream) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
  c->last_stream = st;
  FeatureChainArgs CA{};
  FeatureArgs& A = CA.A;
  A.S = c->scene;
  A.cam = *cam;
  A.W = p->width, A.H = p->height;
  A.flags = cull(c, p->flags);
  A.seed = p->seed;
  A.first = first, A.count = n, A.accumulate = accumulate;
  A.leaf_stop = P.leaf_stop;
  A.blocks_x = (p->width + 7) / 8;
  A.blocks_total = (unsigned long long)P.info.work_items;
  A.counter = c->d_counter;
  A.sums = d_sums;
  HIPCHK(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned long long), st));
  if (ch) {
    CA.max_bounces = ch->max_bounces, CA.chain_flags = ch->flags, CA.max_fuzz = ch->max_fuzz;
    CA.counts = (unsigned long long*)c->fc_counts.p;
    HIPCHK(hipMemsetAsync(c->fc_counts.p, 0, 3 * sizeof(unsigned long long), st));
  }
  const int lds = P.info.dyn_lds_bytes;
  if (lds) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int n_items = P.n_items, entries = P.entries, n_leaves = P.n_leaves;
  // (the global-memory kernels take the first alone; a first-hit kernel the FeatureArgs at the head of `CA`, a
  // slab kernel of either pass the FeatureSlabArgs)
  FeatureSlabArgs SA{CA, G ? *G : SlabGeometry{}};
  void* args[] = {G ? (void*)&SA : ch ? (void*)&CA : (void*)&A, &n_items, &entries, &n_leaves};
  if (!G || G->blocks > 0) HIPCHK(hipLaunchKernel(fn, dim3(P.info.grid), dim3(P.info.block), args, (size_t)lds, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_done, st));
  c->last_feature = P.info;
  if (ch) {
    HIPCHK(hipEventRecord(c->ev_fc, st));
    c->fc_made = true;
    c->fc_samples = (G ? (int64_t)slab_owned_pixels(*G) : (int64_t)p->width * p->height) * n;
  }
  return RT_OK;
}

// The blocking calls' body: a device copy of the caller's sums around the pass on the ctx's stream.
int features_blocking(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* ch, int first,
                      int n, int accumulate, double* sums) {
  DEVICE_SCOPE(c->device);
  const size_t bytes = sizeof(double) * RT_FEATURE_DOUBLES * (size_t)p->width * (size_t)p->height;
  DevBuf buf;
  HIPCHK(hipMalloc(&buf.p, bytes));
  if (accumulate) HIPCHK(hipMemcpy(buf.p, sums, bytes, hipMemcpyHostToDevice));
  const int rc = launch_features(c, cam, p, first, n, accumulate, (double*)buf.p, c->stream, ch);
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  HIPCHK(hipMemcpy(sums, buf.p, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}
}  // namespace

int rt_render_features_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int first_sample,
                             int n_samples, int accumulate, double* d_sums, void* stream) {
  int rc = features_check(c, cam, p, first_sample, n_samples, d_sums);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  return launch_features(c, cam, p, first_sample, n_samples, accumulate, d_sums, (hipStream_t)stream);
}

int rt_render_features(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, int first_sample, int n_samples,
                       int accumulate, double* sums) {
  int rc = features_check(c, cam, p, first_sample, n_samples, sums);
  if (rc) return rc;
  return features_blocking(c, cam, p, nullptr, first_sample, n_samples, accumulate, sums);
}

int rt_render_features_chain_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                                   int first_sample, int n_samples, int accumulate, double* d_sums, void* stream) {
  int rc = chain_check(chain);
  if (rc || (rc = features_check(c, cam, p, first_sample, n_samples, d_sums))) return rc;
  DEVICE_SCOPE(c->device);
  return launch_features(c, cam, p, first_sample, n_samples, accumulate, d_sums, (hipStream_t)stream, chain);
}

int rt_render_features_chain(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                             int first_sample, int n_samples, int accumulate, double* sums) {
  int rc = chain_check(chain);
  if (rc || (rc = features_check(c, cam, p, first_sample, n_samples, sums))) return rc;
  return features_blocking(c, cam, p, chain, first_sample, n_samples, accumulate, sums);
}

int rt_last_feature_chain(rt_ctx* c, rt_feature_chain_stats* out) {
  if (!c || !out) return invalid("null argument");
  if (!c->fc_made) {
    rt::set_error("rt_last_feature_chain: no chain pass was made");
    return RT_E_STATE;
  }
  DEVICE_SCOPE(c->device);
  unsigned long long k[3];  // {ended_miss, ended_cap, bounces}
  HIPCHK(hipEventSynchronize(c->ev_fc));
  HIPCHK(hipMemcpy(k, c->fc_counts.p, sizeof k, hipMemcpyDeviceToHost));
  out->samples = c->fc_samples;
  out->ended_miss = (int64_t)k[0], out->ended_cap = (int64_t)k[1], out->bounces = (int64_t)k[2];
  out->ended_surface = out->samples - out->ended_miss - out->ended_cap;
  return RT_OK;
}

// ------------------------------------------------------------------ material-ID coverage buffers (rt.h)
namespace {
// rt_render_ids' argument checks: the chain's when there is one, then the feature pass's (the ctx last).
int ids_check(const rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* ch, int first,
              int n, const rt_id_record* recs) {
  int rc = ch ? chain_check(ch) : RT_OK;
  if (!rc) rc = features_check(c, cam, p, first, n, reinterpret_cast<const double*>(recs));
  if (rc) {  // (the shared checks name the feature passes)
    std::string msg = rt::last_error();
    const size_t colon = msg.find(": ");
    rt::set_error("rt_render_ids" + (colon == std::string::npos ? ": " + msg : msg.substr(colon)));
  }
  return rc;
}

// launch_features for an id pass: the same plan (a staged pass at the chain passes' 3 waves per SIMD: its kernels
// hold the same walk and chain state), rt_k_ids.hip's kernel, the same place in the ctx's launch order. One kernel
// for both modes: without a chain it runs with max_bounces = 0 and counts nothing.
// `G`: over a shard's slab, as launch_features.
int launch_ids(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* ch, int first, int n,
               int accumulate, rt_id_record* d_recs, hipStream_t st, const SlabGeometry* G = nullptr) {
  rt::FeaturePlan P;
  int rc = rt::plan_features(c->shape, *p, rt::read_knobs(), P, true, G ? G->blocks : -1);
  if (rc) return rc;
  const void* fn = G ? rt::ids_shard_kernel(P) : rt::ids_kernel(P);
  if (ch && (rc = grow(c, c->fc_counts, 3 * sizeof(unsigned long long)))) return rc;
  if (ch && !c->ev_fc) HIPCHK(hipEventCreateWithFlags(&c->ev_fc, hipEventDisableTiming));
  if (st != c->last_stream) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
  c->last_stream = st;
  IdArgs CA{};
  FeatureArgs& A = CA.A;
  A.S = c->scene;
  A.cam = *cam;
  A.W = p->width, A.H = p->height;
  A.flags = cull(c, p->flags);
  A.seed = p->seed;
  A.first = first, A.count = n, A.accumulate = accumulate;
  A.leaf_stop = P.leaf_stop;
  A.blocks_x = (p->width + 7) / 8;
  A.blocks_total = (unsigned long long)P.info.work_items;
  A.counter = c->d_counter;
  A.sums = reinterpret_cast<double*>(d_recs);  // (64 bytes per pixel, as a feature vector)
  HIPCHK(hipMemsetAsync(c->d_counter, 0, sizeof(unsigned long long), st));
  if (ch) {
    CA.max_bounces = ch->max_bounces, CA.chain_flags = ch->flags, CA.max_fuzz = ch->max_fuzz;
    CA.counts = (unsigned long long*)c->fc_counts.p;
    HIPCHK(hipMemsetAsync(c->fc_counts.p, 0, 3 * sizeof(unsigned long long), st));
  }
  const int lds = P.info.dyn_lds_bytes;
  if (lds) HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  int n_items = P.n_items, entries = P.entries, n_leaves = P.n_leaves;
  FeatureSlabArgs SA{CA, G ? *G : SlabGeometry{}};
  void* args[] = {G ? (void*)&SA : (void*)&CA, &n_items, &entries, &n_leaves};  // (the global-memory kernels take the first alone)
  if (!G || G->blocks > 0) HIPCHK(hipLaunchKernel(fn, dim3(P.info.grid), dim3(P.info.block), args, (size_t)lds, st));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(c->ev_done, st));
  c->last_feature = P.info;
  if (ch) {
    HIPCHK(hipEventRecord(c->ev_fc, st));
    c->fc_made = true;
    c->fc_samples = (G ? (int64_t)slab_owned_pixels(*G) : (int64_t)p->width * p->height) * n;
  }
  return RT_OK;
}

// rt_ids_matte*'s and rt_ids_preview*'s argument checks, before any HIP call; the ctx last.
int ids_resolve_check(const char* what, const rt_ctx* c, int64_t pixels, bool pointers, const uint32_t* ids, int n_ids,
                      bool list) {
  const char* bad = list ? rt::ids_list_error(ids, n_ids) : nullptr;
  if (!bad && !pointers) bad = "null records or no output";
  if (!bad && (pixels < 1 || pixels >= (1ll << 32))) bad = "pixels must be in 1..2^32-1";
  if (!bad && !c) bad = "null ctx";
  return bad ? invalid(std::string(what) + ": " + bad) : RT_OK;
}

// A matte (ids non-null) or a preview queued on `st` over device pointers, in the ctx's launch order like a
// feature pass. The list goes through the ctx's staging buffer, which the ordering keeps for this call until its
// kernel has run; the copy from the caller's pageable array has left it when hipMemcpyAsync returns.
int ids_resolve_queue(rt_ctx* c, const rt_id_record* d_recs, int64_t pixels, const uint32_t* ids, int n_ids,
                      double* d_cov, uint8_t* d_u8, hipStream_t st) {
  int rc;
  if (ids && (rc = grow(c, c->id_list, sizeof(uint32_t) * RT_ID_MATTE_MAX))) return rc;
  if (st != c->last_stream) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
  c->last_stream = st;
  int e;
  if (ids) {
    HIPCHK(hipMemcpyAsync(c->id_list.p, ids, sizeof(uint32_t) * (size_t)n_ids, hipMemcpyHostToDevice, st));
    e = rt::ids_matte_launch(d_recs, pixels, (const uint32_t*)c->id_list.p, n_ids, d_cov, d_u8, (void*)st);
  } else {
    e = rt::ids_preview_launch(d_recs, pixels, d_u8, (void*)st);
  }
  if (e) return hip_fail((hipError_t)e, "rt_ids resolve launch");
  HIPCHK(hipEventRecord(c->ev_done, st));
  return RT_OK;
}

// The blocking variants: the records up, the kernel on the ctx's stream, the outputs back, in the ctx's buffers.
int ids_resolve_blocking(rt_ctx* c, const rt_id_record* recs, int64_t pixels, const uint32_t* ids, int n_ids,
                         double* out_cov, uint8_t* out_u8) {
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  const size_t npx = (size_t)pixels, u8_bytes = ids ? npx : 3 * npx;
  int rc;
  if ((rc = grow(c, c->id_recs, sizeof(rt_id_record) * npx)) || (out_cov && (rc = grow(c, c->id_cov, sizeof(double) * npx))) ||
      (out_u8 && (rc = grow(c, c->id_u8, u8_bytes))))
    return rc;
  HIPCHK(hipMemcpy(c->id_recs.p, recs, sizeof(rt_id_record) * npx, hipMemcpyHostToDevice));
  rc = ids_resolve_queue(c, (const rt_id_record*)c->id_recs.p, pixels, ids, n_ids, out_cov ? (double*)c->id_cov.p : nullptr,
                         out_u8 ? (uint8_t*)c->id_u8.p : nullptr, c->stream);
  c->id_allocs = c->allocs;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  if (out_cov) HIPCHK(hipMemcpy(out_cov, c->id_cov.p, sizeof(double) * npx, hipMemcpyDeviceToHost));
  if (out_u8) HIPCHK(hipMemcpy(out_u8, c->id_u8.p, u8_bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}
}  // namespace

int rt_render_ids_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                        int first_sample, int n_samples, int accumulate, rt_id_record* d_records, void* stream) {
  int rc = ids_check(c, cam, p, chain, first_sample, n_samples, d_records);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  rc = launch_ids(c, cam, p, chain, first_sample, n_samples, accumulate, d_records, (hipStream_t)stream);
  c->id_allocs = c->allocs;
  return rc;
}

int rt_render_ids(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                  int first_sample, int n_samples, int accumulate, rt_id_record* records) {
  int rc = ids_check(c, cam, p, chain, first_sample, n_samples, records);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  const size_t bytes = sizeof(rt_id_record) * (size_t)p->width * (size_t)p->height;
  if ((rc = grow(c, c->id_recs, bytes))) return rc;
  if (accumulate) HIPCHK(hipMemcpy(c->id_recs.p, records, bytes, hipMemcpyHostToDevice));
  rc = launch_ids(c, cam, p, chain, first_sample, n_samples, accumulate, (rt_id_record*)c->id_recs.p, c->stream);
  c->id_allocs = c->allocs;
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  HIPCHK(hipMemcpy(records, c->id_recs.p, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_ids_matte_async(rt_ctx* c, const rt_id_record* d_recs, int64_t pixels, const uint32_t* ids, int n_ids,
                       double* d_out_cov, uint8_t* d_out_u8, void* stream) {
  int rc = ids_resolve_check("rt_ids_matte_async", c, pixels, d_recs && (d_out_cov || d_out_u8), ids, n_ids, true);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  rc = ids_resolve_queue(c, d_recs, pixels, ids, n_ids, d_out_cov, d_out_u8, (hipStream_t)stream);
  c->id_allocs = c->allocs;
  return rc;
}

int rt_ids_matte(rt_ctx* c, const rt_id_record* recs, int64_t pixels, const uint32_t* ids, int n_ids, double* out_cov,
                 uint8_t* out_u8) {
  int rc = ids_resolve_check("rt_ids_matte", c, pixels, recs && (out_cov || out_u8), ids, n_ids, true);
  return rc ? rc : ids_resolve_blocking(c, recs, pixels, ids, n_ids, out_cov, out_u8);
}

int rt_ids_preview_async(rt_ctx* c, const rt_id_record* d_recs, int64_t pixels, uint8_t* d_out_rgb8, void* stream) {
  int rc = ids_resolve_check("rt_ids_preview_async", c, pixels, d_recs && d_out_rgb8, nullptr, 0, false);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  rc = ids_resolve_queue(c, d_recs, pixels, nullptr, 0, nullptr, d_out_rgb8, (hipStream_t)stream);
  c->id_allocs = c->allocs;
  return rc;
}

int rt_ids_preview(rt_ctx* c, const rt_id_record* recs, int64_t pixels, uint8_t* out_rgb8) {
  int rc = ids_resolve_check("rt_ids_preview", c, pixels, recs && out_rgb8, nullptr, 0, false);
  return rc ? rc : ids_resolve_blocking(c, recs, pixels, nullptr, 0, nullptr, out_rgb8);
}

// Internal (rt_internal.h): hipMalloc calls the ctx's last rt_render_ids*, rt_ids_matte* or rt_ids_preview* made.
int rt_internal_ids_allocs(rt_ctx* c) { return c ? c->id_allocs : -1; }

// Internal (rt_internal.h; no device needed): the plan an id pass would launch with.
int rt_internal_ids_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count, const rt_render_params* p,
                         const rt_feature_chain* chain, rt_launch_info* out, int32_t* out_extra) {
  const int rc = chain ? chain_check(chain) : RT_OK;
  return rc ? rc : features_plan(desc, upload_flags, cu_count, p, true, out, out_extra);
}

int rt_last_feature_launch(rt_ctx* c, rt_launch_info* out) {
  if (!c || !out) return invalid("null argument");
  *out = c->last_feature;
  return RT_OK;
}

// ------------------------------------------------------------------ sharded feature and ID passes (rt.h)
namespace {
// The slab passes' argument checks, before any HIP call; the ctx last, as features_check. What the image-order
// entries reject other than shard_count > 1, the chain's when there is one, and the shard geometry's.
int features_shard_check(const char* what, const rt_ctx* c, const rt_camera* cam, const rt_render_params* p,
                         const rt_feature_chain* ch, int first, int n, const void* d_slab) {
  const std::string w = std::string(what) + ": ";
  if (ch) {
    const int rc = chain_check(ch);
    if (rc) {  // (chain_check names the chain pass)
      const std::string msg = rt::last_error();
      const size_t colon = msg.find(": ");
      return invalid(w + (colon == std::string::npos ? msg : msg.substr(colon + 2)));
    }
  }
  if (!cam || !p || !d_slab) return invalid(w + "null argument");
  if (const char* bad = slab_params_error(p)) return invalid(w + bad);
  if (p->rng_mode != RT_RNG_PHILOX) return invalid(w + "tier B only (RT_RNG_PHILOX)");
  if (p->flags & RT_FLAG_SHARED_LIBM) return invalid(w + "RT_FLAG_SHARED_LIBM is a tier-A flag");
  if (first < 0 || n < 1 || (long long)first + n > INT32_MAX)
    return invalid(w + "needs first_sample >= 0, n_samples >= 1 and first_sample + n_samples <= INT32_MAX");
  if (!c) return invalid(w + "null ctx");
  if (!c->has_scene) {
    rt::set_error(w + "no scene uploaded");
    return RT_E_STATE;
  }
  return RT_OK;
}
}  // namespace

int rt_render_features_shard_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                                   int first_sample, int n_samples, int accumulate, double* d_slab_sums, void* stream) {
  int rc = features_shard_check("rt_render_features_shard_async", c, cam, p, chain, first_sample, n_samples, d_slab_sums);
  if (rc) return rc;
  const SlabGeometry G = slab_geometry(p);
  DEVICE_SCOPE(c->device);
  return launch_features(c, cam, p, first_sample, n_samples, accumulate, d_slab_sums, (hipStream_t)stream, chain, &G);
}

int rt_render_ids_shard_async(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, const rt_feature_chain* chain,
                              int first_sample, int n_samples, int accumulate, rt_id_record* d_slab_records, void* stream) {
  int rc = features_shard_check("rt_render_ids_shard_async", c, cam, p, chain, first_sample, n_samples, d_slab_records);
  if (rc) return rc;
  const SlabGeometry G = slab_geometry(p);
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  rc = launch_ids(c, cam, p, chain, first_sample, n_samples, accumulate, d_slab_records, (hipStream_t)stream, &G);
  c->id_allocs = c->allocs;
  return rc;
}

int rt_assemble_records_async(rt_ctx* c, const rt_render_params* p, const void* d_slabs, void* d_image, void* stream) {
  if (!p || !d_slabs || !d_image) return invalid("rt_assemble_records_async: null argument");
  if (const char* bad = slab_params_error(p)) return invalid(std::string("rt_assemble_records_async: ") + bad);
  if (!c) return invalid("rt_assemble_records_async: null ctx");
  SlabGeometry G = slab_geometry(p);
  G.shard_rank = 0;
  DEVICE_SCOPE(c->device);  // (the caller's current device may be another ctx's)
  const int e = rt::assemble_records_launch(G, d_slabs, d_image, stream);
  if (e) return hip_fail((hipError_t)e, "rt_assemble_records_async launch");
  return RT_OK;
}

// Internal (rt_internal.h; no device needed): the plan a slab pass of shard (p->tile, p->shard_rank, p->shard_count)
// would launch with.
int rt_internal_features_shard_plan(const rt_scene_desc* desc, uint32_t upload_flags, int cu_count, const rt_render_params* p,
                                    int chain, rt_launch_info* out, int32_t* out_extra) {
  if (!p) return invalid("null argument");
  if (const char* bad = slab_params_error(p)) return invalid(std::string("rt_internal_features_shard_plan: ") + bad);
  return features_plan(desc, upload_flags, cu_count, p, chain != 0, out, out_extra, slab_geometry(p).blocks);
}

int rt_debug_wide_keys(rt_ctx* c, int out[4]) {
  if (!c || !out) return invalid("null argument");
  out[0] = c->last_wide_packed;
  out[1] = c->has_scene && c->d_wnodes && rt_wkey_fits(c->shape.n_wnodes, c->shape.n_leaves);
  out[2] = RT_WKEY_BITS;
  out[3] = kLdsMaxWideNodes;
  return RT_OK;
}

}  // extern "C"

// ------------------------------------------------------------------ progressive frames (rt.h)
namespace {

int state_error(const std::string& s) {
  rt::set_error(s);
  return RT_E_STATE;
}

// A frame that may still be advanced, resolved and saved: its ctx holds the scene it was opened on.
int frame_live(const rt_frame* f, const char* what) {
  if (!f) return invalid(std::string(what) + ": null frame");
  if (!f->valid || !f->ctx->has_scene)
    return state_error(std::string(what) + ": the ctx's scene was replaced (or a launch failed) since the frame was opened");
  return RT_OK;
}

// (the ctx's device is selected)
void frame_free(rt_frame* f) {
  (void)hipFree(f->d_sum);
  (void)hipFree(f->d_rgb);
  (void)hipFree(f->d_lin);
  (void)hipFree(f->d_stage);
  (void)hipFree(f->d_counts);
  (void)hipFree(f->d_q);
  (void)hipFree(f->d_se);
  (void)hipFree(f->d_err);
  (void)hipFree(f->d_kp);
  (void)hipFree(f->d_skip);
  (void)hipFree(f->d_adapt);
  (void)hipFree(f->d_mask);
  (void)hipFree(f->d_kimg);
  for (auto& e : f->events) {
    (void)hipEventDestroy(e.first);
    (void)hipEventDestroy(e.second);
  }
  delete f;
}

// Image pixels in the slab of shard (p.shard_rank, p.shard_count): its tiles, clipped to the image.
long long owned_pixels(const rt_render_params& p) {
  const FrameGeometry g = frame_geometry(&p);
  const int shards = p.shard_count > 0 ? p.shard_count : 1;
  long long n = 0;
  for (long long gt = p.shard_rank; gt < g.tiles_total; gt += shards) {
    const long long ty = gt / g.tiles_x, tx = gt % g.tiles_x;
    n += std::min<long long>(g.tile, p.width - tx * g.tile) * std::min<long long>(g.tile, p.height - ty * g.tile);
  }
  return n;
}

// Image-order calls take unsharded frames, the _shard calls shard frames (rt.h): RT_E_STATE otherwise,
// naming the call to use instead.
int frame_kind(const rt_frame* f, bool shard, const char* what, const char* instead) {
  if (f->shard == shard) return RT_OK;
  return state_error(std::string(what) + (shard ? ": not a shard frame (rt_frame_open_shard); use "
                                                : ": a shard frame keeps slab order; use ") + instead);
}

// The header of the frame's whole-image version-1 blob (rt.h): a shard frame's is the unsharded frame's,
// its shard fields written as 0 / 1.
rt_frame_blob_desc frame_blob_desc(const rt_frame* f) {
  rt_frame_blob_desc b{};
  b.version = RT_FRAME_BLOB_VERSION;
  b.upload_flags = f->ctx->upload_flags;
  b.params = f->p;
  b.params.shard_rank = 0;
  b.params.shard_count = 1;
  b.camera = f->cam;
  b.chunk = f->chunk;
  b.chunks_done = f->chunks_done;
  b.pixels = f->npx;
  b.scene_fingerprint = f->ctx->fingerprint;
  b.payload_bytes = sizeof(double) * 3 * (size_t)f->npx;
  return b;
}
void frame_write_header(const rt_frame* f, uint8_t* buf) { rt::blob_write_header(frame_blob_desc(f), buf); }

// The sections of the frame's own checkpoint (rt.h): Q when it tracks moments, K when a pixel is stopped.
uint32_t frame_sections(const rt_frame* f) {
  return (f->d_q ? RT_CKPT_MOMENTS : 0u) | (f->stopped_nan + f->stopped_other > 0 ? RT_CKPT_STOPS : 0u);
}

// The frame's geometry and sums in launch constants, for its frame_* helper kernels (rt_kernels.h): the
// frame's own shard, an unsharded frame being shard 0 of 1.
void frame_const(const rt_frame* f, LaunchConst& A) {
  fill_frame_geometry(A, &f->p, rt::chunk_knob());
  A.chunk = f->chunk;  // (rt.h's, whatever RTAMD_CHUNK says: frame_new refuses the override)
  A.acc = f->d_sum;
}

// The samples in the frame's sums so far (the last chunk may be short).
int frame_samples(const rt_frame* f) {
  return (int)std::min<long long>(f->p.spp, (long long)f->chunks_done * f->chunk);
}

// Threads of a frame_* helper launch: one per pixel of the frame's order (image, or a shard frame's slab).
long long frame_threads(const rt_frame* f) { return f->shard ? f->slab : f->npx; }
dim3 frame_grid(const rt_frame* f) { return dim3((unsigned)((frame_threads(f) + 255) / 256)); }

// The frame's order selects the helper kernel's instantiation: FRAME_KERNEL(f, frame_scatter, args...); for
// frame_resolve and frame_error so does whether a stop call has given it a kp (FRAME_KERNEL_ADAPT).
#define FRAME_LAUNCH(f, kernel, ...) \
  hipLaunchKernelGGL((kernel), frame_grid(f), dim3(256), 0, (f)->ctx->stream, __VA_ARGS__)
#define FRAME_KERNEL(f, kernel, ...)                 \
  do {                                               \
    if ((f)->shard)                                  \
      FRAME_LAUNCH(f, kernel<true>, __VA_ARGS__);    \
    else                                             \
      FRAME_LAUNCH(f, kernel<false>, __VA_ARGS__);   \
  } while (0)
#define FRAME_KERNEL_ADAPT(f, kernel, ...)                  \
  do {                                                      \
    if ((f)->shard && (f)->d_kp)                            \
      FRAME_LAUNCH(f, (kernel<true, true>), __VA_ARGS__);   \
    else if ((f)->shard)                                    \
      FRAME_LAUNCH(f, (kernel<true, false>), __VA_ARGS__);  \
    else if ((f)->d_kp)                                     \
      FRAME_LAUNCH(f, (kernel<false, true>), __VA_ARGS__);  \
    else                                                    \
      FRAME_LAUNCH(f, (kernel<false, false>), __VA_ARGS__); \
  } while (0)

// A new preview in the frame's own buffers (d_rgb, d_lin) and its counts in f->last (the ctx's device is
// selected, a chunk has been rendered since the last resolve).
int frame_resolve_run(rt_frame* f) {
  rt_ctx* c = f->ctx;
  LaunchConst A{};
  frame_const(f, A);
  A.out_rgb = f->d_rgb;
  A.out_lin = f->d_lin;
  const int samples = frame_samples(f);
  HIPCHK(hipMemsetAsync(f->d_counts, 0, 2 * sizeof(unsigned long long), c->stream));
  // (an adapted frame: each stopped pixel over its own N_p = min(spp, K_p * CH))
  FRAME_KERNEL_ADAPT(f, frame_resolve, A, samples, f->d_counts, (const int*)f->d_kp);
  HIPCHK(hipGetLastError());
  unsigned long long counts[2] = {0, 0};  // (copied in stream order: one wait for the kernel and the counts)
  HIPCHK(hipMemcpyAsync(counts, f->d_counts, sizeof counts, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  double ms = 0.0;
  for (size_t i = 0; i < f->used; ++i) {
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, f->events[i].first, f->events[i].second));
    ms += t;
  }
  f->used = 0;
  f->last.chunks_done = f->chunks_done;
  f->last.samples_done = samples;
  f->last.kernel_ms = ms;
  f->last.nan_pixels = (int64_t)counts[0];
  f->last.bytes_changed = (int64_t)counts[1];
  return RT_OK;
}

// The frame's error summary over its `pixels` image pixels in `out` (may be null) and, when `d_se` is given,
// its se map there in the frame's order (device memory). The ctx's device is selected; returns after the
// stream is drained.
int frame_error_run(rt_frame* f, double abs_tol, double rel_tol, double* d_se, long long pixels, rt_error_stats* out) {
  rt_ctx* c = f->ctx;
  const int blocks = (int)frame_grid(f).x;
  if (!f->d_err) HIPCHK(hipMalloc((void**)&f->d_err, sizeof(unsigned long long) * (4 + (size_t)blocks)));
  LaunchConst A{};
  frame_const(f, A);
  const int chunks = f->chunks_done, samples = frame_samples(f);
  unsigned long long* d_acc = f->d_err;
  double *d_block = reinterpret_cast<double*>(f->d_err + 4), *d_total = reinterpret_cast<double*>(f->d_err + 3);
  HIPCHK(hipMemsetAsync(d_acc, 0, 4 * sizeof(unsigned long long), c->stream));
  // (an adapted frame: each stopped pixel at its own (K_p, N_p))
  FRAME_KERNEL_ADAPT(f, frame_error, A, (const double*)f->d_q, d_se, chunks, samples, abs_tol, rel_tol, d_acc,
                     d_block, (const int*)f->d_kp);
  HIPCHK(hipGetLastError());
  hipLaunchKernelGGL(frame_error_sum, dim3(1), dim3(256), 0, c->stream, (const double*)d_block, blocks, d_total);
  HIPCHK(hipGetLastError());
  unsigned long long acc[4] = {0, 0, 0, 0};  // (copied in stream order: one wait for the kernels and the summary)
  HIPCHK(hipMemcpyAsync(acc, d_acc, sizeof acc, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  if (out) {
    rt_error_stats st{};
    st.chunks_done = chunks;
    st.samples_done = samples;
    st.pixels = (int64_t)pixels;
    st.nonfinite_pixels = (int64_t)acc[0];
    st.unconverged_pixels = (int64_t)acc[1];
    double total;
    std::memcpy(&st.max_se, &acc[2], sizeof(double));
    std::memcpy(&total, &acc[3], sizeof(double));
    const int64_t finite = st.pixels - st.nonfinite_pixels;
    st.mean_se = finite ? total / (double)(3 * finite) : 0.0;
    *out = st;
  }
  return RT_OK;
}

// One of the frame's slab-order buffers (sums, moments) in image order, through the frame's kept stage
// buffer, to the caller's host memory (an unsharded frame; the ctx's device is selected).
int frame_image_out(rt_frame* f, const double* d_src, void* out) {
  rt_ctx* c = f->ctx;
  const size_t bytes = sizeof(double) * 3 * (size_t)f->npx;
  if (!f->d_stage) HIPCHK(hipMalloc((void**)&f->d_stage, bytes));  // (kept: a checkpoint per step allocates once)
  LaunchConst A{};
  frame_const(f, A);
  hipLaunchKernelGGL(assemble<double>, dim3((unsigned)((f->npx + 255) / 256)), dim3(256), 0, c->stream, d_src,
                     f->d_stage, A.W, A.H, A.tile, A.tiles_x, 1, A.slab);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, f->d_stage, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

// A frame of `p` on c with zero sums and a zero previous preview, registered on the ctx; with
// RT_FRAME_MOMENTS in `frame_flags`, zero second moments too.
int frame_new(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, uint32_t frame_flags, const char* what,
              rt_frame** out, bool shard = false) {
  if (frame_flags & ~RT_FRAME_MOMENTS) return invalid(std::string(what) + ": unknown frame flag");
  rt_render_params p = *pin;  // whole image: the shard fields are ignored
  if (!shard) {
    p.shard_rank = 0;
    p.shard_count = 1;
  }
  int rc = check_params(&p);
  if (!rc && shard && p.shard_count == 0) p.shard_count = 1;  // (0 means unsharded, as in rt_shard_geometry)
  if (rc) return rc;
  if (p.rng_mode != RT_RNG_PHILOX)
    return unsupported(std::string(what) + ": progressive frames are tier B (RT_RNG_PHILOX) only");
  if (std::getenv("RTAMD_CHUNK")) return unsupported(std::string(what) + ": RTAMD_CHUNK overrides rt.h's chunk size");
  if (!c->has_scene) return state_error(std::string(what) + ": no scene uploaded");
  DEVICE_SCOPE(c->device);
  rt_frame* f = new rt_frame();
  f->ctx = c;
  f->cam = *cam;
  f->p = p;
  f->slab = frame_geometry(&p).slab;
  f->npx = (long long)p.width * p.height;
  f->shard = shard;
  f->owned = shard ? owned_pixels(p) : f->npx;
  f->chunk = rt_sample_chunk((int64_t)f->npx, p.spp);
  f->chunks_total = (p.spp + f->chunk - 1) / f->chunk;
  f->last.chunk = f->chunk;
  f->last.chunks_total = f->chunks_total;
  f->last.chunks_done = -1;  // (no resolve yet)
  auto init = [&]() -> int {
    // (a shard frame's previews are slab order; their padding slots are zeroed once and never written)
    const size_t sums = sizeof(double) * 3 * (size_t)f->slab, img = (size_t)(shard ? f->slab : f->npx) * 3;
    HIPCHK(hipMalloc((void**)&f->d_sum, sums));
    HIPCHK(hipMalloc((void**)&f->d_rgb, img));
    HIPCHK(hipMalloc((void**)&f->d_lin, sizeof(double) * img));
    HIPCHK(hipMalloc((void**)&f->d_counts, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMemsetAsync(f->d_sum, 0, sums, c->stream));
    HIPCHK(hipMemsetAsync(f->d_rgb, 0, img, c->stream));
    if (shard) HIPCHK(hipMemsetAsync(f->d_lin, 0, sizeof(double) * img, c->stream));
    if (frame_flags & RT_FRAME_MOMENTS) {
      HIPCHK(hipMalloc((void**)&f->d_q, sums));
      HIPCHK(hipMemsetAsync(f->d_q, 0, sums, c->stream));
    }
    return RT_OK;
  };
  if ((rc = init())) {
    frame_free(f);
    return rc;
  }
  c->frames.push_back(f);
  *out = f;
  return RT_OK;
}

// One stop call of an adaptive frame (rt_frame_adapt: `rule`; rt_frame_stop: the caller's `mask`, image
// order): the first one allocates K_p and the skip bitmask (zeroed: every pixel active), the kernel stops
// pixels at the frame's current chunks_done, and the host keeps the exact totals.
int frame_stop_call(rt_frame* f, const rt_adapt_rule* rule, const uint8_t* mask, const char* what,
                    rt_adapt_stats* out) {
  int rc = frame_live(f, what);
  if (rc) return rc;
  if (f->chunks_done == 0) return state_error(std::string(what) + ": no chunk rendered yet");
  if (rule && (rule->flags & RT_ADAPT_CONVERGED) && !f->d_q)
    return state_error(std::string(what) + ": RT_ADAPT_CONVERGED needs a frame opened with RT_FRAME_MOMENTS");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  const size_t words = (size_t)(f->slab / 64);  // (the slab is whole 8x8 blocks)
  if (!f->d_skip) {  // (the mask last: advance, resolve and error take the adaptive path once it is there)
    if (!f->d_adapt) HIPCHK(hipMalloc((void**)&f->d_adapt, 2 * sizeof(unsigned long long)));
    if (!f->d_kp) HIPCHK(hipMalloc((void**)&f->d_kp, sizeof(int) * (size_t)f->slab));
    HIPCHK(hipMemsetAsync(f->d_kp, 0, sizeof(int) * (size_t)f->slab, c->stream));
    HIPCHK(hipMalloc((void**)&f->d_skip, sizeof(unsigned long long) * words));
    HIPCHK(hipMemsetAsync(f->d_skip, 0, sizeof(unsigned long long) * words, c->stream));
  }
  LaunchConst A{};
  frame_const(f, A);
  int K = f->chunks_done, N = frame_samples(f);
  unsigned long long* d_counts = f->d_adapt;
  HIPCHK(hipMemsetAsync(d_counts, 0, 2 * sizeof(unsigned long long), c->stream));
  const dim3 grid((unsigned)((f->slab + 255) / 256));
  if (rule) {
    hipLaunchKernelGGL(frame_adapt, grid, dim3(256), 0, c->stream, A, (const double*)f->d_q, f->d_kp, f->d_skip, K, N,
                       *rule, d_counts);
  } else {
    if (!f->d_mask) HIPCHK(hipMalloc((void**)&f->d_mask, (size_t)f->npx));
    HIPCHK(hipMemcpyAsync(f->d_mask, mask, (size_t)f->npx, hipMemcpyHostToDevice, c->stream));
    hipLaunchKernelGGL(frame_stop_mask, grid, dim3(256), 0, c->stream, A, f->d_kp, f->d_skip,
                       (const uint8_t*)f->d_mask, K, d_counts);
  }
  HIPCHK(hipGetLastError());
  unsigned long long counts[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(counts, d_counts, sizeof counts, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipStreamSynchronize(c->stream));
  f->stopped_nan += (long long)counts[1];
  f->stopped_other += (long long)(counts[0] - counts[1]);
  if (out) {
    rt_adapt_stats st{};
    st.chunks_done = f->chunks_done;
    st.pixels = (int64_t)f->owned;
    st.stopped_nan = f->stopped_nan;
    st.stopped_converged_or_masked = f->stopped_other;
    st.active_pixels = st.pixels - st.stopped_nan - st.stopped_converged_or_masked;
    st.stopped_now = (int64_t)counts[0];
    *out = st;
  }
  return RT_OK;
}

// A frame from a parsed blob `b` (either version), its image-order sums and image-order moments (may be null:
// an untracked frame), in the caller's memory: the scene checks, a new frame of the blob's parameters (a shard
// frame: `p`'s shard of them), then the sums and the moments, the same size and order, each staged on the
// device and scattered into the frame's slab order. An unsharded frame keeps the stage buffer for later
// saves; a shard frame keeps no image-order buffer.
// `stops` (a version-2 checkpoint's K section with a nonzero entry, image order like the other two; else null)
// makes the frame an adapted one: K_p and the skip bitmask are allocated as a first stop call allocates them,
// K is staged the same way, and frame_restore_stops fills both and counts the stopped pixels by their sums.
int frame_from(rt_ctx* c, const rt_frame_blob_desc& b, const void* sums, const void* moments, const void* stops,
               bool shard, int shard_rank, int shard_count, const char* what, rt_frame** out) {
  int rc;
  if (!c->has_scene) return state_error(std::string(what) + ": no scene uploaded");
  if (b.scene_fingerprint != c->fingerprint || b.upload_flags != c->upload_flags)
    return state_error(std::string(what) + ": the blob was saved over another scene (fingerprint or upload flags differ)");
  rt_render_params p = b.params;  // (the blob's tile; the shard is the caller's: frame_new ignores it unsharded)
  p.shard_rank = shard_rank;
  p.shard_count = shard_count;
  rt_frame* f = nullptr;
  if ((rc = frame_new(c, &b.camera, &p, moments ? RT_FRAME_MOMENTS : 0u, what, &f, shard))) return rc;
  auto fill = [&]() -> int {
    DEVICE_SCOPE(c->device);
    const size_t bytes = sizeof(double) * 3 * (size_t)b.pixels;
    DevBuf tmp;  // (a shard frame's stage: the whole image, once per restore)
    HIPCHK(hipMalloc(shard ? &tmp.p : (void**)&f->d_stage, bytes));
    double* stage = shard ? (double*)tmp.p : f->d_stage;
    LaunchConst A{};
    frame_const(f, A);
    const void* src[2] = {sums, moments};
    double* dst[2] = {f->d_sum, f->d_q};
    for (int i = 0; i < (moments ? 2 : 1); ++i) {
      HIPCHK(hipMemcpy(stage, src[i], bytes, hipMemcpyHostToDevice));
      FRAME_KERNEL(f, frame_scatter, A, (const double*)stage, dst[i]);
      HIPCHK(hipGetLastError());
      HIPCHK(hipStreamSynchronize(c->stream));
    }
    if (!stops) return RT_OK;
    const size_t words = (size_t)(f->slab / 64);  // (the slab is whole 8x8 blocks)
    HIPCHK(hipMalloc((void**)&f->d_adapt, 2 * sizeof(unsigned long long)));
    HIPCHK(hipMalloc((void**)&f->d_kp, sizeof(int) * (size_t)f->slab));
    HIPCHK(hipMalloc((void**)&f->d_skip, sizeof(unsigned long long) * words));
    HIPCHK(hipMemsetAsync(f->d_adapt, 0, 2 * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(f->d_kp, 0, sizeof(int) * (size_t)f->slab, c->stream));
    HIPCHK(hipMemsetAsync(f->d_skip, 0, sizeof(unsigned long long) * words, c->stream));
    // (K is a sixth of a sums section's bytes: the same stage holds it; the scatters above are drained)
    HIPCHK(hipMemcpy(stage, stops, sizeof(int) * (size_t)b.pixels, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(frame_restore_stops, dim3((unsigned)((f->slab + 255) / 256)), dim3(256), 0, c->stream, A,
                       (const int*)stage, f->d_kp, f->d_skip, f->d_adapt);
    HIPCHK(hipGetLastError());
    unsigned long long counts[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(counts, f->d_adapt, sizeof counts, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    f->stopped_nan = (long long)counts[1];
    f->stopped_other = (long long)(counts[0] - counts[1]);
    return RT_OK;
  };
  if ((rc = fill())) {
    rt_frame_close(f);
    return rc;
  }
  f->chunks_done = b.chunks_done;
  *out = f;
  return RT_OK;
}

int frame_restore_run(rt_ctx* c, const void* buf, size_t len, const double* moments, bool shard, int shard_rank,
                      int shard_count, const char* what, rt_frame** out) {
  rt_frame_blob_desc b;
  int rc = rt_frame_blob_info(buf, len, &b);
  if (rc) return rc;
  return frame_from(c, b, (const uint8_t*)buf + RT_FRAME_BLOB_HEADER, moments, nullptr, shard, shard_rank, shard_count,
                    what, out);
}

// rt_frame_resume*: a frame from a version-1 or version-2 blob, with the sections it has.
int frame_resume_run(rt_ctx* c, const void* buf, size_t len, bool shard, int shard_rank, int shard_count,
                     const char* what, rt_frame** out) {
  rt_frame_ckpt_desc d;
  int rc = rt_frame_checkpoint_info(buf, len, &d);
  if (rc) return rc;
  const uint8_t* in = (const uint8_t*)buf;
  return frame_from(c, d.blob, in + d.sums_offset, d.moments_offset ? in + d.moments_offset : nullptr,
                    d.stopped_pixels > 0 ? in + d.stops_offset : nullptr, shard, shard_rank, shard_count, what, out);
}

}  // namespace

extern "C" {

int rt_frame_open(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, rt_frame** out) {
  if (!c || !cam || !p || !out) return invalid("rt_frame_open: null argument");
  *out = nullptr;
  return frame_new(c, cam, p, 0, "rt_frame_open", out);
}

int rt_frame_open_ex(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, uint32_t frame_flags, rt_frame** out) {
  if (!c || !cam || !p || !out) return invalid("rt_frame_open_ex: null argument");
  *out = nullptr;
  return frame_new(c, cam, p, frame_flags, "rt_frame_open_ex", out);
}

int rt_frame_advance(rt_frame* f, int max_chunks, int* out_now) {
  if (out_now) *out_now = 0;
  int rc = frame_live(f, "rt_frame_advance");
  if (rc) return rc;
  if (max_chunks < 0) return invalid("rt_frame_advance: max_chunks must not be negative");
  const int n = std::min(max_chunks, f->chunks_total - f->chunks_done);
  if (n == 0) return RT_OK;  // (a complete frame: nothing left to render)
  if (f->shard && f->owned == 0) {  // (more shards than tiles: nothing to launch, the chunks still count)
    f->chunks_done += n;
    if (out_now) *out_now = n;
    return RT_OK;
  }
  if (f->stopped_nan + f->stopped_other == f->owned) return RT_OK;  // (an adaptive frame with no active pixel)
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  if (f->used == f->events.size()) {
    hipEvent_t a = nullptr, b = nullptr;
    HIPCHK(hipEventCreate(&a));
    if (hipError_t e = hipEventCreate(&b)) {
      (void)hipEventDestroy(a);
      return hip_fail(e, "hipEventCreate");
    }
    f->events.emplace_back(a, b);
  }
  ChunkSpan span;
  span.first = f->chunks_done;
  span.count = n;
  span.acc = f->d_sum;
  span.keep = true;
  span.moments = f->d_q;
  span.skip = f->d_skip;
  span.ev_begin = f->events[f->used].first;
  span.ev_end = f->events[f->used].second;
  rc = launch_philox(c, &f->cam, &f->p, nullptr, nullptr, c->stream, nullptr,
                     nullptr, span);  // (unsharded: shard 0 of 1)
  if (rc) {  // (some of the step's launches may have been folded in: the sums are no longer a frame's)
    f->valid = false;
    return rc;
  }
  ++f->used;
  f->chunks_done += n;
  if (out_now) *out_now = n;
  return RT_OK;
}

int rt_frame_resolve(rt_frame* f, uint8_t* out_rgb, double* out_lin, rt_frame_stats* out) {
  int rc = frame_live(f, "rt_frame_resolve");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_resolve", "rt_frame_resolve_shard"))) return rc;
  if (f->chunks_done == 0) return state_error("rt_frame_resolve: no chunk rendered yet");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  // (nothing rendered since the last resolve: the device still holds that preview, and its stats repeat)
  if (f->last.chunks_done != f->chunks_done && (rc = frame_resolve_run(f))) return rc;
  if (out_rgb) HIPCHK(hipMemcpy(out_rgb, f->d_rgb, (size_t)f->npx * 3, hipMemcpyDeviceToHost));
  if (out_lin) HIPCHK(hipMemcpy(out_lin, f->d_lin, sizeof(double) * (size_t)f->npx * 3, hipMemcpyDeviceToHost));
  if (out) *out = f->last;
  return RT_OK;
}

int rt_frame_save(rt_frame* f, void* buf, size_t cap, size_t* out_len) {
  int rc = frame_live(f, "rt_frame_save");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_save", "rt_frame_save_header and rt_frame_shard_state"))) return rc;
  if (f->stopped_nan + f->stopped_other > 0)
    return state_error("rt_frame_save: the frame has stopped pixels (the version-1 blob has no room for their chunk counts)");
  const size_t payload = sizeof(double) * 3 * (size_t)f->npx;
  const size_t need = RT_FRAME_BLOB_HEADER + payload;
  if (out_len) *out_len = need;
  if (!buf || cap < need) return RT_OK;  // (size query)
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  frame_write_header(f, (uint8_t*)buf);
  // the sums in image order (assemble's map at one shard), staged on the device, then copied out
  static_assert(__BYTE_ORDER__ == __ORDER_LITTLE_ENDIAN__, "the blob's payload is copied as the host's doubles");
  return frame_image_out(f, f->d_sum, (uint8_t*)buf + RT_FRAME_BLOB_HEADER);
}

int rt_frame_restore(rt_ctx* c, const void* buf, size_t len, rt_frame** out) {
  return rt_frame_restore_ex(c, buf, len, nullptr, out);
}

int rt_frame_restore_ex(rt_ctx* c, const void* buf, size_t len, const double* moments, rt_frame** out) {
  if (!c || !out) return invalid("rt_frame_restore: null argument");
  *out = nullptr;
  return frame_restore_run(c, buf, len, moments, false, 0, 1, "rt_frame_restore", out);
}

int rt_frame_moments(rt_frame* f, double* out_q) {
  int rc = frame_live(f, "rt_frame_moments");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_moments", "rt_frame_shard_state"))) return rc;
  if (!out_q) return invalid("rt_frame_moments: null argument");
  if (!f->d_q) return state_error("rt_frame_moments: the frame was opened without RT_FRAME_MOMENTS");
  if (f->chunks_done == 0) return state_error("rt_frame_moments: no chunk rendered yet");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  return frame_image_out(f, f->d_q, out_q);
}

int rt_frame_error(rt_frame* f, const rt_error_tol* tol, double* out_se, rt_error_stats* out) {
  int rc = frame_live(f, "rt_frame_error");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_error", "rt_frame_error_shard"))) return rc;
  double abs_tol, rel_tol;
  if (!rt::error_tol(tol, abs_tol, rel_tol)) return invalid("rt_frame_error: abs_tol and rel_tol must be >= 0 and not NaN");
  if (!f->d_q) return state_error("rt_frame_error: the frame was opened without RT_FRAME_MOMENTS");
  if (f->chunks_done < 2) return state_error("rt_frame_error: the estimate needs at least 2 chunks");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  const size_t map_bytes = sizeof(double) * 3 * (size_t)f->npx;
  if (out_se && !f->d_se) HIPCHK(hipMalloc((void**)&f->d_se, map_bytes));  // (kept, as d_stage is)
  if ((rc = frame_error_run(f, abs_tol, rel_tol, out_se ? f->d_se : nullptr, f->npx, out))) return rc;
  if (out_se) HIPCHK(hipMemcpy(out_se, f->d_se, map_bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_frame_adapt(rt_frame* f, const rt_adapt_rule* rule, rt_adapt_stats* out) {
  if (!f) return invalid("rt_frame_adapt: null frame");
  if (!rt::adapt_rule_ok(rule))
    return invalid("rt_frame_adapt: bad rule (null, flags 0 or unknown, a negative or NaN tolerance, or min_chunks < 2 "
                   "with RT_ADAPT_CONVERGED)");
  return frame_stop_call(f, rule, nullptr, "rt_frame_adapt", out);
}

int rt_frame_stop(rt_frame* f, const uint8_t* mask, rt_adapt_stats* out) {
  if (!f || !mask) return invalid("rt_frame_stop: null argument");
  return frame_stop_call(f, nullptr, mask, "rt_frame_stop", out);
}

int rt_frame_chunk_counts(rt_frame* f, int32_t* out_chunks) {
  int rc = frame_live(f, "rt_frame_chunk_counts");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_chunk_counts", "rt_frame_shard_state"))) return rc;
  if (!out_chunks) return invalid("rt_frame_chunk_counts: null argument");
  if (!f->d_kp) {  // (no stop call yet: every pixel is active)
    std::fill(out_chunks, out_chunks + f->npx, (int32_t)f->chunks_done);
    return RT_OK;
  }
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  if (!f->d_kimg) HIPCHK(hipMalloc((void**)&f->d_kimg, sizeof(int) * (size_t)f->npx));
  LaunchConst A{};
  frame_const(f, A);
  FRAME_KERNEL(f, frame_chunk_counts, A, (const int*)f->d_kp, f->d_kimg, f->chunks_done);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out_chunks, f->d_kimg, sizeof(int) * (size_t)f->npx, hipMemcpyDeviceToHost));
  return RT_OK;
}

// ---- shard frames (rt.h): a progressive frame over one shard's slab, its outputs left in device memory

int rt_frame_open_shard(rt_ctx* c, const rt_camera* cam, const rt_render_params* p, uint32_t frame_flags,
                        rt_frame** out) {
  if (!c || !cam || !p || !out) return invalid("rt_frame_open_shard: null argument");
  *out = nullptr;
  return frame_new(c, cam, p, frame_flags, "rt_frame_open_shard", out, true);
}

int rt_frame_resolve_shard(rt_frame* f, uint8_t* d_slab_rgb8, double* d_slab_linear, rt_frame_stats* out) {
  int rc = frame_live(f, "rt_frame_resolve_shard");
  if (rc) return rc;
  if ((rc = frame_kind(f, true, "rt_frame_resolve_shard", "rt_frame_resolve"))) return rc;
  if (f->chunks_done == 0) return state_error("rt_frame_resolve_shard: no chunk rendered yet");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  // (nothing rendered since the last resolve: the frame still holds that preview, and its stats repeat)
  if (f->last.chunks_done != f->chunks_done && (rc = frame_resolve_run(f))) return rc;
  const size_t n3 = (size_t)f->slab * 3;
  if (d_slab_rgb8) HIPCHK(hipMemcpyAsync(d_slab_rgb8, f->d_rgb, n3, hipMemcpyDeviceToDevice, c->stream));
  if (d_slab_linear)
    HIPCHK(hipMemcpyAsync(d_slab_linear, f->d_lin, sizeof(double) * n3, hipMemcpyDeviceToDevice, c->stream));
  if (d_slab_rgb8 || d_slab_linear) HIPCHK(hipStreamSynchronize(c->stream));
  if (out) *out = f->last;
  return RT_OK;
}

int rt_frame_error_shard(rt_frame* f, const rt_error_tol* tol, double* d_slab_se, rt_error_stats* out) {
  int rc = frame_live(f, "rt_frame_error_shard");
  if (rc) return rc;
  if ((rc = frame_kind(f, true, "rt_frame_error_shard", "rt_frame_error"))) return rc;
  double abs_tol, rel_tol;
  if (!rt::error_tol(tol, abs_tol, rel_tol))
    return invalid("rt_frame_error_shard: abs_tol and rel_tol must be >= 0 and not NaN");
  if (!f->d_q) return state_error("rt_frame_error_shard: the frame was opened without RT_FRAME_MOMENTS");
  if (f->chunks_done < 2) return state_error("rt_frame_error_shard: the estimate needs at least 2 chunks");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  return frame_error_run(f, abs_tol, rel_tol, d_slab_se, f->owned, out);
}

int rt_frame_shard_state(rt_frame* f, double* d_slab_sums, double* d_slab_moments, int32_t* d_slab_chunks) {
  int rc = frame_live(f, "rt_frame_shard_state");
  if (rc) return rc;
  if ((rc = frame_kind(f, true, "rt_frame_shard_state", "rt_frame_save, rt_frame_moments and rt_frame_chunk_counts")))
    return rc;
  if (d_slab_moments && !f->d_q)
    return state_error("rt_frame_shard_state: the frame was opened without RT_FRAME_MOMENTS");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  const size_t bytes = sizeof(double) * 3 * (size_t)f->slab;
  if (d_slab_sums) HIPCHK(hipMemcpyAsync(d_slab_sums, f->d_sum, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (d_slab_moments) HIPCHK(hipMemcpyAsync(d_slab_moments, f->d_q, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (d_slab_chunks) {
    LaunchConst A{};
    frame_const(f, A);
    FRAME_KERNEL(f, frame_chunk_counts, A, (const int*)f->d_kp, (int*)d_slab_chunks, f->chunks_done);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_frame_save_header(rt_frame* f, void* buf, size_t cap) {
  int rc = frame_live(f, "rt_frame_save_header");
  if (rc) return rc;
  if (!buf || cap < RT_FRAME_BLOB_HEADER) return invalid("rt_frame_save_header: needs a buffer of RT_FRAME_BLOB_HEADER bytes");
  if (f->stopped_nan + f->stopped_other > 0)
    return state_error("rt_frame_save_header: the frame has stopped pixels (the version-1 blob has no room for their chunk counts)");
  frame_write_header(f, (uint8_t*)buf);
  return RT_OK;
}

int rt_frame_restore_shard(rt_ctx* c, const void* buf, size_t len, const double* moments, int shard_rank,
                           int shard_count, rt_frame** out) {
  if (!c || !out) return invalid("rt_frame_restore_shard: null argument");
  *out = nullptr;
  return frame_restore_run(c, buf, len, moments, true, shard_rank, shard_count, "rt_frame_restore_shard", out);
}

// ---- checkpoints (rt.h): the version-2 blob, with a tracked frame's Q and an adapted frame's K_p

int rt_frame_checkpoint(rt_frame* f, void* buf, size_t cap, size_t* out_len) {
  int rc = frame_live(f, "rt_frame_checkpoint");
  if (rc) return rc;
  if ((rc = frame_kind(f, false, "rt_frame_checkpoint",
                       "rt_frame_checkpoint_header, rt_frame_shard_state and rt_frame_shard_stops")))
    return rc;
  const uint32_t sections = frame_sections(f);
  const size_t need = RT_FRAME_CKPT_HEADER + (size_t)rt::ckpt_payload_bytes(f->npx, sections);
  if (out_len) *out_len = need;
  if (!buf || cap < need) return RT_OK;  // (size query)
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  uint8_t* at = (uint8_t*)buf;
  rt::ckpt_write_header(frame_blob_desc(f), sections, at);
  at += RT_FRAME_CKPT_HEADER;
  const size_t bytes = sizeof(double) * 3 * (size_t)f->npx;
  // S and Q in image order as rt_frame_save and rt_frame_moments write them, then the raw K_p (0 = active)
  if ((rc = frame_image_out(f, f->d_sum, at))) return rc;
  at += bytes;
  if (sections & RT_CKPT_MOMENTS) {
    if ((rc = frame_image_out(f, f->d_q, at))) return rc;
    at += bytes;
  }
  if (sections & RT_CKPT_STOPS) {
    if (!f->d_kimg) HIPCHK(hipMalloc((void**)&f->d_kimg, sizeof(int) * (size_t)f->npx));
    LaunchConst A{};
    frame_const(f, A);
    FRAME_LAUNCH(f, frame_chunk_counts<false>, A, (const int*)f->d_kp, f->d_kimg, 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(at, f->d_kimg, sizeof(int) * (size_t)f->npx, hipMemcpyDeviceToHost));
  }
  return RT_OK;
}

int rt_frame_resume(rt_ctx* c, const void* buf, size_t len, rt_frame** out) {
  if (!c || !out) return invalid("rt_frame_resume: null argument");
  *out = nullptr;
  return frame_resume_run(c, buf, len, false, 0, 1, "rt_frame_resume", out);
}

int rt_frame_resume_shard(rt_ctx* c, const void* buf, size_t len, int shard_rank, int shard_count, rt_frame** out) {
  if (!c || !out) return invalid("rt_frame_resume_shard: null argument");
  *out = nullptr;
  return frame_resume_run(c, buf, len, true, shard_rank, shard_count, "rt_frame_resume_shard", out);
}

int rt_frame_shard_stops(rt_frame* f, int32_t* d_slab_stops) {
  int rc = frame_live(f, "rt_frame_shard_stops");
  if (rc) return rc;
  if ((rc = frame_kind(f, true, "rt_frame_shard_stops", "rt_frame_checkpoint"))) return rc;
  if (!d_slab_stops) return invalid("rt_frame_shard_stops: null argument");
  rt_ctx* c = f->ctx;
  DEVICE_SCOPE(c->device);
  if (!f->d_kp) {  // (no stop call yet: every pixel is active)
    HIPCHK(hipMemsetAsync(d_slab_stops, 0, sizeof(int) * (size_t)f->slab, c->stream));
  } else {
    LaunchConst A{};
    frame_const(f, A);
    FRAME_LAUNCH(f, frame_chunk_counts<true>, A, (const int*)f->d_kp, (int*)d_slab_stops, 0);
    HIPCHK(hipGetLastError());
  }
  HIPCHK(hipStreamSynchronize(c->stream));
  return RT_OK;
}

int rt_frame_checkpoint_header(rt_frame* f, uint32_t sections, int chunks_done, void* buf, size_t cap) {
  int rc = frame_live(f, "rt_frame_checkpoint_header");
  if (rc) return rc;
  if (!buf || cap < RT_FRAME_CKPT_HEADER)
    return invalid("rt_frame_checkpoint_header: needs a buffer of RT_FRAME_CKPT_HEADER bytes");
  if (sections & ~(RT_CKPT_MOMENTS | RT_CKPT_STOPS)) return invalid("rt_frame_checkpoint_header: unknown section bit");
  if ((sections & RT_CKPT_MOMENTS) && !f->d_q)
    return state_error("rt_frame_checkpoint_header: RT_CKPT_MOMENTS on a frame opened without RT_FRAME_MOMENTS");
  if (chunks_done == -1) chunks_done = f->chunks_done;
  if (chunks_done < f->chunks_done || chunks_done > f->chunks_total)
    return invalid("rt_frame_checkpoint_header: chunks_done must be -1 or in [the frame's own, chunks_total]");
  if (chunks_done > f->chunks_done && f->stopped_nan + f->stopped_other != f->owned)
    return state_error("rt_frame_checkpoint_header: chunks_done is ahead of a frame that still has active pixels");
  rt_frame_blob_desc b = frame_blob_desc(f);
  b.chunks_done = chunks_done;
  rt::ckpt_write_header(b, sections, (uint8_t*)buf);
  return RT_OK;
}

void rt_frame_close(rt_frame* f) {
  if (!f) return;
  rt_ctx* c = f->ctx;
  DeviceGuard _dg(c->device);
  (void)hipStreamSynchronize(c->stream);  // (its queued launches write its buffers)
  c->frames.erase(std::remove(c->frames.begin(), c->frames.end(), f), c->frames.end());
  frame_free(f);
}

}  // extern "C"

// ------------------------------------------------------------------ feature-guided denoiser (rt.h)
namespace {

// rt_denoise*'s argument checks (rt.h), before any HIP call; the ctx last, as features_check.
int denoise_check(const char* what, const rt_ctx* c, const rt_denoise_params* p, bool pointers) {
  const char* bad = rt::denoise_params_error(p);
  if (!bad && !pointers) bad = "null color, feature_sums or out_color";
  if (!bad && !c) bad = "null ctx";
  return bad ? invalid(std::string(what) + ": " + bad) : RT_OK;
}

// The kernels of one denoise call queued on `st` over device pointers (the ctx's device is selected), in the ctx's
// own buffers, grown on demand. Like a feature pass it takes its place in the ctx's launch order: after the
// previous launch (ev_done), and the next one, which may be another denoise in the same buffers, waits for it.
// `timed`: the ctx's ev_dn0 / ev_dn1 are recorded around the kernels.
int denoise_queue(rt_ctx* c, const rt_denoise_params* p, const double* d_color, const double* d_se,
                  const double* d_feat, double* d_out, uint8_t* d_rgb, hipStream_t st, bool timed) {
  const size_t npx = (size_t)p->width * (size_t)p->height;
  int rc;
  if ((rc = grow(c, c->dn_guide, 32 * npx)) || (rc = grow(c, c->dn_a, 32 * npx)) || (rc = grow(c, c->dn_b, 32 * npx)) ||
      (rc = grow(c, c->dn_counts, 3 * sizeof(unsigned long long))))
    return rc;
  if (st != c->last_stream) HIPCHK(hipStreamWaitEvent(st, c->ev_done, 0));
  c->last_stream = st;
  if (timed) HIPCHK(hipEventRecord(c->ev_dn0, st));
  const rt::DenoiseBuffers B{c->dn_guide.p, c->dn_a.p, c->dn_b.p, (unsigned long long*)c->dn_counts.p};
  int launches = 0;
  const int e = rt::denoise_launch(rt::denoise_const(*p), p->iterations, d_color, d_se, d_feat, B, d_out, d_rgb,
                                   (void*)st, &launches);
  if (e) return hip_fail((hipError_t)e, "rt_denoise launch");
  if (timed) HIPCHK(hipEventRecord(c->ev_dn1, st));
  HIPCHK(hipEventRecord(c->ev_done, st));
  c->last_denoise = rt_denoise_info{c->allocs, launches, (int32_t)rt::kDenoiseLdsBytes, 0};
  return RT_OK;
}

// A blocking call's kernels on the ctx's stream, then its stats (may be null) from the device's counts.
int denoise_run(rt_ctx* c, const rt_denoise_params* p, const double* d_color, const double* d_se, const double* d_feat,
                double* d_out, uint8_t* d_rgb, rt_denoise_stats* stats) {
  int rc = denoise_queue(c, p, d_color, d_se, d_feat, d_out, d_rgb, c->stream, true);
  unsigned long long counts[3] = {0, 0, 0};
  if (!rc) rc = hip_ok(hipMemcpyAsync(counts, c->dn_counts.p, sizeof counts, hipMemcpyDeviceToHost, c->stream), "hipMemcpyAsync");
  HIPCHK(hipStreamSynchronize(c->stream));
  if (rc) return rc;
  if (stats) {
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, c->ev_dn0, c->ev_dn1));
    stats->pixels = (int64_t)p->width * p->height;
    stats->invalid_in = (int64_t)counts[0];
    stats->invalid_out = (int64_t)counts[1];
    stats->filled = (int64_t)counts[2];
    stats->kernel_ms = ms;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_denoise_async(rt_ctx* c, const rt_denoise_params* p, const double* d_color, const double* d_se,
                     const double* d_feature_sums, double* d_out_color, uint8_t* d_out_rgb8, void* stream) {
  int rc = denoise_check("rt_denoise_async", c, p, d_color && d_feature_sums && d_out_color);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  return denoise_queue(c, p, d_color, d_se, d_feature_sums, d_out_color, d_out_rgb8, (hipStream_t)stream, false);
}

int rt_denoise(rt_ctx* c, const rt_denoise_params* p, const double* color, const double* se, const double* feature_sums,
               double* out_color, uint8_t* out_rgb8, rt_denoise_stats* stats) {
  int rc = denoise_check("rt_denoise", c, p, color && feature_sums && out_color);
  if (rc) return rc;
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  const size_t npx = (size_t)p->width * (size_t)p->height, img = sizeof(double) * 3 * npx;
  if ((rc = grow(c, c->dn_color, img)) || (se && (rc = grow(c, c->dn_se, img))) ||
      (rc = grow(c, c->dn_feat, sizeof(double) * RT_FEATURE_DOUBLES * npx)) || (rc = grow(c, c->dn_out, img)) ||
      (out_rgb8 && (rc = grow(c, c->dn_rgb, 3 * npx))))
    return rc;
  HIPCHK(hipMemcpy(c->dn_color.p, color, img, hipMemcpyHostToDevice));
  if (se) HIPCHK(hipMemcpy(c->dn_se.p, se, img, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(c->dn_feat.p, feature_sums, sizeof(double) * RT_FEATURE_DOUBLES * npx, hipMemcpyHostToDevice));
  if ((rc = denoise_run(c, p, (const double*)c->dn_color.p, se ? (const double*)c->dn_se.p : nullptr,
                        (const double*)c->dn_feat.p, (double*)c->dn_out.p, out_rgb8 ? (uint8_t*)c->dn_rgb.p : nullptr,
                        stats)))
    return rc;
  HIPCHK(hipMemcpy(out_color, c->dn_out.p, img, hipMemcpyDeviceToHost));
  if (out_rgb8) HIPCHK(hipMemcpy(out_rgb8, c->dn_rgb.p, 3 * npx, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_last_denoise(rt_ctx* c, rt_denoise_info* out) {
  if (!c || !out) return invalid("null argument");
  *out = c->last_denoise;
  return RT_OK;
}

int rt_frame_denoise(rt_frame* f, const rt_denoise_params* p, const double* d_feature_sums, uint8_t* out_rgb8,
                     double* out_linear, rt_denoise_stats* stats) {
  if (!f) return invalid("rt_frame_denoise: null frame");
  rt_ctx* c = f->ctx;
  int rc = denoise_check("rt_frame_denoise", c, p, d_feature_sums != nullptr);
  if (rc) return rc;
  if (p->width != f->p.width || p->height != f->p.height)
    return invalid("rt_frame_denoise: params->width and height must be the frame's");
  if ((rc = frame_live(f, "rt_frame_denoise"))) return rc;
  if (f->shard)
    return state_error("rt_frame_denoise: a shard frame cannot be denoised (a tap may lie in another shard's slab: a "
                       "sharded denoise needs a halo exchange); assemble the shards' previews and call rt_denoise_async");
  if (f->chunks_done == 0) return state_error("rt_frame_denoise: no chunk rendered yet");
  DEVICE_SCOPE(c->device);
  c->allocs = 0;
  const size_t npx = (size_t)f->npx, img = sizeof(double) * 3 * npx;
  const bool with_se = f->d_q && f->chunks_done >= 2;
  if ((rc = grow(c, c->dn_color, img)) || (with_se && (rc = grow(c, c->dn_se, img))) || (rc = grow(c, c->dn_out, img)) ||
      (rc = grow(c, c->dn_rgb, 3 * npx)) || (rc = grow(c, c->dn_fcounts, 2 * sizeof(unsigned long long))))
    return rc;
  // The preview, by rt_frame_resolve's kernel into the ctx's buffers: the frame's own preview, the bytes it
  // compares the next resolve with and its counts stay as they are (the scratch bytes are then the denoised ones).
  LaunchConst A{};
  frame_const(f, A);
  A.out_rgb = (uint8_t*)c->dn_rgb.p;
  A.out_lin = (double*)c->dn_color.p;
  HIPCHK(hipMemsetAsync(c->dn_fcounts.p, 0, 2 * sizeof(unsigned long long), c->stream));
  FRAME_KERNEL_ADAPT(f, frame_resolve, A, frame_samples(f), (unsigned long long*)c->dn_fcounts.p, (const int*)f->d_kp);
  HIPCHK(hipGetLastError());
  if (with_se && (rc = frame_error_run(f, 0.0, 0.0, (double*)c->dn_se.p, f->npx, nullptr))) return rc;
  if ((rc = denoise_run(c, p, (const double*)c->dn_color.p, with_se ? (const double*)c->dn_se.p : nullptr, d_feature_sums,
                        (double*)c->dn_out.p, out_rgb8 ? (uint8_t*)c->dn_rgb.p : nullptr, stats)))
    return rc;
  if (out_linear) HIPCHK(hipMemcpy(out_linear, c->dn_out.p, img, hipMemcpyDeviceToHost));
  if (out_rgb8) HIPCHK(hipMemcpy(out_rgb8, c->dn_rgb.p, 3 * npx, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_debug_closest_hits(rt_ctx* c, const double* rays, int n, double tmin, double tmax, uint64_t seed,
                          uint32_t flags, double* out) {
  if (!c || !rays || !out || n < 0) return invalid("null argument");
  if (!c->has_scene) {
    rt::set_error("rt_debug_closest_hits: no scene uploaded");
    return RT_E_STATE;
  }
  if ((flags & (RT_DEBUG_RESUMABLE | RT_DEBUG_WIDE | RT_DEBUG_QNODE)) && !c->shape.replace_ok)
    return unsupported("rt_debug_closest_hits: the resumable walks need a world without media and frames");
  // (a mixed-walk world has d_wnodes too: its re-bounded subtrees' trees, which no plain 4-wide walk from
  // the binary world root may enter)
  if ((flags & (RT_DEBUG_WIDE | RT_DEBUG_QNODE)) && c->scene.ref_walk)
    return unsupported("rt_debug_closest_hits: the 4-wide walks need a world without media and instance frames");
  if ((flags & (RT_DEBUG_WIDE | RT_DEBUG_QNODE)) && !c->d_wnodes)
    return unsupported("rt_debug_closest_hits: no 4-wide tree for this world");
  if (n == 0) return RT_OK;
  DEVICE_SCOPE(c->device);
  DevBuf rays_buf, out_buf;
  HIPCHK(hipMalloc(&rays_buf.p, sizeof(double) * 7 * (size_t)n));
  HIPCHK(hipMalloc(&out_buf.p, sizeof(double) * 12 * (size_t)n));
  double* d_rays = (double*)rays_buf.p;
  double* d_out = (double*)out_buf.p;
  HIPCHK(hipMemcpy(d_rays, rays, sizeof(double) * 7 * (size_t)n, hipMemcpyHostToDevice));
  const int joint = !(cull(c, flags) & RT_FLAG_REFERENCE_CULL);
  const dim3 grid((n + RT_BLOCK - 1) / RT_BLOCK);
  if ((flags & RT_DEBUG_QNODE) && !c->d_qnodes)
    return unsupported("rt_debug_closest_hits: no quantised 4-wide tree for this world (spheres-only worlds)");
  if (flags & RT_DEBUG_QNODE)
    hipLaunchKernelGGL(closest_hits<F_UV | F_WIDE | F_QNODE>, grid, dim3(RT_BLOCK), 0, c->stream, c->scene, d_rays, n,
                       tmin, tmax, seed, joint, 1, d_out);
  else if (flags & RT_DEBUG_WIDE) {
    // the wide_node form and ray set-up the render kernels of this world run: packed sort keys when the tree
    // is within their bound, and the spheres-only variant's walk (fp32 reciprocals from the direction)
    const bool pk = rt::wide_keys_packed(c->shape, rt::read_knobs()), sph = variant_for(c->shape.features) == kVarSpheres;
    const void* fn = sph ? (pk ? (const void*)closest_hits<F_UV | F_WIDE, true> : (const void*)closest_hits<F_UV | F_WIDE>)
                         : (pk ? (const void*)closest_hits<F_ALL | F_UV | F_WIDE, true>
                               : (const void*)closest_hits<F_ALL | F_UV | F_WIDE>);
    int joint_i = joint, walk = 1;
    void* args[] = {&c->scene, &d_rays, &n, &tmin, &tmax, &seed, &joint_i, &walk, &d_out};
    HIPCHK(hipLaunchKernel(fn, grid, dim3(RT_BLOCK), args, 0, c->stream));
    c->last_wide_packed = pk;
  } else
    hipLaunchKernelGGL(closest_hits<F_ALL | F_UV | F_MIXW>, grid, dim3(RT_BLOCK), 0, c->stream, c->scene, d_rays, n,
                       tmin, tmax, seed, joint, (flags & RT_DEBUG_RESUMABLE) ? 1 : 0, d_out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, d_out, sizeof(double) * 12 * (size_t)n, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_debug_exact_trace(rt_ctx* c, const rt_camera* cam, const rt_render_params* pin, const uint64_t* col_gens,
                         int col, double* out, int cap, int* out_n) {
  if (!c || !cam || !pin || !col_gens || !out || !out_n || cap < 0) return invalid("rt_debug_exact_trace: null argument");
  rt_render_params p = *pin;
  p.shard_rank = 0;
  p.shard_count = 1;
  int rc = check_params(&p);
  if (rc) return rc;
  if (p.rng_mode != RT_RNG_EXACT) return invalid("rt_debug_exact_trace: tier A only");
  if (col < 0 || col >= p.width) return invalid("rt_debug_exact_trace: column out of range");
  if (!c->has_scene) {
    rt::set_error("rt_debug_exact_trace: no scene uploaded");
    return RT_E_STATE;
  }
  DEVICE_SCOPE(c->device);
  const long long npx = (long long)p.width * p.height;
  DevBuf img, gens, tr, trn;
  HIPCHK(hipMalloc(&img.p, (size_t)npx * 3));
  HIPCHK(hipMalloc(&gens.p, sizeof(uint64_t) * 2 * (size_t)p.width));
  HIPCHK(hipMalloc(&tr.p, sizeof(double) * 10 * (size_t)std::max(1, cap)));
  HIPCHK(hipMalloc(&trn.p, sizeof(int)));
  HIPCHK(hipMemcpy(gens.p, col_gens, sizeof(uint64_t) * 2 * (size_t)p.width, hipMemcpyHostToDevice));
  HIPCHK(hipMemset(trn.p, 0, sizeof(int)));
  LaunchConst A{};
  A.S = c->scene;
  A.cam = *cam;
  A.W = p.width;
  A.H = p.height;
  A.spp = p.spp;
  A.max_depth = p.max_depth;
  A.flags = cull(c, p.flags);
  A.gens = (uint64_t*)gens.p;
  A.out_rgb = (uint8_t*)img.p;
  A.trace = (double*)tr.p;
  A.trace_n = (int*)trn.p;
  A.trace_col = col;
  A.trace_cap = cap;
  const void* fn = nullptr;
  size_t lds = 0;
  if (int rc = exact_launch(c, (p.flags & RT_FLAG_SHARED_LIBM) != 0, &fn, &lds)) return rc;
  int n_nodes = c->shape.n_nodes;
  void* args[] = {&A, &n_nodes};
  HIPCHK(hipLaunchKernel(fn, dim3(exact_blocks(p.width)), dim3(RT_BLOCK), args, lds, c->stream));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out_n, trn.p, sizeof(int), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out, tr.p, sizeof(double) * 10 * (size_t)std::min(*out_n, cap), hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_debug_probe(rt_ctx* c, const rt_camera* cam, int op, const double* in, int n, uint64_t seed, double* out) {
  if (!c || !in || !out || n < 0 || op < 0 || op > RT_PROBE_BOX || (op == 4 && !cam)) return invalid("rt_debug_probe: bad argument");
  if (!c->has_scene) {
    rt::set_error("rt_debug_probe: no scene uploaded");
    return RT_E_STATE;
  }
  if (n == 0) return RT_OK;
  // ids the device indexes with come from the caller: check them here (an out-of-range id would be
  // an out-of-bounds device read, not an error)
  auto id_ok = [](double x, int count) { return std::isfinite(x) && x >= 0 && x < count && x == std::floor(x); };
  for (int i = 0; i < n; ++i) {
    const double* q = in + (size_t)kProbeIn[op] * i;
    if (op == RT_PROBE_SCATTER && !id_ok(q[17], c->n_materials))
      return invalid("rt_debug_probe: scatter record " + std::to_string(i) + " has a material id out of range");
    if (op == RT_PROBE_TEXTURE && !id_ok(q[0], c->n_textures))
      return invalid("rt_debug_probe: texture record " + std::to_string(i) + " has a texture id out of range");
  }
  if (op == RT_PROBE_HTBL_RANDOM && c->scene.lights < 0)
    return invalid("rt_debug_probe: the scene has no lights tree");
  DEVICE_SCOPE(c->device);
  DevBuf bin, bout;
  const size_t nin = sizeof(double) * kProbeIn[op] * (size_t)n, nout = sizeof(double) * kProbeOut[op] * (size_t)n;
  HIPCHK(hipMalloc(&bin.p, nin));
  HIPCHK(hipMalloc(&bout.p, nout));
  HIPCHK(hipMemcpy(bin.p, in, nin, hipMemcpyHostToDevice));
  rt_camera k{};
  if (cam) k = *cam;
  hipLaunchKernelGGL(fn_probe<F_ALL>, dim3((n + RT_BLOCK - 1) / RT_BLOCK), dim3(RT_BLOCK), 0, c->stream, c->scene, k, op,
                     (const double*)bin.p, n, seed, (double*)bout.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, bout.p, nout, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_debug_math(rt_ctx* c, int op, const double* x, const double* y, int n, double* out) {
  if (!c || !x || !y || !out || n < 0 || op < 0 || op > 19) return invalid("rt_debug_math: bad argument");
  if (n == 0) return RT_OK;
  DEVICE_SCOPE(c->device);
  const size_t bytes = sizeof(double) * (size_t)n;
  DevBuf bx, by, bout;
  HIPCHK(hipMalloc(&bx.p, bytes));
  HIPCHK(hipMalloc(&by.p, bytes));
  HIPCHK(hipMalloc(&bout.p, bytes));
  double *dx = (double*)bx.p, *dy = (double*)by.p, *dout = (double*)bout.p;
  HIPCHK(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dy, y, bytes, hipMemcpyHostToDevice));
  if (op >= 18) hipLaunchKernelGGL(math_probe_sincos<0>, dim3((n + 255) / 256), dim3(256), 0, c->stream, op, dx, n, dout);
  else hipLaunchKernelGGL(math_probe, dim3((n + 255) / 256), dim3(256), 0, c->stream, op, dx, dy, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(c->stream));
  HIPCHK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  return RT_OK;
}

}  // extern "C"
