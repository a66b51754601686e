// rt_frame_blob.cpp — the host half of progressive frames (include/rt.h): the saved frame's header
// (layout, writer, parser and validation) and the scene fingerprint; the version-2 checkpoint's header and
// payload checks, and its offline preview and error map (rt_checkpoint_resolve, rt_checkpoint_error). No
// HIP, no device: it builds for the CPU as is (tests/c/frame_blob_check.c and tests/c/checkpoint_check.c
// drive it under the sanitizers).
#include <cmath>
#include <cstring>
#include <string>

#include "rt.h"
#include "rt_error.h"
#include "rt_frame_blob.h"
#include "rt_internal.h"

namespace rt {
namespace {

// little-endian fields, byte by byte (the layout does not depend on the host's byte order)
void put_u32(uint8_t* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
void put_u64(uint8_t* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (uint8_t)(v >> (8 * i));
}
uint32_t get_u32(const uint8_t* p) {
  uint32_t v = 0;
  for (int i = 0; i < 4; ++i) v |= (uint32_t)p[i] << (8 * i);
  return v;
}
uint64_t get_u64(const uint8_t* p) {
  uint64_t v = 0;
  for (int i = 0; i < 8; ++i) v |= (uint64_t)p[i] << (8 * i);
  return v;
}
void put_f64(uint8_t* p, double x) {
  uint64_t v;
  std::memcpy(&v, &x, 8);
  put_u64(p, v);
}
double get_f64(const uint8_t* p) {
  const uint64_t v = get_u64(p);
  double x;
  std::memcpy(&x, &v, 8);
  return x;
}

constexpr uint8_t kMagic[8] = {'R', 'T', 'F', 'R', 'A', 'M', 'E', 0};
// header offsets (rt.h)
constexpr size_t kOffVersion = 8, kOffUpload = 12, kOffParams = 16, kOffCamera = 64, kOffChunk = 256, kOffDone = 260,
                 kOffPixels = 264, kOffFingerprint = 272, kOffPayload = 280;
static_assert(kOffPayload + 8 == RT_FRAME_BLOB_HEADER, "header size");
// a version-2 checkpoint's further header bytes: the sections word, then reserved bytes
constexpr size_t kOffSections = 288;
static_assert(kOffSections + 4 + 28 == RT_FRAME_CKPT_HEADER, "checkpoint header size");
static_assert(sizeof(rt_camera) == 24 * sizeof(double), "rt_camera is 24 doubles");

uint64_t fnv1a(uint64_t h, const void* data, size_t n) {
  const uint8_t* p = (const uint8_t*)data;
  for (size_t i = 0; i < n; ++i) h = (h ^ p[i]) * 0x100000001b3ULL;
  return h;
}

}  // namespace

uint64_t scene_fingerprint(const rt_scene_desc* d) {
  uint64_t h = 0xcbf29ce484222325ULL;
  auto arr = [&](const void* p, long long count, size_t rec) {
    if (p && count > 0) h = fnv1a(h, p, (size_t)count * rec);
  };
  arr(d->nodes, d->n_nodes, sizeof(rt_node));
  arr(d->materials, d->n_materials, sizeof(rt_material));
  arr(d->textures, d->n_textures, sizeof(rt_texture));
  arr(d->perlins, d->n_perlins, sizeof(rt_perlin));
  arr(d->images, d->n_images, sizeof(rt_image));
  arr(d->image_pool, d->image_pool_bytes, 1);
  uint8_t tail[8 + 24];
  put_u32(tail, (uint32_t)d->world_root);
  put_u32(tail + 4, (uint32_t)d->lights_root);
  for (int i = 0; i < 3; ++i) put_f64(tail + 8 + 8 * i, d->background[i]);
  return fnv1a(h, tail, sizeof tail);
}

void blob_write_header(const rt_frame_blob_desc& b, uint8_t* out) {
  std::memset(out, 0, RT_FRAME_BLOB_HEADER);
  std::memcpy(out, kMagic, 8);
  put_u32(out + kOffVersion, b.version);
  put_u32(out + kOffUpload, b.upload_flags);
  uint8_t* q = out + kOffParams;
  const rt_render_params& p = b.params;
  const uint32_t head[6] = {(uint32_t)p.width,     (uint32_t)p.height,   (uint32_t)p.spp,
                            (uint32_t)p.max_depth, (uint32_t)p.rng_mode, p.flags};
  for (int i = 0; i < 6; ++i) put_u32(q + 4 * i, head[i]);
  put_u64(q + 24, p.seed);
  const uint32_t rest[4] = {(uint32_t)p.tile, (uint32_t)p.shard_rank, (uint32_t)p.shard_count, (uint32_t)p._pad};
  for (int i = 0; i < 4; ++i) put_u32(q + 32 + 4 * i, rest[i]);
  double cam[24];
  std::memcpy(cam, &b.camera, sizeof cam);
  for (int i = 0; i < 24; ++i) put_f64(out + kOffCamera + 8 * i, cam[i]);
  put_u32(out + kOffChunk, (uint32_t)b.chunk);
  put_u32(out + kOffDone, (uint32_t)b.chunks_done);
  put_u64(out + kOffPixels, (uint64_t)b.pixels);
  put_u64(out + kOffFingerprint, b.scene_fingerprint);
  put_u64(out + kOffPayload, b.payload_bytes);
}

namespace {

// The header's fields from offset 8 on into `b` (payload_bytes as stored), with every rule that does not
// depend on the blob's version: nullptr when they hold, else what is wrong. `in` has at least
// RT_FRAME_BLOB_HEADER bytes.
const char* parse_fields(const uint8_t* in, rt_frame_blob_desc& b) {
  std::memset(&b, 0, sizeof b);
  b.version = get_u32(in + kOffVersion);
  b.upload_flags = get_u32(in + kOffUpload);
  const uint8_t* q = in + kOffParams;
  rt_render_params& p = b.params;
  p.width = (int32_t)get_u32(q);
  p.height = (int32_t)get_u32(q + 4);
  p.spp = (int32_t)get_u32(q + 8);
  p.max_depth = (int32_t)get_u32(q + 12);
  p.rng_mode = (int32_t)get_u32(q + 16);
  p.flags = get_u32(q + 20);
  p.seed = get_u64(q + 24);
  p.tile = (int32_t)get_u32(q + 32);
  p.shard_rank = (int32_t)get_u32(q + 36);
  p.shard_count = (int32_t)get_u32(q + 40);
  p._pad = (int32_t)get_u32(q + 44);
  double cam[24];
  for (int i = 0; i < 24; ++i) cam[i] = get_f64(in + kOffCamera + 8 * i);
  std::memcpy(&b.camera, cam, sizeof cam);
  b.chunk = (int32_t)get_u32(in + kOffChunk);
  b.chunks_done = (int32_t)get_u32(in + kOffDone);
  b.pixels = (int64_t)get_u64(in + kOffPixels);
  b.scene_fingerprint = get_u64(in + kOffFingerprint);
  b.payload_bytes = get_u64(in + kOffPayload);
  if (p.width <= 0 || p.height <= 0 || p.spp <= 0 || p.max_depth < 0)
    return "width/height/spp must be positive and max_depth >= 0";
  if (p.spp > INT32_MAX - RT_CHUNK_MAX) return "spp too large for rt_sample_chunk";
  if (p.rng_mode != RT_RNG_PHILOX) return "not a tier-B (RT_RNG_PHILOX) frame";
  if (p.tile != 0 && (p.tile < 8 || p.tile % 8 || p.tile > 256)) return "tile must be 0 or a multiple of 8 in [8, 256]";
  const int64_t pixels = (int64_t)p.width * p.height;
  if (pixels >= (1ll << 32) || b.pixels != pixels) return "pixel count disagrees with width * height";
  if (b.chunk != rt_sample_chunk(pixels, p.spp)) return "chunk size is not rt_sample_chunk(pixels, spp)";
  b.chunks_total = (p.spp + b.chunk - 1) / b.chunk;
  if (b.chunks_done < 0 || b.chunks_done > b.chunks_total) return "chunks_done out of range";
  const int64_t samples = (int64_t)b.chunks_done * b.chunk;
  b.samples_done = (int32_t)(samples < p.spp ? samples : p.spp);
  return nullptr;
}

}  // namespace

const char* blob_parse(const void* buf, size_t len, rt_frame_blob_desc* out) {
  if (!buf) return "null blob";
  if (len < RT_FRAME_BLOB_HEADER) return "truncated: shorter than the header";
  const uint8_t* in = (const uint8_t*)buf;
  if (std::memcmp(in, kMagic, 8) != 0) return "bad magic";
  if (get_u32(in + kOffVersion) != RT_FRAME_BLOB_VERSION) return "unknown blob version";
  rt_frame_blob_desc b;
  if (const char* why = parse_fields(in, b)) return why;
  if (b.payload_bytes != (uint64_t)b.pixels * 24) return "payload size disagrees with the pixel count";
  if (len - RT_FRAME_BLOB_HEADER != b.payload_bytes) return "length disagrees with the header";
  if (out) *out = b;
  return nullptr;
}

uint64_t ckpt_payload_bytes(int64_t pixels, uint32_t sections) {
  return (uint64_t)pixels * (24u + ((sections & RT_CKPT_MOMENTS) ? 24u : 0u) + ((sections & RT_CKPT_STOPS) ? 4u : 0u));
}

void ckpt_write_header(const rt_frame_blob_desc& b, uint32_t sections, uint8_t* out) {
  rt_frame_blob_desc v2 = b;
  v2.version = RT_FRAME_CKPT_VERSION;
  v2.payload_bytes = ckpt_payload_bytes(b.pixels, sections);
  blob_write_header(v2, out);
  std::memset(out + RT_FRAME_BLOB_HEADER, 0, RT_FRAME_CKPT_HEADER - RT_FRAME_BLOB_HEADER);
  put_u32(out + kOffSections, sections);
}

const char* ckpt_parse(const void* buf, size_t len, rt_frame_ckpt_desc* out) {
  if (!buf) return "null blob";
  if (len < RT_FRAME_BLOB_HEADER) return "truncated: shorter than the header";
  const uint8_t* in = (const uint8_t*)buf;
  if (std::memcmp(in, kMagic, 8) != 0) return "bad magic";
  rt_frame_ckpt_desc d;
  std::memset(&d, 0, sizeof d);
  const uint32_t version = get_u32(in + kOffVersion);
  if (version == RT_FRAME_BLOB_VERSION) {
    if (const char* why = blob_parse(buf, len, &d.blob)) return why;
    d.sums_offset = RT_FRAME_BLOB_HEADER;
    d.active_pixels = d.blob.pixels;
    if (out) *out = d;
    return nullptr;
  }
  if (version != RT_FRAME_CKPT_VERSION) return "unknown blob version";
  if (len < RT_FRAME_CKPT_HEADER) return "truncated: shorter than the checkpoint header";
  if (const char* why = parse_fields(in, d.blob)) return why;
  d.sections = get_u32(in + kOffSections);
  if (d.sections & ~(RT_CKPT_MOMENTS | RT_CKPT_STOPS)) return "unknown checkpoint section";
  for (size_t i = kOffSections + 4; i < RT_FRAME_CKPT_HEADER; ++i)
    if (in[i]) return "a reserved header byte is not zero";
  const uint64_t pixels = (uint64_t)d.blob.pixels;
  if (d.blob.payload_bytes != ckpt_payload_bytes(d.blob.pixels, d.sections))
    return "payload size disagrees with the pixel count and the sections";
  if (len - RT_FRAME_CKPT_HEADER != d.blob.payload_bytes) return "length disagrees with the header";
  uint64_t at = RT_FRAME_CKPT_HEADER;
  d.sums_offset = at;
  at += pixels * 24;
  if (d.sections & RT_CKPT_MOMENTS) {
    d.moments_offset = at;
    at += pixels * 24;
  }
  if (d.sections & RT_CKPT_STOPS) {
    d.stops_offset = at;
    for (uint64_t i = 0; i < pixels; ++i) {
      const int32_t k = (int32_t)get_u32(in + at + 4 * i);
      if (k < 0 || k > d.blob.chunks_done) return "a stopped pixel's chunk count is outside [0, chunks_done]";
      if (!k) continue;
      ++d.stopped_pixels;
      const uint8_t* s = in + d.sums_offset + 24 * i;
      const double x = get_f64(s), y = get_f64(s + 8), z = get_f64(s + 16);
      if (x != x || y != y || z != z) ++d.stopped_nan;
    }
  }
  d.active_pixels = d.blob.pixels - d.stopped_pixels;
  if (out) *out = d;
  return nullptr;
}

namespace {

// A checkpoint's payload, read pixel by pixel (byte loads: a caller's buffer need not be aligned).
struct CkptView {
  const uint8_t* in;
  rt_frame_ckpt_desc d;
  void sums(int64_t i, double s[3]) const {
    for (int c = 0; c < 3; ++c) s[c] = get_f64(in + d.sums_offset + 24 * (uint64_t)i + 8 * c);
  }
  void moments(int64_t i, double q[3]) const {
    for (int c = 0; c < 3; ++c) q[c] = get_f64(in + d.moments_offset + 24 * (uint64_t)i + 8 * c);
  }
  // (K_p, N_p) of pixel i: a stopped pixel's own, else the frame's (rt.h, adaptive frames)
  void counts(int64_t i, int& chunks, int& samples) const {
    const int32_t k = d.stops_offset ? (int32_t)get_u32(in + d.stops_offset + 4 * (uint64_t)i) : 0;
    chunks = d.blob.chunks_done;
    samples = d.blob.samples_done;
    if (!k) return;
    const int64_t n = (int64_t)k * d.blob.chunk;
    chunks = k;
    samples = n < d.blob.params.spp ? (int)n : d.blob.params.spp;
  }
};

// The host twin of the device's scale_color (rt_kernels.h; scaleColor, Lib.hs:287-288): the same IEEE
// operations in the same order, NaN -> 0, +inf -> 255. The device's `divide` is one division per channel.
uint8_t scale_color_host(double x) {
  const double s = std::sqrt(x);
  const double cl = s < 0.0 ? 0.0 : (s > 0.999 ? 0.999 : s);
  const double f = std::floor(256 * cl);
  return f == f ? (uint8_t)(int)f : (uint8_t)0;
}

}  // namespace

}  // namespace rt

extern "C" {

int rt_frame_blob_info(const void* buf, size_t len, rt_frame_blob_desc* out) {
  if (const char* why = rt::blob_parse(buf, len, out)) {
    rt::set_error(std::string("frame blob: ") + why);
    return RT_E_INVALID;
  }
  return RT_OK;
}

int rt_frame_checkpoint_info(const void* buf, size_t len, rt_frame_ckpt_desc* out) {
  if (const char* why = rt::ckpt_parse(buf, len, out)) {
    rt::set_error(std::string("frame blob: ") + why);
    return RT_E_INVALID;
  }
  return RT_OK;
}

int rt_checkpoint_resolve(const void* buf, size_t len, uint8_t* out_rgb8, double* out_linear, rt_frame_stats* out) {
  rt::CkptView v{(const uint8_t*)buf, {}};
  int rc = rt_frame_checkpoint_info(buf, len, &v.d);
  if (rc) return rc;
  const rt_frame_blob_desc& b = v.d.blob;
  if (b.chunks_done == 0) {
    rt::set_error("rt_checkpoint_resolve: no chunk rendered yet");
    return RT_E_INVALID;
  }
  rt_frame_stats st{};
  st.chunk = b.chunk;
  st.chunks_total = b.chunks_total;
  st.chunks_done = b.chunks_done;
  st.samples_done = b.samples_done;
  for (int64_t i = 0; i < b.pixels; ++i) {
    double s[3];
    int chunks, samples;
    v.sums(i, s);
    v.counts(i, chunks, samples);
    if (s[0] != s[0] || s[1] != s[1] || s[2] != s[2]) ++st.nan_pixels;
    for (int c = 0; c < 3; ++c) {
      const double avg = s[c] / (double)samples;
      const uint8_t byte = rt::scale_color_host(avg);
      if (byte) ++st.bytes_changed;  // (against an all-zero image)
      if (out_rgb8) out_rgb8[3 * i + c] = byte;
      if (out_linear) out_linear[3 * i + c] = avg;
    }
  }
  if (out) *out = st;
  return RT_OK;
}

int rt_checkpoint_error(const void* buf, size_t len, const rt_error_tol* tol, double* out_se, rt_error_stats* out) {
  rt::CkptView v{(const uint8_t*)buf, {}};
  int rc = rt_frame_checkpoint_info(buf, len, &v.d);
  if (rc) return rc;
  const rt_frame_blob_desc& b = v.d.blob;
  double abs_tol, rel_tol;
  if (!rt::error_tol(tol, abs_tol, rel_tol)) {
    rt::set_error("rt_checkpoint_error: abs_tol and rel_tol must be >= 0 and not NaN");
    return RT_E_INVALID;
  }
  if (!(v.d.sections & RT_CKPT_MOMENTS) || b.chunks_done < 2) {
    rt::set_error("rt_checkpoint_error: needs a checkpoint with RT_CKPT_MOMENTS and at least 2 chunks");
    return RT_E_INVALID;
  }
  rt_error_stats st{};
  st.chunks_done = b.chunks_done;
  st.samples_done = b.samples_done;
  st.pixels = b.pixels;
  const uint64_t nan_bits = 0x7ff8000000000000ull;  // (the device's NaN for a pixel stopped before 2 chunks)
  double total = 0.0;  // (over the finite pixels' channels, in pixel and channel order)
  for (int64_t i = 0; i < b.pixels; ++i) {
    double s[3], q[3], se[3];
    int chunks, samples;
    v.sums(i, s);
    v.moments(i, q);
    v.counts(i, chunks, samples);
    int cls = rt::kPixelNonFinite;
    if (chunks >= 2)
      cls = rt::pixel_error(s, q, chunks, samples, abs_tol, rel_tol, se);
    else
      for (int c = 0; c < 3; ++c) std::memcpy(&se[c], &nan_bits, 8);
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
  const int64_t finite = st.pixels - st.nonfinite_pixels;
  st.mean_se = finite ? total / (double)(3 * finite) : 0.0;
  if (out) *out = st;
  return RT_OK;
}

int rt_frame_chunking(int64_t pixels, int spp, int* out_chunk, int* out_chunks_total) {
  if (pixels <= 0 || pixels >= (1ll << 32) || spp <= 0 || spp > INT32_MAX - RT_CHUNK_MAX || !out_chunk ||
      !out_chunks_total) {
    rt::set_error("rt_frame_chunking: pixels must be in [1, 2^32), spp in [1, 2^31 - 1 - RT_CHUNK_MAX]");
    return RT_E_INVALID;
  }
  *out_chunk = rt_sample_chunk(pixels, spp);
  *out_chunks_total = (spp + *out_chunk - 1) / *out_chunk;
  return RT_OK;
}

int rt_scene_fingerprint(const rt_scene_desc* desc, uint64_t* out) {
  if (!desc || !out) {
    rt::set_error("rt_scene_fingerprint: null argument");
    return RT_E_INVALID;
  }
  *out = rt::scene_fingerprint(desc);
  return RT_OK;
}

}  // extern "C"
