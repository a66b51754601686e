// rt_frame_blob.cpp — the host half of progressive frames (include/rt.h): the saved frame's header
// (layout, writer, parser and validation) and the scene fingerprint. No HIP, no device: it builds
// for the CPU as is (tests/c/frame_blob_check.c drives it under the sanitizers).
#include <cstring>
#include <string>

#include "rt.h"
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

const char* blob_parse(const void* buf, size_t len, rt_frame_blob_desc* out) {
  if (!buf) return "null blob";
  if (len < RT_FRAME_BLOB_HEADER) return "truncated: shorter than the header";
  const uint8_t* in = (const uint8_t*)buf;
  if (std::memcmp(in, kMagic, 8) != 0) return "bad magic";
  rt_frame_blob_desc b;
  std::memset(&b, 0, sizeof b);
  b.version = get_u32(in + kOffVersion);
  if (b.version != RT_FRAME_BLOB_VERSION) return "unknown blob version";
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
  if (b.payload_bytes != (uint64_t)pixels * 24) return "payload size disagrees with the pixel count";
  if (len - RT_FRAME_BLOB_HEADER != b.payload_bytes) return "length disagrees with the header";
  if (out) *out = b;
  return nullptr;
}

}  // namespace rt

extern "C" {

int rt_frame_blob_info(const void* buf, size_t len, rt_frame_blob_desc* out) {
  if (const char* why = rt::blob_parse(buf, len, out)) {
    rt::set_error(std::string("frame blob: ") + why);
    return RT_E_INVALID;
  }
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
