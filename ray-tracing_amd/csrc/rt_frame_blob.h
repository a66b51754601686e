// rt_frame_blob.h — the saved progressive frame's header and the scene fingerprint (rt_frame_blob.cpp,
// host only; layout in include/rt.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include "rt.h"

namespace rt {

// 64-bit FNV-1a over the caller's scene arrays, roots and background (rt.h, blob offset 272).
uint64_t scene_fingerprint(const rt_scene_desc* d);
// The RT_FRAME_BLOB_HEADER bytes of `b` (chunks_total and samples_done are derived, not stored).
void blob_write_header(const rt_frame_blob_desc& b, uint8_t* out);
// Parses and validates a blob of `len` bytes (rt_frame_blob_info's checks): nullptr and *out (may be
// null) filled when it is well formed, else what is wrong with it.
const char* blob_parse(const void* buf, size_t len, rt_frame_blob_desc* out);
// The RT_FRAME_CKPT_HEADER bytes of a version-2 checkpoint of `b` (its version and payload_bytes are
// written as version 2's: the bytes `sections` implies for b.pixels).
void ckpt_write_header(const rt_frame_blob_desc& b, uint32_t sections, uint8_t* out);
// Bytes that follow a checkpoint's header: pixels * (24 + 24 [Q] + 4 [K]).
uint64_t ckpt_payload_bytes(int64_t pixels, uint32_t sections);
// blob_parse for a version-1 or version-2 blob (rt_frame_checkpoint_info's checks and counts).
const char* ckpt_parse(const void* buf, size_t len, rt_frame_ckpt_desc* out);

}  // namespace rt
