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

}  // namespace rt
