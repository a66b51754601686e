/*
 * frame_blob_check.c — rt_frame_blob_info (the saved progressive frame's header, include/rt.h) on the
 * host alone, built with AddressSanitizer + UBSan together with ray-tracing_amd/csrc/rt_frame_blob.cpp
 * (tests/test_progressive_host.py compiles and runs it). The blob is built here from the layout rt.h
 * documents, byte by byte, not with the library's writer. Every buffer handed to the parser is a heap
 * block of exactly the length passed, so a read past the length is a sanitizer report.
 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "rt.h"

static int failures = 0;
#define EXPECT(cond, ...)                 \
  do {                                    \
    if (!(cond)) {                        \
      ++failures;                         \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                \
      printf("\n");                       \
    }                                     \
  } while (0)

static void put32(unsigned char* p, uint32_t v) {
  for (int i = 0; i < 4; ++i) p[i] = (unsigned char)(v >> (8 * i));
}
static void put64(unsigned char* p, uint64_t v) {
  for (int i = 0; i < 8; ++i) p[i] = (unsigned char)(v >> (8 * i));
}

enum { W = 8, H = 8, SPP = 40, PIXELS = W * H, PAYLOAD = PIXELS * 24, TOTAL = RT_FRAME_BLOB_HEADER + PAYLOAD };

/* a well-formed blob of an 8x8 frame at 40 spp (CH = 1: 2560 samples fill no work-item), 7 chunks done */
static void make_blob(unsigned char* b) {
  memset(b, 0, TOTAL);
  memcpy(b, "RTFRAME\0", 8);
  put32(b + 8, RT_FRAME_BLOB_VERSION);
  put32(b + 12, 0);
  put32(b + 16, W);
  put32(b + 20, H);
  put32(b + 24, SPP);
  put32(b + 28, 10);
  put32(b + 32, RT_RNG_PHILOX);
  put32(b + 36, 0);
  put64(b + 40, 1024);
  put32(b + 48, 8);
  put32(b + 52, 0);
  put32(b + 56, 1);
  put32(b + 60, 0);
  for (int i = 0; i < 24; ++i) {
    const double x = 0.5 + i;
    uint64_t bits;
    memcpy(&bits, &x, 8);
    put64(b + 64 + 8 * i, bits);
  }
  put32(b + 256, (uint32_t)rt_sample_chunk(PIXELS, SPP));
  put32(b + 260, 7);
  put64(b + 264, PIXELS);
  put64(b + 272, 0x0123456789abcdefULL);
  put64(b + 280, PAYLOAD);
}

/* the parser's verdict on the first `len` bytes of `src`, handed over in a heap block of that size */
static int info_of(const unsigned char* src, size_t len, rt_frame_blob_desc* out) {
  unsigned char* q = (unsigned char*)malloc(len ? len : 1);
  if (!q) abort();
  memcpy(q, src, len);
  const int rc = rt_frame_blob_info(q, len, out);
  free(q);
  return rc;
}

int main(void) {
  unsigned char* good = (unsigned char*)malloc(TOTAL + 1);
  unsigned char* bad = (unsigned char*)malloc(TOTAL + 1);
  if (!good || !bad) return 2;
  make_blob(good);
  good[TOTAL] = 0;

  rt_frame_blob_desc d;
  EXPECT(info_of(good, TOTAL, &d) == RT_OK, "the well-formed blob is rejected: %s", rt_last_error());
  EXPECT(d.version == 1 && d.params.width == W && d.params.height == H && d.params.spp == SPP, "params");
  EXPECT(d.params.max_depth == 10 && d.params.seed == 1024 && d.params.tile == 8, "params (2)");
  EXPECT(d.chunk == 1 && d.chunks_total == 40 && d.chunks_done == 7 && d.samples_done == 7, "chunks");
  EXPECT(d.pixels == PIXELS && d.payload_bytes == PAYLOAD && d.scene_fingerprint == 0x0123456789abcdefULL, "sizes");
  EXPECT(d.camera.origin[0] == 0.5 && d.camera.t1 == 23.5, "camera");
  EXPECT(info_of(good, TOTAL, NULL) == RT_OK, "a null out is allowed");
  EXPECT(rt_frame_blob_info(NULL, TOTAL, &d) == RT_E_INVALID, "null blob");

  /* every truncation of the blob, header and payload, and one byte too many */
  for (size_t len = 0; len < TOTAL; ++len)
    EXPECT(info_of(good, len, &d) == RT_E_INVALID, "truncated to %zu bytes: accepted", len);
  EXPECT(info_of(good, TOTAL + 1, &d) == RT_E_INVALID, "one byte too long: accepted");

  /* single-field corruptions */
  struct {
    const char* what;
    size_t off;
    int width; /* 4 or 8 bytes */
    uint64_t value;
  } cases[] = {
      {"magic", 0, 4, 0x46545258u},
      {"version 0", 8, 4, 0},
      {"version 2", 8, 4, 2},
      {"width 0", 16, 4, 0},
      {"width -8", 16, 4, 0xfffffff8u},
      {"height 0", 20, 4, 0},
      {"spp 0", 24, 4, 0},
      {"max_depth -1", 28, 4, 0xffffffffu},
      {"tier A", 32, 4, RT_RNG_EXACT},
      {"tile 12", 48, 4, 12},
      {"CH 2", 256, 4, 2},
      {"CH 0", 256, 4, 0},
      {"chunks_done 41", 260, 4, 41},
      {"chunks_done -1", 260, 4, 0xffffffffu},
      {"pixels 65", 264, 8, 65},
      {"payload short", 280, 8, PAYLOAD - 24},
      {"payload huge", 280, 8, ~0ull},
      {"width 2^31 - 1", 16, 4, 0x7fffffffu},
      {"spp 2^31 - 1", 24, 4, 0x7fffffffu},
  };
  for (size_t i = 0; i < sizeof cases / sizeof cases[0]; ++i) {
    memcpy(bad, good, TOTAL);
    if (cases[i].width == 4) put32(bad + cases[i].off, (uint32_t)cases[i].value);
    else put64(bad + cases[i].off, cases[i].value);
    EXPECT(info_of(bad, TOTAL, &d) == RT_E_INVALID, "%s: accepted", cases[i].what);
    EXPECT(strstr(rt_last_error(), "frame blob") != NULL, "%s: error text '%s'", cases[i].what, rt_last_error());
  }
  /* the ends of the chunk range are in range */
  memcpy(bad, good, TOTAL);
  put32(bad + 260, 0);
  EXPECT(info_of(bad, TOTAL, &d) == RT_OK && d.samples_done == 0, "chunks_done 0");
  put32(bad + 260, 40);
  EXPECT(info_of(bad, TOTAL, &d) == RT_OK && d.samples_done == 40, "chunks_done = chunks_total");

  free(good);
  free(bad);
  printf("frame_blob_check: %s (%d failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
