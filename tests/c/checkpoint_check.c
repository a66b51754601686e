/*
 * checkpoint_check.c — the version-2 checkpoint (include/rt.h) on the host alone: rt_frame_checkpoint_info,
 * rt_checkpoint_resolve and rt_checkpoint_error, built with AddressSanitizer + UBSan together with
 * ray-tracing_amd/csrc/rt_frame_blob.cpp (tests/test_checkpoint_host.py compiles and runs it). The blobs are
 * built here from the layout rt.h documents, byte by byte, for all four section combinations. Every buffer
 * handed to the library is a heap block of exactly the length passed, and every output a heap block of
 * exactly the size rt.h states, so a read or write past either is a sanitizer report. Whatever parses, after
 * a header byte was changed or at a shorter length, is also run through the two offline calls.
 */
#include <math.h>
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
static void putf64(unsigned char* p, double x) {
  uint64_t bits;
  memcpy(&bits, &x, 8);
  put64(p, bits);
}

/* an 8x8 frame at 40 spp (CH = 1), 7 chunks done */
enum { W = 8, H = 8, SPP = 40, DONE = 7, PIXELS = W * H, HEADER = RT_FRAME_CKPT_HEADER };

static size_t total_of(uint32_t sections) {
  return HEADER + (size_t)PIXELS * (24 + ((sections & RT_CKPT_MOMENTS) ? 24 : 0) + ((sections & RT_CKPT_STOPS) ? 4 : 0));
}

/* a well-formed checkpoint with `sections`: sums with NaN and infinite channels, moments above S^2 / N, and K
   from 0 to DONE */
static void make_ckpt(unsigned char* b, uint32_t sections) {
  const size_t total = total_of(sections);
  memset(b, 0, total);
  memcpy(b, "RTFRAME\0", 8);
  put32(b + 8, RT_FRAME_CKPT_VERSION);
  put32(b + 16, W);
  put32(b + 20, H);
  put32(b + 24, SPP);
  put32(b + 28, 10);
  put32(b + 32, RT_RNG_PHILOX);
  put64(b + 40, 1024);
  put32(b + 48, 8);
  put32(b + 56, 1);
  for (int i = 0; i < 24; ++i) putf64(b + 64 + 8 * i, 0.5 + i);
  put32(b + 256, (uint32_t)rt_sample_chunk(PIXELS, SPP));
  put32(b + 260, DONE);
  put64(b + 264, PIXELS);
  put64(b + 272, 0x0123456789abcdefULL);
  put64(b + 280, total - HEADER);
  put32(b + 288, sections);
  unsigned char* at = b + HEADER;
  for (int i = 0; i < PIXELS; ++i)
    for (int c = 0; c < 3; ++c) {
      double s = 0.25 * (i + 1) + c;
      if (i % 11 == 3 && c == 1) s = NAN;
      if (i % 13 == 5 && c == 2) s = INFINITY;
      putf64(at + 24 * i + 8 * c, s);
    }
  at += 24 * PIXELS;
  if (sections & RT_CKPT_MOMENTS) {
    for (int i = 0; i < PIXELS; ++i)
      for (int c = 0; c < 3; ++c) {
        const double s = 0.25 * (i + 1) + c;
        putf64(at + 24 * i + 8 * c, s * s / DONE + 0.01 * (i % 5));
      }
    at += 24 * PIXELS;
  }
  if (sections & RT_CKPT_STOPS)
    for (int i = 0; i < PIXELS; ++i) put32(at + 4 * i, (uint32_t)(i % 3 == 0 ? i % (DONE + 1) : 0));
}

/* The three calls on the first `len` bytes of `src`, handed over in a heap block of that size, with outputs of
   exactly the documented sizes. Returns rt_frame_checkpoint_info's verdict. */
static int run_all(const unsigned char* src, size_t len, rt_frame_ckpt_desc* out) {
  unsigned char* q = (unsigned char*)malloc(len ? len : 1);
  if (!q) abort();
  memcpy(q, src, len);
  rt_frame_ckpt_desc d;
  const int rc = rt_frame_checkpoint_info(q, len, &d);
  if (rc == RT_OK) {
    const size_t n = (size_t)d.blob.pixels * 3;
    uint8_t* rgb = (uint8_t*)malloc(n);
    double* lin = (double*)malloc(n * sizeof(double));
    double* se = (double*)malloc(n * sizeof(double));
    if (!rgb || !lin || !se) abort();
    rt_frame_stats fs;
    rt_error_stats es;
    const int r1 = rt_checkpoint_resolve(q, len, rgb, lin, &fs);
    EXPECT(r1 == (d.blob.chunks_done > 0 ? RT_OK : RT_E_INVALID), "resolve of a parsed blob: %d", r1);
    if (r1 == RT_OK) {
      EXPECT(fs.chunks_done == d.blob.chunks_done && fs.kernel_ms == 0.0 && fs.nan_pixels <= d.blob.pixels, "resolve stats");
      EXPECT(rt_checkpoint_resolve(q, len, NULL, NULL, NULL) == RT_OK, "resolve with null outputs");
    }
    const int want = (d.sections & RT_CKPT_MOMENTS) && d.blob.chunks_done >= 2 ? RT_OK : RT_E_INVALID;
    const int r2 = rt_checkpoint_error(q, len, NULL, se, &es);
    EXPECT(r2 == want, "error of a parsed blob: %d, expected %d", r2, want);
    if (r2 == RT_OK) {
      EXPECT(es.pixels == d.blob.pixels && es.nonfinite_pixels <= es.pixels, "error stats");
      EXPECT(rt_checkpoint_error(q, len, NULL, NULL, NULL) == RT_OK, "error with null outputs");
    }
    free(rgb);
    free(lin);
    free(se);
    if (out) *out = d;
  } else {
    EXPECT(strstr(rt_last_error(), "frame blob:") != NULL, "error text '%s'", rt_last_error());
    EXPECT(rt_checkpoint_resolve(q, len, NULL, NULL, NULL) == RT_E_INVALID, "resolve of a rejected blob");
    EXPECT(rt_checkpoint_error(q, len, NULL, NULL, NULL) == RT_E_INVALID, "error of a rejected blob");
  }
  free(q);
  return rc;
}

int main(void) {
  const size_t cap = total_of(3u) + 1;
  unsigned char* good = (unsigned char*)malloc(cap);
  unsigned char* bad = (unsigned char*)malloc(cap);
  if (!good || !bad) return 2;
  long parsed_mutations = 0;

  EXPECT(sizeof(rt_frame_ckpt_desc) == 344 && sizeof(rt_frame_blob_desc) == 288, "descriptor sizes");
  EXPECT(rt_frame_checkpoint_info(NULL, 320, NULL) == RT_E_INVALID, "null blob");
  EXPECT(rt_checkpoint_resolve(NULL, 320, NULL, NULL, NULL) == RT_E_INVALID, "null blob (resolve)");
  EXPECT(rt_checkpoint_error(NULL, 320, NULL, NULL, NULL) == RT_E_INVALID, "null blob (error)");

  for (uint32_t sections = 0; sections < 4; ++sections) {
    const size_t total = total_of(sections);
    make_ckpt(good, sections);
    good[total] = 0;
    rt_frame_ckpt_desc d;
    EXPECT(run_all(good, total, &d) == RT_OK, "sections %u: the well-formed checkpoint is rejected: %s", sections,
           rt_last_error());
    EXPECT(d.blob.version == 2 && d.sections == sections && d.blob.payload_bytes == total - HEADER, "sections %u: header", sections);
    EXPECT(d.blob.chunks_done == DONE && d.blob.samples_done == DONE && d.blob.pixels == PIXELS, "sections %u: counts", sections);
    EXPECT(d.sums_offset == HEADER, "sums offset");
    EXPECT(d.moments_offset == ((sections & RT_CKPT_MOMENTS) ? HEADER + 24u * PIXELS : 0u), "moments offset");
    EXPECT(d.stops_offset == ((sections & RT_CKPT_STOPS) ? total - 4u * PIXELS : 0u), "stops offset");
    EXPECT(d.active_pixels + d.stopped_pixels == PIXELS && d.stopped_nan <= d.stopped_pixels, "pixel counts");
    EXPECT((d.stopped_pixels > 0) == ((sections & RT_CKPT_STOPS) != 0), "stopped pixels");
    EXPECT(rt_frame_checkpoint_info(good, total, NULL) == RT_OK, "a null out is allowed");

    /* every length from 0 to the full blob, and one byte too many */
    for (size_t len = 0; len < total; ++len)
      EXPECT(run_all(good, len, NULL) == RT_E_INVALID, "sections %u truncated to %zu bytes: accepted", sections, len);
    EXPECT(run_all(good, total + 1, NULL) == RT_E_INVALID, "sections %u, one byte too long: accepted", sections);

    /* every header byte, changed three ways; what still parses goes through the offline calls */
    static const unsigned char flips[3] = {0x01, 0x80, 0xff};
    for (size_t off = 0; off < HEADER; ++off)
      for (int m = 0; m < 3; ++m) {
        memcpy(bad, good, total);
        bad[off] ^= flips[m];
        const int rc = run_all(bad, total, &d);
        EXPECT(rc == RT_OK || rc == RT_E_INVALID, "header byte %zu: rc %d", off, rc);
        if (rc == RT_OK) ++parsed_mutations;
        /* magic, version, width, height, CH, the pixel count, the payload size, the sections and the reserved
           bytes cannot change unnoticed (spp, chunks_done, the camera and the like can stay well formed) */
        if (off < 12 || (off >= 16 && off < 24) || (off >= 256 && off < 260) || (off >= 264 && off < 272) || off >= 280)
          EXPECT(rc == RT_E_INVALID, "sections %u: header byte %zu ^ %02x accepted", sections, off, flips[m]);
      }

    /* K outside [0, chunks_done] */
    if (sections & RT_CKPT_STOPS) {
      memcpy(bad, good, total);
      put32(bad + total - 4, 0xffffffffu);
      EXPECT(run_all(bad, total, NULL) == RT_E_INVALID, "K = -1: accepted");
      put32(bad + total - 4, DONE + 1);
      EXPECT(run_all(bad, total, NULL) == RT_E_INVALID, "K = chunks_done + 1: accepted");
      put32(bad + total - 4, DONE);
      EXPECT(run_all(bad, total, NULL) == RT_OK, "K = chunks_done: rejected");
    }
    /* a section flagged but absent */
    if (sections != 3u) {
      memcpy(bad, good, total);
      put32(bad + 288, 3u);
      EXPECT(run_all(bad, total, NULL) == RT_E_INVALID, "sections %u flagged as 3: accepted", sections);
    }
    memcpy(bad, good, total);
    put32(bad + 288, sections | 4u);
    EXPECT(run_all(bad, total, NULL) == RT_E_INVALID, "an unknown section bit: accepted");
  }
  EXPECT(parsed_mutations > 0, "no mutated header parsed: the offline calls ran on the well-formed blobs only");

  free(good);
  free(bad);
  printf("checkpoint_check: %s (%d failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
