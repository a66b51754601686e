// shard_block_check.cpp — the record slab's block map (rt_layout.h slab_geometry, slab_block, slab_slot_pixel,
// slab_owned_pixels) and the host merge that runs on it (rt_features.cpp rt_assemble_records_host) as a stand-alone
// program, for a CPU build under AddressSanitizer + UBSan (tests/test_features_shard_sanitize.py compiles and runs
// it). No HIP, no GPU. Over a grid of small geometries (W, H in 1..40 step 3, tile in {8, 16, 64}, 1..9 shards), over
// all shards, blocks and lanes: every image pixel is produced exactly once, at the slot the assemble kernel's
// formula (restated below) gives it; nothing maps outside the slab; the merge moves every record and reads no
// padding slot (the slabs are allocated to the byte, their padding poisoned).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "rt.h"
#include "rt_layout.h"

static int failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      if (failures < 20) std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                              \
    }                                                          \
  } while (0)

// rt_kernels.h assemble's map, restated: image pixel -> (shard, slot in that shard's slab).
static void assemble_slot(int px, int row, int tile, int tiles_x, int shards, int& shard, long long& slot) {
  const int gt = (row / tile) * tiles_x + (px / tile);
  shard = gt % shards;
  const long long lt = gt / shards;
  const int bpr = tile >> 3;
  const int bx = (px % tile) >> 3, by = (row % tile) >> 3;
  const int within = (by * bpr + bx) * 64 + (row & 7) * 8 + (px & 7);
  slot = lt * tile * tile + within;
}

struct Rec {
  uint64_t w[8];
};
static const uint64_t kPoison = 0xABABABABABABABABull;

int main() {
  long long geometries = 0, pixels_checked = 0;
  for (int W = 1; W <= 40; W += 3) {
    for (int H = 1; H <= 40; H += 3) {
      for (int tile : {8, 16, 64}) {
        for (int shards = 1; shards <= 9; ++shards) {
          rt_render_params p;
          std::memset(&p, 0, sizeof p);
          p.width = W, p.height = H, p.spp = 1, p.max_depth = 1, p.rng_mode = RT_RNG_PHILOX;
          p.tile = tile, p.shard_count = shards;
          CHECK(rtd::slab_params_error(&p) == nullptr);
          std::vector<int> seen((size_t)W * H, 0);
          std::vector<Rec> slabs, image((size_t)W * H);
          long long slab = 0, owned_sum = 0;
          for (int rank = 0; rank < shards; ++rank) {
            p.shard_rank = rank;
            const rtd::SlabGeometry G = rtd::slab_geometry(&p);
            if (rank == 0) {
              slab = G.slab;
              slabs.assign((size_t)(slab * shards), Rec{{kPoison, kPoison, kPoison, kPoison, kPoison, kPoison, kPoison, kPoison}});
            }
            CHECK(G.slab == slab && G.slab % 64 == 0 && G.blocks * 64 <= G.slab && G.blocks == G.owned_tiles * (tile / 8) * (tile / 8));
            long long owned = 0;
            for (long long b = 0; b < G.slab / 64; ++b) {
              int px0 = -1, row0 = -1;
              const bool in_image = rtd::slab_block(G, (uint32_t)b, px0, row0);
              CHECK(in_image == (b < G.blocks));  // (a shard's tiles inside the image are its first owned_tiles)
              for (int lane = 0; lane < 64; ++lane) {
                const long long slot = b * 64 + lane;
                const long long via_slot = rtd::slab_slot_pixel(G, (uint32_t)slot);
                if (!in_image) {
                  CHECK(via_slot == -1);
                  continue;
                }
                const int px = px0 + (lane & 7), row = row0 + (lane >> 3);
                CHECK(px >= 0 && row >= 0);
                if (px >= W || row >= H) {
                  CHECK(via_slot == -1);
                  continue;
                }
                const long long pid = (long long)row * W + px;
                CHECK(via_slot == pid);
                int shard = -1;
                long long want = -1;
                assemble_slot(px, row, tile, G.tiles_x, shards, shard, want);
                CHECK(shard == rank && want == slot && slot < G.slab);
                ++seen[(size_t)pid];
                ++owned;
                Rec& r = slabs[(size_t)(rank * slab + slot)];
                for (int k = 0; k < 8; ++k) r.w[k] = (uint64_t)pid * 8 + (uint64_t)k + 1;
              }
            }
            CHECK(owned == rtd::slab_owned_pixels(G));
            owned_sum += owned;
          }
          CHECK(owned_sum == (long long)W * H);
          for (int c : seen) CHECK(c == 1);
          p.shard_rank = 0;
          CHECK(rt_assemble_records_host(&p, slabs.data(), image.data()) == RT_OK);
          for (size_t i = 0; i < image.size(); ++i)
            for (int k = 0; k < 8; ++k) CHECK(image[i].w[k] == (uint64_t)i * 8 + (uint64_t)k + 1);
          ++geometries;
          pixels_checked += (long long)W * H;
        }
      }
    }
  }
  // what the entries reject of the frame and shard fields
  rt_render_params p;
  std::memset(&p, 0, sizeof p);
  p.width = 37, p.height = 21, p.rng_mode = RT_RNG_PHILOX, p.shard_count = 3;
  CHECK(rtd::slab_params_error(&p) == nullptr);  // (tile 0: the default)
  for (int tile : {12, 264, -8}) {
    p.tile = tile;
    CHECK(rtd::slab_params_error(&p) != nullptr);
  }
  p.tile = 16, p.shard_rank = 3;
  CHECK(rtd::slab_params_error(&p) != nullptr);
  p.shard_rank = 0, p.shard_count = -1;
  CHECK(rtd::slab_params_error(&p) != nullptr);
  p.shard_count = 0, p.shard_rank = 1;
  CHECK(rtd::slab_params_error(&p) != nullptr);
  p.shard_rank = 0, p.width = 0;
  CHECK(rtd::slab_params_error(&p) != nullptr);
  p.width = 65536, p.height = 65536;
  CHECK(rtd::slab_params_error(&p) != nullptr);
  p.width = 65535, p.height = 65536, p.tile = 256, p.shard_count = 1;  // (the slab's padding takes it to 2^32 slots)
  CHECK(rtd::slab_params_error(&p) != nullptr);
  Rec one{};
  CHECK(rt_assemble_records_host(nullptr, &one, &one) == RT_E_INVALID);
  CHECK(rt_assemble_records_host(&p, &one, &one) == RT_E_INVALID);
  std::printf("shard_block_check: %lld geometries, %lld pixels\n", geometries, pixels_checked);
  std::printf("shard_block_check: %s (%d failures)\n", failures ? "FAILED" : "clean", failures);
  return failures ? 1 : 0;
}
