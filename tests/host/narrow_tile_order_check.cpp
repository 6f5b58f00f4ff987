// Stand-alone check of the tile-order folded qkv images for "fused_narrow" (heads of 32 columns in pairs, 16 in quads: embed_dim 256 and
// 128 with 8 heads), built with AddressSanitizer + UBSan and run as an ordinary program by tests/test_fused_narrow_host.py.  Host functions
// of diff3dhpe_amd/csrc/weight_pack.hip only.  A pair / a quad of heads is one 64-column segment, so the images are ordered by D / 64
// pseudo-heads: tile-order row 192 s + 48 wn + 16 part + x is original row D part + 64 s + 16 wn + x (part 0 / 1 / 2 = q / k / v).  That
// formula is stated here with loops of its own; tile_order_src_row is compared against it, not used to form it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "weight_pack.h"

using namespace d3d;

static int g_fail = 0;
#define CHECK(cond, ...)                                                       \
  do {                                                                         \
    if (!(cond)) {                                                             \
      if (++g_fail <= 20) { printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
    }                                                                          \
  } while (0)

static uint32_t h32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static std::vector<float> hvec(uint32_t tag, size_t n, float scale, float offset = 0.f) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i)
    v[i] = offset + scale * ((float)((int32_t)(h32(tag * 0x9e3779b9u + (uint32_t)i) >> 8) - (1 << 23)) / (float)(1 << 23));
  return v;
}

// the expected source row of every tile-order row, D / 64 segments of 192 rows
static std::vector<size_t> expected_rows(size_t D) {
  std::vector<size_t> src;
  for (size_t s = 0; s < D / 64; ++s)
    for (size_t wn = 0; wn < 4; ++wn)
      for (size_t part = 0; part < 3; ++part)
        for (size_t x = 0; x < 16; ++x) src.push_back(D * part + 64 * s + 16 * wn + x);
  return src;
}

struct Model {
  std::vector<std::vector<float>> t;   // per block: n1g n1b qkvw qkvb projw projb n2g n2b fc1w fc1b fc2w fc2b
  std::vector<BlockSrc> src;
};

static Model make_model(size_t D, size_t Dm, size_t nblk, float gain) {
  Model m;
  const float ws = 1.0f / std::sqrt((float)D);
  for (size_t k = 0; k < nblk; ++k) {
    const uint32_t g = 100 * (uint32_t)(k + 1) + (uint32_t)D;
    m.t.push_back(hvec(g + 1, D, 0.2f * gain, gain));      // norm1 gain around `gain`
    m.t.push_back(hvec(g + 2, D, 0.2f));
    m.t.push_back(hvec(g + 3, 3 * D * D, ws));
    m.t.push_back(hvec(g + 4, 3 * D, 0.5f));
    m.t.push_back(hvec(g + 5, D * D, ws));
    m.t.push_back(hvec(g + 6, D, 0.5f));
    m.t.push_back(hvec(g + 7, D, 0.2f, 1.0f));
    m.t.push_back(hvec(g + 8, D, 0.2f));
    m.t.push_back(hvec(g + 9, Dm * D, ws));
    m.t.push_back(hvec(g + 10, Dm, 0.5f));
    m.t.push_back(hvec(g + 11, D * Dm, ws));
    m.t.push_back(hvec(g + 12, D, 0.5f));
  }
  for (size_t k = 0; k < nblk; ++k) {
    const std::vector<float>* p = &m.t[12 * k];
    m.src.push_back(BlockSrc{p[0].data(), p[1].data(), p[2].data(), p[3].data(), p[4].data(), p[5].data(), p[6].data(), p[7].data(),
                             p[8].data(), p[9].data(), p[10].data(), p[11].data()});
  }
  return m;
}

// the whole commit at width D with D / 64 pseudo-heads; tile_s / tile_t: which block types get the images; want_k: the folded qkv exponent
static void check_pack(size_t D, bool tile_s, bool tile_t, float gain, int want_k) {
  const size_t Dm = 2 * D, nblk = 4, rows = 3 * D;
  Model m = make_model(D, Dm, nblk, gain);
  if (want_k < 12) m.t[2][5 * D + 7] = 8.0f;   // block 0's qkv weight: one entry whose folded value leaves the 2^12 range
  PackedWeights pk;
  CHECK(pack_f16x3(m.src, D, Dm, D / 64, tile_s, tile_t, pk), "D = %zu: pack_f16x3 refused (exponent check)", D);
  CHECK(pk.blk.size() == nblk, "D = %zu: %zu blocks", D, pk.blk.size());
  CHECK(!pk.clamped, "D = %zu: finite weights reported as clamped", D);
  const std::vector<size_t> want = expected_rows(D);
  CHECK(want.size() == rows, "D = %zu: %zu expected rows", D, want.size());
  for (size_t k = 0; k < pk.blk.size(); ++k) {
    const BlockOff& b = pk.blk[k];
    const bool has = (k & 1) ? tile_t : tile_s;
    CHECK((b.qkv_f3h != NO_OFF) == has && (b.qkv_csh != NO_OFF) == has && (b.qkv_fbh != NO_OFF) == has, "D = %zu block %zu: images %s", D, k,
          has ? "missing" : "present without being asked for");
    if (k == 0) CHECK(b.qkv_fe == want_k, "D = %zu: folded qkv exponent %d, expected %d", D, b.qkv_fe, want_k);
    if (!has || b.qkv_f3h == NO_OFF) continue;
    CHECK(b.qkv_f3h + 2 * pad256(rows) * D <= pk.planes.size(), "D = %zu block %zu: image leaves the arena", D, k);
    CHECK(b.qkv_fbh + rows <= pk.fold.size() && b.qkv_csh + rows <= pk.fold.size(), "D = %zu block %zu: fold vectors leave the arena", D, k);
    for (size_t r = 0; r < rows; ++r) {
      const size_t s = want[r];
      CHECK(tile_order_src_row(r, D, D / 64) == s, "D = %zu: tile_order_src_row(%zu) = %zu, expected %zu", D, r, tile_order_src_row(r, D, D / 64), s);
      // the same planes as the untiled folded image's row: same values, same exponent
      CHECK(memcmp(&pk.planes[b.qkv_f3h + r * 2 * D], &pk.planes[b.qkv_f3 + s * 2 * D], 2 * D * sizeof(uint16_t)) == 0,
            "D = %zu block %zu: image row %zu is not folded row %zu", D, k, r, s);
      CHECK(memcmp(&pk.fold[b.qkv_csh + r], &pk.fold[b.qkv_cs + s], sizeof(float)) == 0, "D = %zu block %zu: csum row %zu", D, k, r);
      CHECK(memcmp(&pk.fold[b.qkv_fbh + r], &pk.fold[b.qkv_fb + s], sizeof(float)) == 0, "D = %zu block %zu: bias row %zu", D, k, r);
    }
    for (size_t i = b.qkv_f3h + rows * 2 * D; i < b.qkv_f3h + 2 * pad256(rows) * D; ++i) CHECK(pk.planes[i] == 0, "pad element %zu not zero", i);
  }
}

// tile_order_copy alone, as the op hook calls it: a permutation of the rows, every source row exactly once
static void check_copy(size_t D) {
  const size_t rows = 3 * D;
  const std::vector<float> W = hvec(7, rows * D, 1.0f / std::sqrt((float)D)), b = hvec(8, rows, 0.5f), g = hvec(9, D, 0.2f, 1.0f), be = hvec(10, D, 0.2f);
  std::vector<float> wg(rows * D), cs(rows), fb(rows), cs_t(rows), fb_t(rows);
  fold_layernorm(W.data(), b.data(), g.data(), be.data(), rows, D, wg.data(), cs.data(), fb.data());
  std::vector<uint16_t> flat(2 * rows * D, 0), tiled(2 * rows * D, 0);
  const int k0 = split_weight_f16x3(wg.data(), rows, D, flat.data());
  const int k1 = tile_order_copy(wg.data(), cs.data(), fb.data(), D, D / 64, tiled.data(), cs_t.data(), fb_t.data());
  CHECK(k0 == k1, "D = %zu: exponents %d / %d", D, k0, k1);
  const std::vector<size_t> want = expected_rows(D);
  std::vector<int> seen(rows, 0);
  for (size_t r = 0; r < rows; ++r) {
    const size_t s = want[r];
    ++seen[s];
    CHECK(memcmp(&tiled[r * 2 * D], &flat[s * 2 * D], 2 * D * sizeof(uint16_t)) == 0, "D = %zu: copy row %zu is not row %zu", D, r, s);
    CHECK(memcmp(&cs_t[r], &cs[s], sizeof(float)) == 0 && memcmp(&fb_t[r], &fb[s], sizeof(float)) == 0, "D = %zu: fold row %zu", D, r);
  }
  for (size_t s = 0; s < rows; ++s) CHECK(seen[s] == 1, "D = %zu: source row %zu used %d times", D, s, seen[s]);
}

int main() {
  for (size_t D : {(size_t)256, (size_t)128}) {
    check_copy(D);
    check_pack(D, true, true, 1.0f, 12);
    check_pack(D, true, false, 1.0f, 12);    // a window of more than 127 frames: spatial images alone
    check_pack(D, true, true, 6.0f, 10);     // gain 6 x weight 8 = 48: the per-matrix exponent drops to 10 in both images
  }
  if (g_fail) { printf("narrow_tile_order_check: %d failures\n", g_fail); return 1; }
  printf("narrow_tile_order_check: ok\n");
  return 0;
}
