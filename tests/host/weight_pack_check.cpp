// Stand-alone check of the host-side weight packing (diff3dhpe_amd/csrc/weight_pack.hip), built with AddressSanitizer + UBSan and run as an
// ordinary program by tests/test_weight_pack_host.py.  Every expectation is computed here with plain loops of its own, from the formulas in
// the comments of weight_pack.h / d3d_kernels.h -- none of the unit's helpers is used to form an expectation.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
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

// fixed integer hash -> a multiple of 2^-23 in [-1, 1) (exact in fp32), times scale
static uint32_t h32(uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; }
static float hval(uint32_t tag, size_t i, float scale) {
  return scale * ((float)((int32_t)(h32(tag * 0x9e3779b9u + (uint32_t)i) >> 8) - (1 << 23)) / (float)(1 << 23));
}
static std::vector<float> hvec(uint32_t tag, size_t n, float scale, float offset = 0.f) {
  std::vector<float> v(n);
  for (size_t i = 0; i < n; ++i) v[i] = offset + hval(tag, i, scale);
  return v;
}
static double f16(uint16_t b) { _Float16 h; memcpy(&h, &b, 2); return (double)h; }
static bool same(const void* a, const void* b, size_t bytes) { return memcmp(a, b, bytes) == 0; }
// the pair layout, as d3d_kernels.h words it: k-tile t of 32 columns holds its hi values at [64 t, 64 t + 32), lo 32 further on; the
// accumulator order puts column 16 jj + 4 q + r of a group into slot 8 q + 4 jj + r
static size_t pc(size_t c) { return c / 32 * 64 + c % 32; }
static size_t pc_acc(size_t c) { const size_t w = c % 32, jj = w / 16, q = (w % 16) / 4, r = w % 4; return c / 32 * 64 + 8 * q + 4 * jj + r; }
static size_t pad(size_t n) { return (n + 255) / 256 * 256; }

static void check_split_matrix(const std::vector<float>& w, size_t rows, size_t cols, bool acc, int want_k) {
  std::vector<uint16_t> pr(2 * pad(rows) * cols, 0);
  bool clamped = false;
  const int k = split_weight_f16x3(w.data(), rows, cols, pr.data(), acc, &clamped);
  CHECK(k == want_k, "k = %d, expected %d", k, want_k);
  CHECK(!clamped, "finite matrix reported as clamped");
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c) {
      const size_t o = r * 2 * cols + (acc ? pc_acc(c) : pc(c));
      const double s = std::ldexp((double)w[r * cols + c], k), err = std::fabs(f16(pr[o]) + f16(pr[o + 32]) - s);
      CHECK(err <= std::max(std::ldexp(std::fabs(s), -22), std::ldexp(1.0, -25)), "split error %g at (%zu, %zu), s = %g", err, r, c, s);
    }
  for (size_t i = rows * 2 * cols; i < pr.size(); ++i) CHECK(pr[i] == 0, "pad element %zu not zero", i);
}

static void check_split() {
  const size_t rows = 300, cols = 96;   // rows pad to 512; three k-tiles
  std::vector<float> w = hvec(1, rows * cols, 1.0f);
  for (size_t i = 0; i < w.size(); i += 7) w[i] = std::ldexp(w[i], -(int)(i % 23));   // small entries: lo (and hi) halves in fp16 subnormals
  w[5] = 15.99f; w[6] = -15.99f;
  check_split_matrix(w, rows, cols, false, 12);
  check_split_matrix(w, rows, cols, true, 12);
  w[777] = 48.0f;
  check_split_matrix(w, rows, cols, false, 10);
  for (float bad : {std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN()}) {
    std::vector<float> v = hvec(2, 64 * 32, 1.0f);
    v[100] = bad;
    std::vector<uint16_t> pr(2 * pad(64) * 32, 0);
    bool clamped = false;
    (void)split_weight_f16x3(v.data(), 64, 32, pr.data(), false, &clamped);
    CHECK(clamped, "non-finite entry not reported");
  }
}

static void check_bf16() {
  const float inf = std::numeric_limits<float>::infinity();
  auto bits = [](uint32_t u) { float f; memcpy(&f, &u, 4); return f; };
  struct { float in; uint16_t out; bool flag; } cases[] = {
      {1.0f, 0x3f80, false}, {1.0f + std::ldexp(1.0f, -8), 0x3f80, false}, {1.0f + 3 * std::ldexp(1.0f, -8), 0x3f82, false},
      {-2.5f, 0xc020, false}, {0.0f, 0x0000, false}, {bits(0x7f7fffffu), 0x7f80, true}, {inf, 0x7f80, true}};
  for (auto& c : cases) {
    bool flag = false;
    const uint16_t o = bf16_rne(c.in, &flag);
    CHECK(o == c.out && flag == c.flag, "bf16(%g) = %#x flag %d, expected %#x flag %d", c.in, o, flag, c.out, c.flag);
  }
  bool flag = false;
  const uint16_t n = bf16_rne(std::numeric_limits<float>::quiet_NaN(), &flag);
  CHECK((n & 0x7f80) == 0x7f80 && (n & 0x7f) != 0 && flag, "bf16(NaN) = %#x flag %d", n, flag);
  const uint16_t n2 = bf16_rne(bits(0x7f800001u), &flag);   // a NaN whose payload sits below the bf16 mantissa
  CHECK((n2 & 0x7f80) == 0x7f80 && (n2 & 0x7f) != 0, "bf16(NaN, low payload) = %#x", n2);
}

struct Model {   // one spatial + one temporal block of D = 512, H = 8, Dm = 1024
  static constexpr size_t D = 512, H = 8, Dm = 1024;
  struct Blk { std::vector<float> n1g, n1b, qkvw, qkvb, projw, n2g, n2b, fc1w, fc1b, fc2w; } b[2];
  std::vector<BlockSrc> src;
  Model() {
    for (uint32_t k = 0; k < 2; ++k) {
      Blk& x = b[k];
      const uint32_t t = 16 * (k + 1);
      x.n1g = hvec(t + 0, D, 0.5f, 1.0f); x.n1b = hvec(t + 1, D, 0.1f);
      x.qkvw = hvec(t + 2, 3 * D * D, 0.05f); x.qkvb = hvec(t + 3, 3 * D, 0.1f);
      x.projw = hvec(t + 4, D * D, 0.05f);
      x.n2g = hvec(t + 5, D, 0.5f, 1.0f); x.n2b = hvec(t + 6, D, 0.1f);
      x.fc1w = hvec(t + 7, Dm * D, 0.05f); x.fc1b = hvec(t + 8, Dm, 0.1f);
      x.fc2w = hvec(t + 9, D * Dm, 0.05f);
      src.push_back({x.n1g.data(), x.n1b.data(), x.qkvw.data(), x.qkvb.data(), x.projw.data(), nullptr, x.n2g.data(), x.n2b.data(),
                     x.fc1w.data(), x.fc1b.data(), x.fc2w.data(), nullptr});   // (the two biases the packing does not read)
    }
  }
};

// expectations of the fold, with loops of their own
static void expect_fold(const float* W, const float* b, const float* g, const float* be, size_t rows, size_t cols, std::vector<float>& wg,
                        std::vector<float>& cs, std::vector<float>& fb) {
  wg.resize(rows * cols); cs.resize(rows); fb.resize(rows);
  for (size_t r = 0; r < rows; ++r) {
    double c = 0.0, s = (double)b[r];
    for (size_t q = 0; q < cols; ++q) {
      volatile float p = W[r * cols + q] * g[q];   // (volatile: one fp32 rounding, whatever the optimiser would like)
      wg[r * cols + q] = p;
      c += (double)p;
      s += (double)W[r * cols + q] * (double)be[q];
    }
    cs[r] = (float)c; fb[r] = (float)s;
  }
}

static void check_fold_tile_tables(const Model& m) {
  const size_t D = Model::D, H = Model::H, N = 3 * D;
  const Model::Blk& x = m.b[0];
  std::vector<float> wg(N * D), cs(N), fb(N), ewg, ecs, efb;
  fold_layernorm(x.qkvw.data(), x.qkvb.data(), x.n1g.data(), x.n1b.data(), N, D, wg.data(), cs.data(), fb.data());
  expect_fold(x.qkvw.data(), x.qkvb.data(), x.n1g.data(), x.n1b.data(), N, D, ewg, ecs, efb);
  CHECK(same(wg.data(), ewg.data(), N * D * 4), "fold: wg differs");
  CHECK(same(cs.data(), ecs.data(), N * 4), "fold: csum differs");
  CHECK(same(fb.data(), efb.data(), N * 4), "fold: folded bias differs");

  // tile order: planes / csum / fb of row 192 h + 48 wn + 16 part + x = those of folded row 512 part + 64 h + 16 wn + x
  std::vector<uint16_t> pf(2 * pad(N) * D, 0), pt(2 * pad(N) * D, 0);
  std::vector<float> cst(N), fbt(N);
  const int kf = split_weight_f16x3(wg.data(), N, D, pf.data());
  const int kt = tile_order_copy(wg.data(), cs.data(), fb.data(), D, H, pt.data(), cst.data(), fbt.data());
  CHECK(kf == kt, "tile order: exponent %d, folded %d", kt, kf);
  std::vector<int> used(N, 0);
  std::vector<size_t> srcs(N);
  for (size_t part = 0; part < 3; ++part)
    for (size_t h = 0; h < 8; ++h)
      for (size_t wn = 0; wn < 4; ++wn)
        for (size_t xx = 0; xx < 16; ++xx) {
          const size_t r = 192 * h + 48 * wn + 16 * part + xx, s = 512 * part + 64 * h + 16 * wn + xx;
          srcs[r] = s;
          CHECK(tile_order_src_row(r, D, H) == s, "tile_order_src_row(%zu) = %zu, expected %zu", r, tile_order_src_row(r, D, H), s);
          ++used[s];
          CHECK(same(&pt[r * 2 * D], &pf[s * 2 * D], 2 * D * 2), "tile order: planes of row %zu differ from folded row %zu", r, s);
          CHECK(same(&cst[r], &cs[s], 4) && same(&fbt[r], &fb[s], 4), "tile order: csum / fb of row %zu", r);
        }
  for (size_t s = 0; s < N; ++s) CHECK(used[s] == 1, "tile order: source row %zu used %d times", s, used[s]);
  for (size_t i = N * 2 * D; i < pt.size(); ++i) CHECK(pt[i] == 0, "tile order: pad element %zu not zero", i);

  // block-0 tables: G = Wg W_e [3 D][cin], P[j] = Wg (b_e + spos[j]) [J][3 D], rows in tile order, fp64 sums over k ascending
  const int cin = 5;
  const std::vector<float> We = hvec(90, D * cin, 0.2f), be = hvec(91, D, 0.1f);
  for (int J : {17, 15}) {
    const std::vector<float> spos = hvec(92 + J, (size_t)J * D, 0.3f);
    std::vector<float> G(N * cin), P((size_t)J * N);
    block0_tables_host(wg.data(), We.data(), be.data(), spos.data(), (int)D, (int)H, cin, J, G.data(), P.data());
    for (size_t n = 0; n < N; ++n) {
      const float* wr = &wg[srcs[n] * D];
      for (int c = 0; c < cin; ++c) {
        double a = 0.0;
        for (size_t k = 0; k < D; ++k) a += (double)wr[k] * (double)We[k * cin + c];
        const float g = (float)a;
        CHECK(same(&g, &G[n * cin + c], 4), "J = %d: G[%zu][%d] = %g, expected %g", J, n, c, G[n * cin + c], g);
      }
      for (int j = 0; j < J; ++j) {
        double a = 0.0;
        for (size_t k = 0; k < D; ++k) a += (double)wr[k] * ((double)be[k] + (double)spos[(size_t)j * D + k]);
        const float p = (float)a;
        CHECK(same(&p, &P[(size_t)j * N + n], 4), "J = %d: P[%d][%zu] = %g, expected %g", J, j, n, P[(size_t)j * N + n], p);
      }
    }
  }
}

struct Region { size_t off, len; const char* name; };
static void check_regions(std::vector<Region> rg, size_t total, size_t elem, const char* what) {
  std::sort(rg.begin(), rg.end(), [](const Region& a, const Region& b) { return a.off < b.off; });
  size_t end = 0;
  for (const Region& r : rg) {
    CHECK(r.off != NO_OFF, "%s: %s has no offset", what, r.name);
    CHECK(r.off * elem % 16 == 0, "%s: %s at element %zu is not 16-byte aligned", what, r.name, r.off);
    CHECK(r.off >= end, "%s: %s at %zu overlaps the region before it (ends at %zu)", what, r.name, r.off, end);
    CHECK(r.off + r.len <= total, "%s: %s [%zu, %zu) leaves the image of %zu", what, r.name, r.off, r.off + r.len, total);
    end = r.off + r.len;
  }
}

static void check_images(const Model& m) {
  const size_t D = Model::D, H = Model::H, Dm = Model::Dm, nblk = 2, N = 3 * D;
  const size_t per_blk = 2 * (3 * pad(3 * D) * D + pad(D) * D + 2 * pad(Dm) * D + pad(D) * Dm), fold_per_blk = 2 * (3 * D + Dm) + 2 * 3 * D;
  for (int tile = 1; tile >= 0; --tile) {   // with the tile-order copies (spatial and temporal), then without
    PackedWeights pk;
    CHECK(pack_f16x3(m.src, D, Dm, H, tile != 0, tile != 0, pk), "pack_f16x3 failed");
    CHECK(pk.planes.size() == per_blk * nblk && pk.fold.size() == fold_per_blk * nblk && pk.blk.size() == nblk, "image sizes");
    CHECK(!pk.clamped, "finite weights reported as clamped");
    std::vector<Region> r16, rf;
    for (size_t k = 0; k < nblk; ++k) {
      const BlockOff& b = pk.blk[k];
      const Model::Blk& x = m.b[k];
      r16.insert(r16.end(), {{b.qkv_x3, 2 * pad(N) * D, "qkv_x3"}, {b.proj_x3, 2 * pad(D) * D, "proj_x3"}, {b.fc1_x3, 2 * pad(Dm) * D, "fc1_x3"},
                             {b.fc2_x3, 2 * pad(D) * Dm, "fc2_x3"}, {b.qkv_f3, 2 * pad(N) * D, "qkv_f3"}, {b.fc1_f3, 2 * pad(Dm) * D, "fc1_f3"}});
      rf.insert(rf.end(), {{b.qkv_cs, N, "qkv_cs"}, {b.qkv_fb, N, "qkv_fb"}, {b.fc1_cs, Dm, "fc1_cs"}, {b.fc1_fb, Dm, "fc1_fb"}});
      if (tile) {
        r16.push_back({b.qkv_f3h, 2 * pad(N) * D, "qkv_f3h"});
        rf.insert(rf.end(), {{b.qkv_csh, N, "qkv_csh"}, {b.qkv_fbh, N, "qkv_fbh"}});
      } else {
        CHECK(b.qkv_f3h == NO_OFF && b.qkv_csh == NO_OFF && b.qkv_fbh == NO_OFF, "block %zu: a tile-order copy nobody asked for", k);
      }
      CHECK(b.qkv_e == 12 && b.proj_e == 12 && b.fc1_e == 12 && b.fc2_e == 12 && b.qkv_fe == 12 && b.fc1_fe == 12, "block %zu: exponents", k);
      if (g_fail) continue;   // (the content checks below index with the offsets)
      // content: the folded vectors and a sample of plane elements of every matrix, read back where the offsets say they are
      std::vector<float> ewg, ecs, efb;
      expect_fold(x.qkvw.data(), x.qkvb.data(), x.n1g.data(), x.n1b.data(), N, D, ewg, ecs, efb);
      CHECK(same(&pk.fold[b.qkv_cs], ecs.data(), N * 4) && same(&pk.fold[b.qkv_fb], efb.data(), N * 4), "block %zu: qkv csum / fb", k);
      if (k == 0) CHECK(pk.wg0.size() == N * D && same(pk.wg0.data(), ewg.data(), N * D * 4), "wg0 is not W_qkv diag(gamma1) of block 0");
      auto elem_ok = [&](size_t off, const float* w, size_t cols, size_t r, size_t c, bool acc) {
        const size_t o = off + r * 2 * cols + (acc ? pc_acc(c) : pc(c));
        const double s = std::ldexp((double)w[r * cols + c], 12);
        return std::fabs(f16(pk.planes[o]) + f16(pk.planes[o + 32]) - s) <= std::max(std::ldexp(std::fabs(s), -22), std::ldexp(1.0, -25));
      };
      for (size_t i = 0; i < 4096; ++i) {
        const size_t r = h32((uint32_t)i) % D, c = h32((uint32_t)i + 77777u) % D;
        CHECK(elem_ok(b.qkv_x3, x.qkvw.data(), D, r + 2 * D, c, false), "block %zu: qkv_x3 (%zu, %zu)", k, r + 2 * D, c);
        CHECK(elem_ok(b.proj_x3, x.projw.data(), D, r, c, false), "block %zu: proj_x3 (%zu, %zu)", k, r, c);
        CHECK(elem_ok(b.fc1_x3, x.fc1w.data(), D, r + D, c, false), "block %zu: fc1_x3 (%zu, %zu)", k, r + D, c);
        CHECK(elem_ok(b.fc2_x3, x.fc2w.data(), Dm, r, c + D, true), "block %zu: fc2_x3 (%zu, %zu)", k, r, c + D);
        CHECK(elem_ok(b.qkv_f3, ewg.data(), D, r + D, c, false), "block %zu: qkv_f3 (%zu, %zu)", k, r + D, c);
      }
      if (tile)
        for (size_t part = 0; part < 3; ++part)
          for (size_t h = 0; h < 8; ++h)
            for (size_t wn = 0; wn < 4; ++wn)
              for (size_t xx = 0; xx < 16; ++xx) {
                const size_t r = 192 * h + 48 * wn + 16 * part + xx, s = 512 * part + 64 * h + 16 * wn + xx;
                CHECK(same(&pk.planes[b.qkv_f3h + r * 2 * D], &pk.planes[b.qkv_f3 + s * 2 * D], 2 * D * 2), "block %zu: qkv_f3h row %zu", k, r);
                CHECK(pk.fold[b.qkv_csh + r] == ecs[s] && pk.fold[b.qkv_fbh + r] == efb[s], "block %zu: qkv_csh / qkv_fbh row %zu", k, r);
              }
      expect_fold(x.fc1w.data(), x.fc1b.data(), x.n2g.data(), x.n2b.data(), Dm, D, ewg, ecs, efb);
      CHECK(same(&pk.fold[b.fc1_cs], ecs.data(), Dm * 4) && same(&pk.fold[b.fc1_fb], efb.data(), Dm * 4), "block %zu: fc1 csum / fb", k);
    }
    check_regions(r16, pk.planes.size(), 2, tile ? "F16X3 planes" : "F16X3 planes, no tile order");
    check_regions(rf, pk.fold.size(), 4, tile ? "F16X3 fold" : "F16X3 fold, no tile order");
  }
  // BF16: the four matrices of every block, rounded to nearest even
  PackedWeights pb;
  pack_bf16(m.src, D, Dm, pb);
  const size_t per_blk_bf = pad(3 * D) * D + pad(D) * D + pad(Dm) * D + pad(D) * Dm;
  CHECK(pb.planes.size() == per_blk_bf * nblk && pb.fold.empty() && pb.blk.size() == nblk && !pb.clamped, "bf16 image sizes");
  std::vector<Region> rb;
  for (size_t k = 0; k < nblk; ++k) {
    const BlockOff& b = pb.blk[k];
    rb.insert(rb.end(), {{b.qkv_x3, pad(N) * D, "qkv"}, {b.proj_x3, pad(D) * D, "proj"}, {b.fc1_x3, pad(Dm) * D, "fc1"}, {b.fc2_x3, pad(D) * Dm, "fc2"}});
  }
  check_regions(rb, pb.planes.size(), 2, "BF16 image");
  if (!g_fail)
    for (size_t k = 0; k < nblk; ++k)
      for (size_t i = 0; i < D * Dm; ++i) {   // fc2: truncation of the fp32 bits + the round-to-nearest-even increment, written out
        uint32_t u;
        memcpy(&u, &m.b[k].fc2w[i], 4);
        const uint32_t low = u & 0xffffu, up = u >> 16, want = up + ((low > 0x8000u || (low == 0x8000u && (up & 1u))) ? 1u : 0u);
        CHECK(pb.planes[pb.blk[k].fc2_x3 + i] == (uint16_t)want, "bf16 fc2[%zu] of block %zu", i, k);
      }
}

// ---- the per-matrix exponent: the largest k <= 12 with amax 2^k <= 65504, floor -14 (in double: exact for every fp32 amax)
static int expect_k(double amax) {
  int k = 12;
  while (k > -14 && std::ldexp(amax, k) > 65504.0) --k;
  return k;
}
static double amax_of(const std::vector<float>& w) {
  double a = 0.0;
  for (float v : w) a = std::max(a, (double)std::fabs(v));
  return a;
}
static std::vector<float> times_gamma(const std::vector<float>& W, const std::vector<float>& g, size_t rows, size_t cols) {
  std::vector<float> o(rows * cols);
  for (size_t r = 0; r < rows; ++r)
    for (size_t q = 0; q < cols; ++q) { volatile float p = W[r * cols + q] * g[q]; o[r * cols + q] = p; }
  return o;
}

static void check_exponents() {
  const size_t rows = 40, cols = 64;
  std::vector<uint16_t> pr(2 * pad(rows) * cols), pr0(2 * pad(rows) * cols);
  // every boundary: amax = 65504 2^-k is the last value of exponent k, the next float is the first of k - 1 -- below -14 there is no
  // exponent left and the entry is clamped (reported)
  for (int k = 12; k >= -14; --k) {
    std::vector<float> w = hvec(40, rows * cols, 1.0e-4f);
    const float edge = std::ldexp(65504.0f, -k), next = std::nextafterf(edge, std::numeric_limits<float>::infinity());
    bool clamped = false;
    w[123] = -edge;
    int got = split_weight_f16x3(w.data(), rows, cols, pr.data(), false, &clamped);
    CHECK(got == k && !clamped, "amax = 65504 2^%d: k = %d clamped %d", -k, got, (int)clamped);
    w[123] = next;
    got = split_weight_f16x3(w.data(), rows, cols, pr.data(), false, &clamped);
    CHECK(got == std::max(k - 1, -14) && clamped == (k == -14), "the float above 65504 2^%d: k = %d clamped %d", -k, got, (int)clamped);
    CHECK(expect_k(edge) == k && expect_k(next) == std::max(k - 1, -14), "expect_k at the boundary of %d", k);
  }
  {  // finite, but beyond any exponent: reported, planes saturate at +-65504
    std::vector<float> w = hvec(41, rows * cols, 1.0f);
    w[7] = 3.0e9f; w[8] = -3.0e38f;
    bool clamped = false;
    const int got = split_weight_f16x3(w.data(), rows, cols, pr.data(), false, &clamped);
    CHECK(got == -14 && clamped, "finite weight above 65504 2^14: k = %d clamped %d", got, (int)clamped);
    CHECK(f16(pr[pc(7)]) == 65504.0 && f16(pr[pc(8)]) == -65504.0, "saturated planes: %g %g", f16(pr[pc(7)]), f16(pr[pc(8)]));
  }
  {  // planes of 2^j W == planes of W, byte for byte (amax pinned inside (7.995, 15.99], so the exponent is exactly 12 - j)
    std::vector<float> w = hvec(42, rows * cols, 0.125f);
    for (size_t i = 0; i < w.size(); i += 5) w[i] = std::ldexp(w[i], -17);   // lo (and hi) halves in fp16 subnormals
    w[77] = -12.5f;
    for (int acc = 0; acc < 2; ++acc) {
      const int k0 = split_weight_f16x3(w.data(), rows, cols, pr0.data(), acc != 0);
      CHECK(k0 == 12, "base exponent %d", k0);
      for (int j = 1; j <= 26; ++j) {
        std::vector<float> wj(w.size());
        for (size_t i = 0; i < w.size(); ++i) wj[i] = std::ldexp(w[i], j);
        bool clamped = false;
        const int kj = split_weight_f16x3(wj.data(), rows, cols, pr.data(), acc != 0, &clamped);
        CHECK(kj == 12 - j && !clamped, "2^%d W: k = %d clamped %d", j, kj, (int)clamped);
        CHECK(same(pr.data(), pr0.data(), pr.size() * 2), "2^%d W: planes differ from those of W (acc order %d)", j, acc);
      }
    }
  }
  {  // the commit admits exponents down to F16X3_MIN_WEIGHT_EXP: amax = 65504 2^-MIN passes, the next float is reported (finite as it is)
    CHECK(F16X3_MIN_WEIGHT_EXP == 0, "F16X3_MIN_WEIGHT_EXP = %d: this check and DESIGN.md section 4.1 state 0", F16X3_MIN_WEIGHT_EXP);
    const float edge = std::ldexp(65504.0f, -F16X3_MIN_WEIGHT_EXP);
    for (int which = 0; which < 4; ++which)
      for (int over = 0; over < 2; ++over) {
        Model mm;
        Model::Blk& x = mm.b[1];
        std::vector<float>* mat[4] = {&x.qkvw, &x.projw, &x.fc1w, &x.fc2w};
        x.n1g[4321 % Model::D] = 1.0f; x.n2g[4321 % Model::D] = 1.0f;   // (the folded entry is the raw one)
        (*mat[which])[4321] = over ? -std::nextafterf(edge, std::numeric_limits<float>::infinity()) : -edge;
        PackedWeights pk;
        CHECK(pack_f16x3(mm.src, Model::D, Model::Dm, Model::H, true, true, pk), "pack_f16x3 failed at the admission boundary");
        const int e[4] = {pk.blk[1].qkv_e, pk.blk[1].proj_e, pk.blk[1].fc1_e, pk.blk[1].fc2_e};
        CHECK(e[which] == F16X3_MIN_WEIGHT_EXP - over, "matrix %d: exponent %d at the boundary (over %d)", which, e[which], over);
        CHECK(pk.clamped == (over != 0), "matrix %d at exponent %d: clamped = %d", which, e[which], (int)pk.clamped);
      }
  }
  // one block pair whose six matrices carry six different admitted outliers: six different exponents, each where BlockOff says, and the
  // tile-order copy is made of the folded planes at the folded exponent
  Model m;
  const size_t D = Model::D, Dm = Model::Dm, H = Model::H, N = 3 * D;
  for (size_t k = 0; k < 2; ++k) {
    Model::Blk& x = m.b[k];
    x.qkvw[(2 * D + 70) * D + 33] = 100.0f;  x.n1g[33] = 4.0f;     // qkv 9, folded 400 -> 7
    x.projw[17 * D + 301] = -5.0e3f;                               // proj 3
    x.fc1w[900 * D + 12] = 40.0f;            x.n2g[12] = 16.0f;    // fc1 10, folded 640 -> 6
    x.fc2w[300 * Dm + 1000] = 1.0e4f;                              // fc2 2
    if (k == 1) { x.qkvw[5] = -4.0e4f; x.n1g[5] = 0.5f; }          // the second block: qkv 0, folded 2e4 -> 1
  }
  PackedWeights pk;
  CHECK(pack_f16x3(m.src, D, Dm, H, true, true, pk), "pack_f16x3 failed on the outlier model");
  CHECK(!pk.clamped, "outlier model reported as clamped");
  for (size_t k = 0; k < 2 && pk.blk.size() == 2; ++k) {
    const Model::Blk& x = m.b[k];
    const BlockOff& b = pk.blk[k];
    const std::vector<float> qg = times_gamma(x.qkvw, x.n1g, N, D), fg = times_gamma(x.fc1w, x.n2g, Dm, D);
    const int want[6] = {expect_k(amax_of(x.qkvw)), expect_k(amax_of(x.projw)), expect_k(amax_of(x.fc1w)), expect_k(amax_of(x.fc2w)),
                         expect_k(amax_of(qg)), expect_k(amax_of(fg))};
    const int got[6] = {b.qkv_e, b.proj_e, b.fc1_e, b.fc2_e, b.qkv_fe, b.fc1_fe};
    const int fixed[6] = {k ? 0 : 9, 3, 10, 2, k ? 1 : 7, 6};
    for (int i = 0; i < 6; ++i) {
      CHECK(got[i] == want[i] && want[i] == fixed[i], "block %zu matrix %d: exponent %d, own loop %d, intended %d", k, i, got[i], want[i], fixed[i]);
      for (int j = 0; j < i; ++j) CHECK(got[i] != got[j], "block %zu: matrices %d and %d share exponent %d", k, j, i, got[i]);
    }
    // an ordinary entry and the outlier of every matrix, read back at the matrix's own exponent
    auto elem = [&](size_t off, const std::vector<float>& w, size_t cols, size_t r, size_t c, bool acc, int e, const char* name) {
      const size_t o = off + r * 2 * cols + (acc ? pc_acc(c) : pc(c));
      const double s = std::ldexp((double)w[r * cols + c], e), err = std::fabs(f16(pk.planes[o]) + f16(pk.planes[o + 32]) - s);
      CHECK(err <= std::max(std::ldexp(std::fabs(s), -22), std::ldexp(1.0, -25)), "block %zu %s (%zu, %zu): split error %g at exponent %d", k, name, r, c, err, e);
    };
    elem(b.qkv_x3, x.qkvw, D, 2 * D + 70, 33, false, b.qkv_e, "qkv_x3"); elem(b.qkv_x3, x.qkvw, D, 9, 9, false, b.qkv_e, "qkv_x3");
    elem(b.proj_x3, x.projw, D, 17, 301, false, b.proj_e, "proj_x3");    elem(b.proj_x3, x.projw, D, 9, 9, false, b.proj_e, "proj_x3");
    elem(b.fc1_x3, x.fc1w, D, 900, 12, false, b.fc1_e, "fc1_x3");        elem(b.fc1_x3, x.fc1w, D, 9, 9, false, b.fc1_e, "fc1_x3");
    elem(b.fc2_x3, x.fc2w, Dm, 300, 1000, true, b.fc2_e, "fc2_x3");      elem(b.fc2_x3, x.fc2w, Dm, 9, 9, true, b.fc2_e, "fc2_x3");
    elem(b.qkv_f3, qg, D, 2 * D + 70, 33, false, b.qkv_fe, "qkv_f3");    elem(b.qkv_f3, qg, D, 9, 9, false, b.qkv_fe, "qkv_f3");
    elem(b.fc1_f3, fg, D, 900, 12, false, b.fc1_fe, "fc1_f3");           elem(b.fc1_f3, fg, D, 9, 9, false, b.fc1_fe, "fc1_f3");
    // the tile-order copy: the folded planes row by row, hence at qkv_fe (pack_f16x3 refuses a copy whose exponent differs)
    CHECK(b.qkv_f3h != NO_OFF, "block %zu: no tile-order copy", k);
    if (b.qkv_f3h != NO_OFF)
      for (size_t r = 0; r < N; ++r) {
        const size_t c = r % 192, s = ((c % 48) / 16) * D + r / 192 * 64 + 16 * (c / 48) + c % 16;
        CHECK(same(&pk.planes[b.qkv_f3h + r * 2 * D], &pk.planes[b.qkv_f3 + s * 2 * D], 2 * D * 2), "block %zu: qkv_f3h row %zu is not folded row %zu", k, r, s);
      }
    std::vector<uint16_t> pt(2 * pad(N) * D, 0);
    std::vector<float> cs(N), fb(N), cst(N), fbt(N);
    CHECK(tile_order_copy(qg.data(), cs.data(), fb.data(), D, H, pt.data(), cst.data(), fbt.data()) == b.qkv_fe, "block %zu: tile_order_copy's exponent is not qkv_fe", k);
  }
}

int main() {
  check_split();
  check_exponents();
  check_bf16();
  const Model m;
  check_fold_tile_tables(m);
  check_images(m);
  if (g_fail) { printf("weight_pack_check: %d check(s) FAILED\n", g_fail); return 1; }
  printf("weight_pack_check: ok\n");
  return 0;
}
