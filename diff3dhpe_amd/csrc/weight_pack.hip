// Host-side packing of the weight commit (weight_pack.h).  Host code only, compiled with the flags of every other unit: no -march, no
// fast-math, nothing that lets the host contract a product and a sum -- the bits of the images depend on that.
#include "weight_pack.h"

#include <cmath>
#include <cstring>

#include "d3d_kernels.h"   // the pair layout: pair_col, pair_col_acc, PAIR_LO

namespace d3d {

// Host-side weight split: w [rows, cols] -> pair layout (d3d_kernels.h) of hi/lo fp16 of s*w with s = 2^12
// (round-to-nearest-even both times).
// acc_order: the k index of every 32-column group is stored in the order pair_slot_acc() gives it (the layout of the
// hidden activation that the fc1 epilogue writes straight from its accumulators, kernels_gemm_x3p.hip)
int split_weight_f16x3(const float* w, size_t rows, size_t cols, uint16_t* pair, bool acc_order, bool* clamped) {
  // per-matrix scale 2^k: 2^12 whenever the matrix fits (|w| <= 15.99: every matrix of a sane checkpoint -- then the planes are
  // bit for bit what a fixed 4096 gives), smaller when a weight is larger -- LayerNorm-FOLDED weights W diag(gamma) of a
  // checkpoint with big gains get there (gamma 6 x |w| 8 = 48).  The GEMM un-scales by 2^-(3+k) (X3Tail::out_scale); powers of
  // two, so nothing rounds differently.  Small entries whose lo half then falls into fp16 denormals lose bits below
  // 2^-24 2^-k; what that costs a GEMM per exponent, and the exponent below which the commit refuses a matrix
  // (F16X3_MIN_WEIGHT_EXP), is tabulated in weight_pack.h.
  float amax = 0.0f;
  bool finite = true;
  for (size_t i = 0; i < rows * cols; ++i) {
    const float a = fabsf(w[i]);
    if (!(a <= 3.0e38f)) finite = false;
    else if (a > amax) amax = a;
  }
  int k = 12;
  while (k > -14 && ldexpf(amax, k) > 65504.0f) --k;
  const float scale = ldexpf(1.0f, k);
  bool in_range = finite;
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < cols; ++c) {
      float s = w[r * cols + c] * scale;
      if (!(s <= 65504.0f && s >= -65504.0f)) in_range = false;
      if (s > 65504.0f) s = 65504.0f;
      if (s < -65504.0f) s = -65504.0f;
      const _Float16 h = (_Float16)s;
      const _Float16 l = (_Float16)(s - (float)h);
      uint16_t* o = pair + r * 2 * cols + (acc_order ? pair_col_acc((int)c) : pair_col((int)c));
      __builtin_memcpy(o, &h, 2);
      __builtin_memcpy(o + PAIR_LO, &l, 2);
    }
  if (clamped && !in_range) *clamped = true;
  return k;
}

void fold_layernorm(const float* W, const float* b, const float* gamma, const float* beta, size_t rows, size_t cols, float* wg,
                    float* csum, float* fb) {
  for (size_t r = 0; r < rows; ++r) {
    double c = 0.0, bsum = (double)b[r];
    for (size_t q = 0; q < cols; ++q) {
      const float wv = W[r * cols + q] * gamma[q];        // the fp32 product the GEMM operand is split from
      wg[r * cols + q] = wv;
      c += (double)wv;
      bsum += (double)W[r * cols + q] * (double)beta[q];
    }
    csum[r] = (float)c; fb[r] = (float)bsum;
  }
}

int tile_order_copy(const float* wg, const float* csum, const float* fb, size_t D, size_t H, uint16_t* pair, float* csum_t, float* fb_t,
                    bool* clamped) {
  const size_t rows = 3 * D;
  std::vector<float> whm(rows * D);
  for (size_t r = 0; r < rows; ++r) {
    const size_t src = tile_order_src_row(r, D, H);
    memcpy(&whm[r * D], &wg[src * D], D * sizeof(float));
    csum_t[r] = csum[src]; fb_t[r] = fb[src];
  }
  return split_weight_f16x3(whm.data(), rows, D, pair, false, clamped);
}

// "block0_direct": the commit-time tables of block 0 (d3d_engine::b0_tab).  wg: W_qkv diag(gamma1) [3 D][D], the fp32 values the commit
// splits block 0's qkv planes from (q rows as handed over: qk_scale and qkv_bias = False arrive as derived tensors, the LayerNorm's gamma /
// beta / eps live in wg, the folded bias and the kernel argument).  G = Wg W_e [3 D][cin] and P[j] = Wg (b_e + spos[j]) [J][3 D] in the tile
// order of qkv_f3h, summed in fp64 and stored as fp32.  Built where block 0 can take the direct form at all (d3d_engine_commit_weights).
void block0_tables_host(const float* wg, const float* We, const float* be, const float* spos, int D, int H, int cin, int J, float* G, float* P) {
  const size_t N = 3 * (size_t)D;
  std::vector<double> v((size_t)J * D);
  for (int j = 0; j < J; ++j)
    for (int k = 0; k < D; ++k) v[(size_t)j * D + k] = (double)be[k] + (double)spos[(size_t)j * D + k];
  for (size_t n = 0; n < N; ++n) {   // head-major row n <- original row src, as the commit orders qkv_f3h
    const float* wr = wg + tile_order_src_row(n, D, H) * D;
    for (int c = 0; c < cin; ++c) {
      double a = 0.0;
      for (int k = 0; k < D; ++k) a += (double)wr[k] * (double)We[(size_t)k * cin + c];
      G[n * cin + c] = (float)a;
    }
    for (int j = 0; j < J; ++j) {
      double a = 0.0;
      for (int k = 0; k < D; ++k) a += (double)wr[k] * v[(size_t)j * D + k];
      P[(size_t)j * N + n] = (float)a;
    }
  }
}

uint16_t bf16_rne(float f, bool* nonfinite) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint16_t h = (u & 0x7fffffffu) > 0x7f800000u ? (uint16_t)((u >> 16) | 0x40)     // NaN stays NaN
                                                     : (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
  if (nonfinite && (h & 0x7f80u) == 0x7f80u) *nonfinite = true;
  return h;
}

uint16_t f16_rne(float f, bool* nonfinite) {
  uint32_t u;
  memcpy(&u, &f, 4);
  const uint16_t sign = (uint16_t)((u >> 16) & 0x8000u);
  const uint32_t a = u & 0x7fffffffu;
  uint16_t h;
  if (a > 0x7f800000u) {
    h = (uint16_t)(0x7e00u | ((a >> 13) & 0x3ffu));                    // NaN stays NaN (quiet), payload's top bits kept
  } else if (a >= 0x477ff000u) {
    h = 0x7c00u;                                                       // >= 65520 (the tie between 65504 and 2^16 goes to even = 2^16), inf
  } else if (a >= 0x38800000u) {                                       // normal fp16: rebias the exponent (127 -> 15), round 13 bits away
    const uint32_t v = a - 0x38000000u;
    h = (uint16_t)((v + 0xfffu + ((v >> 13) & 1u)) >> 13);             // (a mantissa carry runs into the exponent: correct)
  } else if (a < 0x33000000u) {
    h = 0;                                                             // < 2^-25: zero (2^-25 itself is the tie between 0 and 2^-24 -> 0, below)
  } else {                                                             // subnormal fp16: multiples of 2^-24
    const uint32_t e = a >> 23, m = (a & 0x7fffffu) | 0x800000u;       // value = m 2^(e - 150); wanted: m 2^(e - 126) in units of 2^-24
    const uint32_t sh = 126u - e;                                      // 14 .. 24
    const uint32_t q = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
    h = (uint16_t)(q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u));   // (rounding up to 0x400 is the least normal: correct)
  }
  h |= sign;
  if (nonfinite && (h & 0x7c00u) == 0x7c00u) *nonfinite = true;
  return h;
}

bool pack_f16x3(const std::vector<BlockSrc>& src, size_t D, size_t Dm, size_t H, bool tile_order_s, bool tile_order_t, PackedWeights& out) {
  // fp16 hi/lo pair layout of the four GEMM weights of every block, rows padded to a multiple of 256 (zero rows) so
  // the LDS-DMA of edge tiles never leaves the allocation (kernels_gemm_x3p.hip contract)
  const size_t nblk = src.size(), per_blk = 2 * (3 * pad256(3 * D) * D + pad256(D) * D + 2 * pad256(Dm) * D + pad256(D) * Dm);
  const size_t fold_per_blk = 2 * (3 * D + Dm) + 2 * 3 * D;
  out = PackedWeights{};
  out.planes.assign(per_blk * nblk, 0);
  out.fold.assign(fold_per_blk * nblk, 0.f);
  out.blk.assign(nblk, BlockOff{});
  uint16_t* const host = out.planes.data(); float* const fold = out.fold.data();
  std::vector<float> wg;
  size_t o = 0, fo = 0;   // (running: a block without the tile-order copy leaves no hole, the images' tails stay zero)
  for (size_t k = 0; k < nblk; ++k) {
    const BlockSrc& s = src[k];
    BlockOff& b = out.blk[k];
    auto pair = [&](const float* w, size_t rows, size_t cols, size_t& dst, int& wexp, bool acc_order = false) {
      wexp = split_weight_f16x3(w, rows, cols, host + o, acc_order, &out.clamped);
      if (wexp < F16X3_MIN_WEIGHT_EXP) out.clamped = true;   // the planes of the matrix's ordinary entries are too coarse (weight_pack.h)
      dst = o;
      o += 2 * pad256(rows) * cols;
    };
    pair(s.qkvw, 3 * D, D, b.qkv_x3, b.qkv_e); pair(s.projw, D, D, b.proj_x3, b.proj_e); pair(s.fc1w, Dm, D, b.fc1_x3, b.fc1_e);
    pair(s.fc2w, D, Dm, b.fc2_x3, b.fc2_e, true);   // its A operand (the hidden activation) is in accumulator order
    auto folded = [&](const float* W, const float* bias, const float* g, const float* be, size_t rows, size_t cols, size_t& w3, size_t& cs,
                      size_t& fb, int& wexp) {
      wg.resize(rows * cols);
      cs = fo; fb = fo + rows;
      fold_layernorm(W, bias, g, be, rows, cols, wg.data(), fold + cs, fold + fb);
      fo += 2 * rows;
      pair(wg.data(), rows, cols, w3, wexp);
    };
    folded(s.qkvw, s.qkvb, s.n1g, s.n1b, 3 * D, D, b.qkv_f3, b.qkv_cs, b.qkv_fb, b.qkv_fe);
    if ((k & 1) ? tile_order_t : tile_order_s) {   // the same folded rows once more in tile order (same per-matrix exponent): spatial
                                                   // blocks for kernels_qkv_sattn.hip, temporal blocks for kernels_qkv_tattn.hip
      const size_t rows = 3 * D;                   // (wg still holds W diag(gamma) of this block's qkv)
      const int ke = tile_order_copy(wg.data(), fold + b.qkv_cs, fold + b.qkv_fb, D, H, host + o, fold + fo, fold + fo + rows, &out.clamped);
      if (ke != b.qkv_fe) return false;
      b.qkv_f3h = o;
      o += 2 * pad256(rows) * D;
      b.qkv_csh = fo; b.qkv_fbh = fo + rows;
      fo += 2 * rows;
    }
    if (k == 0) out.wg0 = wg;   // W diag(gamma) of block 0's qkv: the fp32 values its planes are split from
    folded(s.fc1w, s.fc1b, s.n2g, s.n2b, Dm, D, b.fc1_f3, b.fc1_cs, b.fc1_fb, b.fc1_fe);
  }
  return true;
}

void pack_bf16(const std::vector<BlockSrc>& src, size_t D, size_t Dm, PackedWeights& out, bool f16) {
  // [rows padded to 256][K]: the staging of edge tiles never leaves the allocation (kernels_gemm_x3p.hip contract)
  const size_t nblk = src.size(), per_blk = pad256(3 * D) * D + pad256(D) * D + pad256(Dm) * D + pad256(D) * Dm;
  out = PackedWeights{};
  out.planes.assign(per_blk * nblk, 0);
  out.blk.assign(nblk, BlockOff{});
  size_t o = 0;
  auto conv = [&](const float* W, size_t rows, size_t cols, size_t& dst) {
    for (size_t i = 0; i < rows * cols; ++i) out.planes[o + i] = f16 ? f16_rne(W[i], &out.clamped) : bf16_rne(W[i], &out.clamped);
    dst = o;
    o += pad256(rows) * cols;
  };
  for (size_t k = 0; k < nblk; ++k) {
    BlockOff& b = out.blk[k];
    conv(src[k].qkvw, 3 * D, D, b.qkv_x3); conv(src[k].projw, D, D, b.proj_x3);
    conv(src[k].fc1w, Dm, D, b.fc1_x3); conv(src[k].fc2w, D, Dm, b.fc2_x3);
  }
}

}  // namespace d3d
