// Host-side packing of the weight commit: every resident weight image the kernels read, as pure functions from host arrays to host
// arrays.  No device code, no HIP runtime call, no engine: the unit runs (and is sanitised) on a machine without a device
// (tests/host/weight_pack_check.cpp).  engine.hip uploads what these return; engine_ops.hip shares the split and the fold.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace d3d {

// rows of a GEMM weight image: whole 256-row tiles (zero rows), so the staging of edge tiles never leaves the allocation
inline size_t pad256(size_t n) { return (n + 255) / 256 * 256; }
// Planes of 2^k * w, k chosen per matrix: 12 whenever |w| <= 15.99 everywhere, smaller for larger weights (LayerNorm-folded
// weights of checkpoints with big gains).  Returns k (the GEMM's w_exp argument); *clamped is set when an entry is not finite.
int split_weight_f16x3(const float* w, size_t rows, size_t cols, uint16_t* pair, bool acc_order = false, bool* clamped = nullptr);
// LayerNorm folded into the consuming GEMM: LN(x) W^T + b = rstd (x (W diag g)^T) - rstd mean csum + (b + W beta).  W [rows][cols] ->
// wg = W diag(gamma) in fp32, csum[r] = sum_q wg[r][q], fb[r] = b[r] + sum_q W[r][q] beta[q] (fp64 sums, q ascending, stored as fp32)
void fold_layernorm(const float* W, const float* b, const float* gamma, const float* beta, size_t rows, size_t cols, float* wg,
                    float* csum, float* fb);
// tile order of a folded qkv weight (kernels_qkv_sattn.hip): row 192 h + 48 wn + 16 part + x <- original row 512 part + 64 h + 16 wn + x
// (D = 512, H = 8; in general 3 dh rows per head, D per part): one head's q, k, v are one contiguous N-tile and accumulator column tile
// j of every wave is part j.  Returns the original row of tile-order row r.
inline size_t tile_order_src_row(size_t r, size_t D, size_t H) {
  const size_t dh = D / H, c = r % (3 * dh);
  return ((c % 48) / 16) * D + r / (3 * dh) * dh + 16 * (c / 48) + c % 16;
}
// fold_layernorm's qkv results (wg [3 D][D], csum / fb [3 D]) once more in tile order; returns the planes' exponent
int tile_order_copy(const float* wg, const float* csum, const float* fb, size_t D, size_t H, uint16_t* pair, float* csum_t, float* fb_t,
                    bool* clamped = nullptr);
void block0_tables_host(const float* wg, const float* We, const float* be, const float* spos, int D, int H, int cin, int J, float* G, float* P);
// fp32 -> bf16, round to nearest even (as torch's .to(bfloat16) and v_cvt_pk_bf16_f32); *nonfinite is set when the RESULT is inf or NaN
uint16_t bf16_rne(float f, bool* nonfinite = nullptr);

// ---- the whole engine's images: one block's host weights in, images + the offset of every BlockW field (engine.hip) out
struct BlockSrc { const float *n1g, *n1b, *qkvw, *qkvb, *projw, *projb, *n2g, *n2b, *fc1w, *fc1b, *fc2w, *fc2b; };
constexpr size_t NO_OFF = ~(size_t)0;   // the block has no such image
struct BlockOff {
  size_t qkv_x3 = NO_OFF, proj_x3 = NO_OFF, fc1_x3 = NO_OFF, fc2_x3 = NO_OFF, qkv_f3 = NO_OFF, fc1_f3 = NO_OFF, qkv_f3h = NO_OFF;   // uint16 of planes
  size_t qkv_cs = NO_OFF, qkv_fb = NO_OFF, fc1_cs = NO_OFF, fc1_fb = NO_OFF, qkv_csh = NO_OFF, qkv_fbh = NO_OFF;                   // floats of fold
  int qkv_e = 12, proj_e = 12, fc1_e = 12, fc2_e = 12, qkv_fe = 12, fc1_fe = 12;                                                    // exponents of the planes
};
struct PackedWeights {
  std::vector<uint16_t> planes;   // the arena16 image
  std::vector<float> fold;        // F16X3: the arena_fold image
  std::vector<float> wg0;         // F16X3: W_qkv diag(gamma1) of block 0, fp32 [3 D][D] (what the block-0 tables are made from)
  std::vector<BlockOff> blk;      // execution order
  bool clamped = false;           // a GEMM weight was not finite
};
// F16X3: the four GEMM weights of every block as planes, the LayerNorm-folded qkv / fc1 forms and, for the spatial (tile_order_s) /
// temporal (tile_order_t) blocks, the folded qkv once more in tile order.  false: the internal exponent check failed.
bool pack_f16x3(const std::vector<BlockSrc>& src, size_t D, size_t Dm, size_t H, bool tile_order_s, bool tile_order_t, PackedWeights& out);
// BF16: bf16 copies of the four GEMM weights of every block, [rows padded to 256][K]
void pack_bf16(const std::vector<BlockSrc>& src, size_t D, size_t Dm, PackedWeights& out);

}  // namespace d3d
