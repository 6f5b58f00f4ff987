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
// The kernels take any k in [-14, 12]; the commit (pack_f16x3) admits k >= F16X3_MIN_WEIGHT_EXP only.
int split_weight_f16x3(const float* w, size_t rows, size_t cols, uint16_t* pair, bool acc_order = false, bool* clamped = nullptr);
// The lowest exponent the commit admits (|w| <= 65504 everywhere in the matrix); a matrix below it sets PackedWeights::clamped, which
// the engine reports as D3D_RANGE_WEIGHT.  At a low k the lo half -- then the hi half -- of the matrix's ORDINARY entries falls into fp16
// subnormals and each of them is off by up to 2^-25 2^-k, whatever its size: the floor under every output of that GEMM doubles with
// each step of k.  The plane model (tests/plane_model.py; a ~ U(-2, 2), w ~ U(+-1 / sqrt(K)), one outlier) puts it at
//   k          12 .. 5    3        1        0        -1       -4       -14
//   K =  512   1.9e-7     2.8e-7   8.3e-7   1.7e-6   3.1e-6   3.3e-5   2.5e-2
//   K = 1024   1.7e-7     3.1e-7   1.1e-6   2.5e-6   4.9e-6   4.5e-5   4.1e-2
// against the fp32 rounding bound both engines' GEMMs are held to, 2e-6 sqrt(K / 32) = 8.0e-6 / 1.1e-5.  A block chains four GEMMs, so
// a matrix is admitted while its floor stays within a quarter of that bound: k >= 0 at both depths, k = -1 at neither
// (tests/test_plane_model_host.py asserts it).  On the device the engine's distance to the fp64 oracle stops being that of the same
// checkpoint without the outlier at the same exponent, -1 (tests/test_gpu_weight_exponent.py).
constexpr int F16X3_MIN_WEIGHT_EXP = 0;
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
// fp32 -> fp16, round to nearest even with subnormals kept (as torch's .to(float16) and v_cvt_f16_f32); a finite value from 65520 on
// becomes inf; *nonfinite as above
uint16_t f16_rne(float f, bool* nonfinite = nullptr);

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
  bool clamped = false;           // a GEMM weight was not finite, or F16X3: a matrix's exponent is below F16X3_MIN_WEIGHT_EXP
};
// F16X3: the four GEMM weights of every block as planes, the LayerNorm-folded qkv / fc1 forms and, for the spatial (tile_order_s) /
// temporal (tile_order_t) blocks, the folded qkv once more in tile order.  H: the heads of that order -- the model's at head width 64,
// D / 64 pseudo-heads for the fused kernel of narrower heads (a pair of 32 columns, a quad of 16: one 64-column segment); nothing else
// reads it.  false: the internal exponent check failed.
bool pack_f16x3(const std::vector<BlockSrc>& src, size_t D, size_t Dm, size_t H, bool tile_order_s, bool tile_order_t, PackedWeights& out);
// BF16: bf16 copies of the four GEMM weights of every block, [rows padded to 256][K]; f16 (D3D_PREC_F16): fp16 copies, same layout --
// `clamped` then also covers a finite weight beyond the fp16 range (its image is inf)
void pack_bf16(const std::vector<BlockSrc>& src, size_t D, size_t Dm, PackedWeights& out, bool f16 = false);

}  // namespace d3d
