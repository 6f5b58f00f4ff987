// Internal launcher interface between the engine (engine.hip) and the gfx950 kernels.
// Not part of the public ABI (that is include/d3d.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>

#include "weight_pack.h"   // split_weight_f16x3() and the rest of the host-side weight packing

namespace d3d {

// ---- per-device launch state ----------------------------------------------------------------------------------------
// hipFuncSetAttribute(MaxDynamicSharedMemorySize) applies to the CURRENT device's function object, and the CU count is a
// property of a device: both are cached per device (one process may drive several GPUs -- nn.DataParallel, RUN:216-218 --
// from several threads).  `done` holds one bit per device ordinal; racing threads at worst repeat the idempotent call.
// Every kernel that takes dynamic LDS is launched through launch_lds<kernel>: the opt-in word must be one per kernel
// instantiation, and the function-local static of a template keyed on the kernel itself is exactly that -- no launcher
// declares a word of its own.
inline hipError_t lds_optin(const void* fn, size_t bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const unsigned long long bit = 1ull << (dev & 63);
  if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
  e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
  return e;
}
// compute units of the current device; 0 on error
inline int device_cu_count() {
  static std::atomic<int> cache[64];   // race-free: every thread computes the same value for a device
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return 0;
  int n = cache[dev & 63].load(std::memory_order_acquire);
  if (n > 0) return n;
  if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) return 0;
  cache[dev & 63].store(n, std::memory_order_release);
  return n;
}
// Launch of kernel Kfn with lds_bytes of dynamic LDS: opts Kfn in on the current device (once per device), launches, returns the
// launch's error.  optin_bytes: the size opted in to where it is not the launch's own (a kernel whose LDS varies from call to call
// opts in to its maximum once).
template <auto Kfn, class... Args>
hipError_t launch_lds_optin(size_t optin_bytes, dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, Args... args) {
  static std::atomic<unsigned long long> done{0};   // one word per Kfn, one bit per device
  if (hipError_t e = lds_optin(reinterpret_cast<const void*>(Kfn), optin_bytes, done)) return e;
  hipLaunchKernelGGL(Kfn, grid, block, lds_bytes, s, args...);
  return hipGetLastError();
}
template <auto Kfn, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, size_t lds_bytes, hipStream_t s, Args... args) {
  return launch_lds_optin<Kfn>(lds_bytes, grid, block, lds_bytes, s, args...);
}
// grid of the persistent kernels that hold a CU each: one workgroup per CU, at most one per tile
inline hipError_t persistent_grid(long long tiles, int& grid) {
  const int n_cu = device_cu_count();
  if (n_cu <= 0) return hipErrorUnknown;
  if (tiles > 0x7fffffffLL) return hipErrorInvalidValue;
  grid = tiles < n_cu ? (int)tiles : n_cu;
  return hipSuccess;
}
// workgroups of `fn` (block threads, dyn_lds bytes of dynamic LDS) that one CU holds at a time -- registers AND LDS, as the runtime
// computes it; a persistent kernel sized beyond this runs its surplus workgroups as a second, thinner wave of work.  0 on error.
inline int resident_workgroups_per_cu(const void* fn, int block, size_t dyn_lds) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, fn, block, dyn_lds) != hipSuccess) return 0;
  return nb;
}

// Launch context of the calling thread (launches are issued synchronously by the thread that calls the C ABI).  tail_slices:
// whether a persistent GEMM walk cuts the tiles of its partly filled last round into row slices (kernels_gemm_x3p.hip, X3Walk).
// On one stream that fills CUs which would idle for a tile time (+1.3 %); with two half-batches on two streams the other half's
// kernel takes those CUs, and slices -- 4x the workgroups for 0.7-1.0 of a tile time each -- only cost CU time (-0.6 %), so the
// two-stream loop turns them off.  Values do not depend on it.
// range_word: the F16X3 range-guard word (device memory, below) of the ENGINE whose call is being served -- the C ABI entry points of
// an engine set it around their launches; launches outside an engine (the single-op hooks) write to a per-device sink nobody reads.
// deep_stages: the "deep_stages" option of that engine (-1 outside an engine or when the engine has no value of its own: the
// process-wide default below).
struct LaunchCtx { bool tail_slices = true; unsigned* range_word = nullptr; int deep_stages = -1; };
extern thread_local LaunchCtx tl_launch_ctx;
// Option "deep_stages" (default on): the one-tile-per-workgroup GEMM launches (batches of a few sequences) stage three (256 x 128 tiles) /
// four (128 x 128) k-tiles deep instead of two (kernels_gemm_x3p.hip, NST).  Values do not depend on it.  Each engine carries its own
// setting (LaunchCtx::deep_stages); the process-wide default (one atomic, the key with a NULL engine) serves launches outside an engine.
void set_x3q_deep_stages(bool on);
bool x3q_deep_stages_default();
unsigned* range_sink_word();   // engine.hip: 4 bytes of device memory per device, allocated on first use (nullptr if that failed)
inline unsigned* launch_range_word() { return tl_launch_ctx.range_word ? tl_launch_ctx.range_word : range_sink_word(); }

enum Epi { EPI_NONE = 0, EPI_GELU = 1, EPI_RESIDUAL = 2 };

// ---- F16X3 operand ("pair") layout ---------------------------------------------------------------------------------
// A [rows, K] matrix that feeds an F16X3 GEMM lives in HBM as rows of 2K fp16 (K % 32 == 0): for every 32-deep k-tile t
// the 32 hi values sit at [64 t, 64 t + 32) and the 32 lo values at [64 t + 32, 64 t + 64) -- one 128-byte cache line
// per row per k-tile, which is exactly what one GEMM k-tile stages (kernels_gemm_x3p.hip).  Element (r, c):
//   hi at r * 2K + pair_col(c),   lo at r * 2K + pair_col(c) + PAIR_LO.
constexpr int PAIR_LO = 32;
__host__ __device__ __forceinline__ size_t pair_col(int c) { return (size_t)((c >> 5) << 6) + (size_t)(c & 31); }
// "Accumulator order" variant of the pair layout (the hidden activation fc1 -> fc2 only): inside every 32-column group
// column 16 jj + 4 q + r sits in slot 8 q + 4 jj + r, so that the 8 values a lane of the C^T accumulator layout holds of a
// group (q = lane / 16) are one 16-byte piece.  Legal for a GEMM operand because the consumer's weight uses the same order.
__host__ __device__ __forceinline__ size_t pair_col_acc(int c) {
  const int w = c & 31;
  return (size_t)((c >> 5) << 6) + (size_t)(8 * ((w & 15) >> 2) + 4 * (w >> 4) + (w & 3));
}

// ---- F16X3 range guard -------------------------------------------------------------------------------------------------
// An fp16 plane holds 8*x (activations; the q third of a qkv output 1*x) or 2^k*w (weights; k per matrix, 12 unless a weight
// exceeds 15.99): |x| > 8188 does not fit (clamped to +-65504 by the row / attention kernels, inf behind the GEMM epilogues'
// v_fma_mix split).  Every device-side plane writer therefore tracks max |value| per lane and ORs a bit into the sticky word its
// launcher handed it (launch_range_word(): the launching ENGINE's word) when one left the range (one atomic per lane that saw one:
// none in a healthy run).  Bits of the word: 1 = a plane value left the range, 2 = a folded LayerNorm met a row with |mean| > 16 sigma,
// 4 = a timestep index of q_sample / the p_losses tail outside [0, num_timesteps) (not a precision matter: raised in every mode),
// 8 = the head kernel's duplicated dot product disagreed with itself (kernels_elem.hip k_head: repaired by a third evaluation).
constexpr float X3_HALF_MAX = 65504.0f;
constexpr unsigned RANGE_BIT_ACT = 1u, RANGE_BIT_STATS = 2u, RANGE_BIT_INDEX = 4u, RANGE_BIT_RECOMPUTE = 8u;
__device__ __forceinline__ void range_raise(unsigned* rw, unsigned bit) { if (rw) atomicOr(rw, bit); }

// ---- kernels_gemm.hip -------------------------------------------------------------------------------------------
// C[M,N] = epi(A[M,K] @ W[N,K]^T + bias[N]); all row-major fp32, K % 32 == 0.
hipError_t launch_linear_f32(const float* A, const float* W, const float* bias, const float* R, float* C, int M, int N,
                             int K, int epi, hipStream_t s);

// ---- kernels_gemm_f16x3.hip --------------------------------------------------------------------------------------
// Same contract, fp32-accurate product from 3 fp16 MFMAs; A split on the fly, W in the pair layout made by
// split_weight_f16x3() ([rows][2*cols] fp16 of 4096*w: this form takes k = 12 only).
hipError_t launch_linear_f16x3(const float* A, const void* Wpair, const float* bias, const float* R, float* C, int M, int N,
                               int K, int epi, hipStream_t s);

// ---- kernels_gemm_x3p.hip ---------------------------------------------------------------------------------------
// F16X3 with pre-split operands in the pair layout: A (>= ceil(M/256)*256 rows allocated), W (>= ceil(N/256)*256 rows).
// outsplit: 0 = fp32 C; 1 = C as two [M][N] fp16 planes Ch/Cl of 8*c (read by the temporal attention kernel);
// 2 = C in the pair layout at Ch (operand of a following x3p GEMM; N % 32 == 0).  variant 0 = auto tile choice.
// qcols: with outsplit, columns < qcols carry 1*c instead of 8*c (q third of a temporal qkv GEMM).
//
// X3Fold (optional): the LayerNorm-folded / plane-resident forms used by the F16X3 engine path (engine.hip run_blocks):
//   st_in != null  : A holds the RAW rows x (pair layout of 8x), W holds W*diag(gamma), bias holds b + W beta, csum[n] =
//                    sum_k W[n,k] gamma[k]; the epilogue forms  LN(x) W^T + b = rstd (x W'^T) - rstd mu csum + b'  with the
//                    row's mean / rstd from st_in[(m * st_np + p)] = (sum, sum of squares) partials over the K columns
//                    (the buffer spans whole 256-row tiles: the persistent walk stages a tile's block of it by LDS-DMA)
//   Rp != null     : EPI_RESIDUAL takes the residual from a pair-layout plane buffer [M][2N] of 8r (instead of fp32 R);
//                    with outsplit == 2 and Ch == Rp the residual stream is updated in place, plane to plane
//   st_out != null : (with EPI_RESIDUAL) per row and 64-column block the (sum, sum of squares) of the new row values go to
//                    st_out[(m * (N/64) + block)] -- the st_in of the next folded GEMM (st_np = x3q_ntiles() = N/64)
//   pn.g != null   : (with EPI_RESIDUAL, Rp, N == 512) the tile spans whole rows, and the epilogue applies the block's post-norm
//                    to the new rows before they leave the chip:  y = LN(r + a W^T + b; pn.g, pn.b) [+ pos] [+ tvec]  (the
//                    operations of launch_layernorm); outsplit == 2: y -> pair planes Ch (may be Rp) and the (sum, sum of
//                    squares) partials of y -> st_out; outsplit == 0: y -> fp32 C
struct X3PostNorm {
  const float* g; const float* b; float eps;
  const float* pos; int pos_div, pos_mod;                          // nullable, as LnArgs
  const float* tvec; long long tvec_stride; int rows_per_batch;   // nullable, as LnArgs
  // bf16 mode only (launch_linear_bf16_rows): a SECOND LayerNorm of the rows just formed, written as bf16 operand rows -- the
  // norm2 behind proj (then g == nullptr: no post-norm, the rows are x + a W^T + b), the next block's norm1 behind fc2
  const float* g2; const float* b2; float eps2;
};
struct X3Fold {
  const float* st_in; int st_np; const float* csum; float eps;
  const void* Rp;
  float* st_out;
  X3PostNorm pn;
};
bool x3q_postnorm_ok(int N, int K);   // shapes the post-norm form exists for
// w_exp: the exponent k of the weight planes (split_weight_f16x3): the accumulators are un-scaled by 2^-(3 + w_exp)
hipError_t launch_linear_x3p(const void* Apair, const void* Wpair, const float* bias, const float* R, float* C, void* Ch,
                             void* Cl, int M, int N, int K, int epi, int outsplit, int qcols, int variant, hipStream_t s,
                             const X3Fold* fold = nullptr, int w_exp = 12);
int x3q_ntiles(int M, int N);   // statistics partials per row an st_out launch writes
// ---- latency mode (engine option "latency_mode"): fc2 + post-norm of a SMALL call as a split-K x split-N GEMM + an ordered reduce ----
// The whole-row post-norm tile stages all of W2 per workgroup, whatever its height: a launch that cannot fill one round of those tiles
// lasts K/32 k-tiles at one CU's L2 -> LDS rate with most of the chip idle.  Here 128 x 128 tiles x S k-ranges spread the staging:
//   launch_linear_x3p_splitk : P[ks][M][N] (fp32, un-scaled) = A[:, k-range ks] . W[:, k-range ks]^T          (kernels_gemm_x3p.hip)
//   launch_splitk_postnorm   : y = LN(r + bias + P[0] + P[1] + ... + P[S-1]) [+ pos] [+ tvec], the additions in exactly that order; the
//                              operations, outputs and range-guard reporting of launch_layernorm (y_x3 + stats, or fp32 y)  (kernels_fc2_splitk.hip)
// fc2_splitk_choose: S in {2, 4}, or 0 = keep the whole-row form.  A pure function of (M, N, K, CU count) -- the same for eager and
// captured runs --: among S in {1, 2, 4} with K/32/S >= 4 k-tiles and W = ceil(M/128) (N/128) S workgroups, cost(S) = K/32/S where
// W <= CUs, 1.45 K/32/S where W <= 2 CUs (two co-resident 128 x 128 workgroups take 1.33-1.45x a lone one: experiments/NOTES.md), excluded
// beyond; cheapest, the smaller on a tie; 0 unless that is >= 2, the post-norm tile shape applies and ceil(M/64) < CUs.
int fc2_splitk_choose(int M, int N, int K, int n_cu);
bool fc2_splitk_ok(int N, int K, int S);   // shapes the pair of kernels exists for
hipError_t launch_linear_x3p_splitk(const void* Apair, const void* Wpair, float* P, int M, int N, int K, int S, hipStream_t s, int w_exp = 12);
// Rp: residual planes [M][2N] of 8r; Yp (with stats: [M][2], one (sum, sum of squares) per row) may be Rp; Y (fp32) may alias Rp's
// bytes row for row.  Exactly one of Yp / Y.
hipError_t launch_splitk_postnorm(const float* P, int S, const void* Rp, const float* bias, const X3PostNorm& pn, float* Y, void* Yp,
                                  float* stats, int M, int N, hipStream_t s);
// ---- latency mode, proj and fc1 (kernels_splitk_reduce.hip): the same split GEMM + an ordered reduce with the launch's own epilogue ----
//   launch_splitk_residual : x = r + bias + P[0] + ... + P[S-1] -> stream planes Xp (may be Rp) + st_out, one (sum, sum of squares) per row
//                            and 64 columns (x3q_ntiles per row: the st_in of the folded fc1); N == 512
//   launch_splitk_gelu     : h = gelu(rstd (P[0] + ... + P[S-1]) - rstd mean csum + bias) -> Hp, accumulator-order pair layout (the A
//                            operand of either fc2 form); mean / rstd from st_in[(m st_np + p)] over K columns; N % 512 == 0
// proj_splitk_choose / fc1_splitk_choose: S in {2, 4}, or 0 = keep the present launch.  Pure functions of (M, N, K, CU count).  In units
// of one k-tile of a lone 128 x 128 workgroup:
//   present launch (launch_x3q_auto)  K/32 where ceil(M/128) (N/128) <= CUs (128 x 128 tiles), else 1.4 K/32 ceil(tiles of 256 x 128 / CUs)
//   split, S in {2, 4}, K/32/S >= 4   K/32/S, x 1.45 where the W = ceil(M/128) (N/128) S workgroups exceed the CUs, + the reduce launch
//                                     (PLACEHOLDERS, not tuned values: no measurement is on file yet -- the table is to be
//                                     profiles/latency_mode_proj_fc1.json -- so both stand at 16, the present launch's own depth at
//                                     K = 512: the model shows no gain and the rules return 0 everywhere until they are measured)
// W > 2 CUs is excluded; fc1 also excludes W > CUs (two co-resident 128 x 128 workgroups of fc1 lose: NOTES round 6) and M S N beyond
// the engine's scratch buffer.  The cheapest S wins if it beats the present launch, the smaller on a tie; 0 unless N, K are those of
// the D = 512 flow.
constexpr size_t FC1_SPLITK_SCRATCH_FLOATS = (size_t)8192 * 1024;   // fc1 partials, M S <= 8192 rows at Dm = 1024: 32 MiB
int proj_splitk_choose(int M, int N, int K, int n_cu);
int fc1_splitk_choose(int M, int N, int K, int n_cu);
bool proj_splitk_ok(int N, int K, int S);                  // shapes the kernel pairs exist for (a forced S, the op hooks)
bool fc1_splitk_ok(int N, int K, int S);
bool proj_splitk_fits(int M, int N, int S, int n_cu);      // ... and calls they serve: W <= 2 CUs (fc1: and the scratch bound)
bool fc1_splitk_fits(int M, int N, int S, int n_cu);
hipError_t launch_splitk_residual(const float* P, int S, const void* Rp, const float* bias, void* Xp, float* st_out, int M, int N,
                                  hipStream_t s);
hipError_t launch_splitk_gelu(const float* P, int S, const float* st_in, int st_np, const float* csum, const float* bias, float eps,
                              void* Hp, int M, int N, int K, hipStream_t s);
hipError_t launch_unsplit_acc(const void* pair, float* x, size_t rows, int cols, hipStream_t s);   // op hooks only
hipError_t launch_split_x3(const float* x, void* pair, size_t rows, int cols, hipStream_t s);
hipError_t launch_unsplit_x3(const void* pair, float* x, size_t rows, int cols, const float* part, int np, float* stats,
                             hipStream_t s);   // op hooks only
// bf16 operand mode (D3D_PREC_BF16): A / W plain bf16 rows (K % 64 == 0, rows padded as above), one bf16 MFMA per product, fp32
// accumulate.  EPI_NONE / EPI_GELU write Cb = bf16 [M][N] (columns < qcols scaled by 2^-3), EPI_RESIDUAL writes fp32 C = R + ...
// f16 = true, here and on every launcher of this group: the fp16 operand mode (D3D_PREC_F16) -- the same kernels instantiated for fp16
// rows (FX_F16): the f16 twin of each bf16 MFMA, every 16-bit output rounded to fp16 (nearest even, subnormals kept, inf beyond 65504).
hipError_t launch_linear_bf16(const void* A, const void* W, const float* bias, const float* R, float* C, void* Cb, int M, int N,
                              int K, int epi, int qcols, hipStream_t s, bool f16 = false);
// Whole-row form (N == 512, 128-row tiles): X[M,N] fp32 is the residual stream, updated IN PLACE,
//   y = X + A W^T + bias;   if pn.g: y = LN(y; pn.g, pn.b, pn.eps) [+ pos] [+ tvec];   X = y;
//   if pn.g2: Hb = bf16(LN(y; pn.g2, pn.b2, pn.eps2))   (bf16 [M][N], the next GEMM's operand)
// -- proj + norm2 (pn.g == nullptr) and fc2 + post-norm + next norm1 of a bf16-mode block without any row kernel.
bool bf16_rows_ok(int N, int K);
hipError_t launch_linear_bf16_rows(const void* A, const void* W, const float* bias, float* X, void* Hb, int M, int N, int K,
                                   const X3PostNorm& pn, hipStream_t s, bool f16 = false);
// kernels_gemm_bf16q.hip: the plain bf16 GEMMs (qkv, fc1) on the hand-specialised two-phase k-loop; bit-identical to launch_linear_bf16's forms
bool gemm_bf16q_ok(int N, int K);
hipError_t launch_gemm_bf16q(const void* A, const void* W, const float* bias, void* Cb, int M, int N, int K, int epi, int qcols, hipStream_t s,
                             bool f16 = false);
hipError_t launch_f32_to_bf16(const float* x, void* y, size_t n, hipStream_t s, bool f16 = false);
hipError_t launch_bf16_to_f32(const void* x, float* y, size_t n, hipStream_t s, bool f16 = false);
hipError_t launch_scale_cols(float* x, size_t rows, int cols, int ncols_scaled, float f, hipStream_t s);   // op hooks only

// ---- kernels_qkv_sattn.hip: spatial blocks, qkv GEMM (LayerNorm-folded) + J-key attention in one kernel, J = 15, 16, 17 --------------------
// Apair: the residual stream planes (rows up to 255 * ceil(frames / 15) + 1 are staged at 17 joints, never more at 15 / 16); W / bias / csum HEAD-MAJOR (row 192 h +
// 64 part + d); st_in / st_np / eps as X3Fold; out_x3: attention output in the pair layout.  M = frames * J tokens.
bool qkv_sattn_ok(int J, int D, int H, int K);
hipError_t launch_qkv_sattn(const void* Apair, const void* Wpair_headmajor, const float* bias_hm, const float* csum_hm, const float* st_in,
                            int st_np, float eps, int w_exp, void* out_x3, int M, int K, int J, int D, int H, hipStream_t s);
// Block 0 without the K = D GEMM (k_qkv_sattn_direct): its input rows are W_e u + b_e + spos[j] + tv[b] with u the in_chans + 3 raw channels
// of a token, so Wg x = G u + P[j] + Q[b] (fp32; G [3 D][in_chans + 3] and P [J][3 D] in the head-major order of bias_hm / csum_hm, Q [1 or B][3 D]
// in the original column order; Q nullptr without time embedding, q_stride 0 or 3 D floats between batch elements).  in_chans 1 .. 3.  x2d / y / y_bcast_T as launch_embed_planes.  out_x3: the fused form;
// out_x3 == nullptr: the [M][3 D] hi / lo planes launch_attn_temporal_x3 reads, bit for bit the values the fused form keeps in LDS.
bool qkv_sattn_direct_ok(int J, int D, int H, int in_chans);
hipError_t launch_qkv_sattn_direct(const float* x2d, const float* y, int y_bcast_T, int in_chans, const float* G, const float* P, const float* Q,
                                   int q_stride, const float* bias_hm, const float* csum_hm, const float* st_in, int st_np, float eps, void* out_x3,
                                   void* planes_hi, void* planes_lo, int M, int T, int J, int D, int H, hipStream_t s);
// kernels_qkv_tattn.hip: the temporal counterpart -- the LayerNorm-folded qkv GEMM of one (batch, joint) group (T in 193..255 frames; T <= 127:
// of 255 / T joints of one batch element, per-joint key windows) x one head with the T-key attention of k_attn_temporal_x3s run from LDS; the same tile-ordered weight / bias / csum as launch_qkv_sattn.
// kernels_fc1_x3.hip: fc1 (LayerNorm-folded, GELU, accumulator-order pair output) on the hand-specialised k-loop of the fused kernels,
// whole 256 x 256 tiles only (buffers padded to 256 rows, finite pad rows); bit-identical to launch_linear_x3p's form.
// kernels_proj_x3.hip: proj (plane residual in place + row statistics) likewise, whole 192 x 256 tiles (M % 192 == 0: the caller runs the
// remaining rows through launch_linear_x3p); bit-identical to launch_linear_x3p's form.
bool proj_x3_ok(int N, int K);
hipError_t launch_proj_x3(const void* Apair, const void* Wpair, const float* bias, void* Xpair, float* st_out, int w_exp, int M, int N, int K,
                          hipStream_t s);
bool fc1_x3_ok(int N, int K);
hipError_t launch_fc1_x3(const void* Apair, const void* Wpair, const float* bias_f, const float* csum, const float* st_in, int st_np,
                         float eps, int w_exp, void* out_pair, int M, int N, int K, hipStream_t s);
bool qkv_tattn_ok(int T, int J, int D, int H, int K);
hipError_t launch_qkv_tattn(const void* Apair, const void* Wpair_tileorder, const float* bias_to, const float* csum_to, const float* st_in,
                            int st_np, float eps, int w_exp, void* out_x3, int B, int T, int J, int K, int D, int H, hipStream_t s);
// kernels_qkv_attn_x3_small.hip ("small_tiles" under "latency_mode"): the same fused step on 128-row tiles -- floor(127 / N) whole groups of
// N <= 127 tokens x one head per workgroup, one row map for both block types (group u holds rows (u / stride) * N * stride + u % stride +
// t * stride: spatial (B * T, J, 1) with J in 15 .. 17, temporal (B * J, T, J)), one tile per workgroup; the tile-ordered weight / bias /
// csum of launch_qkv_sattn.  Bit-identical to the qkv GEMM followed by launch_attn_temporal_x3.  Only the groups * N rows of Apair are read.
bool qkv_attn_x3_small_ok(int N, int stride, int J, int D, int H, int K);
long long qkv_attn_x3_small_workgroups(long long groups, int N);
hipError_t launch_qkv_attn_x3_small(const void* Apair, const void* Wpair_tileorder, const float* bias_to, const float* csum_to, const float* st_in,
                                    int st_np, float eps, int w_exp, void* out_x3, int groups, int N, int stride, int J, int K, int D, int H,
                                    hipStream_t s);
// "fused_narrow": the same kernel for heads of 32 columns in pairs (D = 32 H, H even) or of 16 columns in quads (D = 16 H, H % 4 == 0): a
// pair / a quad is one 64-column segment, D / 64 workgroups per row tile, the images in the tile order of D / 64 pseudo-heads
// (tile_order_src_row(r, D, D / 64)).  K == D >= 128; spatial groups of any J <= 127 joints, temporal ones of T <= 127 frames.  Bit-identical
// to the folded qkv GEMM followed by launch_attn_x3_h32 / launch_attn_x3_h16.
bool qkv_attn_x3_narrow_ok(int N, int stride, int J, int D, int H, int K);
hipError_t launch_qkv_attn_x3_narrow(const void* Apair, const void* Wpair_tileorder, const float* bias_to, const float* csum_to, const float* st_in,
                                     int st_np, float eps, int w_exp, void* out_x3, int groups, int N, int stride, int J, int K, int D, int H,
                                     hipStream_t s);

// ---- kernels_elem.hip -------------------------------------------------------------------------------------------
// Row LayerNorm; optionally also writes a second LayerNorm of the first result (post-norm -> next block's norm1).
//   y  = LN(x; g1,b1,eps1) [+ pos[(row / pos_div) % pos_mod] ] [+ tvec[(row / rows_per_batch) * tvec_stride]]
//   h  = LN(y; g2,b2,eps2)                       (only when h != nullptr)
struct LnArgs {
  const float* x;
  float* y;          // may alias x; may be nullptr when only h is wanted (then h = LN(x; g1,b1))
  float* h;          // nullable
  void* h_x3;        // nullable: when set, h is written in the F16X3 pair layout (8*h, D % 32 == 0) instead of fp32
                     //           (h itself may then be nullptr)
  void* h_bf16;      // nullable: when set, h is written as plain bf16 rows (operand of a bf16-mode GEMM) instead of fp32
  const float* g1; const float* b1; float eps1;
  const float* g2; const float* b2; float eps2;
  const float* pos;  // nullable, (pos_mod, D)
  int pos_div, pos_mod;
  int skip_ln1;      // 1: y = x (+ pos + tvec) without the first normalisation (entry of block 0)
  void* y_x3;        // nullable: y also / instead goes out in the F16X3 pair layout (8*y): the plane-resident residual stream
  float* stats;      // nullable: (sum, sum of squares) of every y row, [rows][2] -- consumed by an LN-folded GEMM (X3Fold)
  const float* tvec; // nullable, per-batch vector (n, D) with row stride tvec_stride (0 = broadcast)
  int64_t tvec_stride;
  int rows_per_batch;
  int rows, D;
  unsigned* range;   // filled in by launch_layernorm: the range-guard word the plane outputs report to
  int h_f16;         // 1: the h_bf16 rows are fp16 (D3D_PREC_F16: round to nearest even, subnormals kept)
};
hipError_t launch_layernorm(const LnArgs& a, hipStream_t s);

// X[m,:] = W_f [x2d[m], y[m']] + b_f + spos[j] + tvec[b]   (S2S:250, :229-233, :113-116 of block 0)
hipError_t launch_embed(const float* x2d, const float* y, const float* Wf, const float* bf, const float* spos,
                        const float* tvec, int64_t tvec_stride, float* X, int B, int T, int J, int D, int in_chans,
                        int y_bcast_T, hipStream_t s);

// the same, written as the F16X3 residual-stream planes (pair layout of 8 X) + per-row (sum, sum of squares): embed and the
// stream-entry row kernel in one pass (D == 512)
bool embed_planes_ok(int D, int in_chans);
hipError_t launch_embed_planes(const float* x2d, const float* y, const float* Wf, const float* bf, const float* spos,
                               const float* tvec, int64_t tvec_stride, void* XP, float* stats, int B, int T, int J, int D,
                               int in_chans, int y_bcast_T, hipStream_t s);

// sinusoid + trunk + per-block projections: out (n, nblk, D)
hipError_t launch_sinusoid(const float* times, const float* freqs, float* out, int n, int D, hipStream_t s);
// out[n,N] = post(act_pre(in[n,K]) @ W[N,K]^T + b); act: 0 none, 1 gelu(post), 2 silu(pre); b may be nullptr; in_stride: floats between
// input rows (0 = K)
hipError_t launch_small_linear(const float* in, const float* W, const float* b, float* out, int n, int N, int K,
                               int act, hipStream_t s, int64_t in_stride = 0);

// seq2frame frame reduce (S2F:261-263): out[b,j,:] = sum_t w[t] X[b,t,j,:] + bias
hipError_t launch_frame_reduce(const float* X, const float* w, const float* bias, float* out, int B, int T, int J, int D,
                               hipStream_t s);

struct HeadArgs {
  const float* X;        // (rows, D)
  const float* g; const float* b; float eps;   // head.0
  const float* Wh; const float* bh;            // head.1 (3, D), (3,)
  int rows, D;
  // outputs
  float* x0_raw;         // nullable: raw network output (rows,3)
  // DDIM step (all nullable when mode == 0)
  int mode;              // 0: raw only; 1: clamp?/DDIM update; 2: final step (y_out = clamped x0)
  int clip;
  const float* y_cur;    // (rows,3)
  float* y_next;         // (rows,3) (may alias y_cur)
  const float* noise;    // nullable (rows,3)
  float alpha, alpha_next, somac, eta;
  float* traj_rev; float* traj_x0; int traj_rev_stride, traj_x0_stride, traj_idx;   // nullable
  unsigned* range;       // filled in by launch_head: the launching engine's guard word (RANGE_BIT_RECOMPUTE)
  int fence;             // "head_fence" option: every row's dot products evaluated twice and compared (RANGE_BIT_RECOMPUTE)
  int inject;            // tests only ("head_inject" option; implies the fence): perturb the first evaluation of row 0
};
hipError_t launch_head(const HeadArgs& a, hipStream_t s);

hipError_t launch_range_snapshot(unsigned* word, unsigned* host_slot_dev, hipStream_t s);   // d3d_engine_range_post
hipError_t launch_q_sample(const float* x_start, const float* noise, const int32_t* t, const float* sqrt_ac,
                           const float* somac, float* out, int B, int64_t n, int nt, hipStream_t s);

// p_losses tail (DIFF:411-418) and the repeat_n tiling / hypothesis mean of forward() (DIFF:433-448); n = elements per batch row
hipError_t launch_weighted_loss(const float* model_out, const float* target, const int32_t* t, const float* ac, const float* somac,
                                float* out, int B, int64_t n, int l2, int clip, int nt, hipStream_t s);
hipError_t launch_repeat_rows(const float* x, float* out, int B, int64_t n, int R, hipStream_t s);
hipError_t launch_hypothesis_mean(const float* pred, float* out, int B, int64_t n, int R, hipStream_t s);

// joint permutation of the horizontal flip, passed by value as a kernel argument (no device allocation, no copy, no sync)
struct JointPerm { static constexpr int MAXJ = 64; int32_t p[MAXJ]; };
hipError_t launch_tta_mpjpe(const float* pred, const float* pred_flip, const float* gt, const uint8_t* mask, float scale,
                            const JointPerm& perm, float* merged, double* sums, int B, int T, int J, hipStream_t s);
// evaluate()'s other three protocols on the merged prediction (kernels_elem.hip k_pose_metrics; RUN:602-614, LOSS:43-93, 132-142)
hipError_t launch_pose_metrics(const float* pred, const float* gt, const uint8_t* mask, double* sums, int N, int J, hipStream_t s);

hipError_t launch_window_gather(const float* seq, float* out, uint8_t* mask, const JointPerm& perm, int n, int T, int J, int C,
                                int flip, hipStream_t s);
hipError_t launch_window_gather_s2f(const float* seq, float* out, const JointPerm& perm, int n, int T, int J, int C, int first, int count,
                                    int flip, hipStream_t s);

// debug trace: *out += position-weighted 64-bit sum of the buffer's 32-bit words (order-independent)
hipError_t launch_checksum(const void* p, size_t bytes, unsigned long long* out, int rot, hipStream_t s);
// probes.hip: what the chip sustains (what 0: fp16 MFMA TFLOP/s in register loops; 1: L2 -> LDS staging GB/s chip-wide)
hipError_t launch_probe_machine(int what, float ms_target, float* result, hipStream_t s);

// ---- kernels_attn.hip -------------------------------------------------------------------------------------------
// qkv: (B*T*J, 3*D) -> out (B*T*J, D), GRAND core  O = softmax(q k^T * dh^-0.5) v - v
// When out_x3 is non-null the result is written in the F16X3 pair layout (8*o, operand of the proj GEMM; D % 32 == 0)
// and `out` is ignored.
hipError_t launch_attn_spatial_f32(const float* qkv, float* out, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
hipError_t launch_attn_temporal_f32(const float* qkv, float* out, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
hipError_t launch_attn_generic(const float* qkv, float* out, void* out_x3, int B, int T, int J, int D, int H, int temporal,
                               hipStream_t s);
// ---- The attention kernel families of attn_dispatch.h beyond kernels_attn.hip: one contract per operand form -------------------------
// Every launcher takes (B, T, J, D, H): B J groups of T tokens, J tokens apart; spatial blocks call it with (B T, J, 1).  A resident
// launcher holds a group's keys in LDS and serves what its *_ok(N, D, H) predicate accepts (N = the group length); its *_long twin
// streams the keys through LDS in chunks and serves a window of any length, bit-identical to the resident kernel wherever that runs.
// A launch returns hipErrorInvalidValue where its predicate fails or its grid -- for a streaming launch B J (units per token)
// ceil(T / 256) workgroups -- exceeds 2^31 - 1.
//
// Planes form (F16X3 accuracy on fp16 MFMA, attn_x3_tile.h): qkv as hi / lo fp16 planes, [rows][3 D] each, as the qkv GEMM writes them
// with outsplit = 1 (raw q, 8 k, 8 v); the output in the pair layout, its rows 2 ceil32(D) halves apart (2 D wherever D % 32 == 0, as in
// every engine).  The streaming kernels (kernels_attn_x3_long.hip, k_attn_x3_stream<DH, KC>) compute the scores twice, for the exact
// maximum and for the numerators.
//
// Rows form (exact fp32 on v_mfma_f32_32x32x2_f32, attn_f32_tile.h: arithmetic, staging, launch ladder and streaming geometry shared
// with the width-64 kernels of kernels_attn.hip): fp32 rows in, fp32 rows out, no pair-layout form (FP32 engines only).  The scores are
// scaled by 1 / sqrt(DH) after the sum over d and v[query] is subtracted at the store (widths 128, 48 / 96 and 16: the second product
// takes the unnormalised numerators and the store divides by their sum), so the bits are not those of launch_attn_generic.  A head
// reads and writes its own DH columns alone (a half-used accumulator tile takes zeros).  The streaming kernels make three passes at
// widths 64 and 32 (maximum, sum, normalised product), two elsewhere (maximum; numerators, their sum and the product).
//
//   launcher (+ _long)             D / H     heads (units per token)                 resident N <=  chunk      instantiated in
//   launch_attn_temporal_x3        64        any (H)                                 256            256        kernels_attn_x3.hip; _long: kernels_attn_x3_long.hip <64, 8>
//   launch_attn_x3_h32             32        even (H / 2: a pair shares an LDS row)  256            256        kernels_attn_x3_h32.hip; <32, 8>
//   launch_attn_x3_h128            128       any (H: two 64-column halves a head)    128            128        kernels_attn_x3_h128.hip; <128, 4>
//   launch_attn_x3_hx              48 / 96   any (H: DH adjacent plane columns)      256 / 128      256 / 128  kernels_attn_x3_hx.hip; <48, 8> / <96, 4>
//   launch_attn_x3_h16             16        H % 4 == 0 (H / 4: a quad shares a row) 256            256        kernels_attn_x3_h16.hip; <16, 8>
//   launch_attn_temporal_f32_long  64        any (H)                                 (no twin here) 256        kernels_attn_f32_long.hip, k_attn_f32_stream3<64>
//   launch_attn_temporal_f32_h32   32        any (H)                                 256            256        kernels_attn_f32_h32.hip; kernels_attn_f32_h32_long.hip
//   launch_attn_f32_h128           128       any (H)                                 128            128        kernels_attn_f32_h128.hip
//   launch_attn_f32_hx             48 / 96   any (H)                                 256 / 192      256 / 192  kernels_attn_f32_hx.hip, k_attn_f32_hx_stream<48> / <96>
//   launch_attn_f32_h16            16        any (H)                                 256            256        kernels_attn_f32_hx.hip at DH = 16
// launch_attn_temporal_f32_long's resident twin is launch_attn_temporal_f32 of kernels_attn.hip (T <= 256).
// launch_attn_spatial_f32_h32 is the VALU form of width 32 for 15 .. 17 joints; it takes the block's own (B, T, J), as the launchers of
// kernels_attn.hip do.
hipError_t launch_attn_temporal_x3(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                   hipStream_t s);
bool attn_temporal_x3_ok(int T, int D, int H);
hipError_t launch_attn_temporal_x3_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                        hipStream_t s);
bool attn_temporal_x3_long_ok(int T, int D, int H);
hipError_t launch_attn_x3_h32(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h32_ok(int N, int D, int H);
hipError_t launch_attn_x3_h32_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h32_long_ok(int T, int D, int H);
hipError_t launch_attn_x3_h128(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h128_ok(int N, int D, int H);
hipError_t launch_attn_x3_h128_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h128_long_ok(int T, int D, int H);
hipError_t launch_attn_x3_hx(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_hx_ok(int N, int D, int H);
hipError_t launch_attn_x3_hx_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_hx_long_ok(int T, int D, int H);
hipError_t launch_attn_x3_h16(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h16_ok(int N, int D, int H);
hipError_t launch_attn_x3_h16_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_x3_h16_long_ok(int T, int D, int H);
hipError_t launch_attn_temporal_f32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_temporal_f32_long_ok(int T, int D, int H);
hipError_t launch_attn_temporal_f32_h32(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
hipError_t launch_attn_spatial_f32_h32(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_temporal_f32_h32_ok(int T, int D, int H);
bool attn_spatial_f32_h32_ok(int J, int D, int H);
hipError_t launch_attn_temporal_f32_h32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_temporal_f32_h32_long_ok(int T, int D, int H);
hipError_t launch_attn_f32_h128(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_h128_ok(int N, int D, int H);
hipError_t launch_attn_f32_h128_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_h128_long_ok(int T, int D, int H);
hipError_t launch_attn_f32_hx(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_hx_ok(int N, int D, int H);
hipError_t launch_attn_f32_hx_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_hx_long_ok(int T, int D, int H);
hipError_t launch_attn_f32_h16(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_h16_ok(int N, int D, int H);
hipError_t launch_attn_f32_h16_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s);
bool attn_f32_h16_long_ok(int T, int D, int H);
hipError_t launch_split_qkv(const float* x, void* hi, void* lo, size_t rows, int D, hipStream_t s);
hipError_t launch_unsplit_pair(const void* pair, float* x, size_t rows, int cols, hipStream_t s);
bool attn_spatial_fast_ok(int J, int D, int H);
// ---- kernels_attn_bf16.hip: the same core on v_mfma_f32_32x32x16_bf16, one MFMA per product (D3D_PREC_BF16).  qkv: ONE bf16
// buffer [rows][3D] (q third pre-scaled by dh^-0.5, written by launch_linear_bf16 with qcols = D); out: bf16 [rows][D].
// Spatial blocks: call with (B * T, J, 1).  softmax - I is normalised and rounded to bf16 before the second product.
hipError_t launch_attn_bf16(const void* qkv_bf16, void* out_bf16, int B, int T, int J, int D, int H, hipStream_t s, bool f16 = false);
bool attn_bf16_ok(int T, int D, int H);
// ---- kernels_qkv_attn_bf16.hip: the bf16 qkv GEMM and that attention in ONE kernel (k_qkv_sattn_bf16 / k_qkv_tattn_bf16): q / k / v stay
// in LDS; bit-identical to launch_linear_bf16 / launch_gemm_bf16q (qcols = D) followed by launch_attn_bf16.  A: bf16 [groups * N][D]
// (only those rows are read); W: bf16 [3 D][D]; out: bf16 [groups * N][D], NOT A (every head reads whole rows of A).  Group u holds rows
// (u / stride) * N * stride + u % stride + t * stride, t < N -- spatial blocks: (B * T, J, 1), temporal blocks: (B * J, T, J).
// The predicates: head width 64, D % 128 == 0, D >= 256, groups of <= 255 tokens (spatial: <= 32), B * T * J * D * 2 < 2^32.
bool qkv_sattn_bf16_ok(int T, int J, int D, int H, int B);
bool qkv_tattn_bf16_ok(int T, int J, int D, int H, int B);
hipError_t launch_qkv_attn_bf16(const void* A, const void* W, const float* bias, void* out, int groups, int N, int stride, int D, int H,
                                int temporal, hipStream_t s, bool f16 = false);
bool attn_temporal_fast_ok(int T, int D, int H);

}  // namespace d3d
