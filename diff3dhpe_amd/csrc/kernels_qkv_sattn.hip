// Spatial blocks of the F16X3 flow, fused: the LayerNorm-folded qkv GEMM of a frame group with the 17-key (15, 16) GRAND attention of its
// frames run from LDS (S2S:67 + 73-83 for the per-frame groups of S2S:119).  What it removes from the unfused flow
// (k_linear_x3q_persist<qkv form> + k_attn_temporal_x3p<1,8,3>): the q / k / v planes never exist in HBM -- 1.62 GB written and
// 1.62 GB read back per launch pair at the bench shape -- and one kernel launch per spatial block.
//
// (What follows describes the 17-joint form.  15 and 16 joints run the same code on a tile of 16 whole frames -- 240 / 256 rows, slots
// of 6 x J rows, both passes with eight slots: see QsGeo below for what changes with the joint count.)
// Tile = 15 whole frames (255 token rows; 256 are staged and multiplied) x ONE head's q, k, v (192 output columns: the folded weight
// is stored HEAD-MAJOR at commit, rows [192 h, 192 h + 192) = q_h, k_h, v_h, so an N-tile is contiguous).  Eight waves (2 x 4), a
// wave owns 128 rows x 48 columns = 8 x 3 accumulator tiles of 16x16 (96 VGPRs).  The k-loop is the two-phase persistent loop of
// kernels_gemm_x3p.hip (LDS-DMA staging, counted vmcnt waits, W fragments read a phase ahead) on a 256 x 192 x 32 stage of
// 56 KiB; per output element the same MFMAs in the same order as every other F16X3 GEMM shape, and the epilogue arithmetic is that
// of x3q_epilogue8<LN-folded, planes>: the q / k / v values are bit for bit those the unfused qkv GEMM writes to HBM, so the whole
// block is bit-identical to the unfused flow ("fused_spatial" engine option, tests/test_gpu_round4.py).
//
// After the k-loop the tile's 255 x 192 values (196 KB as hi / lo fp16) do not fit the LDS at once; two passes:
//   pass 0: frames 0-3 and 8-11 (rows 0..67 of wave-row 0, 136..203 of wave-row 1: BOTH wave rows write half their accumulators)
//           -> q / k / v hi / lo planes of 8 frame slots (6 x 17 rows x 128 B each, the swizzles of kernels_attn_x3.hip) -> barrier
//           -> wave w runs one frame (scores, softmax, (P - I) V as in k_attn_temporal_x3p) and stores its 17 x 64 outputs as
//           whole 128-byte lines of the pair layout
//   pass 1: frames 4-7 and 12-14 likewise, 7 slots; the next tile's first k-tile is requested in front of its attention step
// (first version: pass 0 = rows 0..135, pass 1 = the rest -- each pass written by ONE wave row while the other waited: 3.8 + 4.4 us
// of a 40.5 us tile, in-kernel stamps; the epilogue steps are VALU-issue-bound with two waves per SIMD)
// LDS map (160 KiB): [0, 56 K) stage 0 | [56 K, 158 K) stage 1, then the frame slots (+ the raw row-statistics block during the
// k-loop) | 2 KiB of per-row LayerNorm statistics.
// Skeletons of 15 and 16 joints (the reference's --dataset humaneva* branch, 16-joint H36M variants) take the same kernels on a tile of
// 16 frames: QsGeo below.  The joint count is a compile-time parameter; the 17-joint instantiations are the code they were before it was.
// Block 0 runs k_qkv_sattn_direct (below): the same tile and the same code behind the accumulators, which it fills from the raw input
// channels of the tokens and commit-time tables instead of a k-loop ("block0_direct" engine option).
#include "d3d_kernels.h"
#include "qkv_fused_kloop.h"

#include <math.h>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "attn_lds.h"

QF_SHAPE(8, 3, 256, 192, 4, 3);                                          // 256 x 192 x 32 stage of 57344 bytes
constexpr int QS_QKV = QF_STAGE;                                         // frame slots start behind stage 0
constexpr int QS_RAW = 2 * QF_STAGE;                                     // raw statistics partials while the k-loop runs (16 KiB)
constexpr int QS_RAW_MAX = 16384;
// The tile geometry of a joint count J (a compile-time parameter of the whole kernel family; J = 17 is the form described above):
//   J = 17: 15 frames, 255 rows (row 255 is the next tile's first)      J = 16: 16 frames, 256 rows, a frame is one 16-row m-tile
//   J = 15: 16 frames, 240 rows; the 16 trailing rows (the next tile's first frame and the first joint of its second) are staged and
//           multiplied like row 255 of the 17-joint form and never written to a slot, attended, stored or counted
// With 16 frames both passes fill all eight slots (same rule: frame fr -> pass (fr >> 2) & 1, slot (fr & 3) + 4 (fr >> 3)).
template <int J>
struct QsGeo {
  static_assert(J == 15 || J == 16 || J == 17, "joint counts with a tile geometry");
  static constexpr int FPT = J == 17 ? 15 : 16, ROWS = J * FPT;          // whole frames / token rows per tile
  static constexpr int PLANE = J * 128;                                  // 1920, 2048, 2176
  // a slot: six planes; its last two (Q hi, Q lo) double as the wave's 4 KiB output patch, which at J = 15 is 256 bytes more than they hold
  static constexpr int SLOT = 4 * PLANE + (2 * PLANE > 4096 ? 2 * PLANE : 4096);   // 11776, 12288, 13056
  static constexpr int STX = QS_QKV + 8 * SLOT;                          // (rstd', -mean rstd) of the tile's 256 rows, 2 KiB (J = 17: 161792)
  static constexpr int LDS = STX + QF_BM * 8;                            // 153600, 157696, 163840
  static_assert(LDS <= 160 * 1024 && QS_RAW + QS_RAW_MAX <= STX, "LDS map");
  // planes of a slot: V hi, V lo, K hi, K lo, Q hi, Q lo.  A fragment read takes 32 rows (K, Q) or the key rows of the 16-key steps it
  // runs (V), so the rows behind a plane's J are whatever follows it.  For V that must be FINITE (0 x NaN in the second product):
  //   J = 17: 15 pad rows; V hi runs into V lo, V lo into K hi, both written in the same pass
  //   J = 16: one 16-key step, all of its rows real: no V read leaves its plane
  //   J = 15: one 16-key step with ONE pad row, key 15: row 0 of V lo behind V hi, row 0 of K hi behind V lo -- the same frame's own
  //           values, written in the same pass
  // Pad keys of K never reach the softmax (-inf scores, or accumulator registers nothing reads) and pad queries of Q are never stored:
  // any bits will do there.  The last slot's Q reads end 32 - J rows behind it, inside the statistics block.
  static constexpr int PV = 0, PK = 2 * PLANE, PQ = 4 * PLANE;
  static_assert(PQ + PLANE + 32 * 128 <= SLOT + QF_BM * 8, "the 32-row reads of the last slot's Q lo plane stay inside the allocation");
};
// tile row R -> its frame R / J: a multiply-shift (a shift at 16), checked against the division for every row of a tile
template <int J>
__host__ __device__ constexpr int qs_frame(int R) { return J == 17 ? (R * 241) >> 12 : (J == 16 ? R >> 4 : (R * 137) >> 11); }
template <int J>
constexpr bool qs_frame_exact() {
  for (int R = 0; R < QF_BM; ++R)
    if (qs_frame<J>(R) != R / J) return false;
  return true;
}
static_assert(qs_frame_exact<15>() && qs_frame_exact<16>() && qs_frame_exact<17>(), "R / J for R < 256");
// m-tiles (bit i: rows 128 wm + 16 i .. + 15) of wave row wm that hold a row of a frame of `pass`: the wave-uniform skip of write_pass
// -- derived from the rule, the per-row test stays the authority (J = 17: m-tiles 0-4 of both wave rows in pass 0, 4-7 and, in wave
// row 1, m-tile 0 in pass 1; J = 16: m-tiles 0-3, then 4-7)
template <int J>
constexpr unsigned qs_mtiles(int wm, int pass) {
  unsigned mk = 0;
  for (int R = 128 * wm; R < 128 * wm + 128; ++R) {
    const int fr = R / J;
    if (fr < QsGeo<J>::FPT && ((fr >> 2) & 1) == pass) mk |= 1u << ((R >> 4) & 7);
  }
  return mk;
}
static_assert(qs_mtiles<17>(0, 0) == 0x1f && qs_mtiles<17>(1, 0) == 0x1f && qs_mtiles<17>(0, 1) == 0xf0 && qs_mtiles<17>(1, 1) == 0xf1, "");
static_assert(qs_mtiles<16>(0, 0) == 0x0f && qs_mtiles<16>(1, 0) == 0x0f && qs_mtiles<16>(0, 1) == 0xf0 && qs_mtiles<16>(1, 1) == 0xf0, "");

// Diagnostic builds only (-DQS_ABL=n, wrong results; experiments/lds_conflict_attribution.sh): 1 no slot writes, 2 no attention units,
// 4 no output patches -- which LDS accesses the bank-conflict counter belongs to.
#ifndef QS_ABL
#define QS_ABL 0
#endif

struct QsArgs {
  const _Float16* Ap;      // residual stream, pair layout [>= 255 mtiles + 1 rows][2 K] of 8 x
  const _Float16* Wp;      // folded qkv weight W diag(gamma), pair layout, 2^k w, rows in TILE order: row 192 h + 48 wn + 16 part + x
                           // = original row 512 part + 64 h + 16 wn + x (wave wn of a tile holds q, k, v columns 16 wn .. + 15 of head h)
  const float* bias;       // b + W beta, head-major
  const float* csum;       // sum_k W[n, k] gamma[k], head-major
  const float* st_in;      // (sum, sum of squares) partials of the rows: [rows][st_np][2]
  int st_np;
  float eps, out_scale;    // LayerNorm eps; 2^-(3 + k)
  _Float16* out;           // attention output, pair layout [M][2 D] of 8 o
  int M, K, F, mtiles, D;  // tokens, GEMM depth, frames (M / J), M-tiles (ceil(F / frames per tile)), model width (8 heads x 64)
  unsigned* range;         // the engine's range-guard word
  _Float16 *ph, *pl;       // plane-writing form only: q / k / v hi / lo planes [M][3 D]
};

// One frame of one head from its LDS slot: the arithmetic of k_attn_temporal_x3p<1, 8, 3> (same MFMAs in the same order, same
// softmax, same conversions), outputs through the wave-private patch (aliasing the slot's Q planes, dead once the query fragments
// are in registers) as whole 128-byte lines.
// J <= 16: every key sits in accumulator registers 0..7 (one 16-key step); registers 8..15 are pad keys in both lane halves, so the base
// kernel's second step of O^T += V^T E carries exact zeros only (its E is exp2(-inf) = 0, its V fragments are masked to zero) and is
// dropped, as are the zero terms of its max and its sum.  J = 15: key 15 is register 7 of lane half 1 and scores -inf.
template <int J>
__device__ __forceinline__ void qs_attention(unsigned char* slot, int lane, _Float16* out_row0, int D) {
  typedef QsGeo<J> Geo;
  constexpr int T = J;
  constexpr int NQ = J > 16 ? 9 : 8;              // accumulator registers that hold a real key in some lane half
  constexpr int NS2 = J > 16 ? 2 : 1;             // 16-key steps of the second product
  constexpr int NIT = (J + 7) / 8;                // 8-row passes of the output patch that carry rows < J
  unsigned char* const sVh = slot + Geo::PV;
  unsigned char* const sVl = slot + Geo::PV + Geo::PLANE;
  unsigned char* const sKh = slot + Geo::PK;
  unsigned char* const sKl = slot + Geo::PK + Geo::PLANE;
  unsigned char* const sQh = slot + Geo::PQ;
  unsigned char* const sQl = slot + Geo::PQ + Geo::PLANE;
  unsigned char* const patch = slot + Geo::PQ;    // 4 KiB over the Q planes (and, at J = 15, the slot's 256 spare bytes behind them)
  const int r = lane & 31, h = lane >> 5;
  h8 qh[4], ql[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {                // rows >= J read the planes behind: their query columns are never stored
    const int qo = kswz(r, 2 * ks + h);
    qh[ks] = *reinterpret_cast<const h8*>(sQh + qo);
    ql[ks] = *reinterpret_cast<const h8*>(sQl + qo);
  }
  f32x16 sacc;
#pragma unroll
  for (int q = 0; q < 16; ++q) sacc[q] = 0.f;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int ko = kswz(r, 2 * ks + h);
    const h8 kh = *reinterpret_cast<const h8*>(sKh + ko);
    const h8 kl = *reinterpret_cast<const h8*>(sKl + ko);
    sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], sacc, 0, 0, 0);
    sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], sacc, 0, 0, 0);
    sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], sacc, 0, 0, 0);
  }
  // keys of accumulator register q in lane half h: (q & 3) + 8 (q >> 2) + 4 h.  With 17 keys, registers 9..15 hold pad keys in both
  // halves and register 8 (key 16 / 20) a real one in half 0 only: their numerators are exact zeros -- no exponentials, no sums
  // (J <= 16: registers 8..15 are pad in both halves; at J = 15 register 7 of half 1 is key 15)
  float m = -INFINITY;
  if (J == 17 && h != 0) sacc[8] = -INFINITY;
  if (J == 15 && h != 0) sacc[7] = -INFINITY;
#pragma unroll
  for (int q = 0; q < NQ; ++q) m = fmaxf(m, sacc[q]);
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  constexpr float C_EXP = 1.4426950408889634f / 64.0f;
  const float mb = m * C_EXP;
  float l = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    float e = 0.0f;
    if (q < NQ) {
      e = __builtin_amdgcn_exp2f(fmaf(sacc[q], C_EXP, -mb));
      l += e;
    }
    sacc[q] = e;
  }
  l += __shfl_xor(l, 32, 64);
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
#pragma unroll
  for (int s2 = 0; s2 < NS2; ++s2) {
    h8 eh, el;
    {
      if (s2 == 0) {
        float e8[8];
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) e8[jj] = sacc[jj];
        split8_e(e8, eh, el);
      } else {   // registers 9..15 are exact zeros: only the first pair carries a numerator
        unsigned a, b;
        split_pair_s(sacc[8], 0.0f, 1024.0f, a, b);
        u32x4 hv = {a, 0u, 0u, 0u}, lv = {b, 0u, 0u, 0u};
        eh = __builtin_bit_cast(h8, hv);
        el = __builtin_bit_cast(h8, lv);
      }
    }
    const int k0 = 16 * s2 + 4 * h;
    const int gi = lane & 15, tq_ = gi >> 2, tp_ = gi & 3;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int d0 = dt * 32 + 16 * ((lane >> 4) & 1);
      const int ch = (d0 >> 3) + (tp_ >> 1), sub = (tp_ & 1) * 8;
      const int o0 = vswz(k0 + tq_, ch) + sub, o1 = vswz(k0 + 8 + tq_, ch) + sub;
      const s4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o0));
      const s4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o1));
      const s4v c0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o0));
      const s4v c1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o1));
      h8 vh, vl;
      {
        const h4 a0h = __builtin_bit_cast(h4, a0), a1h = __builtin_bit_cast(h4, a1);
        const h4 c0h = __builtin_bit_cast(h4, c0), c1h = __builtin_bit_cast(h4, c1);
#pragma unroll
        for (int e = 0; e < 4; ++e) { vh[e] = a0h[e]; vh[4 + e] = a1h[e]; vl[e] = c0h[e]; vl[4 + e] = c1h[e]; }
      }
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, eh, oacc[dt], 0, 0, 0);
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, el, oacc[dt], 0, 0, 0);
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, eh, oacc[dt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
  // O = O^T / (2^13 l) - v_query, packed as hi / lo of 8 o; whole lines out through the patch
  const float inv = 1.0f / (8192.0f * l);
  const int tqc = r < T ? r : 0;
  // (no range tracking here: |o| = |(P - I) V| <= 2.0001 max |v|, and the slot writer raises the guard when a |v| exceeds 4090 --
  // half the plane range --, so an un-flagged run cannot overflow the output planes; 28 VALU instructions per unit less)
  u32x4 pw[2 * NIT];
#pragma unroll
  for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int vo = vswz(tqc, dt * 4 + g4) + 8 * h;
      // -v_query = -(hi + lo) / 8 by two v_fma_mix_f32 on the packed fp16 halves (exact: the pair sums to <= 22 bits), o = O^T inv - v_q
      // in one fma (the rounding every form of this kernel makes), then hi = fp16(8 o), lo = fp16(8 o - hi) by v_fma_mixlo / mixhi:
      // 6 VALU instructions per value where convert / add / scale / fma / clamp / convert / convert back / subtract / convert took 12
      // (same bits whenever |8 o| is inside the fp16 range; beyond it the range guard fires either way)
      const uint2 vqh = *reinterpret_cast<const uint2*>(sVh + vo);
      const uint2 vql = *reinterpret_cast<const uint2*>(sVl + vo);
      float o4[4];
#pragma unroll
      for (int pr = 0; pr < 2; ++pr) {
        const unsigned ph_ = pr ? vqh.y : vqh.x, pl_ = pr ? vql.y : vql.x;
        float n0, n1;
        asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(n0) : "v"(pl_), "v"(-0.125f));
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(n0) : "v"(ph_), "v"(-0.125f), "v"(n0));
        asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(n1) : "v"(pl_), "v"(-0.125f));
        asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(n1) : "v"(ph_), "v"(-0.125f), "v"(n1));
        o4[2 * pr] = __builtin_fmaf(oacc[dt][4 * g4 + 2 * pr], inv, n0);
        o4[2 * pr + 1] = __builtin_fmaf(oacc[dt][4 * g4 + 2 * pr + 1], inv, n1);
      }
      unsigned h0, l0, h1, l1;
      split_pair(o4[0], o4[1], 8.0f, h0, l0);
      split_pair(o4[2], o4[3], 8.0f, h1, l1);
      const h4 oh = __builtin_bit_cast(h4, make_uint2(h0, h1)), ol = __builtin_bit_cast(h4, make_uint2(l0, l1));
      if (!(QS_ABL & 4)) patch_wr(patch, r, h, g4, oh, ol);
      else asm volatile("" ::"v"(oh), "v"(ol));
    }
    asm volatile("" ::: "memory");     // (the rows read back were written by other lanes)
#pragma unroll
    for (int it = 0; it < NIT; ++it) pw[dt * NIT + it] = (QS_ABL & 4) ? u32x4{0u, 0u, 0u, 0u} : patch_rd(patch, 8 * it + (lane >> 3), lane & 7);
    asm volatile("" ::: "memory");
  }
  _Float16* const pw_ptr = out_row0 + (size_t)(lane >> 3) * 2 * D + 8 * (lane & 7);
  const size_t pw_stride = (size_t)8 * 2 * D;
#pragma unroll
  for (int it = 0; it < NIT; ++it)
    if (8 * it + (lane >> 3) < T) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(pw_ptr + it * pw_stride + dt * 64) = pw[dt * NIT + it];
    }
}

// What both forms of the kernel run around their accumulators (k_qkv_sattn: the k-loop; k_qkv_sattn_direct: the block-0 fill) ---------
typedef float qs_f2 __attribute__((ext_vector_type(2)));

// Row statistics -> (rstd * out_scale, -mean rstd) per tile row: every wave reduces 32 rows (lanes 0-31)
template <int J>
__device__ __forceinline__ void qs_row_stats(unsigned char* lds, const QsArgs& a, int m0, int wave, int lane, bool st_dma) {
  float2* const srow = reinterpret_cast<float2*>(lds + QsGeo<J>::STX);
  const int K = a.K;
  if (lane < 32) {
    const int t = wave * 32 + lane, row = m0 + t;
    float sm = 0.f, sq = 0.f;
    if (row < a.M) {
      const float2* raw = st_dma ? reinterpret_cast<const float2*>(lds + QS_RAW) + t * a.st_np
                                 : reinterpret_cast<const float2*>(a.st_in) + (size_t)row * a.st_np;
      for (int p = 0; p < a.st_np; ++p) { sm += raw[p].x; sq += raw[p].y; }
    }
    if (sq >= (X3_HALF_MAX * 0.125f) * (X3_HALF_MAX * 0.125f)) range_raise(a.range, RANGE_BIT_ACT);   // (producer's planes, as x3q_tile)
    const float mean = sm / (float)K;
    const float var = fmaxf(sq / (float)K - mean * mean, 0.0f);
    if (row < a.M && mean * mean > 256.0f * var) range_raise(a.range, RANGE_BIT_STATS);
    const float rstd = 1.0f / sqrtf(var + a.eps);
    srow[t] = make_float2(rstd * a.out_scale, -mean * rstd);
  }
}

// Four accumulator columns of one row -> q / k / v values (LayerNorm fold of x3q_epilogue8) and their hi / lo fp16 pairs of osc v
__device__ __forceinline__ void qs_fold_split(const f32x4& ac, qs_f2 sx, qs_f2 sy, const float4& cs, const float4& bb, float osc, float& amax,
                                              u32x2_alias& hv, u32x2_alias& lv) {
  typedef qs_f2 f2;
  f2 a01, a23, c01, c23, b01, b23;
  a01.x = ac[0]; a01.y = ac[1]; a23.x = ac[2]; a23.y = ac[3];
  c01.x = cs.x; c01.y = cs.y; c23.x = cs.z; c23.y = cs.w;
  b01.x = bb.x; b01.y = bb.y; b23.x = bb.z; b23.y = bb.w;
  const f2 v01 = __builtin_elementwise_fma(sx, a01, __builtin_elementwise_fma(sy, c01, b01));
  const f2 v23 = __builtin_elementwise_fma(sx, a23, __builtin_elementwise_fma(sy, c23, b23));
  amax = fmaxf(fmaxf(amax, fabsf(v01.x)), fabsf(v01.y));
  amax = fmaxf(fmaxf(amax, fabsf(v23.x)), fabsf(v23.y));
  unsigned h0, l0, h1, l1;
  split_pair(v01.x, v01.y, osc, h0, l0);
  split_pair(v23.x, v23.y, osc, h1, l1);
  hv[0] = h0; hv[1] = h1; lv[0] = l0; lv[1] = l1;
}

// Everything behind the accumulators of tile (mt, hd), statistics in LDS and visible.  PLANES = false: the two passes of slot writes and
// attention units.  PLANES = true (block 0 of the two-kernel flow): the same values as [M][3 D] hi / lo planes in HBM, what
// launch_attn_temporal_x3 reads -- column 512 part + 64 hd + 16 wn + x of the original weight order.
template <int J, bool PLANES>
__device__ __forceinline__ void qs_tail(f32x4 (&acc)[QF_TM][QF_NJ], unsigned char* lds, const QsArgs& a, int mt, int hd, int m0, int n0,
                                        int wave, int lane, int wm, int wn, int r16, int q) {
  typedef QsGeo<J> Geo;
  float2 st[QF_TM];
#pragma unroll
  for (int i = 0; i < QF_TM; ++i) st[i] = reinterpret_cast<const float2*>(lds + Geo::STX)[wm * 16 * QF_TM + 16 * i + r16];
  float4 cs4[QF_NJ], b4[QF_NJ];
#pragma unroll
  for (int j = 0; j < QF_NJ; ++j) {
    const int n = n0 + wn * 48 + 16 * j + 4 * q;
    cs4[j] = *reinterpret_cast<const float4*>(a.csum + n);
    b4[j] = *reinterpret_cast<const float4*>(a.bias + n);
  }
  float amaxj[QF_NJ] = {0.0f, 0.0f, 0.0f};   // max |value| per accumulator column tile j = q / k / v (plane scale applied at the end)
  // q / k / v of this pass's frames -> frame slots (LayerNorm fold and hi / lo split of x3q_epilogue8).  Frame fr of the tile:
  // pass (fr >> 2) & 1, slot (fr & 3) + 4 (fr >> 3).  Column tile j of a wave IS part j (the weight rows are ordered that way at
  // commit): q columns 16 wn .. + 15 of the head in j = 0, the same k columns in j = 1, v in j = 2 -- plane and scale are
  // compile-time per j, and one address serves q and k (same row swizzle), one v.  Rows beyond the matrix hold finite values
  // (the engine zeroes the pad rows of the stream; the direct form fills them from zero inputs): nothing non-finite can reach a slot.
  typedef qs_f2 f2;
  const int chunk = 2 * wn + (q >> 1), half8 = (q & 1) << 3;            // this lane's 8 bytes: 16-byte chunk d / 8, half (d & 4)
  constexpr unsigned MT00 = qs_mtiles<J>(0, 0), MT10 = qs_mtiles<J>(1, 0), MT01 = qs_mtiles<J>(0, 1), MT11 = qs_mtiles<J>(1, 1);   // [wm][pass]
  auto write_pass = [&](int pass) {
#pragma unroll
    for (int i = 0; i < QF_TM; ++i) {
      // Wave-uniform: m-tiles without rows of this pass.  Two forms of ONE rule, on purpose: the 17-joint condition is kept as it was written
      // (qs_mtiles<17> is static_assert-ed equal to it above) because the mask form, tried at 17, moves the register allocation of the four
      // fused 17-joint kernels (943 changed lines in the assembly of k_qkv_sattn<17>), and those kernels are to stay the code they were.
      if (J == 17) {
        if (pass == 0 ? (i > 4) : (i < 4 && !(wm == 1 && i == 0))) continue;
      } else if (!(((pass == 0 ? (wm ? MT10 : MT00) : (wm ? MT11 : MT01)) >> i) & 1)) {
        continue;
      }
      const int R = wm * 16 * QF_TM + 16 * i + r16;
      // R / J for R < 256 (qs_frame; written out at 17, where the compiler takes the pass bit straight from the product)
      const int fr = J == 17 ? (R * 241) >> 12 : qs_frame<J>(R), jr = R - fr * J;
      if (((fr >> 2) & 1) != pass || fr >= Geo::FPT) continue;          // (J = 15: the 16 trailing rows are frames 16 and 17)
      unsigned char* const row = lds + QS_QKV + ((fr & 3) + 4 * (fr >> 3)) * Geo::SLOT + jr * 128 + half8;
      unsigned char* const pkq = row + ((chunk ^ ((jr >> 1) & 7)) << 4);
      unsigned char* const pv = row + ((chunk ^ vkey(jr)) << 4);
      const f2 sx = (f2)(st[i].x), sy = (f2)(st[i].y);
#pragma unroll
      for (int j = 0; j < QF_NJ; ++j) {
        const float osc = j == 0 ? 1.0f : 8.0f;
        u32x2_alias hv, lv;
        qs_fold_split(acc[i][j], sx, sy, cs4[j], b4[j], osc, amaxj[j], hv, lv);
        unsigned char* const ph = j == 0 ? pkq + Geo::PQ : (j == 1 ? pkq + Geo::PK : pv + Geo::PV);
        if (!(QS_ABL & 1)) {
          *reinterpret_cast<u32x2_alias*>(ph) = hv;
          *reinterpret_cast<u32x2_alias*>(ph + Geo::PLANE) = lv;
        }
      }
    }
  };
  auto attend = [&](int pass) {
    const int fr = (wave & 3) + 4 * pass + 8 * (wave >> 2);             // frame of the tile this wave takes: slot = wave
    const long long gf = (long long)mt * Geo::FPT + fr;
    if (!(QS_ABL & 2) && fr < Geo::FPT && gf < a.F)
      qs_attention<J>(lds + QS_QKV + wave * Geo::SLOT, lane, a.out + ((size_t)gf * J) * 2 * a.D + hd * 128, a.D);
  };
  auto range_check = [&]() {
    float amax = 0.0f;
#pragma unroll
    for (int j = 0; j < QF_NJ; ++j) amax = fmaxf(amax, amaxj[j] * (j == 0 ? 1.0f : (j == 1 ? 8.0f : 16.015f)));   // v: flagged from |v| > 4090 on
    if (amax > X3_HALF_MAX) range_raise(a.range, RANGE_BIT_ACT);
  };
  if (PLANES) {
#pragma unroll
    for (int i = 0; i < QF_TM; ++i) {
      const int R = wm * 16 * QF_TM + 16 * i + r16, m = m0 + R;
      if (R >= Geo::ROWS || m >= a.M) continue;                          // (rows from Geo::ROWS on are the next tile's)
      const f2 sx = (f2)(st[i].x), sy = (f2)(st[i].y);
      const size_t o = (size_t)m * 3 * a.D + hd * 64 + 16 * wn + 4 * q;
#pragma unroll
      for (int j = 0; j < QF_NJ; ++j) {
        const float osc = j == 0 ? 1.0f : 8.0f;
        u32x2_alias hv, lv;
        qs_fold_split(acc[i][j], sx, sy, cs4[j], b4[j], osc, amaxj[j], hv, lv);
        *reinterpret_cast<u32x2_alias*>(a.ph + o + j * a.D) = hv;
        *reinterpret_cast<u32x2_alias*>(a.pl + o + j * a.D) = lv;
      }
    }
    range_check();
    return;
  }
  write_pass(0);
  __syncthreads();
  attend(0);
  __syncthreads();
  write_pass(1);
  range_check();
  __syncthreads();
  attend(1);
}

template <int J>
__global__ __launch_bounds__(512) void k_qkv_sattn(QsArgs a) {
  constexpr int QS_ROWS = QsGeo<J>::ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int tiles = a.mtiles * 8;
  if (b >= tiles) return;
  const int nitems = (tiles - b + G - 1) / G;
  const int vfull = (a.mtiles / 8) * 64, mrem = a.mtiles % 8;
  // tile ordinal -> (M-tile, head): all heads of an M-tile on one XCD, as the GEMM walks (kernels_gemm_x3p.hip)
  auto tile_of = [&](int o, int& mt, int& hd) {
    if (o < vfull) {
      const int xcd = o & 7, slot = o >> 3;
      mt = (slot >> 3) * 8 + xcd;
      hd = slot & 7;
    } else {
      const int o2 = o - vfull;
      mt = (a.mtiles / 8) * 8 + o2 % mrem;
      hd = o2 / mrem;
    }
  };

  const int K = a.K;
  const size_t K2 = 2 * (size_t)K;
  const int nk = K / 32;
  int mt = 0, hd = 0;
  tile_of(b, mt, hd);
  QF_STAGE_FIRST(a.Ap, a.Wp, mt * QS_ROWS, hd * QF_BN)
  int tid_o = (int)threadIdx.x;
  for (int item = 0; item < nitems; ++item) {
    QF_TILE_LANES;
    QF_TILE_NEXT(mtn, hdn);
    const int m0 = mt * QS_ROWS, n0 = hd * QF_BN;

    // ---- row statistics of the folded LayerNorm: raw partials by LDS-DMA under the k-loop (16-byte aligned blocks), else read later
    const int st_bytes = QF_BM * a.st_np * 8;
    const bool st_dma = st_bytes <= QS_RAW_MAX && (((size_t)m0 * a.st_np * 8) & 15) == 0;   // (uniform)
    int st_issued = 0;
    if (st_dma) {
      const char* src = reinterpret_cast<const char*>(a.st_in + (size_t)m0 * a.st_np * 2);
#pragma unroll
      for (int it = 0; it < QS_RAW_MAX / 1024 / 8; ++it) {
        const int pc = wave + it * 8;
        if (pc * 1024 < st_bytes) {
          KL_GLDS(sgpr_ptr(src + pc * 1024) + lane * 16, QS_RAW + pc * 1024);
          ++st_issued;
        }
      }
    }

    // ---- DMA plan (kloop_common.h KL_DMA_PLAN; a tile stages 256 rows from row QS_ROWS mt on), accumulators, fragment offsets
    QF_TILE_PLAN(a.Ap, a.Wp, m0, n0, mtn * QS_ROWS, hdn * QF_BN);
    QF_TILE_ACC;
    int issued_prev = st_issued;
    QF_KLOOP_HEAD(QF_PIECE)
    // ---- row statistics -> (rstd * out_scale, -mean rstd) per tile row, in front of the last k-tile: every wave reduces 32 rows (lanes
    // 0-31) in the shadow of its SIMD partner's MFMAs -- behind the k-loop this step was 1.1 us of a 38 us tile with half the waves
    // idle.  The raw partials landed long ago (the first counted wait of the tile retired them; phase barriers since).
    qs_row_stats<J>(lds, a, m0, wave, lane, st_dma);
    QF_KLOOP_TAIL(QF_PIECE)
    __builtin_amdgcn_s_setprio(0);

    __syncthreads();   // statistics visible; every wave is out of the k-loop: stage 1 and the LDS behind it become the frame slots

    qs_tail<J, false>(acc, lds, a, mt, hd, m0, n0, wave, lane, wm, wn, r16, q);
    mt = mtn; hd = hdn;
    __syncthreads();   // the slots are read before the next tile's statistics block and second k-tile are staged over them
  }
}

// ---- block 0, direct form ------------------------------------------------------------------------------------------------------------
// The residual stream that enters block 0 is x0[m, :] = W_e u_m + b_e + spos[j(m)] + tv[b(m)] with u_m the CIN <= 8 raw input channels of
// token m (k_embed_planes), so the inner product of the fold identity collapses to
//   Wg[n, :] x0[m, :] = G[n, :] u_m + P[j(m), n] + Q[b(m), n],   G = Wg W_e,  P[j] = Wg (b_e + spos[j]),  Q[b] = Wg tv[b]
// (G, P: fp64 at commit, stored fp32; Q: one small linear per forward).  Same tile, same eight waves, same accumulator ownership as
// k_qkv_sattn, but no operand staging and no k-loop: every lane fills its 8 x 3 x 4 accumulators in true units (out_scale = 1) by
//   acc = 0;  acc = fmaf(u[c], G[n][c], acc) for c = 0 .. CIN - 1;  acc += P[j][n];  acc += Q[b][n]
// in exactly that order, and qs_tail does the rest.  G and P are stored in the HEAD-MAJOR tile order of the folded weight / csum / bias
// (row 192 hd + 48 wn + 16 part + x), so a tile's slices are contiguous; Q comes from the small linear in the ORIGINAL column order
// (512 part + 64 hd + 16 wn + x: the four columns of an accumulator are adjacent there too).
struct QdSrc {
  const float *x2d, *y;    // the inputs of k_embed_planes: [M][CIN2], [M or B J][3]
  const float *G, *P, *Q;  // head-major [3 D][CIN] and [J][3 D]; original order [1 or B][3 D] (Q: nullptr without time embedding)
  int q_stride;            // floats between the Q rows of consecutive batch elements: 0 (all share one) or 3 D
  int TJ, y_bcast_T;       // rows per batch element; y holds one frame per batch element (seq2frame)
};
// LDS, in the stage area the k-loop form fills with operands: the head's 192 columns of G, P and of the Q rows of the tile's batch elements
constexpr int QD_GROW = 8;                                               // G: 192 rows of 8 floats (CIN used)
// A tile's REAL rows (QsGeo::ROWS = 16 J at most) span at most 16 frames, so at most 16 batch elements: one Q slot each.  (At J = 15 the
// 16 trailing rows may belong to a seventeenth batch element: it has no slot, qd_fill clamps their lookup and nothing reads the result.)
constexpr int QD_QSLOTS = 16;
constexpr int QD_G = 0, QD_P = QD_G + QF_BN * QD_GROW * 4;               // P: J x 192 floats, then the Q slots
template <int J>
struct QdGeo {
  static constexpr int Q = QD_P + J * QF_BN * 4;
  static_assert(Q + QD_QSLOTS * QF_BN * 4 <= QS_QKV, "the direct form's tables fit the unused stage area");
  static_assert(QsGeo<J>::ROWS <= QD_QSLOTS * J, "a tile's real rows span at most QD_QSLOTS frames, so at most QD_QSLOTS batch elements");
};

// tile column c = 48 wn + 16 part + x of head hd in the original column order of the qkv weight
__device__ __forceinline__ int qd_col(int c, int hd) { return 512 * ((c % 48) >> 4) + 64 * hd + 16 * (c / 48) + (c & 15); }

template <int J, int CIN2>
__device__ __forceinline__ void qd_stage(unsigned char* lds, const QdSrc& d, int M, int m0, int hd, int tid) {
  constexpr int CIN = CIN2 + 3;
  float* const sG = reinterpret_cast<float*>(lds + QD_G);
  float* const sP = reinterpret_cast<float*>(lds + QD_P);
  float* const sQ = reinterpret_cast<float*>(lds + QdGeo<J>::Q);
  for (int idx = tid; idx < QF_BN * CIN; idx += 512) {                  // (the head's rows of G are one contiguous block)
    const int c = idx / CIN, k = idx - c * CIN;
    sG[c * QD_GROW + k] = d.G[QF_BN * CIN * hd + idx];
  }
  for (int idx = tid; idx < J * QF_BN; idx += 512) {
    const int j = idx / QF_BN, c = idx - j * QF_BN;
    sP[idx] = d.P[j * 1536 + QF_BN * hd + c];
  }
  if (d.Q) {   // slot s: batch element m0 / TJ + s (one slot when all share a row)
    const int b_lo = m0 / d.TJ, nb = d.q_stride ? min(QD_QSLOTS, M / d.TJ - b_lo) : 1;
    for (int idx = tid; idx < nb * QF_BN; idx += 512) {
      const int sl = idx / QF_BN, c = idx - sl * QF_BN;
      sQ[idx] = d.Q[(size_t)(b_lo + sl) * d.q_stride + qd_col(c, hd)];
    }
  }
}

// The accumulators of tile row m0 .. and head hd, tables staged and visible.  The scheduling fences keep one column's G row / one row's P
// and Q values in flight at a time: hoisted together they would not fit the registers beside 96 accumulators and the 8 x CIN inputs.
template <int J, int CIN2>
__device__ __forceinline__ void qd_fill(f32x4 (&acc)[QF_TM][QF_NJ], const unsigned char* lds, const QdSrc& d, int M, int m0, int wm, int wn,
                                        int r16, int q) {
  constexpr int CIN = CIN2 + 3;
  const int c0 = wn * 48 + 4 * q;                                        // first of this lane's four tile columns of part 0
  const int b_lo = m0 / d.TJ;
  const float* const sG = reinterpret_cast<const float*>(lds + QD_G);
  const float* const sP = reinterpret_cast<const float*>(lds + QD_P);
  const float* const sQ = reinterpret_cast<const float*>(lds + QdGeo<J>::Q);
  float u[QF_TM][CIN];
#pragma unroll
  for (int ii = 0; ii < QF_TM; ++ii) {
    const int R = wm * 16 * QF_TM + 16 * ii + r16, m = m0 + R;
    const int fr = qs_frame<J>(R), jr = R - fr * J;                    // R / J for R < 256; jr = m % J: a tile starts on a frame
#pragma unroll
    for (int k = 0; k < CIN; ++k) u[ii][k] = 0.0f;                     // rows beyond the matrix: zero inputs
    if (m < M) {
#pragma unroll
      for (int k = 0; k < CIN2; ++k) u[ii][k] = d.x2d[(size_t)m * CIN2 + k];
      const size_t my = d.y_bcast_T ? ((size_t)(m / d.TJ) * J + jr) : (size_t)m;
#pragma unroll
      for (int k = 0; k < 3; ++k) u[ii][CIN2 + k] = d.y[my * 3 + k];
    }
  }
#pragma unroll
  for (int j = 0; j < QF_NJ; ++j) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float g[CIN];
#pragma unroll
      for (int k = 0; k < CIN; ++k) g[k] = sG[(c0 + 16 * j + e) * QD_GROW + k];
#pragma unroll
      for (int ii = 0; ii < QF_TM; ++ii) {
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < CIN; ++k) v = fmaf(u[ii][k], g[k], v);
        acc[ii][j][e] = v;
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  }
#pragma unroll
  for (int i = 0; i < QF_TM; ++i) {   // (the row's offsets are formed again here: kept from the loop above they cost 16 registers)
    const int R = wm * 16 * QF_TM + 16 * i + r16, m = m0 + R;
    const int po = (R - qs_frame<J>(R) * J) * QF_BN + c0;
    const int qo = c0 + (d.q_stride ? min(m / d.TJ - b_lo, QD_QSLOTS - 1) * QF_BN : 0);
    if (m < M) {   // rows beyond the matrix keep 0, what the k-loop form makes of the zeroed pad rows of the stream
#pragma unroll
      for (int j = 0; j < QF_NJ; ++j) {
        const float4 p4 = *reinterpret_cast<const float4*>(sP + po + 16 * j);
        acc[i][j][0] += p4.x; acc[i][j][1] += p4.y; acc[i][j][2] += p4.z; acc[i][j][3] += p4.w;
      }
      if (d.Q) {
#pragma unroll
        for (int j = 0; j < QF_NJ; ++j) {
          const float4 q4 = *reinterpret_cast<const float4*>(sQ + qo + 16 * j);
          acc[i][j][0] += q4.x; acc[i][j][1] += q4.y; acc[i][j][2] += q4.z; acc[i][j][3] += q4.w;
        }
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

template <int J, int CIN2, bool PLANES>
__global__ __launch_bounds__(512) void k_qkv_sattn_direct(QsArgs a, QdSrc d) {
  constexpr int QS_ROWS = QsGeo<J>::ROWS;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int tiles = a.mtiles * 8;
  if (b >= tiles) return;
  const int nitems = (tiles - b + G - 1) / G;
  KL_XCD_TILE_ORDER(a.mtiles, 8);                                        // the walk of k_qkv_sattn
  int tid_o = (int)threadIdx.x;
  for (int item = 0; item < nitems; ++item) {
    QF_TILE_LANES;                                                       // (per-lane offsets re-derived per tile, not hoisted and spilled)
    int mt = 0, hd = 0;
    tile_of(item * G + b, mt, hd);
    const int m0 = mt * QS_ROWS, n0 = hd * QF_BN;
    // the head's columns of G, P and Q into the (otherwise unused) stage area, the row statistics from HBM
    qd_stage<J, CIN2>(lds, d, a.M, m0, hd, tid);
    qs_row_stats<J>(lds, a, m0, wave, lane, false);
    __syncthreads();
    f32x4 acc[QF_TM][QF_NJ];
    qd_fill<J, CIN2>(acc, lds, d, a.M, m0, wm, wn, r16, q);
    __builtin_amdgcn_sched_barrier(0);
    qs_tail<J, PLANES>(acc, lds, a, mt, hd, m0, n0, wave, lane, wm, wn, r16, q);
    __syncthreads();   // the slots, the tables and the statistics are read before the next tile's are staged over them
  }
}

// whole frames per tile of joint count J (qkv_sattn_ok holds)
int qs_frames_per_tile(int J) { return J == 17 ? QsGeo<17>::FPT : QsGeo<16>::FPT; }

}  // namespace

bool qkv_sattn_ok(int J, int D, int H, int K) { return J >= 15 && J <= 17 && H == 8 && D == 512 && K % 64 == 0 && K >= 128; }

// Tokens M = frames * J; A / st_in must span the rows the last tile stages -- 255 ceil(frames / 15) + 1 at J = 17, 240 ceil(frames / 16)
// + 16 at J = 15, 256 ceil(frames / 16) at J = 16 (the engine's workspace does).
hipError_t launch_qkv_sattn(const void* Apair, const void* Wpair_headmajor, const float* bias_hm, const float* csum_hm, const float* st_in,
                            int st_np, float eps, int w_exp, void* out_x3, int M, int K, int J, int D, int H, hipStream_t s) {
  if (!qkv_sattn_ok(J, D, H, K) || M <= 0 || M % J != 0 || st_np < 1 || !Apair || !Wpair_headmajor || !bias_hm || !csum_hm || !st_in || !out_x3)
    return hipErrorInvalidValue;
  if (w_exp < -14 || w_exp > 12) return hipErrorInvalidValue;
  QsArgs a{};
  a.Ap = (const _Float16*)Apair; a.Wp = (const _Float16*)Wpair_headmajor; a.bias = bias_hm; a.csum = csum_hm; a.st_in = st_in;
  a.st_np = st_np; a.eps = eps; a.out_scale = ldexpf(1.0f, -(3 + w_exp));
  const int fpt = qs_frames_per_tile(J);
  a.out = (_Float16*)out_x3; a.M = M; a.K = K; a.F = M / J; a.mtiles = (a.F + fpt - 1) / fpt; a.D = D;
  a.range = launch_range_word();
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * 8, grid)) return ge;
  switch (J) {
    case 15: return launch_lds<k_qkv_sattn<15>>(dim3(grid), dim3(512), QsGeo<15>::LDS, s, a);
    case 16: return launch_lds<k_qkv_sattn<16>>(dim3(grid), dim3(512), QsGeo<16>::LDS, s, a);
    case 17: return launch_lds<k_qkv_sattn<17>>(dim3(grid), dim3(512), QsGeo<17>::LDS, s, a);
  }
  return hipErrorInvalidValue;
}

// in_chans 4 and 5 (8 x 7 / 8 x 8 input registers beside the 96 accumulators) do not fit the 256 VGPRs of two waves per SIMD without
// spilling: such models keep the GEMM in block 0 ("block0_direct_last" reads 0)
bool qkv_sattn_direct_ok(int J, int D, int H, int in_chans) { return qkv_sattn_ok(J, D, H, D) && in_chans >= 1 && in_chans <= 3; }

// Block 0 of the F16X3 flow from the raw input channels (k_qkv_sattn_direct).  out_x3 != nullptr: the fused form, attention output in the
// pair layout; else planes_hi / planes_lo: the q / k / v planes of the two-kernel flow, the same bits the fused form puts into LDS.
hipError_t launch_qkv_sattn_direct(const float* x2d, const float* y, int y_bcast_T, int in_chans, const float* G, const float* P, const float* Q,
                                   int q_stride, const float* bias_hm, const float* csum_hm, const float* st_in, int st_np, float eps, void* out_x3,
                                   void* planes_hi, void* planes_lo, int M, int T, int J, int D, int H, hipStream_t s) {
  if (!qkv_sattn_direct_ok(J, D, H, in_chans) || M <= 0 || T <= 0 || M % (T * J) != 0 || st_np < 1 || !x2d || !y || !G || !P || !bias_hm || !csum_hm ||
      !st_in || (q_stride != 0 && q_stride != 3 * D) || (!out_x3 && (!planes_hi || !planes_lo)))
    return hipErrorInvalidValue;
  QsArgs a{};
  a.bias = bias_hm; a.csum = csum_hm; a.st_in = st_in; a.st_np = st_np; a.eps = eps; a.out_scale = 1.0f;
  const int fpt = qs_frames_per_tile(J);
  a.out = (_Float16*)out_x3; a.M = M; a.K = D; a.F = M / J; a.mtiles = (a.F + fpt - 1) / fpt; a.D = D;
  a.ph = (_Float16*)planes_hi; a.pl = (_Float16*)planes_lo;
  a.range = launch_range_word();
  QdSrc d{};
  d.x2d = x2d; d.y = y; d.G = G; d.P = P; d.Q = Q; d.q_stride = q_stride; d.TJ = T * J; d.y_bcast_T = y_bcast_T;
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * 8, grid)) return ge;
#define D3D_QD(JJ, C2)                                                                                                  \
  case 4 * JJ + C2:                                                                                                     \
    return out_x3 ? launch_lds<k_qkv_sattn_direct<JJ, C2, false>>(dim3(grid), dim3(512), QsGeo<JJ>::LDS, s, a, d)       \
                  : launch_lds<k_qkv_sattn_direct<JJ, C2, true>>(dim3(grid), dim3(512), QsGeo<JJ>::LDS, s, a, d);
  switch (4 * J + in_chans) {
    D3D_QD(15, 1) D3D_QD(15, 2) D3D_QD(15, 3)
    D3D_QD(16, 1) D3D_QD(16, 2) D3D_QD(16, 3)
    D3D_QD(17, 1) D3D_QD(17, 2) D3D_QD(17, 3)
  }
#undef D3D_QD
  return hipErrorInvalidValue;
}

}  // namespace d3d
