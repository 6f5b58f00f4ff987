// Temporal F16X3 GRAND attention for heads of 32 columns and windows of ANY length: k_attn_x3_h32's arithmetic
// (kernels_attn_x3_h32.hip) inside k_attn_temporal_x3l's key-streaming walk (kernels_attn_x3_long.hip).
//
// Two adjacent heads are one 64-column pair whose K / V rows are the 128-byte LDS rows of the 64-wide kernels; the pair's rows stream
// through the four swizzled planes in chunks of 32 KC frames.  Sub-head p owns d-steps 2 p, 2 p + 1 of the score product and the
// 32-column half dt = p of the PV product and of the output, and has its own maximum, numerators and sum.
//
//   pass 1   per chunk: stage K; per key tile S^T of sub-head 0 and of sub-head 1 (6 + 6 MFMAs), one running maximum each
//   pass 2   per chunk: stage K and V; per key tile the SAME MFMAs again (same bits), e = exp2(fma(s, C32, -m_p C32)), l_p += e in
//            register order, O^T_p += V^T E^T for the two 16-key steps of the sub-head's own d half
//   O_p = O^T_p / (2^13 l_p) - v_query, range guard, one 128-byte pair-layout line per sub-head: k_attn_x3_h32's epilogue
//
// The two sub-heads are independent, so interleaving them per key tile leaves each one's MFMA and addition order as it is in
// k_attn_x3_h32, where a wave runs one sub-head after the other: for T <= 256 the output is bit-identical to launch_attn_x3_h32
// whatever KC is (tests/test_gpu_long_h32.py).  The price is the scores computed twice, 18 instead of 12 MFMAs per 32 x 32 tile and
// sub-head; two score tiles (32 registers) are live at a time.
//
// Launch geometry, staging and the rules are the long kernel's: one workgroup per (batch, joint, head pair, query block), ceil(T / 256)
// balanced query blocks of at most 8 waves, blockDim a run-time value; staging through registers, all global loads of a batch issued
// before its LDS writes; no LDS-DMA, no persistent walk.  Every wave executes every barrier (the trip counts depend on T alone), keys
// >= T score -inf, K / V rows >= T are staged as zeros in every chunk, rows >= T are never stored, surplus workgroups redo the last unit
// and store nothing, and the transposing V reads sit outside divergent branches.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic and the register staging

constexpr int LH32_DH = 32;        // head width
constexpr int LH32_PW = 64;        // columns of a head pair = of an LDS row

template <int KC>
__global__ __launch_bounds__(512) void k_attn_x3l_h32(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                      _Float16* __restrict__ out_x3, int T, int J, int HP, int D, int units, int nqb,
                                                      unsigned* rw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_lh[];
  constexpr int CH = 32 * KC;                         // keys per chunk
  unsigned char* const sKh = lds_lh;                  // [CH][128 B]
  unsigned char* const sKl = lds_lh + CH * 128;
  unsigned char* const sVh = lds_lh + 2 * CH * 128;
  unsigned char* const sVl = lds_lh + 3 * CH * 128;
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit_raw = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus workgroups redo the last unit and store nothing
  const int hp = unit % HP;                           // (b*J + j)*HP + hp, HP = H / 2 head pairs
  const int bj = unit / HP;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // ---- this lane's query row, both heads of the pair (rows >= T: zeros): fragments 2 p, 2 p + 1 are sub-head p's
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  h8 qh[4], ql[4];
  x3_q_global(Ph, Pl, (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hp * LH32_PW + 8 * h, tq < T, qh, ql);

  // ---- pass 1: the exact maximum over all keys of this query column, per sub-head.  Only the unit's last key tile can hold keys >= T.
  float m0 = -INFINITY, m1 = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    x3_stage_rows<false>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hp, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int gt = c * KC + kt;
      f32x16 s0 = x3_score_tile<0, 2>(sKh, sKl, kt * 32, r, h, qh, ql);
      f32x16 s1 = x3_score_tile<2, 2>(sKh, sKl, kt * 32, r, h, qh, ql);
      if (gt == ntiles - 1) {
        x3_mask_keys(s0, gt * 32, h, T);
        x3_mask_keys(s1, gt * 32, h, T);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) { m0 = fmaxf(m0, s0[q]); m1 = fmaxf(m1, s1[q]); }
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m0 = fmaxf(m0, __shfl_xor(m0, 32, 64));
  m1 = fmaxf(m1, __shfl_xor(m1, 32, 64));
  const float mb0 = m0 * x3_c_exp<LH32_DH>(), mb1 = m1 * x3_c_exp<LH32_DH>();

  // ---- pass 2: numerators, their sums, O^T_p[d][query] = sum_key V^T[d][key] * E^T_p[key][query] (oacc[p]: sub-head p's d half)
  float l0 = 0.f, l1 = 0.f;
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    x3_stage_rows<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hp, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int gt = c * KC + kt;
      f32x16 s0 = x3_score_tile<0, 2>(sKh, sKl, kt * 32, r, h, qh, ql);
      f32x16 s1 = x3_score_tile<2, 2>(sKh, sKl, kt * 32, r, h, qh, ql);
      if (gt == ntiles - 1) {
        x3_mask_keys(s0, gt * 32, h, T);
        x3_mask_keys(s1, gt * 32, h, T);
      }
      x3_exp_tile<LH32_DH>(s0, mb0, l0);
      x3_exp_tile<LH32_DH>(s1, mb1, l1);
      x3_pv_tile<false, 0, 1>(s0, sVh, sVl, 0, kt, T, lane, h, oacc);
      x3_pv_tile<false, 1, 1>(s1, sVh, sVl, 0, kt, T, lane, h, oacc);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l0 += __shfl_xor(l0, 32, 64);
  l1 += __shfl_xor(l1, 32, 64);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM: one 128-byte line per sub-head
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const size_t tokq = tok0 + (size_t)tq * J;
    const size_t vo = tokq * D3 + 2 * D + hp * LH32_PW;
    const size_t oo = tokq * 2 * D + hp * 2 * LH32_PW;   // pair layout: a head's 32 columns are one 128-byte line
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const float inv = 1.0f / (8192.0f * (p ? l1 : l0));
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = p * 32 + 8 * g4 + 4 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[p], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// the query blocks of a unit, as in kernels_attn_x3_long.hip: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int lh32_query_blocks(int T) { return (T + 255) / 256; }
static int lh32_block_waves(int T) {
  const int nqb = lh32_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_x3_h32_long_ok(int T, int D, int H) {
  // (the workgroup count B J (H / 2) ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H >= 2 && H % 2 == 0 && D == LH32_DH * H;
}

hipError_t launch_attn_x3_h32_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                   hipStream_t s) {
  if (!attn_x3_h32_long_ok(T, D, H) || !qkv_hi || !qkv_lo || !out_x3 || B <= 0 || J <= 0) return hipErrorInvalidValue;
  constexpr int KC = 8;
  const int nqb = lh32_query_blocks(T), waves = lh32_block_waves(T);
  const long long units = (long long)B * J * (H / 2);
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)4 * 32 * KC * 128;   // K_hi, K_lo, V_hi, V_lo planes of one chunk
  return launch_lds<k_attn_x3l_h32<KC>>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, (const _Float16*)qkv_hi,
                                        (const _Float16*)qkv_lo, (_Float16*)out_x3, T, J, H / 2, D, (int)units, nqb, launch_range_word());
}

}  // namespace d3d
