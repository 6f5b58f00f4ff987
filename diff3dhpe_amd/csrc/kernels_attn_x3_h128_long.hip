// Temporal F16X3 GRAND attention for heads of 128 columns and windows of ANY length: k_attn_x3_h128's arithmetic
// (kernels_attn_x3_h128.hip) inside k_attn_temporal_x3l's key-streaming walk (kernels_attn_x3_long.hip).
//
// A head is two adjacent 64-column halves of the plane rows; every plane is two sub-planes of CH 128-byte rows, half 0 then half 1, and
// the head's rows stream through them in chunks of CH = 32 KC = 128 frames (4 planes x 128 rows x 256 B = 128 KiB).
//
//   pass 1   per chunk: stage K; per key tile S^T over the eight d-steps (24 MFMAs, one chain), the running maximum
//   pass 2   per chunk: stage K and V; per key tile the SAME MFMAs again (same bits), e = exp2(fma(s, C128, -m C128)), l += e in
//            register order, O^T += V^T E^T for the two 16-key steps of each of the four 32-column quarters
//   O = O^T / (2^13 l) - v_query, range guard, one 128-byte pair-layout line per quarter: k_attn_x3_h128's epilogue
//
// Every accumulator (the score chain of a tile, l, each quarter's O^T) sees its terms in the order k_attn_x3_h128 gives them, so for
// T <= 128 the output is bit-identical to launch_attn_x3_h128 (tests/test_gpu_long_h128.py).  The price is the scores computed twice,
// 48 + 24 instead of 24 + 24 MFMAs per 32 x 32 tile; one score tile is live at a time.
//
// Launch geometry, staging and the rules are the long kernel's: one workgroup per (batch, joint, head, query block), ceil(T / 256)
// balanced query blocks of at most 8 waves, blockDim a run-time value; staging through registers, all global loads of a batch issued
// before its LDS writes; no LDS-DMA, no persistent walk.  Every wave executes every barrier (the trip counts depend on T alone), keys
// >= T score -inf, K / V rows >= T are staged as zeros in every chunk, rows >= T are never stored, surplus workgroups redo the last unit
// and store nothing, and the transposing V reads sit outside divergent branches.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic and the register staging

constexpr int LH128_DH = 128;      // head width
constexpr int LH128_HW = 64;       // columns of a head half = of an LDS row

template <int KC>
__global__ __launch_bounds__(512) void k_attn_x3l_h128(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                       _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units, int nqb,
                                                       unsigned* rw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_lh[];
  constexpr int CH = 32 * KC;                         // keys per chunk
  constexpr int PL = CH * 128;                        // bytes of one sub-plane (one half of one plane)
  unsigned char* const sKh = lds_lh;                  // [2 halves][CH][128 B]
  unsigned char* const sKl = lds_lh + 2 * PL;
  unsigned char* const sVh = lds_lh + 4 * PL;
  unsigned char* const sVl = lds_lh + 6 * PL;
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit_raw = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus workgroups redo the last unit and store nothing
  const int hd = unit % H;                            // (b*J + j)*H + hd
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // ---- this lane's query row, both halves (rows >= T: zeros)
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  const size_t tokq = tok0 + (size_t)(tq < T ? tq : 0) * J;
  h8 qh0[4], ql0[4], qh1[4], ql1[4];
  x3_q_global(Ph, Pl, tokq * D3 + hd * LH128_DH + 8 * h, tq < T, qh0, ql0);
  x3_q_global(Ph, Pl, tokq * D3 + hd * LH128_DH + LH128_HW + 8 * h, tq < T, qh1, ql1);

  auto score = [&](int kt) {
    f32x16 s;
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = 0.f;
    x3_score_acc(s, sKh, sKl, kt * 32, r, h, qh0, ql0);
    x3_score_acc(s, sKh + PL, sKl + PL, kt * 32, r, h, qh1, ql1);
    return s;
  };

  // ---- pass 1: the exact maximum over all keys of this query column.  Only the unit's last key tile can hold keys >= T.
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
#pragma unroll
    for (int f = 0; f < 2; ++f)
      x3_stage_rows<false>(Ph, Pl, sKh + f * PL, sKl + f * PL, sVh + f * PL, sVl + f * PL, tok0, J, D, 2 * hd + f, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int gt = c * KC + kt;
      f32x16 s = score(kt);
      if (gt == ntiles - 1) x3_mask_keys(s, gt * 32, h, T);
#pragma unroll
      for (int q = 0; q < 16; ++q) m = fmaxf(m, s[q]);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float mb = m * x3_c_exp<LH128_DH>();

  // ---- pass 2: numerators, their sum, O^T[d][query] = sum_key V^T[d][key] * E^T[key][query] (oa0 / oa1: the quarters of half 0 / 1)
  float l = 0.f;
  f32x16 oa0[2], oa1[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oa0[0][q] = 0.f; oa0[1][q] = 0.f; oa1[0][q] = 0.f; oa1[1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
#pragma unroll
    for (int f = 0; f < 2; ++f)
      x3_stage_rows<true>(Ph, Pl, sKh + f * PL, sKl + f * PL, sVh + f * PL, sVl + f * PL, tok0, J, D, 2 * hd + f, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int gt = c * KC + kt;
      f32x16 s = score(kt);
      if (gt == ntiles - 1) x3_mask_keys(s, gt * 32, h, T);
      x3_exp_tile<LH128_DH>(s, mb, l);
      x3_pv_tile<false>(s, sVh, sVl, 0, kt, T, lane, h, oa0);
      x3_pv_tile<false>(s, sVh + PL, sVl + PL, 0, kt, T, lane, h, oa1);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l += __shfl_xor(l, 32, 64);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM: one 128-byte line per quarter
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const size_t vo = tokq * D3 + 2 * D + (2 * hd + f) * LH128_HW;
      const size_t oo = tokq * 2 * D + (2 * hd + f) * 2 * LH128_HW;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int d = dt * 32 + 8 * g4 + 4 * h;
          h4 oh, ol;
          x3_out_chunk(f ? oa1[dt] : oa0[dt], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d),
                       amax, oh, ol);
          *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
          *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
        }
      }
    }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// the query blocks of a unit, as in kernels_attn_x3_long.hip: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int lh128_query_blocks(int T) { return (T + 255) / 256; }
static int lh128_block_waves(int T) {
  const int nqb = lh128_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_x3_h128_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H >= 1 && D == LH128_DH * H;
}

hipError_t launch_attn_x3_h128_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                    hipStream_t s) {
  if (!attn_x3_h128_long_ok(T, D, H) || !qkv_hi || !qkv_lo || !out_x3 || B <= 0 || J <= 0) return hipErrorInvalidValue;
  constexpr int KC = 4;
  const int nqb = lh128_query_blocks(T), waves = lh128_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)8 * 32 * KC * 128;   // K_hi, K_lo, V_hi, V_lo planes of one chunk, two halves each
  return launch_lds<k_attn_x3l_h128<KC>>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, (const _Float16*)qkv_hi,
                                         (const _Float16*)qkv_lo, (_Float16*)out_x3, T, J, H, D, (int)units, nqb, launch_range_word());
}

}  // namespace d3d
