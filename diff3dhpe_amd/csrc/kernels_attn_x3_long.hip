// Temporal GRAND attention on the fp16 matrix pipe for windows of ANY length: the keys stream through LDS in chunks of 32 KC
// frames instead of all living there (kernels_attn_x3.hip: four planes of T <= 256 rows = 128 of the 160 KiB).
//
// The arithmetic is attn_x3_tile.h's, the pieces k_attn_temporal_x3<NKT, 1> (kernels_attn_x3.hip, the form every other F16X3 attention
// kernel is pinned to) is built from: the exact two-pass softmax, not an online rescaling.
//
//   pass 1   per chunk: stage K, S^T = K Q^T tile by tile, running maximum m of this lane's query column
//   pass 2   per chunk: stage K and V; per key tile the SAME twelve MFMAs again (same bits), e = exp2(fma(s, C, -m C)), l += e in
//            register order, O^T += V^T E^T for the two 16-key steps and the two d halves in the base kernel's order
//   O = O^T / (2^13 l) - v_query, range guard, hi / lo planes out: the base kernel's epilogue
//
// So every exp2 sees the same m, l is summed in the same order and oacc takes the same MFMAs in the same order as in the base
// kernel: for T <= 256 the output is bit-identical to launch_attn_temporal_x3 (tests/test_gpu_long_temporal.py).  The price is the
// scores computed twice, 36 instead of 24 MFMAs per 32 x 32 tile; one score tile (16 registers) is live at a time.
//
// One workgroup per (batch, joint, head, query block): the T queries of a unit are cut into ceil(T / 256) balanced blocks of at most
// 8 waves of 32 queries (T = 300: two blocks of 160), blockDim = 64 x that wave count -- a run-time value, the staging loops stride by
// it.  Staging is the base kernel's: through registers into the four swizzled planes, all global loads of a batch issued before its
// LDS writes; no LDS-DMA, no counters, no persistent walk.  Every wave executes every barrier: the chunk and key-tile trip counts
// depend on T alone, a wave whose queries are all >= T stages and synchronises and only skips its stores.
// Row isolation: keys >= T score -inf (their e is an exact 0) and their K / V rows are staged as zeros, never left over from the
// previous chunk: 0 x NaN cannot enter a clean row.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic and the register staging

constexpr int LDH = 64;   // head width

template <int KC>
__global__ __launch_bounds__(512) void k_attn_temporal_x3l(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                           _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units,
                                                           int nqb, unsigned* rw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_l[];
  constexpr int CH = 32 * KC;                         // keys per chunk
  unsigned char* const sKh = lds_l;                   // [CH][128 B]
  unsigned char* const sKl = lds_l + CH * 128;
  unsigned char* const sVh = lds_l + 2 * CH * 128;
  unsigned char* const sVl = lds_l + 3 * CH * 128;
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit_raw = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus workgroups redo the last unit and store nothing
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // ---- this lane's query row (rows >= T: zeros)
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  h8 qh[4], ql[4];
  x3_q_global(Ph, Pl, (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * LDH + 8 * h, tq < T, qh, ql);

  // S^T tile kt of the staged chunk, keys >= T at -inf.  Only the unit's last key tile (gt == ntiles - 1) can hold such keys.
  auto score_tile = [&](int kt, int gt) -> f32x16 {
    f32x16 sacc = x3_score_tile(sKh, sKl, kt * 32, r, h, qh, ql);
    if (gt == ntiles - 1) x3_mask_keys(sacc, gt * 32, h, T);
    return sacc;
  };

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    x3_stage_rows<false>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) m = fmaxf(m, sacc[q]);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float mb = m * X3_C_EXP;

  // ---- pass 2: numerators, their sum, O^T[d][query] = sum_key V^T[d][key] * E^T[key][query]
  float l = 0.f;
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    x3_stage_rows<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(kt, c * KC + kt);
      x3_exp_tile(sacc, mb, l);
      x3_pv_tile<false>(sacc, sVh, sVl, 0, kt, T, lane, h, oacc);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l += __shfl_xor(l, 32, 64);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
    const size_t tokq = tok0 + (size_t)tq * J;
    const size_t vo = tokq * D3 + 2 * D + hd * LDH;
    const size_t oo = tokq * 2 * D + hd * 2 * LDH;   // pair layout: a head's 64 columns are two 128-byte lines
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[dt], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// the query blocks of a unit: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int long_query_blocks(int T) { return (T + 255) / 256; }
static int long_block_waves(int T) {
  const int nqb = long_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_temporal_x3_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && D == H * LDH;
}

hipError_t launch_attn_temporal_x3_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                        hipStream_t s) {
  if (!attn_temporal_x3_long_ok(T, D, H) || !qkv_hi || !qkv_lo || !out_x3 || B <= 0 || J <= 0) return hipErrorInvalidValue;
  constexpr int KC = 8;
  const int nqb = long_query_blocks(T), waves = long_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)4 * 32 * KC * 128;   // K_hi, K_lo, V_hi, V_lo planes of one chunk
  return launch_lds<k_attn_temporal_x3l<KC>>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, (const _Float16*)qkv_hi,
                                             (const _Float16*)qkv_lo, (_Float16*)out_x3, T, J, H, D, (int)units, nqb, launch_range_word());
}

}  // namespace d3d
