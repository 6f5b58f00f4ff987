// F16X3 GRAND attention for heads of 128 columns (embed_dim 1024 with the runner's 8 heads): groups of N <= 128 tokens, spatial and
// temporal blocks.  A head is two adjacent 64-column halves of the plane rows: half f of head hd is the 64-column "pseudo-head"
// 2 hd + f of k_attn_temporal_x3 (kernels_attn_x3.hip), staged, swizzled and read by the same pieces of attn_x3_tile.h.  Every plane
// (K_hi, K_lo, V_hi, V_lo) is two sub-planes of TP 128-byte rows, half 0 then half 1, so a key row is two LDS rows per plane.
//
//   S^T   one accumulator chain over the eight 16-deep d-steps, half 0 then half 1, ascending d, small terms first (x3_score_acc)
//   e     one softmax per head, exponent constant x3_c_exp<128>()
//   O^T   four 32-column quarters, two per half, each its own accumulator over the key tiles in ascending order
//   O     x3_out_chunk per quarter into the pair layout: one 128-byte line per quarter
//
// Structured like k_attn_x3_h32<NKT, MU>: compiler-scheduled, register staging, one workgroup per (group, head) unit (MU > 1: MU
// single-tile units, one per wave, each in its own 32 KiB LDS slice); no LDS-DMA, no persistent walk.  As there: K / V rows >= N are
// staged as zeros, keys >= N score -inf, rows >= N are never stored, surplus waves redo the last unit and store nothing, every wave
// reaches the one barrier, and no lane leaves before the transposing V reads.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic: query fragments, score tile, softmax, PV steps, output chunk, register staging

constexpr int H128_DH = 128;      // head width
constexpr int H128_HW = 64;       // columns of a head half = of an LDS row

template <int NKT, int MU>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_x3_h128(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                                _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units,
                                                                unsigned* rw) {
  static_assert(MU == 1 || NKT == 1, "several units per workgroup only for single-tile groups");
  static_assert(NKT >= 1 && NKT <= 4, "groups of up to 128 tokens");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  constexpr int TP = 32 * NKT;
  constexpr int PL = TP * 128;                        // bytes of one sub-plane (one half of one plane)
  const int lane = threadIdx.x & 63;
  const int sub = (MU > 1) ? (int)(threadIdx.x >> 6) : 0;          // unit of this workgroup
  const int wave = (MU > 1) ? 0 : (int)(threadIdx.x >> 6);         // 32-query tile of the unit
  const int tid = (MU > 1) ? lane : (int)threadIdx.x;              // thread index within the unit
  unsigned char* const lds = lds_all + sub * (8 * PL);
  unsigned char* const sKh = lds;                     // [2 halves][TP][128 B]
  unsigned char* const sKl = lds + 2 * PL;
  unsigned char* const sVh = lds + 4 * PL;
  unsigned char* const sVl = lds + 6 * PL;

  const int unit_raw = blockIdx.x * MU + sub;         // (b*J + j)*H + hd
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus waves redo the last unit and store nothing
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J

  // ---- stage K and V rows of this (batch, joint, head), one half after the other (pad rows zero)
  __builtin_assume(tid < 64 * NKT);
#pragma unroll
  for (int f = 0; f < 2; ++f)
    x3_stage_rows<true>(Ph, Pl, sKh + f * PL, sKl + f * PL, sVh + f * PL, sVl + f * PL, tok0, J, D, 2 * hd + f, 0, NKT, T, tid, 64 * NKT);

  // ---- this lane's query row, both halves (rows >= T: zeros)
  const int tq = 32 * wave + r;
  const size_t tokq = tok0 + (size_t)(tq < T ? tq : 0) * J;
  h8 qh0[4], ql0[4], qh1[4], ql1[4];
  x3_q_global(Ph, Pl, tokq * D3 + hd * H128_DH + 8 * h, tq < T, qh0, ql0);
  x3_q_global(Ph, Pl, tokq * D3 + hd * H128_DH + H128_HW + 8 * h, tq < T, qh1, ql1);
  __syncthreads();

  // ---- S^T tiles over the head's 128 columns, softmax numerators (in sacc) and their sum
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[kt][q] = 0.f;
    x3_score_acc(sacc[kt], sKh, sKl, kt * 32, r, h, qh0, ql0);
    x3_score_acc(sacc[kt], sKh + PL, sKl + PL, kt * 32, r, h, qh1, ql1);
  }
  const float l = x3_softmax<NKT, H128_DH>(sacc, h, T);

  // ---- O^T[d][query] = sum_key V^T[d][key] * E^T[key][query]: oa0 / oa1 hold the two 32-column quarters of half 0 / half 1
  f32x16 oa0[2], oa1[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oa0[0][q] = 0.f; oa0[1][q] = 0.f; oa1[0][q] = 0.f; oa1[1][q] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    x3_pv_tile<false>(sacc[kt], sVh, sVl, 0, kt, T, lane, h, oa0);
    x3_pv_tile<false>(sacc[kt], sVh + PL, sVl + PL, 0, kt, T, lane, h, oa1);
  }

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
      const size_t vo = tokq * D3 + 2 * D + (2 * hd + f) * H128_HW;
      const size_t oo = tokq * 2 * D + (2 * hd + f) * 2 * H128_HW;   // pair layout: a quarter's 32 columns are one 128-byte line
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

bool attn_x3_h128_ok(int N, int D, int H) { return N >= 1 && N <= 128 && H >= 1 && D == H128_DH * H; }

template <int NKT, int MU = 1>
static hipError_t launch_h128_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)MU * 8 * 32 * NKT * 128;   // per unit: K_hi, K_lo, V_hi, V_lo planes of 2 x TP rows x 128 B
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_x3_h128<NKT, MU>>(dim3((unsigned)((units + MU - 1) / MU)), dim3(64 * NKT * MU), lds_bytes, s, ph, pl, ox, T, J, H,
                                             D, (int)units, launch_range_word());
}

hipError_t launch_attn_x3_h128(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_x3_h128_ok(T, D, H) || B <= 0 || J <= 0 || !qkv_hi || !qkv_lo || !out_x3) return hipErrorInvalidValue;
  const _Float16 *ph = (const _Float16*)qkv_hi, *pl = (const _Float16*)qkv_lo;
  _Float16* ox = (_Float16*)out_x3;
  switch ((T + 31) / 32) {
    case 1:
      // single-tile groups: four units per workgroup (4 x 32 KiB of LDS) from 4096 units on.  The threshold is launch_attn_x3_h32's,
      // itself copied from launch_attn_temporal_x3's multi-unit forms: not measured at this width.
      if ((long long)B * J * H >= 4096) return launch_h128_nkt<1, 4>(ph, pl, ox, B, T, J, D, H, s);
      return launch_h128_nkt<1, 1>(ph, pl, ox, B, T, J, D, H, s);
    case 2: return launch_h128_nkt<2>(ph, pl, ox, B, T, J, D, H, s);
    case 3: return launch_h128_nkt<3>(ph, pl, ox, B, T, J, D, H, s);
    default: return launch_h128_nkt<4>(ph, pl, ox, B, T, J, D, H, s);
  }
}

}  // namespace d3d
