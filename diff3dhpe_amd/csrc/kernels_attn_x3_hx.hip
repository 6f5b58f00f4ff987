// F16X3 GRAND attention for heads of 48 and 96 columns (embed_dim 384 and 768 with the runner's 8 heads): resident groups, spatial and
// temporal blocks.  These widths are no multiple of the 64-column (128-byte) LDS row, so a head is not a "pseudo-head" of
// k_attn_temporal_x3: head hd is the DH adjacent columns of the q / k / v planes from column hd DH on, wherever that falls.  Staging
// (x3_stage_cols), the query fragments and the query's own V read take that column offset; the output goes to the pair layout through
// pair_col(hd DH + d) per 4-column chunk, because a 32-column line of a head can straddle two pair groups at a 16-column boundary.
//
//   DH = 48   one LDS row per key: S^T over three 16-deep d-steps (x3_score_tile<0, 3>), two 32-column PV lines of which the second is
//             half used.  Columns 48 .. 63 of the K and V rows are staged as exact zeros and the query's fourth d-step is zeros: never
//             the neighbouring head's data.  Groups of N <= 256 tokens (the limits of width 64: 4 planes x 256 rows x 128 B = 128 KiB)
//   DH = 96   two LDS rows per key, 64 + 32 columns, each in sub-planes of its own as at width 128: one accumulator chain over the six
//             d-steps, row 0 then row 1, ascending d; three PV lines.  The upper 32 columns of the second row are SKIPPED: neither
//             staged nor read (the score chain takes its two d-steps, the PV product its one line), so they hold no defined bits.
//             Groups of N <= 128 tokens (the limits of width 128)
//
// The arithmetic is attn_x3_tile.h's through x3_head_shape<DH>, the pieces k_attn_x3_stream<DH, KC> (kernels_attn_x3_long.hip) runs, so
// the streaming kernel of a width is bit-identical to this one wherever both run.  The exponent constant is x3_c_exp<DH>().
//
// Structured like k_attn_x3_h128<NKT, MU>: compiler-scheduled, register staging, one workgroup per (group, head) unit (MU > 1: MU
// single-tile units, one per wave, each in its own LDS slice); no LDS-DMA, no persistent walk.  As there: K / V rows >= N are staged as
// zeros, keys >= N score -inf, rows >= N are never stored, surplus waves redo the last unit and store nothing, every wave reaches the
// one barrier, and no lane leaves before the transposing V reads.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic: query fragments, score tile, softmax, PV steps, output chunk, staging, x3_head_shape

template <int DH, int NKT, int MU>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_x3_hx(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                              _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units,
                                                              unsigned* rw) {
  using HS = x3_head_shape<DH>;
  constexpr int SUB = HS::SUB;
  static_assert(DH == 48 || DH == 96, "the widths that are no multiple of an LDS row");
  static_assert(MU == 1 || NKT == 1, "several units per workgroup only for single-tile groups");
  static_assert(NKT >= 1 && NKT * SUB <= 8, "four planes of resident rows in 128 KiB");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  constexpr int TP = 32 * NKT;
  constexpr int PL = TP * 128;                        // bytes of one sub-plane
  const int lane = threadIdx.x & 63;
  const int sub = (MU > 1) ? (int)(threadIdx.x >> 6) : 0;          // unit of this workgroup
  const int wave = (MU > 1) ? 0 : (int)(threadIdx.x >> 6);         // 32-query tile of the unit
  const int tid = (MU > 1) ? lane : (int)threadIdx.x;              // thread index within the unit
  unsigned char* const lds = lds_all + sub * (4 * SUB * PL);
  unsigned char* const sKh = lds;                     // [SUB][TP][128 B]
  unsigned char* const sKl = lds + SUB * PL;
  unsigned char* const sVh = lds + 2 * SUB * PL;
  unsigned char* const sVl = lds + 3 * SUB * PL;

  const int unit_raw = blockIdx.x * MU + sub;         // (b*J + j)*H + hd
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus waves redo the last unit and store nothing
  const int col0 = (unit % H) * DH;                   // the head's first plane column
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J

  // ---- stage K and V rows of this (batch, joint, head), one LDS row of the head after the other (pad rows and pad columns zero)
  __builtin_assume(tid < 64 * NKT);
  x3_stage_segment<DH, true, 0>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, col0, 0, NKT, T, tid, 64 * NKT);
  if constexpr (SUB == 2) x3_stage_segment<DH, true, 1>(Ph, Pl, sKh + PL, sKl + PL, sVh + PL, sVl + PL, tok0, J, D, col0, 0, NKT, T, tid, 64 * NKT);

  // ---- this lane's query row, the head's d-steps of every LDS row (rows >= T and the d-steps behind the head: zeros)
  const int tq = 32 * wave + r;
  const size_t tokq = tok0 + (size_t)(tq < T ? tq : 0) * J;
  h8 qh[SUB][4], ql[SUB][4];
  x3_q_global<(HS::seg_cols(0) / 16)>(Ph, Pl, tokq * D3 + col0 + 8 * h, tq < T, qh[0], ql[0]);
  if constexpr (SUB == 2) x3_q_global<(HS::seg_cols(SUB - 1) / 16)>(Ph, Pl, tokq * D3 + col0 + 64 + 8 * h, tq < T, qh[SUB - 1], ql[SUB - 1]);
  __syncthreads();

  // ---- S^T tiles over the head's columns, softmax numerators (in sacc) and their sum
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32x16 s1[1];
    HS::scores(s1, sKh, sKl, PL, kt * 32, r, h, qh, ql);
    sacc[kt] = s1[0];
  }
  const float l = x3_softmax<NKT, DH>(sacc, h, T);

  // ---- O^T[d][query] = sum_key V^T[d][key] * E^T[key][query]: oacc[f][dt] is 32-column line dt of LDS row f
  f32x16 oacc[SUB][2];
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int f = 0; f < SUB; ++f) { oacc[f][0][q] = 0.f; oacc[f][1][q] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    const f32x16 e1[1] = {sacc[kt]};
    HS::pv(e1, sVh, sVl, PL, kt, T, lane, h, oacc);
  }

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM (out rows of 2 ceil32(D) halves: the row pitch of
  // the pair layout, 2 D wherever an engine runs)
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
    const size_t orow = tokq * (2 * ((D + 31) & ~31));
#pragma unroll
    for (int f = 0; f < SUB; ++f) {
      const int c0 = col0 + 64 * f;
      const size_t vo = tokq * D3 + 2 * D + c0;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int g4 = 0; g4 < HS::line_cols(f, dt) / 8; ++g4) {
          const int d = dt * 32 + 8 * g4 + 4 * h;
          h4 oh, ol;
          x3_out_chunk(oacc[f][dt], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh,
                       ol);
          _Float16* const op = out_x3 + orow + pair_col(c0 + d);
          *reinterpret_cast<h4*>(op) = oh;
          *reinterpret_cast<h4*>(op + PAIR_LO) = ol;
        }
      }
    }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// the width is D / H: 48 (groups of up to 256 tokens) or 96 (up to 128)
bool attn_x3_hx_ok(int N, int D, int H) {
  return N >= 1 && H >= 1 && ((D == 48 * H && N <= 256) || (D == 96 * H && N <= 128));
}

template <int DH, int NKT, int MU = 1>
static hipError_t launch_hx_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)MU * 4 * x3_head_shape<DH>::SUB * 32 * NKT * 128;   // per unit: K_hi, K_lo, V_hi, V_lo of SUB x TP rows x 128 B
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_x3_hx<DH, NKT, MU>>(dim3((unsigned)((units + MU - 1) / MU)), dim3(64 * NKT * MU), lds_bytes, s, ph, pl, ox, T, J, H,
                                               D, (int)units, launch_range_word());
}

hipError_t launch_attn_x3_hx(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_x3_hx_ok(T, D, H) || B <= 0 || J <= 0 || !qkv_hi || !qkv_lo || !out_x3) return hipErrorInvalidValue;
  const _Float16 *ph = (const _Float16*)qkv_hi, *pl = (const _Float16*)qkv_lo;
  _Float16* ox = (_Float16*)out_x3;
  // single-tile groups: several units per workgroup from 4096 units on, as many as the base ladder of the same LDS footprint takes
  // (launch_attn_temporal_x3: eight 16 KiB units; launch_attn_x3_h128: four 32 KiB units).  The threshold is copied from there, not
  // measured at these widths.
  const bool multi = (long long)B * J * H >= 4096;
  if (D == 48 * H) {
    switch ((T + 31) / 32) {
      case 1: return multi ? launch_hx_nkt<48, 1, 8>(ph, pl, ox, B, T, J, D, H, s) : launch_hx_nkt<48, 1, 1>(ph, pl, ox, B, T, J, D, H, s);
      case 2: return launch_hx_nkt<48, 2>(ph, pl, ox, B, T, J, D, H, s);
      case 3: return launch_hx_nkt<48, 3>(ph, pl, ox, B, T, J, D, H, s);
      case 4: return launch_hx_nkt<48, 4>(ph, pl, ox, B, T, J, D, H, s);
      case 5: return launch_hx_nkt<48, 5>(ph, pl, ox, B, T, J, D, H, s);
      case 6: return launch_hx_nkt<48, 6>(ph, pl, ox, B, T, J, D, H, s);
      case 7: return launch_hx_nkt<48, 7>(ph, pl, ox, B, T, J, D, H, s);
      default: return launch_hx_nkt<48, 8>(ph, pl, ox, B, T, J, D, H, s);
    }
  }
  switch ((T + 31) / 32) {
    case 1: return multi ? launch_hx_nkt<96, 1, 4>(ph, pl, ox, B, T, J, D, H, s) : launch_hx_nkt<96, 1, 1>(ph, pl, ox, B, T, J, D, H, s);
    case 2: return launch_hx_nkt<96, 2>(ph, pl, ox, B, T, J, D, H, s);
    case 3: return launch_hx_nkt<96, 3>(ph, pl, ox, B, T, J, D, H, s);
    default: return launch_hx_nkt<96, 4>(ph, pl, ox, B, T, J, D, H, s);
  }
}

}  // namespace d3d
