// F16X3 GRAND attention for heads of 16 columns (embed_dim 128 with the runner's 8 heads): groups of N <= 256 tokens, spatial and
// temporal blocks.  Four adjacent heads are one 64-column segment of the plane rows: its K / V rows are the 128-byte LDS rows of
// k_attn_temporal_x3 (kernels_attn_x3.hip), staged, swizzled and read by the same pieces of attn_x3_tile.h with hd = the quad's index --
// the pair rule of k_attn_x3_h32 (kernels_attn_x3_h32.hip) one level down.
//
//   scores   head p of the quad owns d-step p of the score product: a 16-deep d-step of the 32x32x16 MFMA is exactly the head's 16
//            columns, x3_score_tile<p, 1>, 3 MFMAs per 32 x 32 tile
//   softmax  each head has its own scores, maximum, numerators and sum.  The planes hold raw q and 8 k whatever the width, so the exponent
//            constant is x3_c_exp<16>() = log2(e) / (8 sqrt(16)) = 2 X3_C_EXP, exactly
//   product  two heads share a 32-column PV line (dt = p >> 1), and the 32 x 32 accumulator tile of O^T covers the whole line: each head
//            has a tile of its own, of which rows 16 (p & 1) .. + 15 -- accumulator registers 8 (p & 1) .. + 7 -- are its columns.  The
//            other 16 rows are the line neighbour's V times this head's E: they stay in registers and never reach memory, so a NaN in
//            the neighbour's V cannot reach this head (the MFMA keeps the rows of its A operand apart)
//   output   the head's 16 columns are half a 128-byte line of the pair layout: chunks g4 = 2 (p & 1), 2 (p & 1) + 1 of the line
//
// Structured like k_attn_x3_h32<NKT, MU>: compiler-scheduled, register staging, one workgroup per (group, quad) unit (MU > 1: MU
// single-tile units, one per wave, each in its own LDS slice); no LDS-DMA, no persistent walk.  As there: K / V rows >= N are staged as
// zeros, keys >= N score -inf, rows >= N are never stored, every wave reaches the one barrier, and no lane leaves before the transposing
// V reads.  A wave runs the four heads one after the other, so one head's score tiles and one accumulator are live at a time.
#include "d3d_kernels.h"

#include <math.h>
#include <type_traits>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic: query fragments, score tile, softmax, PV steps, output chunk, register staging

constexpr int H16_DH = 16;        // head width
constexpr int H16_QW = 64;        // columns of a head quad = of an LDS row

template <int NKT, int MU>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_x3_h16(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                               _Float16* __restrict__ out_x3, int T, int J, int HQ, int D, int units,
                                                               unsigned* rw) {
  static_assert(MU == 1 || NKT == 1, "several units per workgroup only for single-tile groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  constexpr int TP = 32 * NKT;
  const int lane = threadIdx.x & 63;
  const int sub = (MU > 1) ? (int)(threadIdx.x >> 6) : 0;          // unit of this workgroup
  const int wave = (MU > 1) ? 0 : (int)(threadIdx.x >> 6);         // 32-query tile of the unit
  const int tid = (MU > 1) ? lane : (int)threadIdx.x;              // thread index within the unit
  unsigned char* const lds = lds_all + sub * (4 * TP * 128);
  unsigned char* const sKh = lds;                     // [TP][128 B]
  unsigned char* const sKl = lds + TP * 128;
  unsigned char* const sVh = lds + 2 * TP * 128;
  unsigned char* const sVl = lds + 3 * TP * 128;

  const int unit_raw = blockIdx.x * MU + sub;         // (b*J + j)*HQ + hq, HQ = H / 4 head quads
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus waves redo the last unit and store nothing
  const int hq = unit % HQ;
  const int bj = unit / HQ;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J

  // ---- stage K and V rows of this (batch, joint, head quad) (pad rows zero): one batch of four slots per thread covers the unit
  __builtin_assume(tid < 64 * NKT);
  x3_stage_rows<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hq, 0, NKT, T, tid, 64 * NKT);

  const int tq = 32 * wave + r;
  const size_t qo = (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hq * H16_QW + 8 * h;   // this lane's query row, the quad's columns
  __syncthreads();

  const bool store = tq < T && unit_ok;
  const size_t tokq = tok0 + (size_t)(tq < T ? tq : 0) * J;
  const size_t vo = tokq * D3 + 2 * D + hq * H16_QW;
  const size_t oo = tokq * 2 * D + hq * 2 * H16_QW;   // pair layout: a head's 16 columns are half a 128-byte line
  float amax = 0.0f;   // range guard
  auto head = [&](auto pc) {
    constexpr int P = decltype(pc)::value, DT = P >> 1;
    // ---- this lane's query row, the head's 16 columns (rows >= T: zeros): fragment P of the quad's four.  Loaded head by head, so that
    // the later heads' fragments are not live under this head's score tiles (24 registers at the first head)
    h8 qh[4], ql[4];   // ([P] alone is used)
    if (tq < T) {
      qh[P] = *reinterpret_cast<const h8*>(Ph + qo + 16 * P);
      ql[P] = *reinterpret_cast<const h8*>(Pl + qo + 16 * P);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { qh[P][e] = (_Float16)0.0f; ql[P][e] = (_Float16)0.0f; }
    }
    // ---- S^T tiles over the head's 16 columns, softmax numerators (in sacc) and their sum, O^T of the head's PV line
    f32x16 sacc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile<P, 1>(sKh, sKl, kt * 32, r, h, qh, ql);
    const float l = x3_softmax<NKT, H16_DH>(sacc, h, T);
    f32x16 oacc[2];   // ([DT] alone is used, and of it the head's 16 rows alone are stored)
    // The 4 NKT V^T read addresses of a PV line depend on the lane alone, so the compiler forms those of all four heads once, up front,
    // and keeps them (64 registers at NKT = 8: scratch from NKT = 7 on).  An opaque copy of the lane per head makes each head form its own.
    int pv_lane = lane;
    asm volatile("" : "+v"(pv_lane));
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[DT][q] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) x3_pv_tile<false, DT, 1>(sacc[kt], sVh, sVl, 0, kt, T, pv_lane, pv_lane >> 5, oacc);
    // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM: rows 16 (P & 1) .. + 15 of the tile
    if (store) {
      const float inv = 1.0f / (8192.0f * l);
#pragma unroll
      for (int g4 = 2 * (P & 1); g4 < 2 * (P & 1) + 2; ++g4) {
        const int d = DT * 32 + 8 * g4 + 4 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[DT], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    }
  };
  head(std::integral_constant<int, 0>{});
  head(std::integral_constant<int, 1>{});
  head(std::integral_constant<int, 2>{});
  head(std::integral_constant<int, 3>{});
  if (store && amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
}

bool attn_x3_h16_ok(int N, int D, int H) { return N >= 1 && N <= 256 && H >= 4 && H % 4 == 0 && D == H16_DH * H; }

template <int NKT, int MU = 1>
static hipError_t launch_h16_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)MU * 4 * 32 * NKT * 128;   // per unit: K_hi, K_lo, V_hi, V_lo planes of TP rows x 128 B
  const long long units = (long long)B * J * (H / 4);
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_x3_h16<NKT, MU>>(dim3((unsigned)((units + MU - 1) / MU)), dim3(64 * NKT * MU), lds_bytes, s, ph, pl, ox, T, J, H / 4,
                                            D, (int)units, launch_range_word());
}

hipError_t launch_attn_x3_h16(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_x3_h16_ok(T, D, H) || B <= 0 || J <= 0 || !qkv_hi || !qkv_lo || !out_x3) return hipErrorInvalidValue;
  const _Float16 *ph = (const _Float16*)qkv_hi, *pl = (const _Float16*)qkv_lo;
  _Float16* ox = (_Float16*)out_x3;
  switch ((T + 31) / 32) {
    case 1:
      // single-tile groups: eight units per workgroup from 4096 units on.  The threshold is launch_attn_x3_h32's (itself copied from
      // launch_attn_temporal_x3: a 64-thread workgroup per unit is bound by the workgroup launch rate), not measured at this width.
      if ((long long)B * J * (H / 4) >= 4096) return launch_h16_nkt<1, 8>(ph, pl, ox, B, T, J, D, H, s);
      return launch_h16_nkt<1, 1>(ph, pl, ox, B, T, J, D, H, s);
    case 2: return launch_h16_nkt<2>(ph, pl, ox, B, T, J, D, H, s);
    case 3: return launch_h16_nkt<3>(ph, pl, ox, B, T, J, D, H, s);
    case 4: return launch_h16_nkt<4>(ph, pl, ox, B, T, J, D, H, s);
    case 5: return launch_h16_nkt<5>(ph, pl, ox, B, T, J, D, H, s);
    case 6: return launch_h16_nkt<6>(ph, pl, ox, B, T, J, D, H, s);
    case 7: return launch_h16_nkt<7>(ph, pl, ox, B, T, J, D, H, s);
    default: return launch_h16_nkt<8>(ph, pl, ox, B, T, J, D, H, s);
  }
}

}  // namespace d3d
