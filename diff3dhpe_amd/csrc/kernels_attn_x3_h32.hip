// F16X3 GRAND attention for heads of 32 columns (embed_dim 256 with the runner's 8 heads): groups of N <= 256 tokens, spatial and
// temporal blocks.  Two adjacent heads are one 64-column "pseudo-head": its K / V rows are the 128-byte LDS rows of k_attn_temporal_x3
// (kernels_attn_x3.hip), staged, swizzled and read by the same pieces of attn_x3_tile.h with hd = the pair's index.  Sub-head p of the pair
// owns d-steps 2 p, 2 p + 1 of the score product and the 32-column half dt = p of the PV product and of the output -- exactly one
// 128-byte line of the pair layout -- and has its own scores, softmax and sum: a wave runs the two one after the other, 6 + 6 MFMAs per
// 32 x 32 tile and sub-head.  The planes hold raw q and 8 k whatever the width, so the exponent constant is x3_c_exp<32>().
//
// Structured like the base kernel k_attn_temporal_x3<NKT, MU>: compiler-scheduled, register staging, one workgroup per (group, pair) unit
// (MU > 1: MU single-tile units, one per wave, each in its own LDS slice); no LDS-DMA, no persistent walk.  As there: K / V rows >= N are
// staged as zeros, keys >= N score -inf, rows >= N are never stored, every wave reaches the one barrier, and no lane leaves before the
// transposing V reads.
#include "d3d_kernels.h"

#include <math.h>
#include <type_traits>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic: query fragments, score tile, softmax, PV steps, output chunk, register staging

constexpr int H32_DH = 32;        // head width
constexpr int H32_PW = 64;        // columns of a head pair = of an LDS row

template <int NKT, int MU>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_x3_h32(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                               _Float16* __restrict__ out_x3, int T, int J, int HP, int D, int units,
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

  const int unit_raw = blockIdx.x * MU + sub;         // (b*J + j)*HP + hp, HP = H / 2 head pairs
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus waves redo the last unit and store nothing
  const int hp = unit % HP;
  const int bj = unit / HP;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J

  // ---- stage K and V rows of this (batch, joint, head pair) (pad rows zero): one batch of four slots per thread covers the unit
  __builtin_assume(tid < 64 * NKT);
  x3_stage_rows<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hp, 0, NKT, T, tid, 64 * NKT);

  // ---- this lane's query row, both heads of the pair (rows >= T: zeros): fragments 2 p, 2 p + 1 are sub-head p's
  const int tq = 32 * wave + r;
  h8 qh[4], ql[4];
  x3_q_global(Ph, Pl, (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hp * H32_PW + 8 * h, tq < T, qh, ql);
  __syncthreads();

  const bool store = tq < T && unit_ok;
  const size_t tokq = tok0 + (size_t)(tq < T ? tq : 0) * J;
  const size_t vo = tokq * D3 + 2 * D + hp * H32_PW;
  const size_t oo = tokq * 2 * D + hp * 2 * H32_PW;   // pair layout: a head's 32 columns are one 128-byte line
  float amax = 0.0f;   // range guard
  auto sub_head = [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    // ---- S^T tiles over the head's 32 columns, softmax numerators (in sacc) and their sum, O^T of the head's 32 columns
    f32x16 sacc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile<2 * P, 2>(sKh, sKl, kt * 32, r, h, qh, ql);
    const float l = x3_softmax<NKT, H32_DH>(sacc, h, T);
    f32x16 oacc[2];   // ([P] alone is used)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[P][q] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) x3_pv_tile<false, P, 1>(sacc[kt], sVh, sVl, 0, kt, T, lane, h, oacc);
    // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM
    if (store) {
      const float inv = 1.0f / (8192.0f * l);
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = P * 32 + 8 * g4 + 4 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[P], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    }
  };
  sub_head(std::integral_constant<int, 0>{});
  sub_head(std::integral_constant<int, 1>{});
  if (store && amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
}

bool attn_x3_h32_ok(int N, int D, int H) { return N >= 1 && N <= 256 && H >= 2 && H % 2 == 0 && D == H32_DH * H; }

template <int NKT, int MU = 1>
static hipError_t launch_h32_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)MU * 4 * 32 * NKT * 128;   // per unit: K_hi, K_lo, V_hi, V_lo planes of TP rows x 128 B
  const long long units = (long long)B * J * (H / 2);
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_x3_h32<NKT, MU>>(dim3((unsigned)((units + MU - 1) / MU)), dim3(64 * NKT * MU), lds_bytes, s, ph, pl, ox, T, J, H / 2,
                                            D, (int)units, launch_range_word());
}

hipError_t launch_attn_x3_h32(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_x3_h32_ok(T, D, H) || B <= 0 || J <= 0 || !qkv_hi || !qkv_lo || !out_x3) return hipErrorInvalidValue;
  const _Float16 *ph = (const _Float16*)qkv_hi, *pl = (const _Float16*)qkv_lo;
  _Float16* ox = (_Float16*)out_x3;
  switch ((T + 31) / 32) {
    case 1:
      // single-tile groups: eight units per workgroup from 4096 units on.  The threshold is launch_attn_temporal_x3's for its own
      // multi-unit forms (a 64-thread workgroup per unit is bound by the workgroup launch rate), copied, not measured at this width.
      if ((long long)B * J * (H / 2) >= 4096) return launch_h32_nkt<1, 8>(ph, pl, ox, B, T, J, D, H, s);
      return launch_h32_nkt<1, 1>(ph, pl, ox, B, T, J, D, H, s);
    case 2: return launch_h32_nkt<2>(ph, pl, ox, B, T, J, D, H, s);
    case 3: return launch_h32_nkt<3>(ph, pl, ox, B, T, J, D, H, s);
    case 4: return launch_h32_nkt<4>(ph, pl, ox, B, T, J, D, H, s);
    case 5: return launch_h32_nkt<5>(ph, pl, ox, B, T, J, D, H, s);
    case 6: return launch_h32_nkt<6>(ph, pl, ox, B, T, J, D, H, s);
    case 7: return launch_h32_nkt<7>(ph, pl, ox, B, T, J, D, H, s);
    default: return launch_h32_nkt<8>(ph, pl, ox, B, T, J, D, H, s);
  }
}

}  // namespace d3d
