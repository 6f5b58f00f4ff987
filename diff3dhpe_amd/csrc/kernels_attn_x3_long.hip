// Temporal GRAND attention on the fp16 matrix pipe for windows of ANY length, at head widths 64, 32, 128, 48, 96 and 16: the keys stream through
// LDS in chunks of 32 KC frames instead of all living there (kernels_attn_x3.hip, kernels_attn_x3_h32.hip, kernels_attn_x3_h128.hip: four
// planes of resident rows = 128 of the 160 KiB).  One kernel template, k_attn_x3_stream<DH, KC>; what differs by width is
// x3_head_shape<DH> (attn_x3_tile.h): the 64-column segments of a unit, its softmax streams, its score tile(s) and PV step(s).
//
//   DH = 64    a unit is a head: one 128-byte LDS row per key, chunks of 256 frames (KC = 8)
//   DH = 32    a unit is a PAIR of adjacent heads in one 128-byte row, chunks of 256 frames; sub-head p owns d-steps 2 p, 2 p + 1 of the score
//              product and the 32-column half p of the PV product and of the output, and has its own maximum, numerators and sum.  The two
//              are independent, so interleaving them per key tile leaves each one's MFMA and addition order as k_attn_x3_h32 has it
//   DH = 16    a unit is a QUAD of adjacent heads in one 128-byte row, chunks of 256 frames; head p owns d-step p of the score product and an
//              O^T accumulator of its own over 32-column line p >> 1, of which rows 16 (p & 1) .. + 15 are its 16 output columns (half a
//              128-byte line of the pair layout; the other rows never reach memory).  Four independent streams, each in k_attn_x3_h16's order
//   DH = 128   a unit is a head of two 64-column halves; every plane is two sub-planes of 32 KC rows, half 0 then half 1, chunks of
//              128 frames (KC = 4: 4 planes x 128 rows x 256 B = 128 KiB).  One score chain over the eight d-steps, four 32-column quarters of PV
//   DH = 48    a unit is a head of 48 plane columns from column 48 hd on -- not a whole 64-column segment: staged from that column, the rest
//              of its 128-byte row zeros; chunks of 256 frames (the walk of DH = 64), three d-steps, two PV lines, 48 output columns
//   DH = 96    a unit is a head of 96 plane columns from column 96 hd on, in two LDS rows of 64 + 32 columns (the upper half of the second
//              neither staged nor read); chunks of 128 frames (the walk of DH = 128), six d-steps, three PV lines
//
// The arithmetic is attn_x3_tile.h's, the pieces the resident kernels are built from: the exact two-pass softmax, not an online rescaling.
//
//   pass 1   per chunk: stage K, S^T = K Q^T tile by tile, running maximum m of this lane's query column (per stream)
//   pass 2   per chunk: stage K and V; per key tile the SAME MFMAs again (same bits), e = exp2(fma(s, C, -m C)), l += e in register order,
//            O^T += V^T E^T for the two 16-key steps of each 32-column line in the resident kernel's order
//   O = O^T / (2^13 l) - v_query, range guard, hi / lo planes out, one 128-byte pair-layout line per 32 columns: the resident epilogue
//
// So every exp2 sees the same m, l is summed in the same order and every accumulator takes the same MFMAs in the same order as in the
// resident kernel of its width: for T <= 256 (DH = 128: T <= 128) the output is bit-identical to launch_attn_temporal_x3 /
// launch_attn_x3_h32 / launch_attn_x3_h128 / launch_attn_x3_hx / launch_attn_x3_h16 whatever KC is (tests/test_gpu_long_temporal.py,
// test_gpu_long_h32.py, test_gpu_long_h128.py, test_gpu_attn_hx.py, test_gpu_attn_h16.py);
// beyond, tests/test_gpu_attn_x3_digests.py and test_gpu_attn_x3_width_digests.py pin the bits.  The price is the scores computed twice;
// one score tile per stream (16 registers) is live at a time.
//
// One workgroup per (batch, joint, unit, query block): the T queries of a unit are cut into ceil(T / 256) balanced blocks of at most
// 8 waves of 32 queries (T = 300: two blocks of 160), blockDim = 64 x that wave count -- a run-time value, the staging loops stride by
// it.  Staging is the base kernel's: through registers into the swizzled planes, all global loads of a batch issued before its LDS
// writes; no LDS-DMA, no counters, no persistent walk.  The rules:
//   - every wave executes every barrier: the chunk and key-tile trip counts depend on T alone, a wave whose queries are all >= T stages
//     and synchronises and only skips its stores
//   - row isolation: keys >= T score -inf (their e is an exact 0) and K / V rows >= T are staged as zeros in EVERY chunk, never left over
//     from the previous one: 0 x NaN cannot enter a clean row.  Only the unit's last key tile can hold such keys and pays for the mask
//   - rows >= T are never stored; surplus workgroups redo the last unit and store nothing
//   - the transposing V reads (x3_pv_tile) sit outside divergent branches
#include "d3d_kernels.h"

#include <math.h>

#include <type_traits>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vswz, split8_e
#include "attn_x3_tile.h"   // the tile arithmetic, the register staging, x3_head_shape

template <int DH, int KC>
__global__ __launch_bounds__(512) void k_attn_x3_stream(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                        _Float16* __restrict__ out_x3, int T, int J, int UPT, int D, int units, int nqb,
                                                        unsigned* rw) {
  using HS = x3_head_shape<DH>;
  constexpr int SUB = HS::SUB, NS = HS::STREAMS;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_st[];
  constexpr int CH = 32 * KC;                         // keys per chunk
  constexpr int PL = CH * 128;                        // bytes of one sub-plane
  unsigned char* const sKh = lds_st;                  // [SUB][CH][128 B]
  unsigned char* const sKl = lds_st + SUB * PL;
  unsigned char* const sVh = lds_st + 2 * SUB * PL;
  unsigned char* const sVl = lds_st + 3 * SUB * PL;
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit_raw = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus workgroups redo the last unit and store nothing
  const int col0 = (unit % UPT) * HS::COLS;           // (b*J + j)*UPT + u, UPT units per token; the unit's first plane column
  const int bj = unit / UPT;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // ---- this lane's query row, every segment (rows >= T: zeros)
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  h8 qh[SUB][4], ql[SUB][4];
#pragma unroll
  for (int f = 0; f < SUB; ++f) {
    const size_t qo = (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + col0 + 64 * f + 8 * h;
    if (f == 0) x3_q_global<(HS::seg_cols(0) / 16)>(Ph, Pl, qo, tq < T, qh[f], ql[f]);
    else x3_q_global<(HS::seg_cols(SUB - 1) / 16)>(Ph, Pl, qo, tq < T, qh[f], ql[f]);
  }

  // the chunk's K (and V) rows, every segment into its sub-planes
  auto stage = [&](auto with_v, int c, int nkt) {
    constexpr bool V = decltype(with_v)::value;
    x3_stage_segment<DH, V, 0>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, col0, c * CH, nkt, T, tid, nthr);
    if constexpr (SUB == 2) x3_stage_segment<DH, V, 1>(Ph, Pl, sKh + PL, sKl + PL, sVh + PL, sVl + PL, tok0, J, D, col0, c * CH, nkt, T, tid, nthr);
  };
  // S^T tile(s) kt of the staged chunk, keys >= T at -inf.  Only the unit's last key tile (gt == ntiles - 1) can hold such keys.
  // (Returned by value: with the tiles filled through a reference the compiler keeps more addresses live across the staging loops --
  // 197 instead of 166 VGPRs at DH = 32; experiments/NOTES.md has the forms that were tried.)
  struct Tiles { f32x16 s[NS]; };
  auto score_tiles = [&](int kt, int gt) -> Tiles {
    Tiles t;
    HS::scores(t.s, sKh, sKl, PL, kt * 32, r, h, qh, ql);
    if (gt == ntiles - 1) {
#pragma unroll
      for (int p = 0; p < NS; ++p) x3_mask_keys(t.s[p], gt * 32, h, T);
    }
    return t;
  };

  // ---- pass 1: the exact maximum over all keys of this query column, per stream
  float m[NS], mb[NS];
#pragma unroll
  for (int p = 0; p < NS; ++p) m[p] = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage(std::false_type{}, c, nkt);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const Tiles t = score_tiles(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q)
#pragma unroll
        for (int p = 0; p < NS; ++p) m[p] = fmaxf(m[p], t.s[p][q]);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
#pragma unroll
  for (int p = 0; p < NS; ++p) {
    m[p] = fmaxf(m[p], __shfl_xor(m[p], 32, 64));
    mb[p] = m[p] * x3_c_exp<DH>();
  }

  // ---- pass 2: numerators, their sums, O^T[d][query] = sum_key V^T[d][key] * E^T[key][query] (oacc[f][dt]: 32-column line dt of segment f; width 16: oacc[p][p >> 1], head p's own tile)
  float l[NS];
  f32x16 oacc[HS::ACCS][2];
#pragma unroll
  for (int p = 0; p < NS; ++p) l[p] = 0.f;
#pragma unroll
  for (int q = 0; q < 16; ++q)
#pragma unroll
    for (int f = 0; f < HS::ACCS; ++f) { oacc[f][0][q] = 0.f; oacc[f][1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage(std::true_type{}, c, nkt);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      Tiles t = score_tiles(kt, c * KC + kt);
#pragma unroll
      for (int p = 0; p < NS; ++p) x3_exp_tile<DH>(t.s[p], mb[p], l[p]);
      HS::pv(t.s, sVh, sVl, PL, kt, T, lane, h, oacc);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
#pragma unroll
  for (int p = 0; p < NS; ++p) l[p] += __shfl_xor(l[p], 32, 64);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM: one 128-byte pair-layout line per 32 columns
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const size_t tokq = tok0 + (size_t)tq * J;
    // pair layout: the 32 columns of a pair group are one 128-byte line.  A unit of whole segments writes whole lines; at widths 48 and 96
    // a line of the head can straddle two groups at a 16-column boundary, so every 4-column chunk takes pair_col of its own plane column
    // (out rows of 2 ceil32(D) halves: the row pitch of the layout, 2 D wherever an engine runs)
    const size_t orow = tokq * (HS::ALIGNED ? 2 * D : 2 * ((D + 31) & ~31));
    if constexpr (DH == 16) {
      // head p of the quad: rows 16 (p & 1) .. + 15 of its own accumulator (registers 8 (p & 1) .. + 7: chunks g4 = 2 (p & 1), + 1) are
      // its 16 columns, half a 128-byte line; the tile's other rows hold the line neighbour's V times this head's E and stay in registers
      const size_t vo = tokq * D3 + 2 * D + col0;
#pragma unroll
      for (int p = 0; p < NS; ++p) {
        const float inv = 1.0f / (8192.0f * l[p]);
#pragma unroll
        for (int g4 = 2 * (p & 1); g4 < 2 * (p & 1) + 2; ++g4) {
          const int d = (p >> 1) * 32 + 8 * g4 + 4 * h;
          h4 oh, ol;
          x3_out_chunk(oacc[p][p >> 1], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax,
                       oh, ol);
          _Float16* const op = out_x3 + orow + (size_t)(2 * col0) + pair_col(d);
          *reinterpret_cast<h4*>(op) = oh;
          *reinterpret_cast<h4*>(op + PAIR_LO) = ol;
        }
      }
    } else {
#pragma unroll
      for (int f = 0; f < SUB; ++f) {
        const int c0 = col0 + 64 * f;
        const size_t vo = tokq * D3 + 2 * D + c0;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const float inv = 1.0f / (8192.0f * l[HS::line_stream(dt)]);
#pragma unroll
          for (int g4 = 0; g4 < HS::line_cols(f, dt) / 8; ++g4) {
            const int d = dt * 32 + 8 * g4 + 4 * h;
            h4 oh, ol;
            x3_out_chunk(oacc[f][dt], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d),
                         *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
            _Float16* const op = out_x3 + orow + (HS::ALIGNED ? (size_t)(2 * c0) + pair_col(d) : pair_col(c0 + d));
            *reinterpret_cast<h4*>(op) = oh;
            *reinterpret_cast<h4*>(op + PAIR_LO) = ol;
          }
        }
      }
    }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

template <int DH>
static bool attn_x3_stream_ok(int T, int D, int H) {
  // (the workgroup count is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && x3_head_shape<DH>::heads_ok(H) && D == H * DH;
}

// The query blocks of a unit: ceil(T / 256) of them, balanced, in whole waves of 32 queries.  LDS: the K_hi, K_lo, V_hi, V_lo planes of
// one chunk, SUB sub-planes each.
template <int DH, int KC>
static hipError_t launch_attn_x3_stream(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_x3_stream_ok<DH>(T, D, H) || !qkv_hi || !qkv_lo || !out_x3 || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const int nqb = (T + 255) / 256;
  const int waves = ((T + nqb - 1) / nqb + 31) / 32;   // <= 8: ceil(T / nqb) <= 256
  const int upt = x3_head_shape<DH>::units_per_token(H);
  const long long units = (long long)B * J * upt;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)4 * x3_head_shape<DH>::SUB * 32 * KC * 128;
  return launch_lds<k_attn_x3_stream<DH, KC>>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, (const _Float16*)qkv_hi,
                                              (const _Float16*)qkv_lo, (_Float16*)out_x3, T, J, upt, D, (int)units, nqb, launch_range_word());
}

bool attn_temporal_x3_long_ok(int T, int D, int H) { return attn_x3_stream_ok<64>(T, D, H); }
bool attn_x3_h32_long_ok(int T, int D, int H) { return attn_x3_stream_ok<32>(T, D, H); }
bool attn_x3_h128_long_ok(int T, int D, int H) { return attn_x3_stream_ok<128>(T, D, H); }
bool attn_x3_hx_long_ok(int T, int D, int H) { return attn_x3_stream_ok<48>(T, D, H) || attn_x3_stream_ok<96>(T, D, H); }
bool attn_x3_h16_long_ok(int T, int D, int H) { return attn_x3_stream_ok<16>(T, D, H); }

hipError_t launch_attn_temporal_x3_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                        hipStream_t s) {
  return launch_attn_x3_stream<64, 8>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
}
hipError_t launch_attn_x3_h32_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  return launch_attn_x3_stream<32, 8>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
}
hipError_t launch_attn_x3_h128_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  return launch_attn_x3_stream<128, 4>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
}
// widths 48 and 96 (the width is D / H): the walks of <64, 8> and <128, 4>
hipError_t launch_attn_x3_hx_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  if (H > 0 && D == 48 * H) return launch_attn_x3_stream<48, 8>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
  return launch_attn_x3_stream<96, 4>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
}
// width 16: a quad of heads per unit, the walk of <32, 8> with four streams
hipError_t launch_attn_x3_h16_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H, hipStream_t s) {
  return launch_attn_x3_stream<16, 8>(qkv_hi, qkv_lo, out_x3, B, T, J, D, H, s);
}

}  // namespace d3d
