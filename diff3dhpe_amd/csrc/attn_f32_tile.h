// The exact-fp32 MFMA attention arithmetic (v_mfma_f32_32x32x2_f32), once, for head widths DH = 16, 32, 48, 64, 96 and 128: the resident kernels
// k_attn_temporal_f32<NKT> (kernels_attn.hip), k_attn_temporal_f32_h32<NKT> (kernels_attn_f32_h32.hip), k_attn_f32_h128<NKT>
// (kernels_attn_f32_h128.hip) and k_attn_f32_hx<DH, NKT> (kernels_attn_f32_hx.hip; widths 48, 96 and 16) and the key-streaming kernels
// k_attn_f32_stream3<DH> (the template at the end of this header; widths 64 and 32), k_attn_f32_h128_stream (kernels_attn_f32_h128.hip) and
// k_attn_f32_hx_stream<DH> (kernels_attn_f32_hx.hip) are their own walks around these pieces, so staging, query load, MFMA order, key
// index, pad mask, exp argument, PV order and store each have one copy, and a streaming kernel gives its resident twin's bits by
// construction (tests/test_gpu_attn_f32_digests.py pins the bits of all of them).  Compiler-scheduled, staged through registers,
// builtins only: no inline assembly, no LDS-DMA, no persistent walk.
//
//   O = (softmax(q k^T / sqrt(DH)) - I) v,   packed fp32 qkv rows (tokens, 3 D) in, fp32 rows (tokens, D) out
//
//   scores   swapped operands, S^T = K Q^T, one query column per lane: lane (r, hh) of a wave holds d in [DH/2 hh, DH/2 hh + DH/2) of
//            query row r of its wave in DH / 2 registers.  A 32 x 32 score tile is DH / 2 MFMAs, d ascending, each ds_read_b128 of K
//            feeding four of them; an MFMA adds the pair (d, d + DH / 2).  Register q of lane half hh is key (q & 3) + 8 (q >> 2) + 4 hh of
//            the tile (the C/D map of the 32 x 32 MFMA): f32_key.
//   softmax  exact and max-subtracted: keys >= N, which only the unit's last key tile can hold, score -inf (e = 0 exactly); m = the
//            maximum over all keys (registers, then one cross-half shuffle in the kernel), e = expf(s - m), l = the sum of e per lane in
//            key order (key tiles ascending, registers ascending), then one cross-half add.
//   product  O^T[d][query] += V^T P^T with P straight from the accumulator registers as the B operand, into NDT = ceil(DH / 32)
//            accumulator tiles of 32 x 32, one per 32 columns of the head; per key register the tiles ascending, keys ascending.  Width 48:
//            the second tile covers columns 32 .. 63 and only 32 .. 47 belong to the head; its V operand at columns >= 48 is the exact
//            zero of the padded LDS row (V_LD = 32 NDT), never the next head's columns, and those rows of O^T are never stored.  Width 16
//            likewise: its one tile covers columns 0 .. 31, of which 16 .. 31 are staged zeros and rows 16 .. 31 of O^T are never stored.
//
// What differs between the widths is named in F32Tile<DH> and must stay different: each width keeps the bits it was introduced with.
//
// LDS: K rows padded to DH + 4 floats, V rows 32 NDT floats (DH wherever DH % 32 == 0; 64 at width 48, columns 48 .. 63 staged as zeros;
// 32 at width 16, columns 16 .. 31 staged as zeros),
// 128 (DH + 4 + 32 NDT) B per key tile (F32Tile::lds_bytes): 256 DH + 512 B at widths 32, 64, 96 and 128, 14 848 B at width 48, 6 656 B at width 16.  Banks of the K fragment read (ds_read_b128,
// bank = (a / 4) mod 64, served in four groups of 16 lanes: lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): lane
// (r, hh) reads dword (DH + 4) r + DH/2 hh + 4 u.  Within a group hh and u are constant, so the 16-byte slot of a lane is
// ((DH/4 + 1) r + const) mod 16, and r -> (DH/4 + 1) r mod 16 is a bijection of r mod 16 for DH/4 = 4, 8, 12, 16, 24, 32 (multipliers 5, 9, 13, 1,
// 9, 1: all odd; const = DH/8 hh + u is a whole number of slots since DH/2 is a multiple of 4 at every width).  The
// 16 rows of either group are distinct mod 16 ({0-3, 12-15, 4-11} and {4-11, 0-3, 12-15}), so the 16 lanes cover the 16 four-bank slots
// once: conflict-free.  (Unpadded rows would put them on two slots at width 32 and on one at 64 and 128.)  The V read is a ds_read_b32
// of dword V_LD key + 32 dt + r with key and dt uniform over a 32-lane half and V_LD a multiple of 32: bank r, conflict-free.  The staging writes are ds_write_b128
// of 16 consecutive bytes per lane along a row.
//
// Row isolation: K / V rows >= N are staged as zeros -- in a streaming kernel in every chunk, never the previous chunk's bytes -- and
// their scores are -inf, so 0 x NaN cannot enter a clean row.  Rows >= N are never stored.
#pragma once

#include "d3d_kernels.h"

#include <math.h>

#include <type_traits>

namespace d3d {

typedef float f32x16 __attribute__((ext_vector_type(16)));

template <int DH>
struct F32Tile {
  static_assert(DH == 16 || DH == 32 || DH == 48 || DH == 64 || DH == 96 || DH == 128, "head widths with a tile form");
  static constexpr int NDT = (DH + 31) / 32;       // 32 x 32 accumulator tiles of O^T (width 48: the second one half used; width 16: the one)
  static constexpr int K_LD = DH + 4, V_LD = 32 * NDT;   // LDS row strides in floats; V columns >= DH are staged as zeros
  static constexpr int QR = DH / 2;                // query registers per lane (a multiple of 4 at every width)
  // Scale.  64^-1/2 = 2^-3 is exact: width 64 scales q.  At 32 and 128 dh^-1/2 is no power of two and scaling q would round every operand
  // of the dot product (and so would it at 48 and 96): the sums are multiplied by 1.0f / sqrtf(DH) AFTER the sum over d (k_attn_generic's constant and the reference's
  // order, (q k^T) * scale), and that product is a rounded fp32 value wherever the maximum or the mask takes it.  16^-1/2 = 2^-2 is exact
  // too, so scaling q or the sum gives the same bits there; width 16 scales the SUM, like every width it shares its kernels with.
  static constexpr bool SCALE_Q = DH == 64;
  // Exp argument at width 32: "s * scale - m" is ONE fma(s, scale, -m) in every key tile in front of the unit's last and the rounded
  // product, then the subtraction, in the last (where the -inf select of the pad mask stands between the two).  The resident kernel was
  // introduced with what the compiler contracted; f32_exp_tile states it.  Widths 48, 96 and 128 never have the fused form.
  static constexpr bool EXP_FMA_FRONT = DH == 32;
  // Normalisation.  Widths 32 and 64 divide by l before the second product (the streaming form needs l before the first V product: three
  // passes over the keys); widths 16, 48, 96 and 128 take the unnormalised numerators and divide at the store (two passes).
  static constexpr bool NORM_AT_STORE = DH == 128 || DH == 48 || DH == 96 || DH == 16;
  // Diagonal.  Width 64 puts the - 1 into P where the keys are resident (T <= 256).  With p[query] - 1 inside the product the accumulator
  // stands at |v| for the rest of the key walk and every later product is rounded to an ulp of |v| (4.56e-6 at N = 219; T = 769, hashed
  // inputs at scale 2.0: 6.4e-6 against fp64 where plain fp32 math loses 3.1e-6, tests/test_gpu_group_lengths.py), so beyond 256 keys,
  // and always at the other widths, the products are summed alone and v[query] is subtracted once, at the store.
  static constexpr bool DIAG_IN_P_RESIDENT = DH == 64;
  // key tiles per chunk of the streaming kernel: a chunk fills the resident maximum.  Width 96: six tiles (150 528 B) are the most K + V
  // that 160 KiB of LDS hold, seven (175 616 B) do not fit
  static constexpr int STREAM_KC = DH == 128 ? 4 : DH == 96 ? 6 : 8;
  static constexpr size_t lds_bytes(int nkt) { return (size_t)32 * nkt * (K_LD + V_LD) * sizeof(float); }   // K and V of nkt key tiles
};

// a * b rounded to fp32 whatever consumes it: never one half of a contracted fma
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// the key (of a unit, or the row of a staged chunk) that accumulator register q of lane half hh holds in key tile kt
__device__ __forceinline__ int f32_key(int kt, int q, int hh) { return 32 * kt + (q & 3) + 8 * (q >> 2) + 4 * hh; }

// Rows [row0, row0 + 32 nkt) of the unit's K (and V) into LDS rows [0, 32 nkt); rows >= N as zeros.  Four 16-byte slots per thread and
// batch (and array), all of a batch's global loads issued before its LDS writes.  token(row) = tok0 + row * stride.  Where the V rows are
// wider than the head (widths 48 and 16) their pad columns are written as zeros with every staging, rows >= N included.
template <int DH, bool WITH_V>
__device__ __forceinline__ void f32_stage_rows(const float* __restrict__ qkv, float* Ks, float* Vs, size_t tok0, int stride, int D, int hd,
                                               int row0, int nkt, int N, int tid, int nthr) {
  constexpr int NIT = 4, C4 = DH / 4, K_LD = F32Tile<DH>::K_LD, V_LD = F32Tile<DH>::V_LD;
  const int slots = nkt * 32 * C4;
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    float4 kk[NIT], vv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx / C4, c4 = idx % C4;
      kk[it] = make_float4(0, 0, 0, 0); vv[it] = kk[it];
      if (idx < slots && row0 + row < N) {
        const float* p = qkv + (tok0 + (size_t)(row0 + row) * stride) * D3 + hd * DH + c4 * 4;
        kk[it] = *reinterpret_cast<const float4*>(p + D);
        if (WITH_V) vv[it] = *reinterpret_cast<const float4*>(p + 2 * D);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx / C4, c4 = idx % C4;
      if (idx < slots) {
        *reinterpret_cast<float4*>(&Ks[row * K_LD + c4 * 4]) = kk[it];
        if (WITH_V) *reinterpret_cast<float4*>(&Vs[row * V_LD + c4 * 4]) = vv[it];
        if constexpr (WITH_V && V_LD > DH)      // the pad columns DH .. V_LD of the row, by its first (V_LD - DH) / 4 slots
          if (c4 < (V_LD - DH) / 4) *reinterpret_cast<float4*>(&Vs[row * V_LD + DH + c4 * 4]) = make_float4(0, 0, 0, 0);
      }
    }
  }
}

// this lane's query row tq (F32Tile::SCALE_Q: times the exact 2^-3; else as it stands, the scale follows the sum); rows >= N as zeros
template <int DH>
__device__ __forceinline__ void f32_load_query(const float* __restrict__ qkv, float (&qreg)[DH / 2], size_t tok0, int stride, int D, int hd,
                                               int tq, int N, int hh) {
  constexpr int QR = F32Tile<DH>::QR;
  const float* qp = qkv + (tok0 + (size_t)(tq < N ? tq : 0) * stride) * (3 * D) + hd * DH + QR * hh;
#pragma unroll
  for (int c = 0; c < QR; c += 4) {
    const float4 v = (tq < N) ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
    if constexpr (F32Tile<DH>::SCALE_Q) {
      qreg[c] = v.x * 0.125f; qreg[c + 1] = v.y * 0.125f; qreg[c + 2] = v.z * 0.125f; qreg[c + 3] = v.w * 0.125f;
    } else {
      qreg[c] = v.x; qreg[c + 1] = v.y; qreg[c + 2] = v.z; qreg[c + 3] = v.w;
    }
  }
}

// Where a key tile stands in its unit: its global index, whether it is the unit's last -- the only one that can hold keys >= N -- and
// the unit's key count.  One value per tile, handed to every piece that looks at the tile.
struct F32KeyTile {
  int gt;
  bool last;
  int N;
};

// the scaled scores of a tile of sums over d (the product rounded; widths that scale q: the sums as they are), keys >= N at -inf
template <int DH>
__device__ __forceinline__ f32x16 f32_finish_scores(f32x16 s, const F32KeyTile& at, int hh) {
  if constexpr (!F32Tile<DH>::SCALE_Q) {
    const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = mul_rounded(s[q], scale);
  }
  if (at.last) {
#pragma unroll
    for (int q = 0; q < 16; ++q)
      if (f32_key(at.gt, q, hh) >= at.N) s[q] = -INFINITY;
  }
  return s;
}

// S^T tile kt of the staged rows as the softmax holds it: rows = keys f32_key(at.gt, q, hh), column = this lane's query.  What it
// holds depends on the width alone: the finished scores (f32_finish_scores) -- at width 32 (EXP_FMA_FRONT) the bare sums over d, which
// f32_tile_max and f32_exp_tile finish, each under ONE branch on at.last (a streaming kernel, where at.last is a run-time value,
// takes one wave-uniform branch per tile and pass).
template <int DH>
__device__ __forceinline__ f32x16 f32_score_tile(const float* Ks, const float (&qreg)[DH / 2], int kt, const F32KeyTile& at, int r, int hh) {
  using Tl = F32Tile<DH>;
  f32x16 s;
#pragma unroll
  for (int q = 0; q < 16; ++q) s[q] = 0.f;
  const float* kp = &Ks[(kt * 32 + r) * Tl::K_LD + Tl::QR * hh];
#pragma unroll
  for (int u = 0; u < Tl::QR / 4; ++u) {
    const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * u);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[4 * u + 0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[4 * u + 1], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[4 * u + 2], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[4 * u + 3], s, 0, 0, 0);
  }
  if constexpr (Tl::EXP_FMA_FRONT)
    return s;
  else
    return f32_finish_scores<DH>(s, at, hh);
}

// the running maximum over a tile of f32_score_tile, registers ascending (at width 32: of the rounded product)
template <int DH>
__device__ __forceinline__ float f32_tile_max(const f32x16& s, const F32KeyTile& at, int hh, float m) {
  if (F32Tile<DH>::EXP_FMA_FRONT && at.last) {
    const f32x16 t = f32_finish_scores<DH>(s, at, hh);
#pragma unroll
    for (int q = 0; q < 16; ++q) m = fmaxf(m, t[q]);
  } else if (F32Tile<DH>::EXP_FMA_FRONT) {
    const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
    for (int q = 0; q < 16; ++q) m = fmaxf(m, mul_rounded(s[q], scale));
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) m = fmaxf(m, s[q]);
  }
  return m;
}

// the numerators of a tile of f32_score_tile, in place
template <int DH>
__device__ __forceinline__ void f32_exp_tile(f32x16& s, const F32KeyTile& at, int hh, float m) {
  if (F32Tile<DH>::EXP_FMA_FRONT && at.last) {
    s = f32_finish_scores<DH>(s, at, hh);
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = expf(s[q] - m);
  } else if (F32Tile<DH>::EXP_FMA_FRONT) {
    const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = expf(fmaf(s[q], scale, -m));
  } else {
#pragma unroll
    for (int q = 0; q < 16; ++q) s[q] = expf(s[q] - m);
  }
}

// l += the numerators of a tile, registers ascending
__device__ __forceinline__ void f32_sum_tile(const f32x16& e, float& l) {
#pragma unroll
  for (int q = 0; q < 16; ++q) l += e[q];
}

// P = e / l in place (the widths that normalise before the second product)
__device__ __forceinline__ void f32_normalise_tile(f32x16& e, float l) {
#pragma unroll
  for (int q = 0; q < 16; ++q) e[q] = e[q] / l;
}

// attn - I inside P (S2S:82-83): - 1 where the key of global tile gt is the lane's query
__device__ __forceinline__ void f32_sub_diag_tile(f32x16& p, int gt, int tq, int hh) {
#pragma unroll
  for (int q = 0; q < 16; ++q)
    if (f32_key(gt, q, hh) == tq) p[q] -= 1.0f;
}

// O^T[d][query] += sum over the keys of staged tile kt of V[key][d] * p[key][query]; B operand = the accumulator registers as they stand
template <int DH>
__device__ __forceinline__ void f32_pv_tile(const float* Vs, const f32x16& p, f32x16 (&oacc)[F32Tile<DH>::NDT], int kt, int r, int hh) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float* vp = &Vs[f32_key(kt, q, hh) * F32Tile<DH>::V_LD + r];
#pragma unroll
    for (int dt = 0; dt < F32Tile<DH>::NDT; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * dt], p[q], oacc[dt], 0, 0, 0);
  }
}

template <int DH>
__device__ __forceinline__ void f32_zero_acc(f32x16 (&oacc)[F32Tile<DH>::NDT]) {
#pragma unroll
  for (int dt = 0; dt < F32Tile<DH>::NDT; ++dt)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[dt][q] = 0.f;
}

// rows d = 32 dt + (reg & 3) + 8 (reg >> 2) + 4 hh of this lane's query column, token tok: / l where F32Tile::NORM_AT_STORE, - v[query]
// where sub_v (the diagonal that is not in P), once; columns >= DH are neither read nor stored
template <int DH>
__device__ __forceinline__ void f32_store_query(const float* __restrict__ qkv, float* __restrict__ out, const f32x16 (&oacc)[F32Tile<DH>::NDT], float l,
                                                size_t tok, int D, int hd, int hh, bool sub_v) {
  const float* vq = qkv + tok * (3 * D) + 2 * D + hd * DH;
  float* op = out + tok * D + hd * DH;
#pragma unroll
  for (int dt = 0; dt < F32Tile<DH>::NDT; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      if (32 * dt + 8 * g4 >= DH) continue;   // (width 48: rows 48 .. 63 of the second tile are no columns of the head, width 16: rows 16 .. 31 of the one; DH % 8 == 0)
      const int col = 32 * dt + 8 * g4 + 4 * hh;
      float4 o = make_float4(oacc[dt][4 * g4], oacc[dt][4 * g4 + 1], oacc[dt][4 * g4 + 2], oacc[dt][4 * g4 + 3]);
      if constexpr (F32Tile<DH>::NORM_AT_STORE) { o.x = o.x / l; o.y = o.y / l; o.z = o.z / l; o.w = o.w / l; }
      if (sub_v) {
        const float4 v = *reinterpret_cast<const float4*>(vq + col);
        o.x -= v.x; o.y -= v.y; o.z -= v.z; o.w -= v.w;
      }
      *reinterpret_cast<float4*>(op + col) = o;
    }
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
// Resident kernels: one workgroup of NKT = ceil(N / 32) <= MAXNKT waves per unit.  launch(std::integral_constant<int, NKT>) launches
// the instantiation.
template <int MAXNKT, int NKT = 1, class F>
hipError_t f32_resident_ladder(int N, F&& launch) {
  if constexpr (NKT == MAXNKT)
    return launch(std::integral_constant<int, NKT>{});
  else
    return (N + 31) / 32 <= NKT ? launch(std::integral_constant<int, NKT>{}) : f32_resident_ladder<MAXNKT, NKT + 1>(N, launch);
}

// Streaming kernels: one workgroup per (unit, query block); the T queries of a unit are cut into ceil(T / 256) balanced blocks of whole
// waves of 32 queries, at most 8 (T = 300: two blocks of 160; T = 513: three of 192).  blockDim = 64 x that wave count is a run-time
// value, the staging loops stride by it.  Refuses B J H ceil(T / 256) workgroups beyond 2^31 - 1.
inline int f32_stream_query_blocks(int T) { return (T + 255) / 256; }
inline int f32_stream_block_waves(int T) {
  const int nqb = f32_stream_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}
template <auto Kfn, int DH>
hipError_t f32_launch_stream(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  const int nqb = f32_stream_query_blocks(T), waves = f32_stream_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = F32Tile<DH>::lds_bytes(F32Tile<DH>::STREAM_KC);   // K and V of one chunk
  return launch_lds<Kfn>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, qkv, out, T, J, H, D, nqb);
}

// ---- the three-pass key-streaming walk of the widths that normalise before the second product (32 and 64) -----------------------------
// Instantiated and launched by kernels_attn_f32_long.hip (DH = 64) and kernels_attn_f32_h32_long.hip (DH = 32); described there.
template <int DH>
__global__ __launch_bounds__(512) void k_attn_f32_stream3(const float* __restrict__ qkv, float* __restrict__ out, int T, int J, int H,
                                                          int D, int nqb) {
  using Tl = F32Tile<DH>;
  static_assert(!Tl::NORM_AT_STORE, "the three-pass walk is the one of the widths that normalise before the second product");
  constexpr int KC = Tl::STREAM_KC, CH = 32 * KC;   // key tiles / keys per chunk
  extern __shared__ __attribute__((aligned(16))) float lds_f32l[];
  float* const Ks = lds_f32l;                   // [CH][K_LD]
  float* const Vs = lds_f32l + CH * Tl::K_LD;   // [CH][V_LD]
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);   // unit = (b*J + j)*H + h
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;
  const bool late_diag = !Tl::DIAG_IN_P_RESIDENT || nchunks > 1;   // - v[query] at the store instead of - 1 in P (block-uniform)

  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  float qreg[Tl::QR];
  f32_load_query<DH>(qkv, qreg, tok0, J, D, hd, tq, T, hh);

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    f32_stage_rows<DH, false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const F32KeyTile at{c * KC + kt, c * KC + kt == ntiles - 1, T};
      m = f32_tile_max<DH>(f32_score_tile<DH>(Ks, qreg, kt, at, r, hh), at, hh, m);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---- pass 2: the sum of the numerators, key tiles ascending, registers ascending
  float l = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    f32_stage_rows<DH, false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const F32KeyTile at{c * KC + kt, c * KC + kt == ntiles - 1, T};
      f32x16 sacc = f32_score_tile<DH>(Ks, qreg, kt, at, r, hh);
      f32_exp_tile<DH>(sacc, at, hh, m);
      f32_sum_tile(sacc, l);
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);

  // ---- pass 3: P^T = softmax (- I), O^T[d][query] = sum_key V[key][d] * P^T[key][query]
  f32x16 oacc[Tl::NDT];
  f32_zero_acc<DH>(oacc);
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    f32_stage_rows<DH, true>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const F32KeyTile at{c * KC + kt, c * KC + kt == ntiles - 1, T};
      f32x16 sacc = f32_score_tile<DH>(Ks, qreg, kt, at, r, hh);
      f32_exp_tile<DH>(sacc, at, hh, m);
      f32_normalise_tile(sacc, l);
      if (!late_diag) f32_sub_diag_tile(sacc, at.gt, tq, hh);
      f32_pv_tile<DH>(Vs, sacc, oacc, kt, r, hh);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }

  if (tq < T) f32_store_query<DH>(qkv, out, oacc, l, tok0 + (size_t)tq * J, D, hd, hh, late_diag);
}

}  // namespace d3d
