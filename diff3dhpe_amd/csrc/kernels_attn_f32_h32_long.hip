// Temporal GRAND attention in exact fp32 on the matrix pipe for heads of 32 columns and windows of ANY length:
// k_attn_temporal_f32_h32<NKT>'s arithmetic (kernels_attn_f32_h32.hip) inside k_attn_temporal_f32l's three-pass key-streaming walk
// (kernels_attn_f32_long.hip).  The keys stream through LDS in chunks of 256 frames instead of all living there.
//
// v_mfma_f32_32x32x2_f32 on swapped operands, S^T = K Q^T: lane (r, hh) holds d in [16 hh, 16 hh + 16) of query row r of its wave, 16
// MFMAs per 32 x 32 score tile; the scale 1.0f / sqrtf(32.0f) follows the sum over d; the exact max-subtracted softmax, NORMALISED
// BEFORE the second product, which needs l before the first V product, so three passes over the keys:
//
//   pass 1   per chunk: stage K; per key tile the 16 MFMAs of S^T, s * scale, keys >= T at -inf, running fmaxf in register order;
//            cross-half shuffle
//   pass 2   per chunk: stage K; the SAME 16 MFMAs again (same bits), e = expf(s * scale - m), l += e with key tiles and registers
//            ascending; cross-half add
//   pass 3   per chunk: stage K and V; the same MFMAs a third time, p = expf(s * scale - m) / l, the 16 MFMAs of O^T per tile into ONE
//            32 x 32 accumulator in the resident kernel's order
//   O = O^T - v[query]: subtracted once, at the store; the - 1 of the diagonal never enters P (as in the resident kernel)
//
// Bit identity with launch_attn_temporal_f32_h32 for T <= 256 (tests/test_gpu_long_f32_h32.py) needs every expf to see the argument
// the resident kernel gives it, and there "s * scale - m" is two different roundings: the compiler contracts it into ONE fma(s, scale,
// -m) in every key tile but the last, where the -inf select of the key mask stands between the product and the difference and the
// product is rounded first (the maximum takes the rounded product everywhere).  What is implicit there is spelled out here -- fmaf in
// the tiles in front of the unit's last, a product kept from contraction and a subtraction in the last -- because in a loop over key
// tiles the compiler would choose one form for all of them.
//
// The price is the scores computed three times, 64 instead of 32 MFMAs per 32 x 32 tile (and expf twice); one score tile (16
// registers) is live at a time.
//
// Launch geometry as the other long kernels: one workgroup per (batch, joint, head, query block), ceil(T / 256) balanced query blocks
// of at most 8 waves of 32 queries, blockDim = 64 x that wave count, a run-time value the staging loops stride by.  Staged through
// registers, all global loads of a batch issued before its LDS writes; no LDS-DMA, no inline assembly, no persistent walk.  K rows are
// padded to 36 floats (the conflict-free fragment read of kernels_attn_f32_h32.hip), V rows are 32 floats: a chunk is 36 864 + 32 768 =
// 69 632 B, two workgroups per CU by LDS.
// Every wave executes every barrier: the chunk and key-tile trip counts depend on T alone, a wave whose queries are all >= T stages
// and synchronises and only skips its stores.  Row isolation: keys >= T score -inf (their e is an exact 0) and their K / V rows are
// staged as zeros in every chunk, never left over from the previous one: 0 x NaN cannot enter a clean row.  Rows >= T are never stored.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LDH = 32;             // head width
constexpr int K_LD = 36, V_LD = 32; // LDS row strides in floats (as in kernels_attn_f32_h32.hip)
constexpr int KC = 8, CH = 32 * KC; // key tiles / keys per chunk

// a * b rounded to fp32 whatever consumes it: never one half of a contracted fma
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Rows [row0, row0 + 32 nkt) of the unit's K (and V) into LDS rows [0, 32 nkt); rows >= T as zeros.  Four 16-byte slots per thread and
// batch, all of a batch's global loads issued before its LDS writes.
template <bool WITH_V>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ qkv, float* Ks, float* Vs, size_t tok0, int J, int D, int hd,
                                            int row0, int nkt, int T, int tid, int nthr) {
  constexpr int NIT = 4;
  const int slots = nkt * 32 * 8;
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    float4 kk[NIT], vv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 3, c4 = idx & 7;
      kk[it] = make_float4(0, 0, 0, 0); vv[it] = kk[it];
      if (idx < slots && row0 + row < T) {
        const float* p = qkv + (tok0 + (size_t)(row0 + row) * J) * D3 + hd * LDH + c4 * 4;
        kk[it] = *reinterpret_cast<const float4*>(p + D);
        if (WITH_V) vv[it] = *reinterpret_cast<const float4*>(p + 2 * D);
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 3, c4 = idx & 7;
      if (idx < slots) {
        *reinterpret_cast<float4*>(&Ks[row * K_LD + c4 * 4]) = kk[it];
        if (WITH_V) *reinterpret_cast<float4*>(&Vs[row * V_LD + c4 * 4]) = vv[it];
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(512) void k_attn_temporal_f32l_h32(const float* __restrict__ qkv, float* __restrict__ out, int T, int J,
                                                                int H, int D, int nqb) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32lh32[];
  float* const Ks = lds_f32lh32;                 // [CH][K_LD]
  float* const Vs = lds_f32lh32 + CH * K_LD;     // [CH][V_LD]
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);   // unit = (b*J + j)*H + h
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // this lane's query row, as it stands (the scale follows the sum): lane half hh holds d in [16hh, 16hh+16)
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  float qreg[16];
  {
    const float* qp = qkv + (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * LDH + 16 * hh;
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
      const float4 v = (tq < T) ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
      qreg[c] = v.x; qreg[c + 1] = v.y; qreg[c + 2] = v.z; qreg[c + 3] = v.w;
    }
  }
  const float scale = 1.0f / sqrtf((float)LDH);

  // the sums over d of S^T tile kt of the staged chunk, unscaled: rows = keys (reg&3) + 8*(reg>>2) + 4*hh of the tile, column = query tq
  auto score_tile = [&](int kt) -> f32x16 {
    f32x16 sacc;
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[q] = 0.f;
    const float* kp = &Ks[(kt * 32 + r) * K_LD + 16 * hh];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * u);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[4 * u + 0], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[4 * u + 1], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[4 * u + 2], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[4 * u + 3], sacc, 0, 0, 0);
    }
    return sacc;
  };
  // the scaled score of register q of the unit's LAST key tile gt, the only one that can hold keys >= T: those at -inf
  auto last_score = [&](float s, int gt, int q) -> float {
    const int key = gt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
    return key >= T ? -INFINITY : mul_rounded(s, scale);
  };
  // the numerators of tile gt in place (see the head of the file for the two forms of the argument)
  auto exp_tile = [&](f32x16& sacc, int gt, float m) {
    if (gt == ntiles - 1) {
#pragma unroll
      for (int q = 0; q < 16; ++q) sacc[q] = expf(last_score(sacc[q], gt, q) - m);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) sacc[q] = expf(fmaf(sacc[q], scale, -m));
    }
  };

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const int gt = c * KC + kt;
      const f32x16 sacc = score_tile(kt);
      if (gt == ntiles - 1) {
#pragma unroll
        for (int q = 0; q < 16; ++q) m = fmaxf(m, last_score(sacc[q], gt, q));
      } else {
#pragma unroll
        for (int q = 0; q < 16; ++q) m = fmaxf(m, mul_rounded(sacc[q], scale));
      }
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---- pass 2: the sum of the numerators, key tiles ascending, registers ascending
  float l = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(kt);
      exp_tile(sacc, c * KC + kt, m);
#pragma unroll
      for (int q = 0; q < 16; ++q) l += sacc[q];
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);

  // ---- pass 3: P^T = softmax, O^T[d][query] = sum_key V[key][d] * P^T[key][query]; B operand = the accumulator registers as they stand
  f32x16 oacc;
#pragma unroll
  for (int q = 0; q < 16; ++q) oacc[q] = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<true>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(kt);
      exp_tile(sacc, c * KC + kt, m);
#pragma unroll
      for (int q = 0; q < 16; ++q) sacc[q] = sacc[q] / l;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int lkey = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;   // row of the chunk
        oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[lkey * V_LD + r], sacc[q], oacc, 0, 0, 0);
      }
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }

  // rows d = (reg&3) + 8*(reg>>2) + 4*hh of column tq; - v[query] of the diagonal here, once
  if (tq < T) {
    const size_t tok = tok0 + (size_t)tq * J;
    const float* vq = qkv + tok * D3 + 2 * D + hd * LDH;
    float* op = out + tok * D + hd * LDH;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int col = 8 * g4 + 4 * hh;
      const float4 v = *reinterpret_cast<const float4*>(vq + col);
      *reinterpret_cast<float4*>(op + col) =
          make_float4(oacc[4 * g4] - v.x, oacc[4 * g4 + 1] - v.y, oacc[4 * g4 + 2] - v.z, oacc[4 * g4 + 3] - v.w);
    }
  }
}

// the query blocks of a unit, as in kernels_attn_f32_long.hip: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int lh32_query_blocks(int T) { return (T + 255) / 256; }
static int lh32_block_waves(int T) {
  const int nqb = lh32_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_temporal_f32_h32_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && D == H * LDH;
}

hipError_t launch_attn_temporal_f32_h32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_h32_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const int nqb = lh32_query_blocks(T), waves = lh32_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)CH * (K_LD + V_LD) * sizeof(float);   // K and V of one chunk
  return launch_lds<k_attn_temporal_f32l_h32>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, qkv, out, T, J, H, D, nqb);
}

}  // namespace d3d
