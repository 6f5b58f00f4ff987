// Temporal GRAND attention in exact fp32 on the matrix pipe for windows of ANY length: the keys stream through LDS in chunks of 256
// frames instead of all living there (kernels_attn.hip k_attn_temporal_f32<NKT>: K and V of T <= 256 rows = 132 of the 160 KiB).
//
// The arithmetic is that of k_attn_temporal_f32<NKT>: v_mfma_f32_32x32x2_f32 on swapped operands, S^T = K Q'^T with q' = q * 0.125, a
// lane holds one query column; the exact max-subtracted softmax, NORMALISED BEFORE the second product (pv = e / l, - 1 on the diagonal,
// then O^T += V^T P^T).  An order-preserving streaming form of that needs l before the first V product, so three passes over the keys:
//
//   pass 1   per chunk: stage K; per key tile the 32 MFMAs of S^T, keys >= T at -inf, running fmaxf in register order; cross-half shuffle
//   pass 2   per chunk: stage K; the SAME 32 MFMAs again (same bits), e = expf(s - m), l += e with key tiles and registers ascending;
//            cross-half add
//   pass 3   per chunk: stage K and V; the same MFMAs a third time, pv = expf(s - m) / l, - 1 where the global key index is the lane's
//            query, the 16 x 2 MFMAs of O^T per tile in the resident kernel's order (oacc[0] then oacc[1] per register)
//
// So every expf sees the same m, l is summed in the same order and oacc takes the same MFMAs in the same order as in the resident
// kernel: for T <= 256 the output is bit-identical to launch_attn_temporal_f32 (tests/test_gpu_long_temporal_f32.py).  The price is the
// scores computed three times, 128 instead of 64 MFMAs per 32 x 32 tile (and expf twice); one score tile (16 registers) is live at a
// time.
//
// The - 1 of the diagonal, T > 256 (no resident kernel to agree with): once - v[query] is in the accumulator it stands at |v| instead of
// |sum p v| << |v|, and every product behind it is rounded to an ulp of |v| -- an error that grows with the keys still to come (T = 769,
// hashed inputs at scale 2.0: 6.4e-6 against fp64 where plain fp32 math loses 3.1e-6; tests/test_gpu_group_lengths.py).  There the
// products are summed without it and v[query] is subtracted once, at the store.
//
// One workgroup per (batch, joint, head, query block): the T queries of a unit are cut into ceil(T / 256) balanced blocks of at most
// 8 waves of 32 queries (T = 300: two blocks of 160; T = 513: three of 192), blockDim = 64 x that wave count -- a run-time value, the
// staging loops stride by it.  Staging is the resident kernel's: through registers, all global loads of a batch issued before its LDS
// writes; no LDS-DMA, no counters, no persistent walk.  K rows are padded to 68 floats (272-B rows: the ds_read_b128 of 16 consecutive
// keys is conflict-free), V rows are 64 floats: a chunk is 69 632 + 65 536 B = 132 KiB, the resident kernel's footprint at NKT = 8.
// Every wave executes every barrier: the chunk and key-tile trip counts depend on T alone, a wave whose queries are all >= T stages
// and synchronises and only skips its stores.
// Row isolation: keys >= T score -inf (their e is an exact 0) and their K / V rows are staged as zeros, never left over from the
// previous chunk: 0 x NaN cannot enter a clean row.  Rows >= T are never stored.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int LDH = 64;             // head width
constexpr int K_LD = 68, V_LD = 64; // LDS row strides in floats (as in kernels_attn.hip)
constexpr int KC = 8, CH = 32 * KC; // key tiles / keys per chunk

// Rows [row0, row0 + 32 nkt) of the unit's K (and V) into LDS rows [0, 32 nkt); rows >= T as zeros.  Four 16-byte slots per thread and
// batch, all of a batch's global loads issued before its LDS writes.
template <bool WITH_V>
__device__ __forceinline__ void stage_chunk(const float* __restrict__ qkv, float* Ks, float* Vs, size_t tok0, int J, int D, int hd,
                                            int row0, int nkt, int T, int tid, int nthr) {
  constexpr int NIT = 4;
  const int slots = nkt * 32 * 16;
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    float4 kk[NIT], vv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 4, c4 = idx & 15;
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
      const int row = idx >> 4, c4 = idx & 15;
      if (idx < slots) {
        *reinterpret_cast<float4*>(&Ks[row * K_LD + c4 * 4]) = kk[it];
        if (WITH_V) *reinterpret_cast<float4*>(&Vs[row * V_LD + c4 * 4]) = vv[it];
      }
    }
  }
}

}  // namespace

__global__ __launch_bounds__(512) void k_attn_temporal_f32l(const float* __restrict__ qkv, float* __restrict__ out, int T, int J, int H,
                                                            int D, int nqb) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32l[];
  float* const Ks = lds_f32l;                 // [CH][K_LD]
  float* const Vs = lds_f32l + CH * K_LD;     // [CH][V_LD]
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
  const bool late_diag = nchunks > 1;                 // T > 256: - v[query] at the store instead of - 1 in P (block-uniform)

  // this lane's query row, pre-scaled by dh^-0.5 = 2^-3 (exact): lane half hh holds d in [32hh, 32hh+32)
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  float qreg[32];
  {
    const float* qp = qkv + (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * LDH + 32 * hh;
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
      float4 v = (tq < T) ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
      qreg[c] = v.x * 0.125f; qreg[c + 1] = v.y * 0.125f; qreg[c + 2] = v.z * 0.125f; qreg[c + 3] = v.w * 0.125f;
    }
  }

  // S^T tile kt of the staged chunk (rows = keys (reg&3) + 8*(reg>>2) + 4*hh of the tile, column = query tq), keys >= T at -inf.  Only
  // the unit's last key tile (gt == ntiles - 1) can hold such keys.
  auto score_tile = [&](int kt, int gt) -> f32x16 {
    f32x16 sacc;
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[q] = 0.f;
    const float* kp = &Ks[(kt * 32 + r) * K_LD + 32 * hh];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * u);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[4 * u + 0], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[4 * u + 1], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[4 * u + 2], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[4 * u + 3], sacc, 0, 0, 0);
    }
    if (gt == ntiles - 1) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int key = gt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
        if (key >= T) sacc[q] = -INFINITY;
      }
    }
    return sacc;
  };

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) m = fmaxf(m, sacc[q]);
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
      const f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float e = expf(sacc[q] - m);
        l += e;
      }
    }
    __syncthreads();
  }
  l += __shfl_xor(l, 32, 64);

  // ---- pass 3: P^T = softmax - I, O^T[d][query] = sum_key V[key][d] * P^T[key][query]; B operand = the accumulator registers as they stand
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<true>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int lkey = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;   // row of the chunk
        const float e = expf(sacc[q] - m);
        float pv = e / l;
        if (!late_diag && c * CH + lkey == tq) pv -= 1.0f;   // attn - I (S2S:82-83)
        sacc[q] = pv;
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int lkey = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
        const float v0 = Vs[lkey * V_LD + r];
        const float v1 = Vs[lkey * V_LD + 32 + r];
        oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(v0, sacc[q], oacc[0], 0, 0, 0);
        oacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(v1, sacc[q], oacc[1], 0, 0, 0);
      }
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }

  if (tq < T) {
    const size_t oo = (tok0 + (size_t)tq * J) * D + hd * LDH;
    const float* vq = qkv + (tok0 + (size_t)tq * J) * D3 + 2 * D + hd * LDH;   // this query's own v row: the columns the lane stores
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int col = dt * 32 + 8 * g4 + 4 * hh;
        float4 o = make_float4(oacc[dt][4 * g4], oacc[dt][4 * g4 + 1], oacc[dt][4 * g4 + 2], oacc[dt][4 * g4 + 3]);
        if (late_diag) {
          const float4 v = *reinterpret_cast<const float4*>(vq + col);
          o.x -= v.x; o.y -= v.y; o.z -= v.z; o.w -= v.w;
        }
        *reinterpret_cast<float4*>(out + oo + col) = o;
      }
  }
}

// the query blocks of a unit: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int long_query_blocks(int T) { return (T + 255) / 256; }
static int long_block_waves(int T) {
  const int nqb = long_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_temporal_f32_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && D == H * LDH;
}

hipError_t launch_attn_temporal_f32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const int nqb = long_query_blocks(T), waves = long_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)CH * (K_LD + V_LD) * sizeof(float);   // K and V of one chunk
  return launch_lds<k_attn_temporal_f32l>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, qkv, out, T, J, H, D, nqb);
}

}  // namespace d3d
