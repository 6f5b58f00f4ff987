// GRAND attention cores in exact fp32 on the matrix pipe for heads of 128 columns (D == 128 H: embed_dim 1024 with the runner's 8 heads):
//   O = (softmax(q k^T / sqrt(128)) - I) v,   packed fp32 qkv rows in, fp32 rows out, no pair-layout form (only FP32 engines take these
// kernels; option "attn_f32_h128").  The structure is that of kernels_attn_f32_h32.hip and kernels_attn_f32_long.hip: compiler-scheduled,
// staged through registers, builtins only -- no inline assembly, no LDS-DMA, no persistent walk.
//
//   resident   k_attn_f32_h128<NKT>, one workgroup of NKT waves per (group, head), groups of N <= 32 NKT <= 128 tokens `stride` tokens
//              apart: temporal blocks (B, T, J), spatial blocks (B T, J, 1) -- any joint count 1 .. 128.  The scores are computed once
//              and kept in registers.
//   streaming  k_attn_f32_h128_stream, any T >= 1: the keys pass through LDS in chunks of 128 frames (KC = 4 key tiles); one workgroup
//              per (batch, joint, head, query block), ceil(T / 256) balanced query blocks of at most 8 waves of 32 queries, blockDim = 64 x
//              that wave count, a run-time value the staging loops stride by (launch_attn_temporal_f32_long's geometry).
//
// One order of additions serves both, every step of it one device function of this file, so that for T <= 128 the streaming kernel
// gives the resident kernel's bits (tests/test_gpu_attn_f32_h128.py):
//   scores     v_mfma_f32_32x32x2_f32 on swapped operands, S^T = K Q^T, one query column per lane: lane (r, hh) holds d in
//              [64 hh, 64 hh + 64) of query row r of its wave in 64 registers; a 32 x 32 score tile is 64 MFMAs, 16 ds_read_b128 of K each
//              feeding 4 of them, d ascending -- each MFMA adds the pair (d, d + 64).
//   scale      128^-1/2 is no power of two: scaling q by it would round every operand of the dot product.  The sums are multiplied by
//              1.0f / sqrtf(128.0f) AFTER the sum over d, k_attn_generic's constant and the reference's order ((q k^T) * scale).  The
//              product is kept from contraction (mul_rounded): "s * scale - m" as one fma in one kernel and two roundings in the other is
//              what kernels_attn_f32_h32_long.hip had to spell out per tile; here neither kernel ever has the fused form.
//   softmax    exact, two passes: keys >= N score -inf, m = the maximum over all keys (registers, then one cross-half shuffle), e =
//              expf(s - m), l = the sum of e per lane in key order (key tiles ascending, registers ascending), then one cross-half add.
//   product    P is NOT normalised before the second product (the narrower fp32 kernels divide first because their 64-wide twin
//              does; no twin's bits exist to keep at this width): O^T[d][query] += V^T E^T with the unnormalised e straight from the
//              accumulator registers as the B operand, into four 32 x 32 accumulator tiles, one per 32-column quarter of the head: 64
//              MFMAs per key tile, keys ascending.  The streaming kernel therefore needs two passes over the keys, not three: pass 1
//              stages K chunk by chunk for m; pass 2 stages K and V, recomputes each score tile with the same MFMAs (the same bits), and
//              runs e, l += e and the PV MFMAs per tile in the resident kernel's order.
//   store      out = oacc / l - v[query]: the - I is not put into P (with e[query] - l inside the product the accumulator would stand at
//              |v| l for the rest of the key walk and every later product be rounded to an ulp of that: kernels_attn_f32_long.hip); it is
//              subtracted once, here.
//
// LDS: K rows padded to 132 floats (528 B), V rows 128 floats: 16 896 + 16 384 = 33 280 B per key tile, 133 120 B per chunk of the
// streaming kernel and per group of the resident one at NKT = 4 -- under 160 KiB, one workgroup per CU there; the launches go through
// launch_lds.  Banks of the K fragment read (ds_read_b128, bank = (a / 4) mod 64, served in four groups of 16 lanes: lanes {0-3, 12-15,
// 20-27}, {4-11, 16-19, 28-31} and the same + 32; kernels_attn_f32_h32.hip): lane (r, hh) reads dword 132 r + 64 hh + 4 u.  Within a group
// hh and u are constant and 64 hh = 0 mod 64, so the 16-byte slot of a lane is (33 r + const) mod 16 = (r + const) mod 16; the 16 rows
// of either group are distinct mod 16 ({0-3, 12-15, 4-11} and {4-11, 0-3, 12-15}), so the 16 lanes cover the 16 four-bank slots once:
// conflict-free.  (Unpadded 128-float rows would put all 16 lanes on one slot.)  The V read is a ds_read_b32 of dword 128 key + 32 dt + r
// with key and dt uniform over a 32-lane half: bank r, conflict-free.  The staging writes are ds_write_b128 of 16 consecutive bytes per
// lane along a row.
//
// Every wave executes every barrier: the chunk and key-tile trip counts depend on T alone; a wave whose queries are all >= T stages and
// synchronises and only skips its stores.  All global loads of a staging batch are issued before its LDS writes.
// Row isolation: K / V rows >= N are staged as zeros -- in the streaming kernel in every chunk, never the previous chunk's bytes -- and
// their scores are -inf (e = 0 exactly), so 0 x NaN cannot enter a clean row.  Rows >= N are never stored.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DH = 128;                  // head width
constexpr int K_LD = 132, V_LD = 128;    // LDS row strides in floats
constexpr int KC = 4, CH = 32 * KC;      // key tiles / keys per chunk of the streaming kernel

// a * b rounded to fp32 whatever consumes it: never one half of a contracted fma
__device__ __forceinline__ float mul_rounded(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// Rows [row0, row0 + 32 nkt) of the unit's K (and V) into LDS rows [0, 32 nkt); rows >= N as zeros.  Four 16-byte slots per thread and
// batch (and array), all of a batch's global loads issued before its LDS writes.  token(row) = tok0 + row * stride.
template <bool WITH_V>
__device__ __forceinline__ void stage_rows(const float* __restrict__ qkv, float* Ks, float* Vs, size_t tok0, int stride, int D, int hd,
                                           int row0, int nkt, int N, int tid, int nthr) {
  constexpr int NIT = 4;
  const int slots = nkt * 32 * (DH / 4);
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    float4 kk[NIT], vv[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 5, c4 = idx & 31;
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
      const int row = idx >> 5, c4 = idx & 31;
      if (idx < slots) {
        *reinterpret_cast<float4*>(&Ks[row * K_LD + c4 * 4]) = kk[it];
        if (WITH_V) *reinterpret_cast<float4*>(&Vs[row * V_LD + c4 * 4]) = vv[it];
      }
    }
  }
}

// this lane's query row, as it stands (the scale follows the sum): lane half hh holds d in [64 hh, 64 hh + 64); rows >= N as zeros
__device__ __forceinline__ void load_query(const float* __restrict__ qkv, float (&qreg)[64], size_t tok0, int stride, int D, int hd, int tq,
                                           int N, int hh) {
  const float* qp = qkv + (tok0 + (size_t)(tq < N ? tq : 0) * stride) * (3 * D) + hd * DH + 64 * hh;
#pragma unroll
  for (int c = 0; c < 64; c += 4) {
    const float4 v = (tq < N) ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
    qreg[c] = v.x; qreg[c + 1] = v.y; qreg[c + 2] = v.z; qreg[c + 3] = v.w;
  }
}

// The scaled scores of S^T tile kt of the staged rows, global key tile gt of ntiles: rows = keys 32 gt + (reg&3) + 8*(reg>>2) + 4*hh,
// column = this lane's query (C/D map of the 32x32 MFMA).  Keys >= N, which only the unit's last key tile can hold, at -inf.
__device__ __forceinline__ f32x16 score_tile(const float* Ks, const float (&qreg)[64], int kt, int gt, int ntiles, int N, int r, int hh) {
  f32x16 sacc;
#pragma unroll
  for (int q = 0; q < 16; ++q) sacc[q] = 0.f;
  const float* kp = &Ks[(kt * 32 + r) * K_LD + 64 * hh];
#pragma unroll
  for (int u = 0; u < 16; ++u) {
    const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * u);
    sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[4 * u + 0], sacc, 0, 0, 0);
    sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[4 * u + 1], sacc, 0, 0, 0);
    sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[4 * u + 2], sacc, 0, 0, 0);
    sacc = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[4 * u + 3], sacc, 0, 0, 0);
  }
  const float scale = 1.0f / sqrtf((float)DH);
#pragma unroll
  for (int q = 0; q < 16; ++q) sacc[q] = mul_rounded(sacc[q], scale);
  if (gt == ntiles - 1) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int key = gt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
      if (key >= N) sacc[q] = -INFINITY;
    }
  }
  return sacc;
}

__device__ __forceinline__ float tile_max(const f32x16& sacc, float m) {
#pragma unroll
  for (int q = 0; q < 16; ++q) m = fmaxf(m, sacc[q]);
  return m;
}

// the numerators of a score tile in place, added to l in register order
__device__ __forceinline__ void exp_tile(f32x16& sacc, float m, float& l) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float e = expf(sacc[q] - m);
    sacc[q] = e;
    l += e;
  }
}

// O^T[d][query] += sum over the keys of staged tile kt of V[key][d] * e[key][query]; B operand = the accumulator registers as they stand
__device__ __forceinline__ void pv_tile(const float* Vs, const f32x16& e, f32x16 (&oacc)[4], int kt, int r, int hh) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float* vp = &Vs[(kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * V_LD + r];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(vp[32 * dt], e[q], oacc[dt], 0, 0, 0);
  }
}

// rows d = 32 dt + (reg&3) + 8*(reg>>2) + 4*hh of this lane's query column: the division by l and the - v[query] of the diagonal, once
__device__ __forceinline__ void store_query(const float* __restrict__ qkv, float* __restrict__ out, const f32x16 (&oacc)[4], float l,
                                            size_t tok, int D, int hd, int hh) {
  const float* vq = qkv + tok * (3 * D) + 2 * D + hd * DH;
  float* op = out + tok * D + hd * DH;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int col = 32 * dt + 8 * g4 + 4 * hh;
      const float4 v = *reinterpret_cast<const float4*>(vq + col);
      *reinterpret_cast<float4*>(op + col) = make_float4(oacc[dt][4 * g4] / l - v.x, oacc[dt][4 * g4 + 1] / l - v.y,
                                                         oacc[dt][4 * g4 + 2] / l - v.z, oacc[dt][4 * g4 + 3] / l - v.w);
    }
}

}  // namespace

// =============================================================================================== resident
// groups: G of N tokens `stride` apart; unit = (g * H + h), group g = (g / stride, g % stride): tok0 = (g / stride) * N * stride + g % stride
template <int NKT>
__global__ __launch_bounds__(64 * NKT) void k_attn_f32_h128(const float* __restrict__ qkv, float* __restrict__ out, int N, int stride,
                                                            int H, int D) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32h128[];
  constexpr int TP = 32 * NKT;
  float* const Ks = lds_f32h128;               // [TP][K_LD]
  float* const Vs = lds_f32h128 + TP * K_LD;   // [TP][V_LD]

  const int unit = blockIdx.x;
  const int hd = unit % H;
  const int g = unit / H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)(g / stride) * N * stride + g % stride;   // token(t) = tok0 + t * stride

  stage_rows<true>(qkv, Ks, Vs, tok0, stride, D, hd, 0, NKT, N, tid, 64 * NKT);
  const int tq = 32 * wave + r;
  float qreg[64];
  load_query(qkv, qreg, tok0, stride, D, hd, tq, N, hh);
  __syncthreads();

  f32x16 sacc[NKT];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    sacc[kt] = score_tile(Ks, qreg, kt, kt, NKT, N, r, hh);
    m = tile_max(sacc[kt], m);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  float l = 0.f;
  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[dt][q] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    exp_tile(sacc[kt], m, l);
    pv_tile(Vs, sacc[kt], oacc, kt, r, hh);
  }
  l += __shfl_xor(l, 32, 64);

  if (tq < N) store_query(qkv, out, oacc, l, tok0 + (size_t)tq * stride, D, hd, hh);
}

bool attn_f32_h128_ok(int N, int D, int H) { return N >= 1 && N <= 128 && H > 0 && D == H * DH; }

template <int NKT>
static hipError_t launch_h128_nkt(const float* qkv, float* out, long long units, int N, int stride, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)32 * NKT * (K_LD + V_LD) * sizeof(float);
  return launch_lds<k_attn_f32_h128<NKT>>(dim3((unsigned)units), dim3(64 * NKT), lds_bytes, s, qkv, out, N, stride, H, D);
}

// groups as launch_attn_x3_h128: B * J of them, T tokens each, J tokens apart
hipError_t launch_attn_f32_h128(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_h128_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  switch ((T + 31) / 32) {
    case 1: return launch_h128_nkt<1>(qkv, out, units, T, J, D, H, s);
    case 2: return launch_h128_nkt<2>(qkv, out, units, T, J, D, H, s);
    case 3: return launch_h128_nkt<3>(qkv, out, units, T, J, D, H, s);
    default: return launch_h128_nkt<4>(qkv, out, units, T, J, D, H, s);
  }
}

// =============================================================================================== streaming
__global__ __launch_bounds__(512) void k_attn_f32_h128_stream(const float* __restrict__ qkv, float* __restrict__ out, int T, int J, int H,
                                                              int D, int nqb) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32h128s[];
  float* const Ks = lds_f32h128s;                 // [CH][K_LD]
  float* const Vs = lds_f32h128s + CH * K_LD;     // [CH][V_LD]
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

  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  float qreg[64];
  load_query(qkv, qreg, tok0, J, D, hd, tq, T, hh);

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_rows<false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) m = tile_max(score_tile(Ks, qreg, kt, c * KC + kt, ntiles, T, r, hh), m);
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---- pass 2: the same scores again (same MFMAs, same bits), their numerators, l and O^T per key tile in the resident kernel's order
  float l = 0.f;
  f32x16 oacc[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[dt][q] = 0.f;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_rows<true>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(Ks, qreg, kt, c * KC + kt, ntiles, T, r, hh);
      exp_tile(sacc, m, l);
      pv_tile(Vs, sacc, oacc, kt, r, hh);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l += __shfl_xor(l, 32, 64);

  if (tq < T) store_query(qkv, out, oacc, l, tok0 + (size_t)tq * J, D, hd, hh);
}

// the query blocks of a unit, as in kernels_attn_f32_long.hip: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int h128_query_blocks(int T) { return (T + 255) / 256; }
static int h128_block_waves(int T) {
  const int nqb = h128_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_f32_h128_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && D == H * DH;
}

hipError_t launch_attn_f32_h128_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_h128_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const int nqb = h128_query_blocks(T), waves = h128_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)CH * (K_LD + V_LD) * sizeof(float);   // K and V of one chunk
  return launch_lds<k_attn_f32_h128_stream>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, qkv, out, T, J, H, D, nqb);
}

}  // namespace d3d
