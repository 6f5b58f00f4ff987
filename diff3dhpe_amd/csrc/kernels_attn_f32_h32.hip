// GRAND attention cores in exact fp32 for heads of 32 columns (D == 32 H: embed_dim 256 with the runner's 8 heads):
//   O = (softmax(q k^T / sqrt(32)) - I) v,   packed qkv rows in, fp32 rows out -- the contract of kernels_attn.hip without its pair-layout
// form (only FP32 engines take these kernels; option "attn_f32_h32").  The structure is that of the two 64-wide kernels there: compiler-
// scheduled (two scheduling fences, each explained where it stands, keep every instantiation free of spills), staged through registers,
// no LDS-DMA, no inline assembly, no persistent walk.
//
//   temporal  k_attn_temporal_f32_h32<NKT>, one workgroup of NKT waves per (batch, joint, head), T <= 32 NKT <= 256.
//             v_mfma_f32_32x32x2_f32 on swapped operands, S^T = K Q^T: lane (r, hh) holds d in [16 hh, 16 hh + 16) of query row r of its
//             wave, 16 MFMAs per 32 x 32 score tile; the exact two-pass softmax over the accumulator registers + one cross-half shuffle;
//             O^T[d][query] += V^T P^T straight from those registers into ONE 32 x 32 accumulator tile, 16 MFMAs per key tile.
//   spatial   k_attn_spatial_f32_h32<NJ>, NJ = 15, 16, 17: the VALU form of k_attn_spatial_f32 -- one lane owns one query row (q[32] in
//             registers), a wave runs 64 / NJ (frame, head) units, K then V of the unit staged in LDS and broadcast-read, lane-local softmax.
//
// The scale.  32^-1/2 is no power of two: scaling q by it would round every operand of the dot product.  The scores are multiplied by
// 1.0f / sqrtf(32.0f) AFTER the sum over d, k_attn_generic's constant and the reference's order ((q k^T) * scale).
// The diagonal.  The - I is not put into P: with p[query] - 1 inside the product the accumulator stands at |v| for the rest of the key
// walk and every later product is rounded to an ulp of |v| (kernels_attn_f32_long.hip; 4.56e-6 at N = 219 in the 64-wide resident kernel).
// These kernels have no twin whose bits they must keep: the products are summed alone and v[query] is subtracted once, at the store.
//
// LDS of the temporal kernel: K rows padded to 36 floats (144 B), V rows 32 floats; 4 608 + 4 096 B per key tile, 69 632 B at NKT = 8, so
// the launch goes through launch_lds.  Banks of the K fragment read (ds_read_b128, bank = (a / 4) mod 64, four groups of 16 lanes: lanes
// {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and the same + 32): lane (r, hh) reads dword 36 r + 16 hh + 4 u, bank 4 (9 r mod 16) + const
// within a group; r -> 9 r mod 16 is a bijection of r mod 16 and the 16 rows of either group are distinct mod 16 ({0-3, 12-15, 4-11} and
// {4-11, 0-3, 12-15}), so the 16 lanes cover the 16 four-bank slots once: conflict-free.  (Unpadded 32-float rows would put them on two
// slots, 8-way.)  The V read is a ds_read_b32 of dword 32 key + r with key uniform over a 32-lane half: bank r, conflict-free.
// LDS of the spatial kernel: a unit is NJ rows of 32 floats + 4 floats, so the 64 / NJ broadcast addresses of a wave (one per unit) fall
// into different four-bank slots (unit stride mod 64 dwords = 36, 4, 36 for NJ = 15, 16, 17).
//
// Row isolation: K / V rows >= T are staged as zeros and their scores set to -inf (e = 0 exactly), so 0 x NaN cannot enter a clean row;
// rows >= T (lanes without a unit) are never stored; every wave reaches every barrier.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int DH = 32;                 // head width
constexpr int K_LD = 36, V_LD = 32;    // LDS row strides of the temporal kernel, in floats

}  // namespace

// =============================================================================================== temporal (MFMA f32)
template <int NKT>
__global__ __launch_bounds__(64 * NKT) void k_attn_temporal_f32_h32(const float* __restrict__ qkv, float* __restrict__ out, int T, int J,
                                                                    int H, int D) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32h32[];
  constexpr int TP = 32 * NKT;
  float* const Ks = lds_f32h32;               // [TP][K_LD]
  float* const Vs = lds_f32h32 + TP * K_LD;   // [TP][V_LD]

  const int unit = blockIdx.x;     // (b*J + j)*H + h
  const int h = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;   // token(t) = tok0 + t*J

  // K and V rows [0, TP) of the unit, rows >= T as zeros: TP * 8 16-byte slots = 4 per thread, all global loads issued before the LDS writes
  {
    float4 kk[4], vv[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = tid + it * 64 * NKT;
      const int row = idx >> 3, c4 = idx & 7;
      kk[it] = make_float4(0, 0, 0, 0); vv[it] = kk[it];
      if (row < T) {
        const float* p = qkv + (tok0 + (size_t)row * J) * D3 + h * DH + c4 * 4;
        kk[it] = *reinterpret_cast<const float4*>(p + D);
        vv[it] = *reinterpret_cast<const float4*>(p + 2 * D);
      }
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int idx = tid + it * 64 * NKT;
      const int row = idx >> 3, c4 = idx & 7;
      *reinterpret_cast<float4*>(&Ks[row * K_LD + c4 * 4]) = kk[it];
      *reinterpret_cast<float4*>(&Vs[row * V_LD + c4 * 4]) = vv[it];
    }
  }

  // this lane's query row, as it stands (the scale follows the sum): lane half hh holds d in [16hh, 16hh+16)
  const int tq = 32 * wave + r;
  float qreg[16];
  {
    const float* qp = qkv + (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + h * DH + 16 * hh;
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
      const float4 v = (tq < T) ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
      qreg[c] = v.x; qreg[c + 1] = v.y; qreg[c + 2] = v.z; qreg[c + 3] = v.w;
    }
  }
  __syncthreads();

  // S^T tile kt: rows = keys kt*32 + (reg&3) + 8*(reg>>2) + 4*hh, column = query tq   (C/D map of the 32x32 MFMA)
  const float scale = 1.0f / sqrtf((float)DH);
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[kt][q] = 0.f;
    const float* kp = &Ks[(kt * 32 + r) * K_LD + 16 * hh];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const float4 k4 = *reinterpret_cast<const float4*>(kp + 4 * u);
      sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.x, qreg[4 * u + 0], sacc[kt], 0, 0, 0);
      sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.y, qreg[4 * u + 1], sacc[kt], 0, 0, 0);
      sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.z, qreg[4 * u + 2], sacc[kt], 0, 0, 0);
      sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x2f32(k4.w, qreg[4 * u + 3], sacc[kt], 0, 0, 0);
    }
  }

  // exact (max-subtracted, two-pass) softmax over the keys of this query column.  Keys >= T sit in the last key tile only: the launch
  // picks NKT = ceil(T / 32)
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int key = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
      const float sc = sacc[kt][q] * scale;
      sacc[kt][q] = (kt == NKT - 1 && key >= T) ? -INFINITY : sc;
      m = fmaxf(m, sacc[kt][q]);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float e = expf(sacc[kt][q] - m);
      sacc[kt][q] = e;
      l += e;
    }
    // one key tile per scheduling region: expf's range selects live in SGPR pairs, and a scheduler free to batch the compares of several
    // tiles runs out of them (SGPR spills at NKT = 5 and 8)
    __builtin_amdgcn_sched_barrier(0);
  }
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[kt][q] = sacc[kt][q] / l;

  // O^T[d][query] = sum_key V[key][d] * P^T[key][query]; B operand = the accumulator registers as they stand
  f32x16 oacc;
#pragma unroll
  for (int q = 0; q < 16; ++q) oacc[q] = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int key = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh;
      oacc = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[key * V_LD + r], sacc[kt][q], oacc, 0, 0, 0);
    }

  // rows d = (reg&3) + 8*(reg>>2) + 4*hh of column tq; - v[query] of the diagonal here, once
  if (tq < T) {
    const size_t tok = tok0 + (size_t)tq * J;
    const float* vq = qkv + tok * D3 + 2 * D + h * DH;
    float* op = out + tok * D + h * DH;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const int col = 8 * g4 + 4 * hh;
      const float4 v = *reinterpret_cast<const float4*>(vq + col);
      *reinterpret_cast<float4*>(op + col) =
          make_float4(oacc[4 * g4] - v.x, oacc[4 * g4 + 1] - v.y, oacc[4 * g4 + 2] - v.z, oacc[4 * g4 + 3] - v.w);
    }
  }
}

bool attn_temporal_f32_h32_ok(int T, int D, int H) { return T >= 1 && T <= 256 && H > 0 && D == H * DH; }

template <int NKT>
static hipError_t launch_temporal_h32_nkt(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)32 * NKT * (K_LD + V_LD) * sizeof(float);
  const long long grid = (long long)B * J * H;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_temporal_f32_h32<NKT>>(dim3((unsigned)grid), dim3(64 * NKT), lds_bytes, s, qkv, out, T, J, H, D);
}

hipError_t launch_attn_temporal_f32_h32(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_h32_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  switch ((T + 31) / 32) {
    case 1: return launch_temporal_h32_nkt<1>(qkv, out, B, T, J, D, H, s);
    case 2: return launch_temporal_h32_nkt<2>(qkv, out, B, T, J, D, H, s);
    case 3: return launch_temporal_h32_nkt<3>(qkv, out, B, T, J, D, H, s);
    case 4: return launch_temporal_h32_nkt<4>(qkv, out, B, T, J, D, H, s);
    case 5: return launch_temporal_h32_nkt<5>(qkv, out, B, T, J, D, H, s);
    case 6: return launch_temporal_h32_nkt<6>(qkv, out, B, T, J, D, H, s);
    case 7: return launch_temporal_h32_nkt<7>(qkv, out, B, T, J, D, H, s);
    default: return launch_temporal_h32_nkt<8>(qkv, out, B, T, J, D, H, s);
  }
}

// =============================================================================================== spatial (VALU)
template <int NJ>
__global__ __launch_bounds__(256) void k_attn_spatial_f32_h32(const float* __restrict__ qkv, float* __restrict__ out, int units, int H,
                                                              int D) {
  constexpr int UPW = 64 / NJ;                   // (frame, head) units per wave
  constexpr int UNIT_LD = NJ * DH + 4;           // +16 B so the UPW broadcast addresses fall in different banks
  constexpr int ROWS4 = NJ * (DH / 4);           // float4 per unit
  __shared__ __attribute__((aligned(16))) float kv_all[4 * UPW * UNIT_LD];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float* kv = kv_all + wave * UPW * UNIT_LD;
  const int base = (blockIdx.x * 4 + wave) * UPW;
  const int slot_raw = lane / NJ, i = lane % NJ;
  const int slot = slot_raw < UPW ? slot_raw : 0;
  const int unit = base + slot;
  const bool valid = (slot_raw < UPW) && (unit < units);
  const int D3 = 3 * D;

  // staging as in k_attn_spatial_f32: all global loads of a phase in flight together, V fetched while the scores are computed; units
  // behind the last one are staged as zeros
  constexpr int NIT = (UPW * ROWS4 + 63) / 64;
  auto gload = [&](int which, float4 (&tmp)[NIT]) {  // which: 1 = K, 2 = V
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = lane + 64 * it;
      const int s = idx / ROWS4, rem = idx % ROWS4;
      const int j = rem / (DH / 4), c4 = rem % (DH / 4);
      const int u = base + s;
      tmp[it] = make_float4(0, 0, 0, 0);
      if (idx < UPW * ROWS4 && u < units) {
        const int gg = u / H, hd = u % H;
        tmp[it] = *reinterpret_cast<const float4*>(qkv + ((size_t)gg * NJ + j) * D3 + which * D + hd * DH + c4 * 4);
      }
    }
  };
  auto lstore = [&](const float4 (&tmp)[NIT]) {
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = lane + 64 * it;
      if (idx < UPW * ROWS4) {
        const int s = idx / ROWS4, rem = idx % ROWS4;
        *reinterpret_cast<float4*>(&kv[s * UNIT_LD + rem * 4]) = tmp[it];
      }
    }
  };

  float4 stg[NIT];
  gload(1, stg);
  float q[DH];
  const int g = valid ? unit / H : 0, h = valid ? unit % H : 0;
  {
    const float* qp = qkv + ((size_t)g * NJ + i) * D3 + h * DH;
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
      const float4 v = valid ? *reinterpret_cast<const float4*>(qp + c) : make_float4(0, 0, 0, 0);
      q[c] = v.x; q[c + 1] = v.y; q[c + 2] = v.z; q[c + 3] = v.w;
    }
  }
  lstore(stg);
  __syncthreads();
  gload(2, stg);   // V in flight while the scores are computed from K

  const float scale = 1.0f / sqrtf((float)DH);
  float p[NJ];
  const float* ku = kv + slot * UNIT_LD;
#pragma unroll
  for (int j = 0; j < NJ; ++j) p[j] = 0.f;
  // The branch is always taken (a launch has units > 0).  It keeps the score phase a basic block of its own, in front of the barrier:
  // at NJ = 16, where no staging slot is guarded, the phases would otherwise be one block, the FMAs and expf would sink behind the
  // barrier to their uses, and all 128 float4 of K would be live across it (256 VGPRs + 256 AGPRs and scratch).
  if (units > 0) {
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      float acc = 0.f;
#pragma unroll
      for (int c = 0; c < DH; c += 4) {
        const float4 k4 = *reinterpret_cast<const float4*>(ku + j * DH + c);
        acc = fmaf(q[c], k4.x, acc); acc = fmaf(q[c + 1], k4.y, acc);
        acc = fmaf(q[c + 2], k4.z, acc); acc = fmaf(q[c + 3], k4.w, acc);
      }
      p[j] = acc * scale;
    }
    float m = p[0];
#pragma unroll
    for (int j = 1; j < NJ; ++j) m = fmaxf(m, p[j]);
    float l = 0.f;
#pragma unroll
    for (int j = 0; j < NJ; ++j) { p[j] = expf(p[j] - m); l += p[j]; }
#pragma unroll
    for (int j = 0; j < NJ; ++j) p[j] = p[j] / l;
  }

  __syncthreads();
  lstore(stg);
  __syncthreads();

  float o[DH];
#pragma unroll
  for (int c = 0; c < DH; ++c) o[c] = 0.f;
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
      const float4 v4 = *reinterpret_cast<const float4*>(ku + j * DH + c);
      o[c] = fmaf(p[j], v4.x, o[c]); o[c + 1] = fmaf(p[j], v4.y, o[c + 1]);
      o[c + 2] = fmaf(p[j], v4.z, o[c + 2]); o[c + 3] = fmaf(p[j], v4.w, o[c + 3]);
    }
  }
  if (valid) {
    const size_t oo = ((size_t)g * NJ + i) * D + h * DH;
    const float* vi = ku + i * DH;   // this query's own v row (attn - I, S2S:82-83): subtracted here, once
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(vi + c);
      *reinterpret_cast<float4*>(out + oo + c) = make_float4(o[c] - v.x, o[c + 1] - v.y, o[c + 2] - v.z, o[c + 3] - v.w);
    }
  }
}

// 15, 16 and 17 joints, as k_attn_spatial_f32 (other counts take k_attn_generic)
bool attn_spatial_f32_h32_ok(int J, int D, int H) { return J >= 15 && J <= 17 && H > 0 && D == H * DH; }

template <int NJ>
static hipError_t launch_spatial_h32_nj(const float* qkv, float* out, long long units, int D, int H, hipStream_t s) {
  constexpr int UPB = 4 * (64 / NJ);             // units per block: four waves of 64 / NJ
  const long long grid = (units + UPB - 1) / UPB;
  if (units > 0x7fffffffLL || grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(k_attn_spatial_f32_h32<NJ>, dim3((unsigned)grid), dim3(256), 0, s, qkv, out, (int)units, H, D);
  return hipGetLastError();
}

hipError_t launch_attn_spatial_f32_h32(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_spatial_f32_h32_ok(J, D, H) || !qkv || !out || B <= 0 || T <= 0) return hipErrorInvalidValue;
  const long long units = (long long)B * T * H;
  switch (J) {
    case 15: return launch_spatial_h32_nj<15>(qkv, out, units, D, H, s);
    case 16: return launch_spatial_h32_nj<16>(qkv, out, units, D, H, s);
    case 17: return launch_spatial_h32_nj<17>(qkv, out, units, D, H, s);
  }
  return hipErrorInvalidValue;
}

}  // namespace d3d
