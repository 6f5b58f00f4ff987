// GRAND attention cores in exact fp32 for heads of 32 columns (D == 32 H: embed_dim 256 with the runner's 8 heads):
//   O = (softmax(q k^T / sqrt(32)) - I) v,   packed qkv rows in, fp32 rows out -- the contract of kernels_attn.hip without its pair-layout
// form (only FP32 engines take these kernels; option "attn_f32_h32").
//
//   temporal  k_attn_temporal_f32_h32<NKT>, one workgroup of NKT waves per (batch, joint, head), T <= 32 NKT <= 256, on the pieces of
//             attn_f32_tile.h at DH = 32: 16 MFMAs per 32 x 32 score tile, the exact two-pass softmax over the accumulator registers,
//             normalised before the second product, ONE 32 x 32 accumulator tile, 16 MFMAs per key tile.  Compiler-scheduled; one
//             scheduling fence, explained where it stands, keeps every instantiation free of spills.
//   spatial   k_attn_spatial_f32_h32<NJ>, NJ = 15, 16, 17: the VALU form of k_attn_spatial_f32 -- one lane owns one query row (q[32] in
//             registers), a wave runs 64 / NJ (frame, head) units, K then V of the unit staged in LDS and broadcast-read, lane-local softmax.
//
// The scale.  32^-1/2 is no power of two: scaling q by it would round every operand of the dot product.  The scores are multiplied by
// 1.0f / sqrtf(32.0f) AFTER the sum over d, k_attn_generic's constant and the reference's order ((q k^T) * scale).
// The diagonal.  The - I is not put into P (F32Tile::DIAG_IN_P_RESIDENT): these kernels have no twin whose bits they must keep, the
// products are summed alone and v[query] is subtracted once, at the store.
//
// LDS of the temporal kernel: 8 704 B per key tile, 69 632 B at NKT = 8.
// LDS of the spatial kernel: a unit is NJ rows of 32 floats + 4 floats, so the 64 / NJ broadcast addresses of a wave (one per unit) fall
// into different four-bank slots (unit stride mod 64 dwords = 36, 4, 36 for NJ = 15, 16, 17).
//
// Row isolation: K / V rows >= T are staged as zeros and their scores set to -inf (e = 0 exactly), so 0 x NaN cannot enter a clean row;
// rows >= T (lanes without a unit) are never stored; every wave reaches every barrier.
#include "attn_f32_tile.h"

namespace d3d {

namespace {
constexpr int DH = 32;                 // head width
using Tl = F32Tile<DH>;
}  // namespace

// =============================================================================================== temporal (MFMA f32)
template <int NKT>
__global__ __launch_bounds__(64 * NKT) void k_attn_temporal_f32_h32(const float* __restrict__ qkv, float* __restrict__ out, int T, int J,
                                                                    int H, int D) {
  extern __shared__ __attribute__((aligned(16))) float lds_f32h32[];
  constexpr int TP = 32 * NKT;
  float* const Ks = lds_f32h32;                   // [TP][K_LD]
  float* const Vs = lds_f32h32 + TP * Tl::K_LD;   // [TP][V_LD]

  const int unit = blockIdx.x;     // (b*J + j)*H + h
  const int h = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;   // token(t) = tok0 + t*J

  // K and V rows [0, TP) of the unit: TP * 8 16-byte slots = 4 per thread, one batch
  f32_stage_rows<DH, true>(qkv, Ks, Vs, tok0, J, D, h, 0, NKT, T, tid, 64 * NKT);
  const int tq = 32 * wave + r;
  float qreg[Tl::QR];
  f32_load_query<DH>(qkv, qreg, tok0, J, D, h, tq, T, hh);
  __syncthreads();

  // exact (max-subtracted, two-pass) softmax over the keys of this query column.  Keys >= T sit in the last key tile only: the launch
  // picks NKT = ceil(T / 32)
  f32x16 sacc[NKT];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    sacc[kt] = f32_score_tile<DH>(Ks, qreg, kt, {kt, kt == NKT - 1, T}, r, hh);
    m = f32_tile_max<DH>(sacc[kt], {kt, kt == NKT - 1, T}, hh, m);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32_exp_tile<DH>(sacc[kt], {kt, kt == NKT - 1, T}, hh, m);
    f32_sum_tile(sacc[kt], l);
    // one key tile per scheduling region: expf's range selects live in SGPR pairs, and a scheduler free to batch the compares of several
    // tiles runs out of them (SGPR spills at NKT = 5 and 8)
    __builtin_amdgcn_sched_barrier(0);
  }
  l += __shfl_xor(l, 32, 64);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) f32_normalise_tile(sacc[kt], l);

  f32x16 oacc[Tl::NDT];
  f32_zero_acc<DH>(oacc);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) f32_pv_tile<DH>(Vs, sacc[kt], oacc, kt, r, hh);

  if (tq < T) f32_store_query<DH>(qkv, out, oacc, l, tok0 + (size_t)tq * J, D, h, hh, true);
}

bool attn_temporal_f32_h32_ok(int T, int D, int H) { return T >= 1 && T <= 256 && H > 0 && D == H * DH; }

hipError_t launch_attn_temporal_f32_h32(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_h32_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const long long grid = (long long)B * J * H;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  return f32_resident_ladder<8>(T, [&](auto nkt) {
    constexpr int NKT = decltype(nkt)::value;
    return launch_lds<k_attn_temporal_f32_h32<NKT>>(dim3((unsigned)grid), dim3(64 * NKT), Tl::lds_bytes(NKT), s, qkv, out, T, J, H, D);
  });
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
