// Latency mode (engine option "latency_mode"): the second half of fc2 + post-norm for calls too small to fill one round of whole-row
// tiles -- the ordered reduce of the split-K partials with the block's post-norm -- and the host rule that picks the split.
//
//   y = LN(r + b + P[0] + P[1] + ... + P[S-1]; g, beta, eps) [+ pos] [+ tvec]          (S2S:131-135 + 236/245, 238-242, 113-116)
//
// P[ks] are the un-scaled fp32 partials of k_linear_x3q_splitk (kernels_gemm_x3p.hip), r the residual stream's planes.  The additions
// run in exactly the order written, so a row's value depends on S and on nothing else (not on M, the tile position or the launch).
// One 64-lane wave owns one 512-column row, a lane 8 consecutive columns: every access is a 16-byte one (two float4 of a partial,
// 8 fp16 of a plane half), one pass over the partials.  LayerNorm as launch_layernorm does it (two-pass variance in registers).
// Built without the SLP vectoriser like the other row kernels (build.py EXTRA_FLAGS): no packed fp32 forms.
#include "d3d_kernels.h"

namespace d3d {

namespace {

typedef _Float16 h8v __attribute__((ext_vector_type(8)));

constexpr int SK_WAVES = 4;     // rows per workgroup
constexpr int SK_N = 512;       // row length the kernel is written for (the post-norm tile shape: x3q_postnorm_ok)
constexpr int SK_MAXS = 4;

struct SplitkPnArgs {
  const float* P; size_t pstride; int S;
  const _Float16* Rp; const float* bias;
  X3PostNorm pn;
  float* Y; _Float16* Yp; float* stats;
  int M;
  unsigned* range;
};

// Sum over the 64 lanes of a wave, the total in every lane: the DPP butterfly + v_readlane form of kernels_elem.hip (wave_sum).
__device__ __forceinline__ float sk_wave_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x140, 0xF, 0xF, true));
  const int b = __builtin_bit_cast(int, v);
  const float r0 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)), r1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16));
  const float r2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)), r3 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48));
  return (r0 + r1) + (r2 + r3);
}

__device__ __forceinline__ void ld8(const float* p, float (&o)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}

// (Rp, Y and Yp may share bytes row for row: a wave has read its row before it writes it -- every store depends on the row's mean)
__global__ __launch_bounds__(64 * SK_WAVES) void k_splitk_postnorm(SplitkPnArgs a) {
  constexpr int N = SK_N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * SK_WAVES + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int c = 8 * lane;
  const size_t pc = pair_col(c);
  float v[8], t[8], p[SK_MAXS][8];
  const _Float16* rp = a.Rp + (size_t)row * 2 * N + pc;
  const h8v hh = *reinterpret_cast<const h8v*>(rp), ll = *reinterpret_cast<const h8v*>(rp + PAIR_LO);
  const float* pr = a.P + (size_t)row * N + c;
#pragma unroll
  for (int s = 0; s < SK_MAXS; ++s)
    if (s < a.S) ld8(pr + (size_t)s * a.pstride, p[s]);   // (S is uniform: the partials are requested together, added in order)
  ld8(a.bias + c, t);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = __fadd_rn(__fmul_rn(__fadd_rn((float)hh[j], (float)ll[j]), 0.125f), t[j]);   // r + b
#pragma unroll
  for (int s = 0; s < SK_MAXS; ++s)
    if (s < a.S) {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = __fadd_rn(v[j], p[s][j]);                                                // ... + P[s]
    }
  // LayerNorm, two-pass variance (ln_row of kernels_elem.hip)
  float sm = ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
  const float mean = sk_wave_sum(sm) / (float)N;
  float q = 0.f;
#pragma unroll
  for (int j = 0; j < 8; j += 2) {
    const float d0 = v[j] - mean, d1 = v[j + 1] - mean;
    q += d0 * d0 + d1 * d1;
  }
  const float rstd = 1.0f / sqrtf(sk_wave_sum(q) / (float)N + a.pn.eps);
  float g[8];
  ld8(a.pn.g + c, g);
  ld8(a.pn.b + c, t);
#pragma unroll
  for (int j = 0; j < 8; ++j) v[j] = (v[j] - mean) * rstd * g[j] + t[j];
  if (a.pn.pos) {
    ld8(a.pn.pos + (size_t)((row / a.pn.pos_div) % a.pn.pos_mod) * N + c, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += t[j];
  }
  if (a.pn.tvec) {
    ld8(a.pn.tvec + (size_t)(row / a.pn.rows_per_batch) * a.pn.tvec_stride + c, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] += t[j];
  }
  if (a.Y) {
    float* yr = a.Y + (size_t)row * N + c;
    *reinterpret_cast<float4*>(yr) = make_float4(v[0], v[1], v[2], v[3]);
    *reinterpret_cast<float4*>(yr + 4) = make_float4(v[4], v[5], v[6], v[7]);
  }
  if (a.Yp) {   // the residual stream as GEMM operand planes of 8 y + the row's (sum, sum of squares) for the next folded LayerNorm
    float amax = 0.0f;
    h8v hi, lo;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      amax = fmaxf(amax, fabsf(v[j] * 8.0f));
      const float sc = __builtin_amdgcn_fmed3f(v[j] * 8.0f, -65504.0f, 65504.0f);
      hi[j] = (_Float16)sc;
      lo[j] = (_Float16)(sc - (float)hi[j]);
    }
    _Float16* yp = a.Yp + (size_t)row * 2 * N + pc;
    *reinterpret_cast<h8v*>(yp) = hi;
    *reinterpret_cast<h8v*>(yp + PAIR_LO) = lo;
    if (amax > X3_HALF_MAX) range_raise(a.range, RANGE_BIT_ACT);
    if (a.stats) {
      sm = __fadd_rn(__fadd_rn(__fadd_rn(v[0], v[1]), __fadd_rn(v[2], v[3])), __fadd_rn(__fadd_rn(v[4], v[5]), __fadd_rn(v[6], v[7])));
      float sq = __fadd_rn(__fadd_rn(__fmaf_rn(v[0], v[0], __fmul_rn(v[1], v[1])), __fmaf_rn(v[2], v[2], __fmul_rn(v[3], v[3]))),
                           __fadd_rn(__fmaf_rn(v[4], v[4], __fmul_rn(v[5], v[5])), __fmaf_rn(v[6], v[6], __fmul_rn(v[7], v[7]))));
      sm = sk_wave_sum(sm);
      sq = sk_wave_sum(sq);
      if (lane == 0) *reinterpret_cast<float2*>(a.stats + 2 * (size_t)row) = make_float2(sm, sq);
    }
  }
}

}  // namespace

bool fc2_splitk_ok(int N, int K, int S) {
  return x3q_postnorm_ok(N, K) && N == SK_N && (S == 2 || S == 4) && (K / 32) % S == 0;
}

int fc2_splitk_choose(int M, int N, int K, int n_cu) {
  if (M <= 0 || n_cu <= 0 || !x3q_postnorm_ok(N, K) || N != SK_N) return 0;
  if ((M + 63) / 64 >= n_cu) return 0;   // the whole-row launch fills a round: nothing to win
  const int nk = K / 32;
  const long long tiles = (long long)((M + 127) / 128) * (N / 128);
  int best = 0;
  double best_cost = 0.0;
  for (int S = 1; S <= SK_MAXS; S *= 2) {
    if (nk % S != 0 || nk / S < 4) continue;
    const long long W = tiles * S;
    if (W > 2LL * n_cu) continue;
    const double cost = (double)(nk / S) * (W <= n_cu ? 1.0 : 1.45);
    if (best == 0 || cost < best_cost) { best = S; best_cost = cost; }
  }
  return best >= 2 ? best : 0;
}

hipError_t launch_splitk_postnorm(const float* P, int S, const void* Rp, const float* bias, const X3PostNorm& pn, float* Y, void* Yp,
                                  float* stats, int M, int N, hipStream_t s) {
  if (N != SK_N || M <= 0 || S < 1 || S > SK_MAXS || !P || !Rp || !bias || !pn.g || !pn.b) return hipErrorInvalidValue;
  if ((Y != nullptr) == (Yp != nullptr) || (stats && !Yp)) return hipErrorInvalidValue;
  if (pn.pos && (pn.pos_div < 1 || pn.pos_mod < 1)) return hipErrorInvalidValue;
  if (pn.tvec && pn.tvec_stride != 0 && pn.rows_per_batch < 1) return hipErrorInvalidValue;
  SplitkPnArgs a{};
  a.P = P; a.pstride = (size_t)M * N; a.S = S;
  a.Rp = (const _Float16*)Rp; a.bias = bias; a.pn = pn;
  if (!pn.pos) { a.pn.pos_div = 1; a.pn.pos_mod = 1; }
  if (a.pn.rows_per_batch < 1) a.pn.rows_per_batch = 1;
  a.Y = Y; a.Yp = (_Float16*)Yp; a.stats = stats; a.M = M;
  a.range = launch_range_word();   // F16X3 range guard: the launching engine's word (d3d_kernels.h)
  hipLaunchKernelGGL(k_splitk_postnorm, dim3((M + SK_WAVES - 1) / SK_WAVES), dim3(64 * SK_WAVES), 0, s, a);
  return hipGetLastError();
}

}  // namespace d3d
