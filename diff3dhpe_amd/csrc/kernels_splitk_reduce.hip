// Latency mode (engine option "latency_mode"), proj and fc1 of a call too small to fill the chip: the ordered reduces behind the
// split-K x split-N GEMM (k_linear_x3q_splitk, kernels_gemm_x3p.hip: P[ks][M][N], fp32, the plane scales 2^(3 + k) already taken out by
// that kernel's epilogue -- a power of two, exact) and the host rules that pick S.
//
//   k_splitk_residual (proj):  x = r + b + P[0] + P[1] + ... + P[S-1]                                        (S2S:84 + 127)
//       -> the stream planes (pair layout of 8 x, in place over r) + one (sum, sum of squares) per row and 64 columns (st_out of X3Fold)
//   k_splitk_gelu     (fc1):   h = gelu(rstd (P[0] + ... + P[S-1]) - rstd mean csum + b'),  LayerNorm folded     (S2S:46-48 behind 101)
//       -> the hidden activation in the accumulator-order pair layout (pair_col_acc) fc2 reads
//
// The additions run in exactly the order written: a row's value depends on S and on nothing else.  One 64-lane wave owns one row and a
// lane 8 columns per pass, every access a 16-byte one.  The epilogue arithmetic is that of x3q_epilogue8 / x3q_epilogue_acc (the same
// fmas, gelu_fast2, split8_x3), so what leaves here has the form the default kernels write.  Built without the SLP vectoriser like the
// other row kernels (build.py EXTRA_FLAGS).
#include "d3d_kernels.h"

namespace d3d {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
constexpr float P_A_SCALE = 8.0f;
__device__ __forceinline__ void range_note(unsigned* rw, float amax) {
  if (amax > X3_HALF_MAX) range_raise(rw, RANGE_BIT_ACT);
}
#define D3D_PATCH_FENCE() asm volatile("" ::: "memory")
#include "x3q_epilogue_acc.h"   // f2, gelu_fast2, split8_x3

constexpr int RK_WAVES = 4;      // rows per workgroup
constexpr int RK_MAXS = 4;
constexpr int RK_PROJ_N = 512;   // row length k_splitk_residual is written for (one pass of 64 lanes x 8 columns)

struct SplitkResArgs {
  const float* P; size_t pstride; int S;
  const _Float16* Rp; const float* bias;
  _Float16* Xp; float* st_out;
  int M;
  unsigned* range;
};
struct SplitkGeluArgs {
  const float* P; size_t pstride; int S;
  const float* st_in; int st_np; const float* csum; const float* bias; float eps;
  _Float16* Hp;
  int M, N, K;
  unsigned* range;
};

__device__ __forceinline__ void ld8(const float* p, float (&o)[8]) {
  const float4 a = *reinterpret_cast<const float4*>(p), b = *reinterpret_cast<const float4*>(p + 4);
  o[0] = a.x; o[1] = a.y; o[2] = a.z; o[3] = a.w; o[4] = b.x; o[5] = b.y; o[6] = b.z; o[7] = b.w;
}
// sum over the 8 lanes that share one 64-column block, the total in all of them (row8_sum of gemm_x3p_epilogue.h)
__device__ __forceinline__ float rk_row8_sum(float v) {
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0xB1, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x4E, 0xF, 0xF, true));
  v += __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x141, 0xF, 0xF, true));
  return v;
}

// (Rp and Xp may be the same buffer: a lane reads its 8 residual values before it writes them, and nobody else touches them)
__global__ __launch_bounds__(64 * RK_WAVES) void k_splitk_residual(SplitkResArgs a) {
  constexpr int N = RK_PROJ_N;
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * RK_WAVES + (threadIdx.x >> 6);
  if (row >= a.M) return;
  const int c = 8 * lane;
  const size_t pc = pair_col(c);
  float x[8], t[8], p[RK_MAXS][8];
  const _Float16* rp = a.Rp + (size_t)row * 2 * N + pc;
  const h8 hh = *reinterpret_cast<const h8*>(rp), ll = *reinterpret_cast<const h8*>(rp + PAIR_LO);
  const float* pr = a.P + (size_t)row * N + c;
#pragma unroll
  for (int s = 0; s < RK_MAXS; ++s)
    if (s < a.S) ld8(pr + (size_t)s * a.pstride, p[s]);   // (S is uniform: the partials are requested together, added in order)
  ld8(a.bias + c, t);
#pragma unroll
  for (int j = 0; j < 8; ++j) x[j] = __fmaf_rn(__fadd_rn((float)hh[j], (float)ll[j]), 0.125f, t[j]);          // r + b
#pragma unroll
  for (int s = 0; s < RK_MAXS; ++s)
    if (s < a.S) {
#pragma unroll
      for (int j = 0; j < 8; ++j) x[j] = __fadd_rn(x[j], p[s][j]);                                             // ... + P[s]
    }
  // (sum, sum of squares) of the 64-column block: sums8 + row8_sum of the proj epilogue
  float sm = __fadd_rn(__fadd_rn(__fadd_rn(x[0], x[2]), __fadd_rn(x[4], x[6])), __fadd_rn(__fadd_rn(x[1], x[3]), __fadd_rn(x[5], x[7])));
  float sq = __fadd_rn(__fadd_rn(__fmaf_rn(x[0], x[0], __fmul_rn(x[2], x[2])), __fmaf_rn(x[4], x[4], __fmul_rn(x[6], x[6]))),
                       __fadd_rn(__fmaf_rn(x[1], x[1], __fmul_rn(x[3], x[3])), __fmaf_rn(x[5], x[5], __fmul_rn(x[7], x[7]))));
  sm = rk_row8_sum(sm);
  sq = rk_row8_sum(sq);
  if ((lane & 7) == 0) *reinterpret_cast<float2*>(a.st_out + 2 * ((size_t)row * (N / 64) + (lane >> 3))) = make_float2(sm, sq);
  f2 v[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e].x = x[2 * e]; v[e].y = x[2 * e + 1]; }
  h8 oh, ol;
  float amax = 0.0f;
  split8_x3<true>(v, P_A_SCALE, oh, ol, amax);
  _Float16* xp = a.Xp + (size_t)row * 2 * N + pc;
  *reinterpret_cast<h8*>(xp) = oh;
  *reinterpret_cast<h8*>(xp + PAIR_LO) = ol;
  range_note(a.range, amax * P_A_SCALE);   // |x| > 8188 does not fit the planes: D3D_RANGE_ACT
}

__global__ __launch_bounds__(64 * RK_WAVES) void k_splitk_gelu(SplitkGeluArgs a) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * RK_WAVES + (threadIdx.x >> 6);
  if (row >= a.M) return;
  // the row's LayerNorm statistics from the producer's partials, added in column order (x3_row_stats of x3q_tile)
  float sm = 0.f, sq = 0.f;
  for (int q = 0; q < a.st_np; ++q) {
    const float2 t = *reinterpret_cast<const float2*>(a.st_in + 2 * ((size_t)row * a.st_np + q));
    sm += t.x; sq += t.y;
  }
  const float mean = sm / (float)a.K;
  const float var = fmaxf(sq / (float)a.K - mean * mean, 0.0f);
  if (lane == 0) {   // the guards of the consumer of these statistics: the planes of x (their producer's range), |mean| > 16 sigma
    if (sq >= (X3_HALF_MAX * 0.125f) * (X3_HALF_MAX * 0.125f)) range_raise(a.range, RANGE_BIT_ACT);
    if (mean * mean > 256.0f * var) range_raise(a.range, RANGE_BIT_STATS);
  }
  const float rstd = 1.0f / sqrtf(var + a.eps);
  const float sx = rstd, sy = -mean * rstd;   // (the partials carry no plane scale)
  float amax = 0.0f;
  const int N = a.N;
  const float* prow = a.P + (size_t)row * N;
  _Float16* hrow = a.Hp + (size_t)row * 2 * N;
  for (int idx = lane; idx < N / 8; idx += 64) {   // piece idx: 32-column group idx / 4, accumulator quarter idx % 4 (pair_col_acc)
    const int g = idx >> 2, q = idx & 3;
    const int cA = 32 * g + 4 * q, cB = cA + 16;
    float acc[8], t[8], cs[8], b[8];
    {
      const float4 u = *reinterpret_cast<const float4*>(prow + cA), w = *reinterpret_cast<const float4*>(prow + cB);
      acc[0] = u.x; acc[1] = u.y; acc[2] = u.z; acc[3] = u.w; acc[4] = w.x; acc[5] = w.y; acc[6] = w.z; acc[7] = w.w;
    }
#pragma unroll
    for (int s = 1; s < RK_MAXS; ++s)
      if (s < a.S) {
        const float4 u = *reinterpret_cast<const float4*>(prow + (size_t)s * a.pstride + cA);
        const float4 w = *reinterpret_cast<const float4*>(prow + (size_t)s * a.pstride + cB);
        t[0] = u.x; t[1] = u.y; t[2] = u.z; t[3] = u.w; t[4] = w.x; t[5] = w.y; t[6] = w.z; t[7] = w.w;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = __fadd_rn(acc[j], t[j]);                                          // P[0] + ... + P[s]
      }
    {
      const float4 u = *reinterpret_cast<const float4*>(a.csum + cA), w = *reinterpret_cast<const float4*>(a.csum + cB);
      cs[0] = u.x; cs[1] = u.y; cs[2] = u.z; cs[3] = u.w; cs[4] = w.x; cs[5] = w.y; cs[6] = w.z; cs[7] = w.w;
      const float4 u2 = *reinterpret_cast<const float4*>(a.bias + cA), w2 = *reinterpret_cast<const float4*>(a.bias + cB);
      b[0] = u2.x; b[1] = u2.y; b[2] = u2.z; b[3] = u2.w; b[4] = w2.x; b[5] = w2.y; b[6] = w2.z; b[7] = w2.w;
    }
    f2 v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {   // LN(x) W^T + b = rstd (x W'^T) - rstd mean csum + b'
      v[e].x = __fmaf_rn(sx, acc[2 * e], __fmaf_rn(sy, cs[2 * e], b[2 * e]));
      v[e].y = __fmaf_rn(sx, acc[2 * e + 1], __fmaf_rn(sy, cs[2 * e + 1], b[2 * e + 1]));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = gelu_fast2(v[e]);
    h8 oh, ol;
    split8_x3<true>(v, P_A_SCALE, oh, ol, amax);
    _Float16* hp = hrow + 64 * g + 8 * q;
    *reinterpret_cast<h8*>(hp) = oh;
    *reinterpret_cast<h8*>(hp + PAIR_LO) = ol;
  }
  range_note(a.range, amax * P_A_SCALE);
}

// accumulator-order pair layout of 8 h -> fp32 [rows][cols]: read-back side of d3d_op_linear_splitk_gelu, not on the engine's path
__global__ __launch_bounds__(256) void k_unsplit_acc(const _Float16* __restrict__ pair, float* __restrict__ x, size_t n, int cols) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t row = i / cols;
  const int c = (int)(i - row * cols);
  const _Float16* p = pair + row * 2 * cols + pair_col_acc(c);
  x[i] = ((float)p[0] + (float)p[PAIR_LO]) * 0.125f;
}

// ---- the rules (d3d_kernels.h) ----
// Unit: one k-tile of a lone 128 x 128 workgroup.  The split launch: K/32/S k-tiles, x RK_SHARE where two workgroups share a CU.
constexpr double RK_SHARE = 1.45;      // two co-resident 128 x 128 workgroups against a lone one (experiments/NOTES.md, fc2 rule)
constexpr double RK_TALL = 1.4;        // a k-tile of the present 256 x 128 stage against the 128 x 128 one (fc1 at B = 1: 28.7 vs 20.7 us)
// the reduce launch, additive.  PLACEHOLDERS, not tuned values: profiles/latency_mode_proj_fc1.json does not exist yet (no GPU run of
// experiments/latency_mode.py --proj-fc1 has been made).  Until it does the constant is the depth of the present launch itself
// (K / 32 = 16 k-tiles at K = 512), with which the model shows no gain anywhere and the rules keep the present kernels: an unmeasured
// split is never switched in by default.  "proj_split" / "fc1_split" force it.  (The estimate to check: proj ~6, fc1 ~8.)
constexpr double RK_REDUCE_PROJ = 16.0;
constexpr double RK_REDUCE_FC1 = 16.0;

// what runs today for (M, N, K): launch_x3q_auto -- 128 x 128 tiles while each finds a CU, else 256 x 128 tiles in rounds
double present_cost(int M, int N, int K, int n_cu) {
  const int nk = K / 32;
  const long long t128 = (long long)((M + 127) / 128) * (N / 128);
  if (t128 <= n_cu) return (double)nk;
  const long long t256 = (long long)((M + 255) / 256) * (N / 128);
  return (double)nk * RK_TALL * (double)((t256 + n_cu - 1) / n_cu);
}

int splitk_choose(int M, int N, int K, int n_cu, double reduce_cost, bool one_round, long long max_rows) {
  if (M <= 0 || n_cu <= 0) return 0;
  const int nk = K / 32;
  const long long tiles = (long long)((M + 127) / 128) * (N / 128);
  const double now = present_cost(M, N, K, n_cu);
  int best = 0;
  double best_cost = now;
  for (int S = 2; S <= RK_MAXS; S *= 2) {
    if (nk % S != 0 || nk / S < 4) continue;
    const long long W = tiles * S;
    if (W > 2LL * n_cu || (one_round && W > n_cu)) continue;
    if (max_rows && (long long)M * S > max_rows) continue;
    const double cost = (double)(nk / S) * (W <= n_cu ? 1.0 : RK_SHARE) + reduce_cost;
    if (cost < best_cost) { best = S; best_cost = cost; }   // (the smaller S on a tie)
  }
  return best;
}

}  // namespace

bool proj_splitk_ok(int N, int K, int S) {
  return N == RK_PROJ_N && K % 32 == 0 && K > 0 && (S == 2 || S == 4) && (K / 32) % S == 0 && K / 32 / S >= 4;
}
bool fc1_splitk_ok(int N, int K, int S) {
  return N > 0 && N % 512 == 0 && K > 0 && K % 64 == 0 && (S == 2 || S == 4) && (K / 32) % S == 0 && K / 32 / S >= 4;
}
bool proj_splitk_fits(int M, int N, int S, int n_cu) {
  return M > 0 && n_cu > 0 && (long long)((M + 127) / 128) * (N / 128) * S <= 2LL * n_cu;
}
bool fc1_splitk_fits(int M, int N, int S, int n_cu) {
  return proj_splitk_fits(M, N, S, n_cu) && (long long)M * S * N <= (long long)FC1_SPLITK_SCRATCH_FLOATS;
}

int proj_splitk_choose(int M, int N, int K, int n_cu) {
  if (N != RK_PROJ_N || K != RK_PROJ_N) return 0;   // the flow of DESIGN 4.8: D = 512
  return splitk_choose(M, N, K, n_cu, RK_REDUCE_PROJ, false, 0);
}
int fc1_splitk_choose(int M, int N, int K, int n_cu) {
  if (K != RK_PROJ_N || N <= 0 || N % 512 != 0) return 0;
  // one round only: two 128 x 128 workgroups of fc1 on one CU lose against the present launch (NOTES round 6: 28.7 -> 38.2 us)
  return splitk_choose(M, N, K, n_cu, RK_REDUCE_FC1, true, (long long)(FC1_SPLITK_SCRATCH_FLOATS / (size_t)N));
}

hipError_t launch_splitk_residual(const float* P, int S, const void* Rp, const float* bias, void* Xp, float* st_out, int M, int N,
                                  hipStream_t s) {
  if (N != RK_PROJ_N || M <= 0 || S < 1 || S > RK_MAXS || !P || !Rp || !bias || !Xp || !st_out) return hipErrorInvalidValue;
  SplitkResArgs a{};
  a.P = P; a.pstride = (size_t)M * N; a.S = S;
  a.Rp = (const _Float16*)Rp; a.bias = bias;
  a.Xp = (_Float16*)Xp; a.st_out = st_out; a.M = M;
  a.range = launch_range_word();
  hipLaunchKernelGGL(k_splitk_residual, dim3((M + RK_WAVES - 1) / RK_WAVES), dim3(64 * RK_WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_splitk_gelu(const float* P, int S, const float* st_in, int st_np, const float* csum, const float* bias, float eps,
                              void* Hp, int M, int N, int K, hipStream_t s) {
  if (M <= 0 || N <= 0 || N % 512 != 0 || K <= 0 || S < 1 || S > RK_MAXS || st_np < 1) return hipErrorInvalidValue;
  if (!P || !st_in || !csum || !bias || !Hp) return hipErrorInvalidValue;
  SplitkGeluArgs a{};
  a.P = P; a.pstride = (size_t)M * N; a.S = S;
  a.st_in = st_in; a.st_np = st_np; a.csum = csum; a.bias = bias; a.eps = eps;
  a.Hp = (_Float16*)Hp; a.M = M; a.N = N; a.K = K;
  a.range = launch_range_word();
  hipLaunchKernelGGL(k_splitk_gelu, dim3((M + RK_WAVES - 1) / RK_WAVES), dim3(64 * RK_WAVES), 0, s, a);
  return hipGetLastError();
}

hipError_t launch_unsplit_acc(const void* pair, float* x, size_t rows, int cols, hipStream_t s) {
  if (cols <= 0 || cols % 32) return hipErrorInvalidValue;
  const size_t n = rows * cols;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(k_unsplit_acc, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const _Float16*)pair, x, n, cols);
  return hipGetLastError();
}

}  // namespace d3d
