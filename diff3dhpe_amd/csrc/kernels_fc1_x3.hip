// fc1 of the F16X3 block flow as its own kernel: hidden = gelu(norm2(x) W1^T + b1), LayerNorm folded (S2S:46-48 behind S2S:101), on the
// hand-specialised two-phase k-loop of the fused qkv + attention kernels (qkv_fused_kloop.h) with a 256 x 256 x 32 stage -- eight waves
// (2 x 4) of 128 rows x 64 columns, the shape and the MFMA order of k_linear_x3q_persist<8,2,4, EPI_GELU, pair-out, LN-folded>, whose
// epilogue (x3q_epilogue_acc: LayerNorm fold, erfc-series GELU, hi / lo split, accumulator-order pair output, no transpose) it calls:
// per element the same MFMAs in the same order and the same epilogue arithmetic, so the hidden activation is bit for bit the template's.
// What the template's persistent walk carries and this kernel does not: tail slices / ragged-tile instantiations and run-time group
// ranges (every tile is whole: the engine's buffers are padded to 256 rows and the pad rows of the stream are zeroed), the one-barrier
// fallback, the generic epilogue dispatch.  Measured against it: experiments/NOTES.md 0.11.
#include "d3d_kernels.h"
#include "qkv_fused_kloop.h"

#include <math.h>
#include <stdio.h>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "gemm_x3p_prelude.h"
#include "x3q_epilogue_acc.h"

QF_SHAPE(8, 4, 256, 256, 4, 4);                                          // 256 x 256 x 32 stage of 65536 bytes
constexpr int F1_RAW = 2 * QF_STAGE;                                     // raw statistics partials while the k-loop runs (16 KiB)
constexpr int F1_RAW_MAX = 16384;
constexpr int F1_STX = F1_RAW + F1_RAW_MAX;                              // (rstd', -mean rstd) of the tile's 256 rows, 2 KiB
constexpr int F1_LDS = F1_STX + QF_BM * 8;                               // 149504
static_assert(F1_LDS <= 160 * 1024, "LDS map");

struct F1Args {
  const _Float16* Ap;      // residual stream, pair layout [>= 256 mtiles rows][2 K] of 8 x
  const _Float16* Wp;      // folded fc1 weight W diag(gamma), pair layout, 2^k w, [N padded to 256][2 K]
  const float* bias;       // b + W beta
  const float* csum;       // sum_k W[n, k] gamma[k]
  const float* st_in;      // (sum, sum of squares) partials of the rows: [>= 256 mtiles rows][st_np][2]
  int st_np;
  float eps, out_scale;    // LayerNorm eps; 2^-(3 + k)
  _Float16* out;           // hidden activation, pair layout in accumulator order, [>= 256 mtiles rows][2 N]
  int M, N, K, mtiles, ntiles;
  unsigned* range;
};

__global__ __launch_bounds__(512) void k_fc1_x3(F1Args a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  QF_GEMM_WALK(a.Ap, a.Wp, a.mtiles, a.ntiles, a.K);
  for (int item = 0; item < nitems; ++item) {
    QF_GEMM_TILE_TOP;

    // ---- row statistics of the folded LayerNorm: raw partials by LDS-DMA under the k-loop, else read at the reduction
    const int st_bytes = QF_BM * a.st_np * 8;
    const bool st_dma = st_bytes <= F1_RAW_MAX;   // (uniform; the block of a 256-row tile is 16-byte aligned)
    int st_issued = 0;
    if (st_dma) {
      const char* src = reinterpret_cast<const char*>(a.st_in + (size_t)m0 * a.st_np * 2);
#pragma unroll
      for (int it = 0; it < F1_RAW_MAX / 1024 / 8; ++it) {
        const int pc = wave + it * 8;
        if (pc * 1024 < st_bytes) {
          KL_GLDS(sgpr_ptr(src + pc * 1024) + lane * 16, F1_RAW + pc * 1024);
          ++st_issued;
        }
      }
    }

    QF_GEMM_TILE_PLAN(a.Ap, a.Wp);
    int issued_prev = st_issued;
    QF_KLOOP_HEAD(QF_PIECE)
    // ---- row statistics -> (rstd * out_scale, -mean rstd) per tile row, in the shadow of the last k-tile (x3q_tile's x3_row_stats: the
    // partials added in column order)
    {
      float2* const srow = reinterpret_cast<float2*>(lds + F1_STX);
      if (lane < 32) {
        const int t = wave * 32 + lane, row = m0 + t;
        float sm = 0.f, sq = 0.f;
        if (row < a.M) {
          const float2* raw = st_dma ? reinterpret_cast<const float2*>(lds + F1_RAW) + t * a.st_np
                                     : reinterpret_cast<const float2*>(a.st_in) + (size_t)row * a.st_np;
          for (int p = 0; p < a.st_np; ++p) { sm += raw[p].x; sq += raw[p].y; }
        }
        if (sq >= (X3_HALF_MAX * 0.125f) * (X3_HALF_MAX * 0.125f)) range_raise(a.range, RANGE_BIT_ACT);
        const float mean = sm / (float)K;
        const float var = fmaxf(sq / (float)K - mean * mean, 0.0f);
        if (row < a.M && mean * mean > 256.0f * var) range_raise(a.range, RANGE_BIT_STATS);
        const float rstd = 1.0f / sqrtf(var + a.eps);
        srow[t] = make_float2(rstd * a.out_scale, -mean * rstd);
      }
    }
    QF_KLOOP_TAIL(QF_PIECE)
    __builtin_amdgcn_s_setprio(0);
    __syncthreads();   // statistics visible
    {
      const int mt0 = m0 + wm * 16 * QF_TM, nt0 = n0 + wn * 64;
      _Float16* Cht = a.out + 2 * ((size_t)mt0 * a.N + nt0);
      x3q_epilogue_acc<QF_TM, 2, 4, FX_LNF, false>(acc, lds + F1_STX, a.bias, Cht, a.csum, mt0, nt0, wm * 16 * QF_TM, lane, a.M, a.N, 0, QF_TM,
                                                    a.out_scale, a.range);
    }
    mt = mtn; nt = ntn;
    __syncthreads();   // the statistics rows are read before the next tile's reduction writes them
  }
}

}  // namespace

bool fc1_x3_ok(int N, int K) { return N % 256 == 0 && K % 64 == 0 && K >= 128; }

// hidden[M, N] = gelu(LN(x) W^T + b), operands and statistics as launch_linear_x3p's LN-folded GELU form; every buffer spans whole
// 256-row tiles and the pad rows of the stream hold finite values (the engine zeroes them).
hipError_t launch_fc1_x3(const void* Apair, const void* Wpair, const float* bias_f, const float* csum, const float* st_in, int st_np,
                         float eps, int w_exp, void* out_pair, int M, int N, int K, hipStream_t s) {
  if (!fc1_x3_ok(N, K) || M <= 0 || st_np < 1 || !Apair || !Wpair || !bias_f || !csum || !st_in || !out_pair) return hipErrorInvalidValue;
  if (w_exp < -14 || w_exp > 12) return hipErrorInvalidValue;
  F1Args a{};
  a.Ap = (const _Float16*)Apair; a.Wp = (const _Float16*)Wpair; a.bias = bias_f; a.csum = csum; a.st_in = st_in; a.st_np = st_np;
  a.eps = eps; a.out_scale = ldexpf(1.0f, -(3 + w_exp)); a.out = (_Float16*)out_pair;
  a.M = M; a.N = N; a.K = K; a.mtiles = (M + QF_BM - 1) / QF_BM; a.ntiles = N / QF_BN;
  a.range = launch_range_word();
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * a.ntiles, grid)) return ge;
  return launch_lds<k_fc1_x3>(dim3(grid), dim3(512), F1_LDS, s, a);
}

}  // namespace d3d
