// proj of the F16X3 block flow as its own kernel: x += attn Wproj^T + b, plane to plane in place, with the (sum, sum of squares) row
// partials of the new x for the LayerNorm folded into fc1 (S2S:84 + 127 behind S2S:101) -- on the hand-specialised two-phase k-loop of the
// fused kernels (qkv_fused_kloop.h) with a 192 x 256 x 32 stage: eight waves (2 x 4) of 96 rows x 64 columns, the shape and the MFMA order of
// k_linear_x3q_persist<6,2,4, EPI_RESIDUAL, pair-out, plane residual + row statistics>, whose epilogue function (x3q_epilogue8) it calls.
// Per element the same MFMAs in the same order and the same epilogue arithmetic: bit for bit the template's result.  Whole tiles only:
// the launcher hands the rows beyond the last whole 192-row tile to the template (their unguarded stores would reach the stream's pad rows).
#include "d3d_kernels.h"
#include "qkv_fused_kloop.h"

#include <math.h>
#include <stdio.h>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "gemm_x3p_prelude.h"
#include "gemm_x3p_epilogue.h"

QF_SHAPE(6, 4, 192, 256, 3, 4);                                          // 192 x 256 x 32 stage of 57344 bytes
constexpr int PJ_PATCH = QF_STAGE;                                       // eight 8 KiB transpose patches over stage 1 (and beyond)
constexpr int PJ_STATP = PJ_PATCH + 65536;                               // a kilobyte per wave for the rows' statistics
constexpr int PJ_LDS = PJ_STATP + 8 * 1024;                              // 131072
static_assert(PJ_LDS <= 160 * 1024 && PJ_PATCH + 65536 >= 2 * QF_STAGE, "LDS map");

struct PjArgs {
  const _Float16* Ap;      // attention output, pair layout [>= 192 mtiles rows][2 K] of 8 o
  const _Float16* Wp;      // proj weight, pair layout, 2^k w, [N padded to 256][2 K]
  const float* bias;
  _Float16* X;             // the stream planes (pair layout [rows][2 N] of 8 x): residual in, new x out, in place
  float* st_out;           // (sum, sum of squares) partials of the new rows: [rows][N / 64][2]
  float out_scale;         // 2^-(3 + k)
  int M, N, K, mtiles, ntiles;   // M = 192 mtiles: whole tiles only
  unsigned* range;
};

__global__ __launch_bounds__(512) void k_proj_x3(PjArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  QF_GEMM_WALK(a.Ap, a.Wp, a.mtiles, a.ntiles, a.K);
  for (int item = 0; item < nitems; ++item) {
    QF_GEMM_TILE_TOP;
    QF_GEMM_TILE_PLAN(a.Ap, a.Wp);
    int issued_prev = 0;
    QF_KLOOP_HEAD(QF_PIECE)
    QF_KLOOP_TAIL(QF_PIECE)
    __builtin_amdgcn_s_setprio(0);
    {
      const int mt0 = m0 + wm * 16 * QF_TM, nt0 = n0 + wn * 64;
      const size_t tbase = (size_t)mt0 * a.N + nt0;
      float* const patch = reinterpret_cast<float*>(lds + PJ_PATCH) + wave * (2 * 16 * 64);
      float2* const statp = reinterpret_cast<float2*>(lds + PJ_STATP) + wave * 128;
      x3q_epilogue8<QF_TM, 2, 4, EPI_RESIDUAL, 2, FX_RP | FX_SO, false>(acc, patch, lds + PJ_STATP, a.bias, nullptr, a.X + 2 * tbase, nullptr,
                                                                         a.X + 2 * tbase, nullptr, a.st_out, mt0, nt0, wm * 16 * QF_TM, lane,
                                                                         a.M, a.N, 0, 0, QF_TM, a.out_scale, a.range, statp);
    }
    mt = mtn; nt = ntn;
    __syncthreads();   // the patches (stage 1) are read before the next tile's second k-tile is staged there
  }
}

}  // namespace

bool proj_x3_ok(int N, int K) { return N % 256 == 0 && K % 64 == 0 && K >= 128; }

// X[rows < 192 * (M / 192)] += A W^T + b with the row partials; the caller runs rows beyond the last whole tile through launch_linear_x3p.
hipError_t launch_proj_x3(const void* Apair, const void* Wpair, const float* bias, void* Xpair, float* st_out, int w_exp, int M, int N, int K,
                          hipStream_t s) {
  if (!proj_x3_ok(N, K) || M < QF_BM || M % QF_BM != 0 || !Apair || !Wpair || !bias || !Xpair || !st_out) return hipErrorInvalidValue;
  if (w_exp < -14 || w_exp > 12) return hipErrorInvalidValue;
  PjArgs a{};
  a.Ap = (const _Float16*)Apair; a.Wp = (const _Float16*)Wpair; a.bias = bias; a.X = (_Float16*)Xpair; a.st_out = st_out;
  a.out_scale = ldexpf(1.0f, -(3 + w_exp));
  a.M = M; a.N = N; a.K = K; a.mtiles = M / QF_BM; a.ntiles = N / QF_BN;
  a.range = launch_range_word();
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * a.ntiles, grid)) return ge;
  return launch_lds<k_proj_x3>(dim3(grid), dim3(512), PJ_LDS, s, a);
}

}  // namespace d3d
