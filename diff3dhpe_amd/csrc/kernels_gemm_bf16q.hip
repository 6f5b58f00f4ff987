// The two plain GEMMs of the bf16 operand mode (D3D_PREC_BF16, second-class: DESIGN.md section 4.4) -- qkv = h Wqkv^T + b (q third
// pre-scaled by dh^-1/2) and hidden = gelu(h W1^T + b1), bf16 rows in, bf16 rows out (S2S:67, 46-48 on operands rounded to bf16) -- on the
// hand-specialised two-phase k-loop of the fused F16X3 kernels (qkv_fused_kloop.h) with a 256 x 256 stage of 64-deep bf16 k-tiles: eight
// waves (2 x 4) of 128 rows x 64 columns, the shape and the MFMA order of k_linear_x3q_persist<8,2,4, EPI, bf16-out, FX_BF16>, whose
// epilogue function (x3q_epilogue8) it calls.  Per element the same MFMAs in the same order and the same epilogue arithmetic: bit for bit
// the template's result (tests/test_gpu_round5.py).  What this kernel does not carry: tail slices, run-time group ranges, the one-barrier
// fallback; the ragged last M-tile goes through the checked instantiation of the same epilogue.
#include "d3d_kernels.h"
typedef __bf16 bq_bf8 __attribute__((ext_vector_type(8)));
#define QF_MMA(ACC, BH, BL, AH, AL)                                                                                                   \
  do {                                                                                                                                \
    if constexpr (F16) {   /* (the kernel's template parameter: fp16 operand rows, the f16 twin of the pair) */                       \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BH, AH, ACC, 0, 0, 0);                                                             \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BL, AL, ACC, 0, 0, 0);                                                             \
    } else {                                                                                                                          \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bq_bf8, BH), __builtin_bit_cast(bq_bf8, AH), ACC, 0, 0, 0);    \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bq_bf8, BL), __builtin_bit_cast(bq_bf8, AL), ACC, 0, 0, 0);    \
    }                                                                                                                                 \
  } while (0)
#include "qkv_fused_kloop.h"

#include <math.h>
#include <stdio.h>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "gemm_x3p_prelude.h"
#include "gemm_x3p_epilogue.h"

QF_SHAPE(8, 4, 256, 256, 4, 4);                                          // 256 x 256 stage of 65536 bytes, 64-deep bf16 k-tiles
constexpr int BQ_PATCH = QF_STAGE;                                       // eight 8 KiB transpose patches over stage 1
constexpr int BQ_LDS = 2 * QF_STAGE;                                     // 131072
static_assert(BQ_PATCH + 65536 <= BQ_LDS, "LDS map");

struct BqArgs {
  const _Float16* Ap;      // bf16 operand rows [>= 256 mtiles rows][K] (passed as 16-bit words; "pair columns" K2 = K / 2 per 4 bytes)
  const _Float16* Wp;      // bf16 weight rows [N padded to 256][K]
  const float* bias;
  _Float16* out;           // bf16 rows [M][N]
  int M, N, Kp, mtiles, ntiles, qcols;   // Kp = K / 2: a row is 4 Kp bytes = Kp / 32 staged 128-byte lines
  unsigned* range;
};

// F16: fp16 operand rows (D3D_PREC_F16) -- the f16 MFMA pair and the FX_F16 epilogue; the bf16 instantiations are what they were.
template <int EPI, bool F16>
__global__ __launch_bounds__(512) void k_gemm_bf16q(BqArgs a) {
  constexpr int FXQ = F16 ? (FX_BF16 | FX_F16) : FX_BF16;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  QF_GEMM_WALK(a.Ap, a.Wp, a.mtiles, a.ntiles, a.Kp);   // (K2 = K: 16-bit words per operand row)
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
      float* const patch = reinterpret_cast<float*>(lds + BQ_PATCH) + wave * (2 * 16 * 64);
      if (m0 + QF_BM <= a.M)     // (wave-uniform: a whole tile)
        x3q_epilogue8<QF_TM, 2, 4, EPI, 3, FXQ, false>(acc, patch, lds, a.bias, nullptr, a.out + tbase, nullptr, nullptr, nullptr, nullptr,
                                                        mt0, nt0, wm * 16 * QF_TM, lane, a.M, a.N, a.qcols, 0, QF_TM, 1.0f, a.range);
      else                       // the ragged last M-tile: rows >= M are computed from the operand buffer's pad rows and not stored
        x3q_epilogue8<QF_TM, 2, 4, EPI, 3, FXQ, true>(acc, patch, lds, a.bias, nullptr, a.out + tbase, nullptr, nullptr, nullptr, nullptr,
                                                       mt0, nt0, wm * 16 * QF_TM, lane, a.M, a.N, a.qcols, 0, QF_TM, 1.0f, a.range);
    }
    mt = mtn; nt = ntn;
    __syncthreads();   // the patches (stage 1) are read before the next tile's second k-tile is staged there
  }
}

}  // namespace

// N a multiple of 256 (whole N-tiles: weight rows padded alike), K a multiple of 128 (an even number >= 2 of 64-deep k-tiles)
bool gemm_bf16q_ok(int N, int K) { return N % 256 == 0 && K % 128 == 0 && K >= 256; }

// Cb[M][N] (bf16) = epi(A[Mp][K] W[N][K]^T + bias), q scaling for columns < qcols; A's buffer spans whole 256-row tiles (pad rows finite or not:
// their results are not stored).  epi: EPI_NONE or EPI_GELU.
hipError_t launch_gemm_bf16q(const void* A, const void* W, const float* bias, void* Cb, int M, int N, int K, int epi, int qcols, hipStream_t s,
                             bool f16) {
  if (!gemm_bf16q_ok(N, K) || M < 1 || !A || !W || !bias || !Cb || (epi != EPI_NONE && epi != EPI_GELU)) return hipErrorInvalidValue;
  BqArgs a{};
  a.Ap = (const _Float16*)A; a.Wp = (const _Float16*)W; a.bias = bias; a.out = (_Float16*)Cb;
  a.M = M; a.N = N; a.Kp = K / 2; a.mtiles = (M + QF_BM - 1) / QF_BM; a.ntiles = N / QF_BN; a.qcols = qcols;
  a.range = launch_range_word();
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * a.ntiles, grid)) return ge;
  if (f16)
    return epi == EPI_GELU ? launch_lds<k_gemm_bf16q<EPI_GELU, true>>(dim3(grid), dim3(512), BQ_LDS, s, a)
                           : launch_lds<k_gemm_bf16q<EPI_NONE, true>>(dim3(grid), dim3(512), BQ_LDS, s, a);
  return epi == EPI_GELU ? launch_lds<k_gemm_bf16q<EPI_GELU, false>>(dim3(grid), dim3(512), BQ_LDS, s, a)
                         : launch_lds<k_gemm_bf16q<EPI_NONE, false>>(dim3(grid), dim3(512), BQ_LDS, s, a);
}

}  // namespace d3d
