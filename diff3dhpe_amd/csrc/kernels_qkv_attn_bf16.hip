// bf16 operand mode (D3D_PREC_BF16), fused: the qkv GEMM of a tile of token groups x ONE head and the GRAND attention of those groups in
// one kernel -- q / k / v are rounded to bf16 where the un-fused qkv GEMM rounds them for its [M][3 D] output and stay in LDS; the
// attention of k_attn_bf16 (kernels_attn_bf16.hip) then runs from LDS.  What it removes from the two-kernel flow: the [M][3 D] bf16
// tensor written by the GEMM and read back by the attention kernel, and one launch per block.
//
// A tile = g = floor(255 / N) whole groups of N tokens (spatial blocks: N = J joints of a frame, token stride 1, 15 frames at J = 17;
// temporal blocks: N = T frames of one (batch, joint), token stride J; 3 joints at T = 81, 1 at T = 243) x the 192 weight rows of one
// head (q, k, v: 64 each).  The operand rows are GATHERED by the LDS-DMA's per-lane source addresses, so both block types share one
// row map; stage rows behind the tile's last group (and groups behind the last one of the launch) repeat a real row: every staged
// value is finite whenever the operand rows are, and nothing outside the M operand rows is read.
//
// The k-loop is the two-phase loop of qkv_fused_kloop.h on a 256 x 192 stage of 64-deep bf16 k-tiles (the stage shape of k_qkv_sattn,
// the MFMA form of k_gemm_bf16q): eight waves (2 x 4), a wave owns 128 rows x 48 columns.  Stage row 48 wn + 16 part + x holds weight
// row part * D + 64 head + 16 wn + x, so accumulator column tile j of wave wn IS part j (q, k, v) at head columns 16 wn .. + 15.  Per
// output element: the same v_mfma_f32_16x16x32_bf16 products in the same k order as launch_gemm_bf16q / launch_linear_bf16, the same
// epilogue arithmetic (fma(acc, 1, bias), q third times 2^-3, round to nearest even) -- the LDS planes hold bit for bit what the
// un-fused GEMM writes to HBM.  The attention step is k_attn_bf16's arithmetic instruction for instruction on those planes.  Pad keys
// of a group are other groups' rows here and zeros there: their scores are overwritten with -inf in both, and their V^T fragment
// elements are replaced by zeros in registers before the second product, so a non-finite value of a neighbouring group (another frame,
// joint or batch element) cannot reach this group's output -- as in the two-kernel flow, a sequence's result depends on its own rows
// only.  The block is bit-identical to the two-kernel flow (tests/test_gpu_bf16_fused_attn.py).
//
// LDS map (156 KiB): [0, 56 K) stage 0 | [56 K, 112 K) stage 1 | from 56 K on, after the k-loop: Q plane (256 rows x 128 B), K plane
// (256 rows), V plane (288 rows: rows 256 .. 287, read for the pad keys of the tile's last group, are zeroed).  Stage 0 stays free behind the
// k-loop: the next tile's first k-tile lands there under this tile's attention step (persistent walk, one workgroup per CU).
#include "d3d_kernels.h"
typedef __bf16 qa_bf8 __attribute__((ext_vector_type(8)));
#define QF_MMA(ACC, BH, BL, AH, AL)                                                                                                   \
  do {                                                                                                                                \
    if constexpr (F16) {   /* (the kernel's template parameter: fp16 operand rows, the f16 twin of the pair) */                       \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BH, AH, ACC, 0, 0, 0);                                                             \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_f16(BL, AL, ACC, 0, 0, 0);                                                             \
    } else {                                                                                                                          \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(qa_bf8, BH), __builtin_bit_cast(qa_bf8, AH), ACC, 0, 0, 0);    \
      ACC = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(qa_bf8, BL), __builtin_bit_cast(qa_bf8, AL), ACC, 0, 0, 0);    \
    }                                                                                                                                 \
  } while (0)
#include "qkv_fused_kloop.h"

#include <math.h>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "attn_lds.h"

typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf4 __attribute__((ext_vector_type(4)));
typedef _Float16 hf8 __attribute__((ext_vector_type(8)));
typedef _Float16 hf4 __attribute__((ext_vector_type(4)));
// The operand element of a kernel: bf16 (D3D_PREC_BF16), or fp16 (F16 = true, D3D_PREC_F16).  E(float) rounds to nearest even in both;
// fp16 keeps subnormals and gives inf beyond 65504.  The two 32x32x16 MFMAs share their lane layouts.
template <bool F16> struct Op16 { typedef __bf16 E; typedef bf8 V8; typedef bf4 V4; };
template <> struct Op16<true> { typedef _Float16 E; typedef hf8 V8; typedef hf4 V4; };
// An fp16 rounding point rounds an fp32 VALUE (as torch's .to(float16) does).  Left to itself the compiler folds the multiply or fma in
// front of some conversions into v_fma_mix{lo,hi}_f16, which rounds the exact product ONCE -- a different result wherever the fp32
// rounding moves the value across an fp16 boundary, and a different one from kernel to kernel (the fused kernel and the stand-alone
// attention kernel got different mixes of the two forms and were not bit-identical).  The register is made opaque: v_cvt of the fp32 value.
__device__ __forceinline__ float f16_point(float x) {
  asm("" : "+v"(x));
  return x;
}
template <bool F16, typename V8>
__device__ __forceinline__ f32x16 op16_mfma32(V8 a, V8 b, f32x16 c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

QF_SHAPE(8, 3, 256, 192, 4, 3);                                          // 256 x 192 stage of 57344 bytes, 64-deep bf16 k-tiles
constexpr int QA_ROWS = 255;                                             // token rows of a tile at most
constexpr int QA_PQ = QF_STAGE, QA_PK = QA_PQ + 256 * 128, QA_PV = QA_PK + 256 * 128;
constexpr int QA_VROWS = 288;
constexpr int QA_LDS = QA_PV + QA_VROWS * 128;                           // 159744
static_assert(QA_LDS <= 160 * 1024, "LDS map");

struct QaArgs {
  const char* A;        // bf16 operand rows [M][D] (norm1(x))
  const char* W;        // bf16 qkv weight rows [3 D][D]
  const float* bias;    // [3 D]
  void* out;            // attention output, bf16 (fp16) [M][D]
  int D, H;             // model width (the GEMM depth), heads (D / 64)
  int N, udiv;          // tokens of a group, token stride: token t of group u is row (u / udiv) * N * udiv + u % udiv + t * udiv
  int g, units, mtiles; // groups per tile, groups of the launch, ceil(units / g)
};

// first row of group `unit` (clamped to the launch's last group)
__device__ __forceinline__ unsigned qa_unit_row(const QaArgs& a, int unit) {
  if (unit >= a.units) unit = a.units - 1;
  const int o = unit / a.udiv;
  return (unsigned)(o * a.N * a.udiv + (unit - o * a.udiv));
}
// operand row of stage row i of M-tile mt: rows behind the tile's last group repeat that group's last row
__device__ __forceinline__ unsigned qa_row(const QaArgs& a, int mt, int i) {
  int u = i / a.N, t = i - u * a.N;
  if (u >= a.g) { u = a.g - 1; t = a.N - 1; }
  return qa_unit_row(a, mt * a.g + u) + (unsigned)(t * a.udiv);
}
// first weight row of the 8 stage rows [s0, s0 + 8): stage row 48 wn + 16 part + x <- weight row part * D + 64 hd + 16 wn + x
__device__ __forceinline__ int qa_wrow(const QaArgs& a, int s0, int hd) {
  const int wn = s0 / 48, rem = s0 - wn * 48;
  return (rem >> 4) * a.D + 64 * hd + 16 * wn + (rem & 15);
}

// One 32-query tile `qt` of the group whose rows start at tile row rb: k_attn_bf16's arithmetic on the LDS planes.
template <int NKT, bool F16>
__device__ __forceinline__ void qa_attention(const unsigned char* lds, int lane, int rb, int qt, int T, typename Op16<F16>::E* out0, size_t tstride,
                                             bool store) {
  typedef typename Op16<F16>::E E;
  typedef typename Op16<F16>::V8 bf8;   // (the names of the bf16 form, for either element type)
  typedef typename Op16<F16>::V4 bf4;
  const unsigned char* const sQ = lds + QA_PQ;
  const unsigned char* const sK = lds + QA_PK;
  const unsigned char* const sV = lds + QA_PV;
  const int r = lane & 31, h = lane >> 5;
  const int tq = 32 * qt + r;
  bf8 qf[4];
  {
    const int qrow = rb + (tq < T ? tq : 0);                       // rows >= T reuse row 0: never stored
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = *reinterpret_cast<const bf8*>(sQ + kswz(qrow, 2 * ks + h));
  }
  const unsigned char* kb[4];
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) kb[ks] = sK + kswz(rb + r, 2 * ks + h);                    // + 4096 kt
  const unsigned char* vb[2][2];
  {
    const int gi = lane & 15, tq_ = gi >> 2, tp_ = gi & 3;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
      const int d0 = dt * 32 + 16 * ((lane >> 4) & 1);
      const int ch = (d0 >> 3) + (tp_ >> 1), sb = (tp_ & 1) * 8;
      vb[dt][0] = sV + vswz(rb + 4 * h + tq_, ch) + sb;                                      // + 2048 (2 kt + s)
      vb[dt][1] = sV + vswz(rb + 4 * h + 8 + tq_, ch) + sb;
    }
  }
  // ---- S^T tiles: rows = keys kt * 32 + (reg & 3) + 8 (reg >> 2) + 4 h, column = query tq
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[kt][q] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const bf8 kf = *reinterpret_cast<const bf8*>(kb[ks] + kt * 4096);
      sacc[kt] = op16_mfma32<F16>(kf, qf[ks], sacc[kt]);
    }
  }
  // ---- exact softmax over the keys of this query column (fp32); only the last key tile can hold keys of other groups
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (kt == NKT - 1) {
        const int key = kt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (key >= T) sacc[kt][q] = -INFINITY;
      }
      m = fmaxf(m, sacc[kt][q]);
    }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  constexpr float LOG2E = 1.4426950408889634f;
  const float mb = m * LOG2E;
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const float e = __builtin_amdgcn_exp2f(fmaf(sacc[kt][q], LOG2E, -mb));
      sacc[kt][q] = e;
      l += e;
    }
  l += __shfl_xor(l, 32, 64);
  const float inv = 1.0f / l;
  {  // softmax - I: the diagonal's numerator becomes e - l (k_attn_bf16)
    const int didx = (((r >> 2) & 1) == h) ? (8 * (r >> 4) + 4 * ((r >> 3) & 1) + (r & 3)) : -1;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      if (kt == qt) {
#pragma unroll
        for (int q = 0; q < 16; ++q) sacc[kt][q] -= (q == didx) ? l : 0.0f;
      }
  }
  // ---- O^T[d][query] = sum_key V^T[d][key] (P - I)^T[key][query]
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf8 pf;
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) pf[jj] = F16 ? (E)f16_point(sacc[kt][8 * s + jj] * inv) : (E)(sacc[kt][8 * s + jj] * inv);
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const s4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(vb[dt][0] + (2 * kt + s) * 2048));
        const s4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(vb[dt][1] + (2 * kt + s) * 2048));
        bf8 vf;
        const bf4 a0b = __builtin_bit_cast(bf4, a0), a1b = __builtin_bit_cast(bf4, a1);
#pragma unroll
        for (int e = 0; e < 4; ++e) { vf[e] = a0b[e]; vf[4 + e] = a1b[e]; }
        if (kt == NKT - 1) {   // pad keys are other groups' rows here: zeros, as the two-kernel flow stages them (0 x NaN / Inf of a neighbour)
#pragma unroll
          for (int jj = 0; jj < 8; ++jj)
            if (kt * 32 + 16 * s + 8 * (jj >> 2) + 4 * h + (jj & 3) >= T) vf[jj] = (E)0.0f;
        }
        oacc[dt] = op16_mfma32<F16>(vf, pf, oacc[dt]);
      }
      __builtin_amdgcn_sched_barrier(0);   // keeps the conversions / V^T reads of later k-steps from being hoisted (VGPR pressure)
    }
  }
  // ---- O rows out as bf16: lane (query tq, half h) holds d = dt * 32 + 8 g4 + 4 h + e
  if (tq < T && store) {
    E* orow = out0 + (size_t)tq * tstride;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        bf4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (E)oacc[dt][4 * g4 + e];
        *reinterpret_cast<bf4*>(orow + dt * 32 + 8 * g4 + 4 * h) = o;
      }
  }
}

template <int NKT, bool F16>
__device__ __forceinline__ void qa_tiles(const QaArgs& a, unsigned char* lds) {
  typedef typename Op16<F16>::E E;
  typedef typename Op16<F16>::V4 bf4;
  const int G = (int)gridDim.x, b = (int)blockIdx.x;
  const int H = a.H;
  const int tiles = a.mtiles * H;
  if (b >= tiles) return;
  const int nitems = (tiles - b + G - 1) / G;
  // tile ordinal -> (M-tile, head): all heads of an M-tile on one XCD, as the GEMMs walk
  KL_XCD_TILE_ORDER(a.mtiles, H);

  const int K = a.D;
  const unsigned rowB = 2u * (unsigned)K;         // bytes of an operand / weight row
  const int nk = K / 64;
  int mt = 0, hd = 0;
  tile_of(b, mt, hd);
  {   // first k-tile of the first tile
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int lr = lane >> 3, csrc = (lane & 7) ^ (((wave & 1) << 2) | (lr >> 1));
#pragma unroll
    for (int it = 0; it < QF_AIT; ++it)
      KL_GLDS(sgpr_ptr(a.A) + (qa_row(a, mt, it * 64 + wave * 8 + lr) * rowB + (unsigned)csrc * 16u), wave * 1024 + lane * 16 + it * 8192);
    const unsigned lofs = (unsigned)lr * rowB + (unsigned)csrc * 16u;
#pragma unroll
    for (int it = 0; it < QF_BIT; ++it)
      KL_GLDS(sgpr_ptr(a.W + (size_t)qa_wrow(a, it * 64 + wave * 8, hd) * rowB) + lofs, QF_AREG + wave * 1024 + lane * 16 + it * 8192);
  }
  int tid_o = (int)threadIdx.x;
  for (int item = 0; item < nitems; ++item) {
    QF_TILE_LANES;
    const bool has_next = item + 1 < nitems;
    int mtn = mt, hdn = hd;
    if (has_next) tile_of((item + 1) * G + b, mtn, hdn);

    // ---- DMA plan: A rows gathered through per-lane offsets from the operand base, W rows from a wave-uniform base per piece
    const int lr_ = lane >> 3;
    const int csrc_ = (lane & 7) ^ (((wave & 1) << 2) | (lr_ >> 1));
    unsigned lofs_ = (unsigned)lr_ * rowB + (unsigned)csrc_ * 16u;
    unsigned offA[QF_AIT], offAn[QF_AIT];
#pragma unroll
    for (int it = 0; it < QF_AIT; ++it) {
      offA[it] = qa_row(a, mt, it * 64 + wave * 8 + lr_) * rowB + (unsigned)csrc_ * 16u;
      offAn[it] = qa_row(a, mtn, it * 64 + wave * 8 + lr_) * rowB + (unsigned)csrc_ * 16u;
    }
    const int dstA = wave * 1024 + lane * 16, dstB = QF_AREG + wave * 1024 + lane * 16;
    // piece IT (A: 0..3, W: 4..6) of k-tile KTT of this tile, or (KTT == nk) of k-tile 0 of the next one
#define QA_PIECE(KTT, IT)                                                                                               \
    do {                                                                                                                \
      const bool nxt_ = (KTT) >= nk;                                                                                    \
      const int st_ = ((KTT) & 1) * QF_STAGE;                                                                           \
      const size_t kofs_ = nxt_ ? (size_t)0 : (size_t)(KTT) * 128;                                                      \
      if ((IT) < QF_AIT) {                                                                                              \
        KL_GLDS(sgpr_ptr(a.A + kofs_) + (nxt_ ? offAn[(IT) % QF_AIT] : offA[(IT) % QF_AIT]), st_ + dstA + (IT) * 8192);  \
      } else {                                                                                                          \
        const char* b_ = a.W + (size_t)qa_wrow(a, ((IT) - QF_AIT) * 64 + wave * 8, nxt_ ? hdn : hd) * rowB + kofs_;     \
        KL_GLDS(sgpr_ptr(b_) + lofs_, st_ + dstB + ((IT) - QF_AIT) * 8192);                                             \
      }                                                                                                                 \
    } while (0)

    QF_TILE_ACC;
    int issued_prev = 0;
    QF_KLOOP_HEAD(QA_PIECE)
    QF_KLOOP_TAIL(QA_PIECE)
    __builtin_amdgcn_s_setprio(0);

    __syncthreads();   // every wave is out of the k-loop: stage 1 and the LDS behind it become the q / k / v planes

    // ---- q / k / v -> planes: fma(acc, 1, bias), the q third times 2^-3, round to nearest even (x3q_epilogue8<.., FX_BF16>)
    if (tid < 256) *reinterpret_cast<uint4*>(lds + QA_PV + 256 * 128 + tid * 16) = make_uint4(0, 0, 0, 0);
    {
      float4 b4[QF_NJ];
#pragma unroll
      for (int j = 0; j < QF_NJ; ++j) b4[j] = *reinterpret_cast<const float4*>(a.bias + j * a.D + 64 * hd + 16 * wn + 4 * q);
      const int chunk = 2 * wn + (q >> 1), half8 = (q & 1) << 3;          // this lane's 8 bytes: 16-byte chunk d / 8, half (d & 4)
#pragma unroll
      for (int i = 0; i < QF_TM; ++i) {
        const int R = wm * 16 * QF_TM + 16 * i + r16;
        unsigned char* const pkq = lds + kswz(R, chunk) + half8;
        unsigned char* const pv = lds + QA_PV + vswz(R, chunk) + half8;
#pragma unroll
        for (int j = 0; j < QF_NJ; ++j) {
          const float osc = j == 0 ? 0.125f : 1.0f;
          const float bj[4] = {b4[j].x, b4[j].y, b4[j].z, b4[j].w};
          bf4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) o[e] = F16 ? (E)f16_point(__builtin_fmaf(acc[i][j][e], 1.0f, bj[e]) * osc) : (E)(__builtin_fmaf(acc[i][j][e], 1.0f, bj[e]) * osc);
          *reinterpret_cast<bf4*>(j == 0 ? pkq + QA_PQ : (j == 1 ? pkq + QA_PK : pv)) = o;
        }
      }
    }
    __syncthreads();

    // ---- attention: (group, 32-query tile) jobs of the tile over the eight waves
    {
      const int jobs = a.g * NKT;
      for (int job = wave; job < jobs; job += 8) {
        const int u = job / NKT, qt = job - u * NKT;
        if (32 * qt >= a.N) continue;
        const int unit = mt * a.g + u;
        const bool ok = unit < a.units;                                   // (wave-uniform)
        if (!ok) continue;
        E* const out0 = reinterpret_cast<E*>(a.out) + (size_t)qa_unit_row(a, unit) * a.D + 64 * hd;
        qa_attention<NKT, F16>(lds, lane, u * a.N, qt, a.N, out0, (size_t)a.udiv * a.D, true);
      }
    }
    mt = mtn; hd = hdn;
    __syncthreads();   // the planes are read before the next tile's second k-tile is staged over them
  }
}

}  // namespace

// spatial blocks: groups of N <= 32 tokens (the joints of a frame), one key tile
template <bool F16>
__global__ __launch_bounds__(512) void k_qkv_sattn_bf16(QaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  qa_tiles<1, F16>(a, lds);
}
// temporal blocks: groups of N <= 255 tokens (the frames of one joint), NKT = ceil(N / 32) key tiles
template <int NKT, bool F16>
__global__ __launch_bounds__(512) void k_qkv_tattn_bf16(QaArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  qa_tiles<NKT, F16>(a, lds);
}

// Shapes the fused kernels exist for: head width 64, GEMM depth D a multiple of 128 from 256 on (whole pairs of 64-deep k-tiles, as
// launch_gemm_bf16q), groups of at most 255 tokens (one tile holds whole groups), operand offsets that fit 32 bits.
static bool qkv_attn_bf16_shape_ok(long long groups, int N, int D, int H) {
  return N >= 1 && N <= QA_ROWS && H > 0 && D == 64 * H && D % 128 == 0 && D >= 256 && groups >= 1 && groups * N * (long long)D * 2 < (1LL << 32);
}
bool qkv_sattn_bf16_ok(int T, int J, int D, int H, int B) { return J <= 32 && qkv_attn_bf16_shape_ok((long long)B * T, J, D, H); }
bool qkv_tattn_bf16_ok(int T, int J, int D, int H, int B) { return qkv_attn_bf16_shape_ok((long long)B * J, T, D, H); }

template <auto Kfn>
static hipError_t qa_launch(const QaArgs& a, hipStream_t s) {
  int grid = 0;
  if (hipError_t ge = persistent_grid((long long)a.mtiles * a.H, grid)) return ge;
  return launch_lds<Kfn>(dim3(grid), dim3(512), QA_LDS, s, a);
}

// A: bf16 [groups * N][D]; W: bf16 [3 D][D]; bias: [3 D]; out: bf16 [groups * N][D] (not A: every head reads whole rows of A).
// Group u holds rows (u / stride) * N * stride + u % stride + t * stride, t < N -- spatial blocks: (B * T, J, 1), temporal: (B * J, T, J).
template <bool F16>
static hipError_t qa_launch_form(const QaArgs& a, int temporal, hipStream_t s) {
  if (!temporal) return qa_launch<k_qkv_sattn_bf16<F16>>(a, s);
  switch ((a.N + 31) / 32) {
    case 1: return qa_launch<k_qkv_tattn_bf16<1, F16>>(a, s);
    case 2: return qa_launch<k_qkv_tattn_bf16<2, F16>>(a, s);
    case 3: return qa_launch<k_qkv_tattn_bf16<3, F16>>(a, s);
    case 4: return qa_launch<k_qkv_tattn_bf16<4, F16>>(a, s);
    case 5: return qa_launch<k_qkv_tattn_bf16<5, F16>>(a, s);
    case 6: return qa_launch<k_qkv_tattn_bf16<6, F16>>(a, s);
    case 7: return qa_launch<k_qkv_tattn_bf16<7, F16>>(a, s);
    default: return qa_launch<k_qkv_tattn_bf16<8, F16>>(a, s);
  }
}

// f16: fp16 operand rows / weights / output (D3D_PREC_F16).
hipError_t launch_qkv_attn_bf16(const void* A, const void* W, const float* bias, void* out, int groups, int N, int stride, int D, int H,
                                int temporal, hipStream_t s, bool f16) {
  if (!A || !W || !bias || !out || A == out || stride < 1 || groups < 1 || groups % stride != 0) return hipErrorInvalidValue;
  if (!qkv_attn_bf16_shape_ok(groups, N, D, H) || (!temporal && N > 32)) return hipErrorInvalidValue;
  QaArgs a{};
  a.A = (const char*)A; a.W = (const char*)W; a.bias = bias; a.out = out;
  a.D = D; a.H = H; a.N = N; a.udiv = stride;
  a.g = QA_ROWS / N; a.units = groups; a.mtiles = (groups + a.g - 1) / a.g;
  return f16 ? qa_launch_form<true>(a, temporal, s) : qa_launch_form<false>(a, temporal, s);
}

}  // namespace d3d
