// F16X3 flow, fused, SMALL tiles (the "small_tiles" engine option of "latency_mode"): the LayerNorm-folded qkv GEMM of a 128-row tile of
// token groups x ONE head and the GRAND attention of those groups in one kernel -- q / k / v hi / lo planes stay in LDS.  What
// kernels_qkv_sattn.hip / kernels_qkv_tattn.hip do on 256-row tiles, for calls so small that those leave most CUs idle (one window at a
// time: 48 workgroups at T = 81, B = 1): half the rows per workgroup, twice the workgroups, half the k-loop MFMAs per workgroup.
// Structured like the bf16 fused kernels (kernels_qkv_attn_bf16.hip), not like the two large F16X3 ones.
//
// A tile = g = floor(127 / N) whole groups of N tokens (spatial blocks: N = J joints of a frame, token stride 1, 7 frames at J = 17;
// temporal blocks: N = T <= 127 frames of one (batch, joint), token stride J; 4 joints at T = 27, 1 at T = 81) x the 192 weight rows of
// one head (q, k, v: 64 each, the TILE ORDER of the folded weight: kernels_qkv_sattn.hip).  The operand rows are GATHERED by the
// LDS-DMA's per-lane source addresses, so both block types share one row map; stage rows behind the tile's last group (and groups behind
// the last one of the launch) repeat a real row: nothing outside the M operand rows is read.  One tile per workgroup, grid = tiles x 8.
//
// The k-loop is the two-phase loop of qkv_fused_kloop.h on a 128 x 192 x 32 stage: eight waves (2 x 4), a wave owns 64 rows x 48
// columns; accumulator column tile j of wave wn IS part j (q, k, v) at head columns 16 wn .. + 15.  Per output element the same three
// fp16 MFMAs in the same k order as every other F16X3 GEMM shape, and the epilogue arithmetic of x3q_epilogue8<LN-folded, planes> (fold
// with the row statistics partials, bias, hi / lo split): the LDS planes hold bit for bit what the unfused qkv GEMM writes to HBM.  The
// attention step is attn_x3_tile.h's arithmetic, the pieces of k_attn_temporal_x3<NKT> (what launch_attn_temporal_x3 runs for N <= 127, and what qs_attention of
// kernels_qkv_sattn.hip reproduces for the joints of a frame) on those planes, per (group, 32-query tile) job over the eight waves.
// The planes are COMPACT: group u of the tile starts at plane row u N, so the pad keys [N, 32 ceil(N / 32)) of a group are the next
// group's rows (or the tile's pad rows, or the rows behind the plane): their scores are overwritten with -inf and their V^T fragment
// elements are replaced by zeros in registers before the second product, so a non-finite value of a neighbouring group (another
// frame, joint or batch element) cannot reach this group's output.  The block is bit-identical to the two-kernel flow
// (tests/test_gpu_small_tiles.py).
//
// Synchronisation: workgroup barriers only (the k-loop's phase barriers, one in front of the plane writes, one behind them); every wave
// reaches every barrier, trip counts depend on (N, groups per tile) alone.
//
// LDS map (137 KiB, one workgroup per CU): [0, 40 K) stage 0 | [40 K, 80 K) stage 1; after the k-loop, from 0: Q hi | Q lo | K hi | K lo
// planes of 128 rows x 128 B, V hi | V lo planes of 160 rows (rows 128 .. 159, read for the pad keys of the tile's last group, are
// zeroed), one 4 KiB output patch per wave; behind them 1 KiB of per-row LayerNorm statistics.
//
// NARROW heads (the "fused_narrow" engine option, not tied to "latency_mode"): the same kernel for heads of 32 columns in pairs (D = 32 H)
// or of 16 columns in quads (D = 16 H) -- a pair / a quad is one 64-column segment of the plane rows, the "head" of everything above, and
// a row tile has D / 64 of them.  Only the attention step differs (qm_attention_narrow: every head of the segment with its own scores,
// softmax and sum, as k_attn_x3_h32 / k_attn_x3_h16) and is bit-identical to the folded qkv GEMM followed by those kernels
// (tests/test_gpu_fused_narrow.py).
#include "d3d_kernels.h"
#include "qkv_fused_kloop.h"

#include <math.h>
#include <type_traits>

namespace d3d {
namespace {

#include "kloop_common.h"
#include "attn_lds.h"
#include "attn_x3_tile.h"

QF_SHAPE(4, 3, 128, 192, 2, 3);                                          // 128 x 192 x 32 stage of 40960 bytes
constexpr int QM_ROWS = 127;                                             // token rows of a tile at most
constexpr int QM_PLANE = QF_BM * 128;                                    // one fp16 plane of 128 rows x 64 dims
constexpr int QM_VROWS = 160, QM_VPLANE = QM_VROWS * 128;
constexpr int QM_Q = 0, QM_K = 2 * QM_PLANE, QM_V = 4 * QM_PLANE;        // lo plane: + QM_PLANE (Q, K), + QM_VPLANE (V)
constexpr int QM_PATCH = QM_V + 2 * QM_VPLANE;                           // eight 4 KiB output patches
constexpr int QM_STX = QM_PATCH + 8 * 4096;                              // (rstd', -mean rstd) of the tile's 128 rows
constexpr int QM_LDS = QM_STX + QF_BM * 8;                               // 140288
static_assert(QM_LDS <= 160 * 1024 && 2 * QF_STAGE <= QM_STX, "LDS map");
// the 32-row fragment reads of a group's last key tile end at most 31 rows behind the last real row: inside the next plane
static_assert(QM_ROWS + 31 < QM_VROWS && QM_K + QM_PLANE + (QM_ROWS + 32) * 128 <= QM_PATCH, "pad-key reads stay inside the planes");
constexpr int QM_STREG = 8;                                              // statistics partials per row held in registers over the k-loop

struct QmArgs {
  const char* A;           // residual stream, pair layout [M rows][2 K] of 8 x
  const char* W;           // folded qkv weight W diag(gamma), pair layout, 2^k w, rows in TILE order (kernels_qkv_sattn.hip)
  const float* bias;       // b + W beta, tile order
  const float* csum;       // sum_k W[n, k] gamma[k], tile order
  const float* st_in;      // (sum, sum of squares) partials of the rows: [rows][st_np][2]
  int st_np;
  float eps, out_scale;    // LayerNorm eps; 2^-(3 + k)
  _Float16* out;           // attention output, pair layout [M][2 D] of 8 o
  int K, D;                // GEMM depth, model width (8 heads x 64)
  int N, udiv;             // tokens of a group, token stride: token t of group u is row (u / udiv) * N * udiv + u % udiv + t * udiv
  int g, units, mtiles;    // groups per tile, groups of the launch, ceil(units / g)
  int nseg;                // 64-column segments of a row = workgroups per M-tile: D / 64 (read by the narrow forms alone; 8 at width 64)
  unsigned* range;         // the engine's range-guard word
};

// first row of group `unit` (clamped to the launch's last group)
__device__ __forceinline__ unsigned qm_unit_row(const QmArgs& a, int unit) {
  if (unit >= a.units) unit = a.units - 1;
  const int o = unit / a.udiv;
  return (unsigned)(o * a.N * a.udiv + (unit - o * a.udiv));
}
// operand row of stage row i of M-tile mt: rows behind the tile's last group repeat that group's last row
__device__ __forceinline__ unsigned qm_row(const QmArgs& a, int mt, int i) {
  int u = i / a.N, t = i - u * a.N;
  if (u >= a.g) { u = a.g - 1; t = a.N - 1; }
  return qm_unit_row(a, mt * a.g + u) + (unsigned)(t * a.udiv);
}

// One 32-query tile `qt` of the group whose plane rows start at rb: the pieces of attn_x3_tile.h (k_attn_temporal_x3<NKT>'s arithmetic) on
// the LDS planes; outputs through the wave's patch as whole 128-byte lines of the pair layout.
template <int NKT>
__device__ __forceinline__ void qm_attention(unsigned char* lds, int wave, int lane, int rb, int qt, int T, _Float16* out0, size_t tstride,
                                             unsigned* rw) {
  const unsigned char* const sQh = lds + QM_Q;
  const unsigned char* const sKh = lds + QM_K;
  const unsigned char* const sVh = lds + QM_V;
  const unsigned char* const sVl = lds + QM_V + QM_VPLANE;
  unsigned char* const patch = lds + QM_PATCH + wave * 4096;
  const int r = lane & 31, h = lane >> 5;
  const int tq = 32 * qt + r;
  const int tqc = tq < T ? tq : 0;                                   // rows >= T reuse row 0: never stored
  h8 qh[4], ql[4];
  x3_q_lds(sQh, sQh + QM_PLANE, rb + tqc, h, qh, ql);
  // ---- S^T tiles, softmax numerators (in sacc) and their sum; only the last key tile can hold keys of other groups
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile(sKh, sKh + QM_PLANE, rb + kt * 32, r, h, qh, ql);
  const float l = x3_softmax<NKT>(sacc, h, T);
  // ---- O^T; the pad keys [T, 32 NKT) are other groups' rows here and zeros in the stand-alone kernel: their V bits are masked
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) x3_pv_tile<true>(sacc[kt], sVh, sVl, rb, kt, T, lane, h, oacc);
  // ---- O = O^T / (2^13 l) - v_query (v_query from the V planes), packed as hi / lo of 8 o; whole lines out through the patch
  u32x4 po[8];                  // [dt * 4 + pp]: row 32 qt + 8 pp + (lane >> 3), chunk lane & 7 of line dt
  {
    const float inv = 1.0f / (8192.0f * l);
    float amax = 0.0f;          // range guard (rows tq >= T are never stored)
#pragma unroll
    for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int vo = vswz(rb + tqc, dt * 4 + g4) + 8 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[dt], g4, inv, *reinterpret_cast<const h4*>(sVh + vo), *reinterpret_cast<const h4*>(sVl + vo), amax, oh, ol);
        patch_wr(patch, r, h, g4, oh, ol);
      }
      asm volatile("" ::: "memory");     // (the rows read back were written by other lanes)
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) po[dt * 4 + pp] = patch_rd(patch, 8 * pp + (lane >> 3), lane & 7);
      asm volatile("" ::: "memory");     // (line dt + 1, and the wave's next job, reuse the patch)
    }
    if (tq < T && amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
  _Float16* const po_ptr = out0 + (size_t)(32 * qt + (lane >> 3)) * tstride + 8 * (lane & 7);
#pragma unroll
  for (int pp = 0; pp < 4; ++pp)
    if (32 * qt + 8 * pp + (lane >> 3) < T) {
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(po_ptr + (size_t)(8 * pp) * tstride + dt * 64) = po[dt * 4 + pp];
    }
}

// The same job for heads NARROWER than the 64-column segment ("fused_narrow"): DH = 32, two heads per segment, or DH = 16, four.  The streams
// of x3_head_shape<DH> one after the other, each with its own scores, softmax and sum, as k_attn_x3_h32 / k_attn_x3_h16 run them on the
// planes in HBM: head p of a pair takes d-steps 2 p, 2 p + 1 and 32-column line p; head p of a quad takes d-step p and rows
// 16 (p & 1) .. + 15 of an accumulator of its own over line p >> 1 (the other 16 rows, the line neighbour's V times this head's E, stay in
// registers).  A line leaves through the patch as soon as its heads are done, so one stream's tiles are live at a time.
template <int NKT, int DH>
__device__ __forceinline__ void qm_attention_narrow(unsigned char* lds, int wave, int lane, int rb, int qt, int T, _Float16* out0, size_t tstride,
                                                    unsigned* rw) {
  static_assert(DH == 32 || DH == 16, "two or four heads per 64-column segment");
  const unsigned char* const sQh = lds + QM_Q;
  const unsigned char* const sKh = lds + QM_K;
  const unsigned char* const sVh = lds + QM_V;
  const unsigned char* const sVl = lds + QM_V + QM_VPLANE;
  unsigned char* const patch = lds + QM_PATCH + wave * 4096;
  const int tq = 32 * qt + (lane & 31);
  const int tqc = tq < T ? tq : 0;                                   // rows >= T reuse row 0: never stored
  _Float16* const po_ptr = out0 + (size_t)(32 * qt + (lane >> 3)) * tstride + 8 * (lane & 7);
  float amax = 0.0f;            // range guard (rows tq >= T are never stored)
  auto stream = [&](auto pc) {
    constexpr int P = decltype(pc)::value;
    constexpr int KS0 = DH == 32 ? 2 * P : P, NKS = DH == 32 ? 2 : 1;   // the head's d-steps of the segment
    constexpr int DT = DH == 32 ? P : P >> 1;                           // its 32-column line
    constexpr int G0 = DH == 32 ? 0 : 2 * (P & 1), NG = DH == 32 ? 4 : 2;   // its 8-column chunks of that line
    // Every LDS address of a stream depends on (lane, rb) alone, so the compiler forms those of all streams up front and overlaps the
    // streams' tiles (scratch at NKT = 4).  A scheduling barrier and an opaque copy of the lane per stream keep them one after the other.
    __builtin_amdgcn_sched_barrier(0);
    int lane_s = lane;
    asm volatile("" : "+v"(lane_s));
    const int r = lane_s & 31, h = lane_s >> 5;
    h8 qh[4], ql[4];            // ([KS0, KS0 + NKS) alone are used)
#pragma unroll
    for (int ks = KS0; ks < KS0 + NKS; ++ks) {
      const int qo = kswz(rb + tqc, 2 * ks + h);
      qh[ks] = *reinterpret_cast<const h8*>(sQh + qo);
      ql[ks] = *reinterpret_cast<const h8*>(sQh + QM_PLANE + qo);
    }
    f32x16 sacc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile<KS0, NKS>(sKh, sKh + QM_PLANE, rb + kt * 32, r, h, qh, ql);
    const float l = x3_softmax<NKT, DH>(sacc, h, T);
    f32x16 oacc[2];             // ([DT] alone is used; at width 16 only the head's 16 rows of it are stored)
#pragma unroll
    for (int q = 0; q < 16; ++q) oacc[DT][q] = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) x3_pv_tile<true, DT, 1>(sacc[kt], sVh, sVl, rb, kt, T, lane_s, h, oacc);
    const float inv = 1.0f / (8192.0f * l);
#pragma unroll
    for (int g4 = G0; g4 < G0 + NG; ++g4) {
      const int vo = vswz(rb + tqc, DT * 4 + g4) + 8 * h;
      h4 oh, ol;
      x3_out_chunk(oacc[DT], g4, inv, *reinterpret_cast<const h4*>(sVh + vo), *reinterpret_cast<const h4*>(sVl + vo), amax, oh, ol);
      patch_wr(patch, r, h, g4, oh, ol);
    }
    if constexpr (DH == 32 || (P & 1)) {   // line DT is whole: out as 128-byte lines of the pair layout
      asm volatile("" ::: "memory");       // (the rows read back were written by other lanes)
      u32x4 po[4];                         // [pp]: row 32 qt + 8 pp + (lane >> 3), chunk lane & 7 of line DT
#pragma unroll
      for (int pp = 0; pp < 4; ++pp) po[pp] = patch_rd(patch, 8 * pp + (lane_s >> 3), lane_s & 7);
      asm volatile("" ::: "memory");       // (the next line, and the wave's next job, reuse the patch)
#pragma unroll
      for (int pp = 0; pp < 4; ++pp)
        if (32 * qt + 8 * pp + (lane_s >> 3) < T) *reinterpret_cast<u32x4*>(po_ptr + (size_t)(8 * pp) * tstride + DT * 64) = po[pp];
    }
  };
  stream(std::integral_constant<int, 0>{});
  stream(std::integral_constant<int, 1>{});
  if constexpr (DH == 16) {
    stream(std::integral_constant<int, 2>{});
    stream(std::integral_constant<int, 3>{});
  }
  if (tq < T && amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
}

}  // namespace

// NKT = ceil(N / 32) key tiles of a group: 1 for the spatial blocks and temporal groups of <= 32 frames, up to 4 (N <= 127)
// DH: the head width -- 64: one head per 64-column segment, eight segments ("small_tiles"); 32 / 16: a pair / a quad of heads per segment,
// D / 64 segments ("fused_narrow").  Everything but the attention step and the segment count is the width's own copy of the same code.
template <int NKT, int DH = 64>
__global__ __launch_bounds__(512) void k_qkv_attn_x3_small(QmArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  const int b = (int)blockIdx.x;
  const int nseg = DH == 64 ? 8 : a.nseg;
  KL_XCD_TILE_ORDER(a.mtiles, nseg);   // all heads of an M-tile on one XCD, as the GEMMs walk
  int mt = 0, hd = 0;
  tile_of(b, mt, hd);
  const int K = a.K;
  const unsigned rowB = 4u * (unsigned)K;          // bytes of an operand / weight row (pair layout)
  const int nk = K / 32;
  constexpr bool has_next = false;                 // one tile per workgroup
  int tid_o = (int)threadIdx.x;
  QF_TILE_LANES;

  // ---- DMA plan: A rows gathered through per-lane offsets from the operand base, W rows (contiguous: tile order) from a wave-uniform base
  const int lr_ = lane >> 3;
  const int csrc_ = (lane & 7) ^ (((wave & 1) << 2) | (lr_ >> 1));
  unsigned lofs_ = (unsigned)lr_ * rowB + (unsigned)csrc_ * 16u;
  unsigned offA[QF_AIT];
#pragma unroll
  for (int it = 0; it < QF_AIT; ++it) offA[it] = qm_row(a, mt, it * 64 + wave * 8 + lr_) * rowB + (unsigned)csrc_ * 16u;
  const char* const ubB = a.W + (size_t)(hd * QF_BN + wave * 8) * rowB;
  const size_t it_stride = (size_t)64 * rowB;
  const int dstA = wave * 1024 + lane * 16, dstB = QF_AREG + wave * 1024 + lane * 16;
  // piece IT (A: 0, 1; W: 2..4) of k-tile KTT of this tile
#define QM_PIECE(KTT, IT)                                                                                               \
  do {                                                                                                                  \
    const int st_ = ((KTT) & 1) * QF_STAGE;                                                                             \
    const size_t kofs_ = (size_t)(KTT) * 128;                                                                           \
    if ((IT) < QF_AIT) {                                                                                                \
      KL_GLDS(sgpr_ptr(a.A + kofs_) + offA[(IT) % QF_AIT], st_ + dstA + (IT) * 8192);                                   \
    } else {                                                                                                            \
      KL_GLDS(sgpr_ptr(ubB + kofs_ + ((IT) - QF_AIT) * it_stride) + lofs_, st_ + dstB + ((IT) - QF_AIT) * 8192);        \
    }                                                                                                                   \
  } while (0)
  QM_PIECE(0, 0); QM_PIECE(0, 1); QM_PIECE(0, 2); QM_PIECE(0, 3); QM_PIECE(0, 4);   // first k-tile

  // ---- row statistics of the folded LayerNorm: thread t < 128 serves tile row t; up to QM_STREG raw partials are requested here and
  // summed in front of the last k-tile (they landed long before), more than that are read there
  const bool st_reg = a.st_np <= QM_STREG;   // (uniform)
  float2 straw[QM_STREG];
  const float2* straw_p = nullptr;
  if (tid < QF_BM) {
    straw_p = reinterpret_cast<const float2*>(a.st_in) + (size_t)qm_row(a, mt, tid) * a.st_np;
#pragma unroll
    for (int p = 0; p < QM_STREG; ++p) straw[p] = (st_reg && p < a.st_np) ? straw_p[p] : make_float2(0.f, 0.f);
  }

  QF_TILE_ACC;
  int issued_prev = 0;
  QF_KLOOP_HEAD(QM_PIECE)
  if (tid < QF_BM) {   // (rstd * out_scale, -mean rstd) of tile row tid: the arithmetic of the fused kernels' statistics step
    float sm = 0.f, sq = 0.f;
    if (st_reg) {
#pragma unroll
      for (int p = 0; p < QM_STREG; ++p)
        if (p < a.st_np) { sm += straw[p].x; sq += straw[p].y; }
    } else {
      for (int p = 0; p < a.st_np; ++p) { sm += straw_p[p].x; sq += straw_p[p].y; }
    }
    if (sq >= (X3_HALF_MAX * 0.125f) * (X3_HALF_MAX * 0.125f)) range_raise(a.range, RANGE_BIT_ACT);   // (producer's planes, as x3q_tile)
    const float mean = sm / (float)K;
    const float var = fmaxf(sq / (float)K - mean * mean, 0.0f);
    if (mean * mean > 256.0f * var) range_raise(a.range, RANGE_BIT_STATS);
    const float rstd = 1.0f / sqrtf(var + a.eps);
    reinterpret_cast<float2*>(lds + QM_STX)[tid] = make_float2(rstd * a.out_scale, -mean * rstd);
  }
  QF_KLOOP_TAIL(QM_PIECE)
#undef QM_PIECE
  __builtin_amdgcn_s_setprio(0);

  __syncthreads();   // statistics visible; every wave is out of the k-loop: the stages become the q / k / v planes

  // ---- q / k / v -> planes (LayerNorm fold and hi / lo split of x3q_epilogue8; column tile j of a wave is q / k / v: plane and scale are
  // compile-time per j).  Lane: rows 64 wm + 16 i + r16, head dims 16 wn + 4 q .. + 3 = 8 bytes of 16-byte chunk 2 wn + (q >> 1).
  {   // V rows 128 .. 159 of both planes
    const int pl = tid >> 8, rem = tid & 255;
    *reinterpret_cast<uint4*>(lds + QM_V + pl * QM_VPLANE + QF_BM * 128 + rem * 16) = make_uint4(0, 0, 0, 0);
  }
  {
    typedef float f2 __attribute__((ext_vector_type(2)));
    float4 cs4[QF_NJ], b4[QF_NJ];
#pragma unroll
    for (int j = 0; j < QF_NJ; ++j) {
      const int n = hd * QF_BN + wn * 48 + 16 * j + 4 * q;
      cs4[j] = *reinterpret_cast<const float4*>(a.csum + n);
      b4[j] = *reinterpret_cast<const float4*>(a.bias + n);
    }
    const int chunk = 2 * wn + (q >> 1), half8 = (q & 1) << 3;
    float amaxj[QF_NJ] = {0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < QF_TM; ++i) {
      const int R = wm * 16 * QF_TM + 16 * i + r16;
      const float2 st = reinterpret_cast<const float2*>(lds + QM_STX)[R];
      const f2 sx = (f2)(st.x), sy = (f2)(st.y);
      unsigned char* const pkq = lds + kswz(R, chunk) + half8;
      unsigned char* const pv = lds + QM_V + vswz(R, chunk) + half8;
#pragma unroll
      for (int j = 0; j < QF_NJ; ++j) {
        const float osc = j == 0 ? 1.0f : 8.0f;
        f2 a01, a23, c01, c23, b01, b23;
        a01.x = acc[i][j][0]; a01.y = acc[i][j][1]; a23.x = acc[i][j][2]; a23.y = acc[i][j][3];
        c01.x = cs4[j].x; c01.y = cs4[j].y; c23.x = cs4[j].z; c23.y = cs4[j].w;
        b01.x = b4[j].x; b01.y = b4[j].y; b23.x = b4[j].z; b23.y = b4[j].w;
        const f2 v01 = __builtin_elementwise_fma(sx, a01, __builtin_elementwise_fma(sy, c01, b01));
        const f2 v23 = __builtin_elementwise_fma(sx, a23, __builtin_elementwise_fma(sy, c23, b23));
        amaxj[j] = fmaxf(fmaxf(amaxj[j], fabsf(v01.x)), fabsf(v01.y));
        amaxj[j] = fmaxf(fmaxf(amaxj[j], fabsf(v23.x)), fabsf(v23.y));
        unsigned h0, l0, h1, l1;
        split_pair(v01.x, v01.y, osc, h0, l0);
        split_pair(v23.x, v23.y, osc, h1, l1);
        u32x2_alias hv, lv;
        hv[0] = h0; hv[1] = h1; lv[0] = l0; lv[1] = l1;
        unsigned char* const ph = j == 0 ? pkq + QM_Q : (j == 1 ? pkq + QM_K : pv);
        *reinterpret_cast<u32x2_alias*>(ph) = hv;
        *reinterpret_cast<u32x2_alias*>(ph + (j == 2 ? QM_VPLANE : QM_PLANE)) = lv;
      }
    }
    if (fmaxf(fmaxf(amaxj[1], amaxj[2]) * 8.0f, amaxj[0]) > X3_HALF_MAX) range_raise(a.range, RANGE_BIT_ACT);
  }
  __syncthreads();   // the planes are written

  // ---- attention: (group, 32-query tile) jobs of the tile over the eight waves
  const int jobs = a.g * NKT;
  for (int job = wave; job < jobs; job += 8) {
    const int u = job / NKT, qt = job - u * NKT;
    const int unit = mt * a.g + u;
    if (32 * qt >= a.N || unit >= a.units) continue;                    // (wave-uniform)
    _Float16* const out0 = a.out + (size_t)qm_unit_row(a, unit) * 2 * a.D + hd * 128;
    if constexpr (DH == 64) qm_attention<NKT>(lds, wave, lane, u * a.N, qt, a.N, out0, (size_t)a.udiv * 2 * a.D, a.range);
    else qm_attention_narrow<NKT, DH>(lds, wave, lane, u * a.N, qt, a.N, out0, (size_t)a.udiv * 2 * a.D, a.range);
  }
}

// Shapes the kernel exists for: the model width of the fused F16X3 kernels (8 heads x 64), whole pairs of 32-deep k-tiles, groups of at
// most 127 tokens; spatial groups (stride 1) are the joints of a frame, 15 .. 17 as kernels_qkv_sattn.hip, temporal ones the frames of a joint
bool qkv_attn_x3_small_ok(int N, int stride, int J, int D, int H, int K) {
  if (!(D == 512 && H == 8 && K % 64 == 0 && K >= 128 && N >= 1 && N <= QM_ROWS && J >= 1)) return false;
  return stride == 1 && N == J ? (J >= 15 && J <= 17) : stride == J;
}

// Apair: pair layout [groups * N][2 K] (only those rows are read); W / bias / csum: the tile-order folded qkv images of the weight commit;
// out_x3: pair layout [groups * N][2 D], not Apair.  Group u holds rows (u / stride) * N * stride + u % stride + t * stride, t < N --
// spatial blocks: (B * T, J, 1), temporal blocks: (B * J, T, J).
hipError_t launch_qkv_attn_x3_small(const void* Apair, const void* Wpair_tileorder, const float* bias_to, const float* csum_to, const float* st_in,
                                    int st_np, float eps, int w_exp, void* out_x3, int groups, int N, int stride, int J, int K, int D, int H,
                                    hipStream_t s) {
  if (!qkv_attn_x3_small_ok(N, stride, J, D, H, K) || groups < 1 || groups % stride != 0 || st_np < 1 || !Apair || !Wpair_tileorder || !bias_to ||
      !csum_to || !st_in || !out_x3 || Apair == out_x3)
    return hipErrorInvalidValue;
  if (w_exp < -14 || w_exp > 12) return hipErrorInvalidValue;
  if ((long long)groups * N * 4 * K >= (1LL << 32)) return hipErrorInvalidValue;   // 32-bit lane offsets
  QmArgs a{};
  a.A = (const char*)Apair; a.W = (const char*)Wpair_tileorder; a.bias = bias_to; a.csum = csum_to; a.st_in = st_in;
  a.st_np = st_np; a.eps = eps; a.out_scale = ldexpf(1.0f, -(3 + w_exp));
  a.out = (_Float16*)out_x3; a.K = K; a.D = D; a.N = N; a.udiv = stride;
  a.g = QM_ROWS / N; a.units = groups; a.mtiles = (groups + a.g - 1) / a.g; a.nseg = 8;
  a.range = launch_range_word();
  if ((long long)a.mtiles * 8 > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.mtiles * 8));
  switch ((N + 31) / 32) {
    case 1: return launch_lds<k_qkv_attn_x3_small<1>>(grid, dim3(512), QM_LDS, s, a);
    case 2: return launch_lds<k_qkv_attn_x3_small<2>>(grid, dim3(512), QM_LDS, s, a);
    case 3: return launch_lds<k_qkv_attn_x3_small<3>>(grid, dim3(512), QM_LDS, s, a);
    default: return launch_lds<k_qkv_attn_x3_small<4>>(grid, dim3(512), QM_LDS, s, a);
  }
}

// "fused_narrow": the same tiles for heads of 32 columns in pairs (D = 32 H, H even) or of 16 columns in quads (D = 16 H, H % 4 == 0) -- a
// pair / a quad is one 64-column segment, and the tile-order images are built with D / 64 pseudo-heads.  K = D >= 128 in whole pairs of
// k-tiles (both widths make D a multiple of 64).  Spatial groups are the J <= 127 joints of a frame, ANY J: nothing here mirrors
// kernels_qkv_sattn.hip; temporal ones the T <= 127 frames of a joint.
static int qm_narrow_width(int D, int H) {
  if (H >= 2 && H % 2 == 0 && D == 32 * H) return 32;
  if (H >= 4 && H % 4 == 0 && D == 16 * H) return 16;
  return 0;
}
bool qkv_attn_x3_narrow_ok(int N, int stride, int J, int D, int H, int K) {
  if (!(qm_narrow_width(D, H) != 0 && K == D && K >= 128 && N >= 1 && N <= QM_ROWS && J >= 1)) return false;
  return stride == 1 && N == J ? true : stride == J;
}

template <int DH>
static hipError_t launch_narrow_nkt(const dim3 grid, int nkt, hipStream_t s, const QmArgs& a) {
  switch (nkt) {
    case 1: return launch_lds<k_qkv_attn_x3_small<1, DH>>(grid, dim3(512), QM_LDS, s, a);
    case 2: return launch_lds<k_qkv_attn_x3_small<2, DH>>(grid, dim3(512), QM_LDS, s, a);
    case 3: return launch_lds<k_qkv_attn_x3_small<3, DH>>(grid, dim3(512), QM_LDS, s, a);
    default: return launch_lds<k_qkv_attn_x3_small<4, DH>>(grid, dim3(512), QM_LDS, s, a);
  }
}

// arguments as launch_qkv_attn_x3_small; the images in the tile order of D / 64 pseudo-heads
hipError_t launch_qkv_attn_x3_narrow(const void* Apair, const void* Wpair_tileorder, const float* bias_to, const float* csum_to, const float* st_in,
                                     int st_np, float eps, int w_exp, void* out_x3, int groups, int N, int stride, int J, int K, int D, int H,
                                     hipStream_t s) {
  if (!qkv_attn_x3_narrow_ok(N, stride, J, D, H, K) || groups < 1 || groups % stride != 0 || st_np < 1 || !Apair || !Wpair_tileorder || !bias_to ||
      !csum_to || !st_in || !out_x3 || Apair == out_x3)
    return hipErrorInvalidValue;
  if (w_exp < -14 || w_exp > 12) return hipErrorInvalidValue;
  if ((long long)groups * N * 4 * K >= (1LL << 32)) return hipErrorInvalidValue;   // 32-bit lane offsets
  QmArgs a{};
  a.A = (const char*)Apair; a.W = (const char*)Wpair_tileorder; a.bias = bias_to; a.csum = csum_to; a.st_in = st_in;
  a.st_np = st_np; a.eps = eps; a.out_scale = ldexpf(1.0f, -(3 + w_exp));
  a.out = (_Float16*)out_x3; a.K = K; a.D = D; a.N = N; a.udiv = stride;
  a.g = QM_ROWS / N; a.units = groups; a.mtiles = (groups + a.g - 1) / a.g; a.nseg = D / 64;
  a.range = launch_range_word();
  if ((long long)a.mtiles * a.nseg > 0x7fffffffLL) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.mtiles * a.nseg));
  return qm_narrow_width(D, H) == 32 ? launch_narrow_nkt<32>(grid, (N + 31) / 32, s, a) : launch_narrow_nkt<16>(grid, (N + 31) / 32, s, a);
}

// workgroups of a launch over `groups` groups of N tokens (the engine's plan)
long long qkv_attn_x3_small_workgroups(long long groups, int N) {
  const int g = QM_ROWS / N;
  return (groups + g - 1) / g * 8;
}

}  // namespace d3d
