// GRAND attention cores in exact fp32 on the matrix pipe for heads of 48 and 96 columns (D == 48 H or 96 H: embed_dim 384 / 768 with the
// runner's 8 heads; the width is D / H) and, further down, of 16 columns, on the pieces of attn_f32_tile.h at DH = 48 and 96: packed fp32 qkv rows in, fp32 rows out, no
// pair-layout form (only FP32 engines take these kernels; option "attn_f32_hx").
//
//   resident   k_attn_f32_hx<DH, NKT>, one workgroup of NKT waves per (group, head), groups of N <= 32 NKT tokens `stride` tokens apart,
//              N <= 256 at width 48 (8 key tiles) and N <= 192 at width 96 (6 key tiles): temporal blocks (B, T, J), spatial blocks
//              (B T, J, 1) -- any joint count up to that maximum.  The scores are computed once and kept in registers.
//   streaming  k_attn_f32_hx_stream<DH>, any T >= 1: the keys pass through LDS in chunks of 256 / 192 frames (8 / 6 key tiles); one
//              workgroup per (batch, joint, head, query block), f32_launch_stream's geometry.
//
// The traits of these widths are those of width 128 (F32Tile<48>, F32Tile<96>): 1 / sqrt(DH) is no power of two, so the scaled sums are
// rounded products everywhere and neither kernel has the fused exp argument; P is NOT normalised before the second product (no twin's bits
// exist to keep), so the streaming kernel needs two passes over the keys: pass 1 stages K chunk by chunk for m; pass 2 stages K and V,
// recomputes each score tile with the same MFMAs (the same bits), and runs e, l += e and the PV MFMAs per tile in the resident kernel's
// order.  The store is out = oacc / l - v[query].  For T <= the resident maximum the streaming kernel gives the resident kernel's bits
// (tests/test_gpu_attn_f32_hx.py).
//
// Width 48 is no multiple of the 32 x 32 accumulator tile: its second O^T tile covers columns 32 .. 63.  The V rows in LDS are 64 floats
// with columns 48 .. 63 staged as zeros (never the next head's columns, never stale bytes), and the store skips those rows of the tile, so
// a NaN in the neighbouring head cannot reach this one.
//
// Width 16 (D == 16 H: embed_dim 128 with 8 heads; option "attn_f32_h16") walks the same two templates at DH = 16 behind entry points of its
// own (attn_f32_h16_ok / launch_attn_f32_h16 and their _long twins), resident up to 256 tokens, chunks of 256 frames.  Its one O^T tile is
// half used, like width 48's second: V rows in LDS are 32 floats with columns 16 .. 31 staged as zeros -- never the next head's columns --
// and rows 16 .. 31 of the tile are never stored.  1 / sqrt(16) = 0.25 is exact; the sums are scaled after the sum over d like the others.
// 6 656 B of LDS per key tile, 53 248 B per chunk: three workgroups per CU at the largest.
//
// LDS: 14 848 B (width 48) / 25 088 B (width 96) per key tile; 118 784 B / 150 528 B per chunk of the streaming kernel and per group of
// the resident one at its largest NKT -- under 160 KiB, one workgroup per CU there.
// Every wave executes every barrier: the chunk and key-tile trip counts depend on T alone; a wave whose queries are all >= T stages and
// synchronises and only skips its stores.
#include "attn_f32_tile.h"

namespace d3d {

namespace {
// the head width of a call, 0 where it is none of this unit's
int hx_width(int D, int H) { return H > 0 && D == 48 * H ? 48 : H > 0 && D == 96 * H ? 96 : 0; }
}  // namespace

// =============================================================================================== resident
// groups: G of N tokens `stride` apart; unit = (g * H + h), group g = (g / stride, g % stride): tok0 = (g / stride) * N * stride + g % stride
template <int DH, int NKT>
__global__ __launch_bounds__(64 * NKT) void k_attn_f32_hx(const float* __restrict__ qkv, float* __restrict__ out, int N, int stride, int H,
                                                          int D) {
  using Tl = F32Tile<DH>;
  extern __shared__ __attribute__((aligned(16))) float lds_f32hx[];
  constexpr int TP = 32 * NKT;
  float* const Ks = lds_f32hx;                   // [TP][K_LD]
  float* const Vs = lds_f32hx + TP * Tl::K_LD;   // [TP][V_LD]

  const int unit = blockIdx.x;
  const int hd = unit % H;
  const int g = unit / H;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, hh = lane >> 5;
  const size_t tok0 = (size_t)(g / stride) * N * stride + g % stride;   // token(t) = tok0 + t * stride

  f32_stage_rows<DH, true>(qkv, Ks, Vs, tok0, stride, D, hd, 0, NKT, N, tid, 64 * NKT);
  const int tq = 32 * wave + r;
  float qreg[Tl::QR];
  f32_load_query<DH>(qkv, qreg, tok0, stride, D, hd, tq, N, hh);
  __syncthreads();

  f32x16 sacc[NKT];
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    sacc[kt] = f32_score_tile<DH>(Ks, qreg, kt, {kt, kt == NKT - 1, N}, r, hh);
    m = f32_tile_max<DH>(sacc[kt], {kt, kt == NKT - 1, N}, hh, m);
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  float l = 0.f;
  f32x16 oacc[Tl::NDT];
  f32_zero_acc<DH>(oacc);
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
    f32_exp_tile<DH>(sacc[kt], {kt, kt == NKT - 1, N}, hh, m);
    f32_sum_tile(sacc[kt], l);
    f32_pv_tile<DH>(Vs, sacc[kt], oacc, kt, r, hh);
  }
  l += __shfl_xor(l, 32, 64);

  if (tq < N) f32_store_query<DH>(qkv, out, oacc, l, tok0 + (size_t)tq * stride, D, hd, hh, true);
}

bool attn_f32_hx_ok(int N, int D, int H) {
  const int dh = hx_width(D, H);
  return dh != 0 && N >= 1 && N <= 32 * (dh == 48 ? F32Tile<48>::STREAM_KC : F32Tile<96>::STREAM_KC);
}

namespace {
template <int DH>
hipError_t launch_resident(const float* qkv, float* out, unsigned units, int N, int stride, int D, int H, hipStream_t s) {
  return f32_resident_ladder<F32Tile<DH>::STREAM_KC>(N, [&](auto nkt) {
    constexpr int NKT = decltype(nkt)::value;
    return launch_lds<k_attn_f32_hx<DH, NKT>>(dim3(units), dim3(64 * NKT), F32Tile<DH>::lds_bytes(NKT), s, qkv, out, N, stride, H, D);
  });
}
}  // namespace

// groups as launch_attn_f32_h128: B * J of them, T tokens each, J tokens apart
hipError_t launch_attn_f32_hx(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_hx_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return hx_width(D, H) == 48 ? launch_resident<48>(qkv, out, (unsigned)units, T, J, D, H, s)
                              : launch_resident<96>(qkv, out, (unsigned)units, T, J, D, H, s);
}

// width 16: the same ladder at DH = 16 (8 key tiles)
bool attn_f32_h16_ok(int N, int D, int H) { return H > 0 && D == 16 * H && N >= 1 && N <= 32 * F32Tile<16>::STREAM_KC; }

hipError_t launch_attn_f32_h16(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_h16_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_resident<16>(qkv, out, (unsigned)units, T, J, D, H, s);
}

// =============================================================================================== streaming
template <int DH>
__global__ __launch_bounds__(512) void k_attn_f32_hx_stream(const float* __restrict__ qkv, float* __restrict__ out, int T, int J, int H,
                                                            int D, int nqb) {
  using Tl = F32Tile<DH>;
  constexpr int KC = Tl::STREAM_KC, CH = 32 * KC;   // key tiles / keys per chunk
  extern __shared__ __attribute__((aligned(16))) float lds_f32hxs[];
  float* const Ks = lds_f32hxs;                   // [CH][K_LD]
  float* const Vs = lds_f32hxs + CH * Tl::K_LD;   // [CH][V_LD]
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
  float qreg[Tl::QR];
  f32_load_query<DH>(qkv, qreg, tok0, J, D, hd, tq, T, hh);

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    f32_stage_rows<DH, false>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const F32KeyTile at{c * KC + kt, c * KC + kt == ntiles - 1, T};
      m = f32_tile_max<DH>(f32_score_tile<DH>(Ks, qreg, kt, at, r, hh), at, hh, m);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));

  // ---- pass 2: the same scores again (same MFMAs, same bits), their numerators, l and O^T per key tile in the resident kernel's order
  float l = 0.f;
  f32x16 oacc[Tl::NDT];
  f32_zero_acc<DH>(oacc);
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    f32_stage_rows<DH, true>(qkv, Ks, Vs, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const F32KeyTile at{c * KC + kt, c * KC + kt == ntiles - 1, T};
      f32x16 sacc = f32_score_tile<DH>(Ks, qreg, kt, at, r, hh);
      f32_exp_tile<DH>(sacc, at, hh, m);
      f32_sum_tile(sacc, l);
      f32_pv_tile<DH>(Vs, sacc, oacc, kt, r, hh);
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l += __shfl_xor(l, 32, 64);

  if (tq < T) f32_store_query<DH>(qkv, out, oacc, l, tok0 + (size_t)tq * J, D, hd, hh, true);
}

bool attn_f32_hx_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && hx_width(D, H) != 0;
}

hipError_t launch_attn_f32_hx_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_hx_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  return hx_width(D, H) == 48 ? f32_launch_stream<k_attn_f32_hx_stream<48>, 48>(qkv, out, B, T, J, D, H, s)
                              : f32_launch_stream<k_attn_f32_hx_stream<96>, 96>(qkv, out, B, T, J, D, H, s);
}

bool attn_f32_h16_long_ok(int T, int D, int H) { return T >= 1 && H > 0 && D == 16 * H; }

hipError_t launch_attn_f32_h16_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_f32_h16_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  return f32_launch_stream<k_attn_f32_hx_stream<16>, 16>(qkv, out, B, T, J, D, H, s);
}

}  // namespace d3d
