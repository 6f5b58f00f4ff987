// Temporal GRAND attention on the fp16 matrix pipe for windows of ANY length: the keys stream through LDS in chunks of 32 KC
// frames instead of all living there (kernels_attn_x3.hip: four planes of T <= 256 rows = 128 of the 160 KiB).
//
// The arithmetic is that of k_attn_temporal_x3<NKT, 1> (kernels_attn_x3.hip, the form every other F16X3 attention kernel is pinned
// to): the exact two-pass softmax, not an online rescaling.
//
//   pass 1   per chunk: stage K, S^T = K Q^T tile by tile, running maximum m of this lane's query column
//   pass 2   per chunk: stage K and V; per key tile the SAME twelve MFMAs again (same bits), e = exp2(fma(s, C, -m C)), l += e in
//            register order, O^T += V^T E^T for the two 16-key steps and the two d halves in the base kernel's order
//   O = O^T / (2^13 l) - v_query, range guard, hi / lo planes out: the base kernel's epilogue
//
// So every exp2 sees the same m, l is summed in the same order and oacc takes the same MFMAs in the same order as in the base
// kernel: for T <= 256 the output is bit-identical to launch_attn_temporal_x3 (tests/test_gpu_long_temporal.py).  The price is the
// scores computed twice, 36 instead of 24 MFMAs per 32 x 32 tile; one score tile (16 registers) is live at a time.
//
// One workgroup per (batch, joint, head, query block): the T queries of a unit are cut into ceil(T / 256) balanced blocks of at most
// 8 waves of 32 queries (T = 300: two blocks of 160), blockDim = 64 x that wave count -- a run-time value, the staging loops stride by
// it.  Staging is the base kernel's: through registers into the four swizzled planes, all global loads of a batch issued before its
// LDS writes; no LDS-DMA, no counters, no persistent walk.  Every wave executes every barrier: the chunk and key-tile trip counts
// depend on T alone, a wave whose queries are all >= T stages and synchronises and only skips its stores.
// Row isolation: keys >= T score -inf (their e is an exact 0) and their K / V rows are staged as zeros, never left over from the
// previous chunk: 0 x NaN cannot enter a clean row.
#include "d3d_kernels.h"

#include <math.h>

namespace d3d {

#include "attn_lds.h"   // typedefs, kswz / vswz, split8_e

namespace {

constexpr int LDH = 64;   // head width

// Rows [32 KC c, 32 KC c + 32 nkt) of the unit's K (and V) planes into LDS rows [0, 32 nkt); rows >= T as zeros.  Four 16-byte slots
// per thread and batch, as in the base kernel (there one batch covers the unit; here 32 nkt rows x 8 slots / blockDim of them).
template <bool WITH_V>
__device__ __forceinline__ void stage_chunk(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, unsigned char* sKh,
                                            unsigned char* sKl, unsigned char* sVh, unsigned char* sVl, size_t tok0, int J, int D, int hd,
                                            int row0, int nkt, int T, int tid, int nthr) {
  constexpr int NIT = 4;
  const int slots = nkt * 32 * 8;
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    uint4 kh[NIT], kl[NIT], vh[NIT], vl[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 3, c8 = idx & 7;
      kh[it] = make_uint4(0, 0, 0, 0); kl[it] = kh[it]; vh[it] = kh[it]; vl[it] = kh[it];
      if (idx < slots && row0 + row < T) {
        const size_t o = (tok0 + (size_t)(row0 + row) * J) * D3 + hd * LDH + c8 * 8;
        kh[it] = *reinterpret_cast<const uint4*>(Ph + o + D);
        kl[it] = *reinterpret_cast<const uint4*>(Pl + o + D);
        if (WITH_V) {
          vh[it] = *reinterpret_cast<const uint4*>(Ph + o + 2 * D);
          vl[it] = *reinterpret_cast<const uint4*>(Pl + o + 2 * D);
        }
      }
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx >> 3, c8 = idx & 7;
      if (idx < slots) {
        const int ko = kswz(row, c8), vo = vswz(row, c8);
        *reinterpret_cast<uint4*>(sKh + ko) = kh[it];
        *reinterpret_cast<uint4*>(sKl + ko) = kl[it];
        if (WITH_V) {
          *reinterpret_cast<uint4*>(sVh + vo) = vh[it];
          *reinterpret_cast<uint4*>(sVl + vo) = vl[it];
        }
      }
    }
  }
}

}  // namespace

template <int KC>
__global__ __launch_bounds__(512) void k_attn_temporal_x3l(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                           _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units,
                                                           int nqb, unsigned* rw) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_l[];
  constexpr int CH = 32 * KC;                         // keys per chunk
  unsigned char* const sKh = lds_l;                   // [CH][128 B]
  unsigned char* const sKl = lds_l + CH * 128;
  unsigned char* const sVh = lds_l + 2 * CH * 128;
  unsigned char* const sVl = lds_l + 3 * CH * 128;
  const int nthr = (int)blockDim.x, tid = (int)threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);       // 32-query tile of the query block
  const int unit_raw = (int)(blockIdx.x / (unsigned)nqb), qb = (int)(blockIdx.x % (unsigned)nqb);
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus workgroups redo the last unit and store nothing
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J
  const int ntiles = (T + 31) >> 5;                   // key tiles of the unit
  const int nchunks = (ntiles + KC - 1) / KC;

  // ---- this lane's query row as MFMA B fragments: d = 16 ks + 8 h .. +7
  const int tq = qb * (nthr >> 1) + 32 * wave + r;    // (a query block is blockDim / 2 queries)
  h8 qh[4], ql[4];
  {
    const size_t o = (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * LDH + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      if (tq < T) {
        qh[ks] = *reinterpret_cast<const h8*>(Ph + o + 16 * ks);
        ql[ks] = *reinterpret_cast<const h8*>(Pl + o + 16 * ks);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) { qh[ks][e] = (_Float16)0.0f; ql[ks][e] = (_Float16)0.0f; }
      }
    }
  }

  // S^T tile kt of the staged chunk (rows = keys (reg&3) + 8*(reg>>2) + 4*h of the tile, column = query tq; acc = 64 * s), keys >= T
  // at -inf.  Only the unit's last key tile (gt == ntiles - 1) can hold such keys.
  auto score_tile = [&](int kt, int gt) -> f32x16 {
    f32x16 sacc;
#pragma unroll
    for (int q = 0; q < 16; ++q) sacc[q] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const int ko = kswz(kt * 32 + r, 2 * ks + h);
      const h8 kh = *reinterpret_cast<const h8*>(sKh + ko);
      const h8 kl = *reinterpret_cast<const h8*>(sKl + ko);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], sacc, 0, 0, 0);
      sacc = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], sacc, 0, 0, 0);
    }
    if (gt == ntiles - 1) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int key = gt * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (key >= T) sacc[q] = -INFINITY;
      }
    }
    return sacc;
  };

  // ---- pass 1: the exact maximum over all keys of this query column
  float m = -INFINITY;
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<false>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      const f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) m = fmaxf(m, sacc[q]);
    }
    __syncthreads();      // everybody is done with this chunk's K
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  constexpr float C_EXP = 1.4426950408889634f / 64.0f;
  const float mb = m * C_EXP;

  // ---- pass 2: numerators, their sum, O^T[d][query] = sum_key V^T[d][key] * E^T[key][query]
  float l = 0.f;
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
  for (int c = 0; c < nchunks; ++c) {
    const int nkt = ntiles - c * KC < KC ? ntiles - c * KC : KC;
    stage_chunk<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hd, c * CH, nkt, T, tid, nthr);
    __syncthreads();
    for (int kt = 0; kt < nkt; ++kt) {
      f32x16 sacc = score_tile(kt, c * KC + kt);
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const float e = __builtin_amdgcn_exp2f(fmaf(sacc[q], C_EXP, -mb));
        sacc[q] = e;
        l += e;
      }
      // k-step (kt, s) takes accumulator registers 8s..8s+7: element jj of lane half h is key kt*32 + 16 s + 8 (jj>>2) + 4 h + (jj&3);
      // the V^T fragment is read in that order (ds_read_b64_tr_b16, see kernels_attn_x3.hip)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        h8 eh, el;                                                  // e in [0,1] -> hi/lo of 2^10 e
        {
          float e8[8];
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) e8[jj] = sacc[8 * s + jj];
          split8_e(e8, eh, el);
        }
        const int k0 = kt * 32 + 16 * s + 4 * h;
        const int gi = lane & 15, tq_ = gi >> 2, tp_ = gi & 3;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const int d0 = dt * 32 + 16 * ((lane >> 4) & 1);
          const int ch = (d0 >> 3) + (tp_ >> 1), sub = (tp_ & 1) * 8;
          const int o0 = vswz(k0 + tq_, ch) + sub, o1 = vswz(k0 + 8 + tq_, ch) + sub;
          const s4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o0));
          const s4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o1));
          const s4v c0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o0));
          const s4v c1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o1));
          h8 vh, vl;
          {
            const h4 a0h = __builtin_bit_cast(h4, a0), a1h = __builtin_bit_cast(h4, a1);
            const h4 c0h = __builtin_bit_cast(h4, c0), c1h = __builtin_bit_cast(h4, c1);
#pragma unroll
            for (int e = 0; e < 4; ++e) { vh[e] = a0h[e]; vh[4 + e] = a1h[e]; vl[e] = c0h[e]; vl[4 + e] = c1h[e]; }
          }
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, eh, oacc[dt], 0, 0, 0);
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, el, oacc[dt], 0, 0, 0);
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, eh, oacc[dt], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();      // everybody is done with this chunk's K and V
  }
  l += __shfl_xor(l, 32, 64);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
    const size_t tokq = tok0 + (size_t)tq * J;
    const size_t vo = tokq * D3 + 2 * D + hd * LDH;
    const size_t oo = tokq * 2 * D + hd * 2 * LDH;   // pair layout: a head's 64 columns are two 128-byte lines
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * h;
        const h4 vqh = *reinterpret_cast<const h4*>(Ph + vo + d);
        const h4 vql = *reinterpret_cast<const h4*>(Pl + vo + d);
        h4 oh, ol;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float vq = ((float)vqh[e] + (float)vql[e]) * 0.125f;
          const float o = __builtin_fmaf(oacc[dt][4 * g4 + e], inv, -vq);   // stated: every form of this kernel must round the same way
          amax = fmaxf(amax, fabsf(o));
          const float sc = __builtin_amdgcn_fmed3f(o * 8.0f, -65504.0f, 65504.0f);
          oh[e] = (_Float16)sc;
          ol[e] = (_Float16)(sc - (float)oh[e]);
        }
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// the query blocks of a unit: ceil(T / 256) of them, balanced, in whole waves of 32 queries
static int long_query_blocks(int T) { return (T + 255) / 256; }
static int long_block_waves(int T) {
  const int nqb = long_query_blocks(T);
  return ((T + nqb - 1) / nqb + 31) / 32;             // <= 8: ceil(T / nqb) <= 256
}

bool attn_temporal_x3_long_ok(int T, int D, int H) {
  // (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
  return T >= 1 && H > 0 && D == H * LDH;
}

hipError_t launch_attn_temporal_x3_long(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J, int D, int H,
                                        hipStream_t s) {
  if (!attn_temporal_x3_long_ok(T, D, H) || !qkv_hi || !qkv_lo || !out_x3 || B <= 0 || J <= 0) return hipErrorInvalidValue;
  constexpr int KC = 8;
  const int nqb = long_query_blocks(T), waves = long_block_waves(T);
  const long long units = (long long)B * J * H;
  if (units * nqb > 0x7fffffffLL) return hipErrorInvalidValue;
  const size_t lds_bytes = (size_t)4 * 32 * KC * 128;   // K_hi, K_lo, V_hi, V_lo planes of one chunk
  return launch_lds<k_attn_temporal_x3l<KC>>(dim3((unsigned)(units * nqb)), dim3(64 * waves), lds_bytes, s, (const _Float16*)qkv_hi,
                                             (const _Float16*)qkv_lo, (_Float16*)out_x3, T, J, H, D, (int)units, nqb, launch_range_word());
}

}  // namespace d3d
