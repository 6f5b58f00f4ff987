// Temporal GRAND attention (S2S:75-83, groups = the T <= 256 frames of one joint) on the fp16 matrix pipe with
// fp32-equivalent accuracy (the F16X3 scheme of kernels_gemm_x3p.hip applied to both attention products):
//
//   S^T = K Q^T / 8     3 x v_mfma_f32_32x32x16_f16 per 16-deep d-step on hi/lo planes of 8k and of q' = q/8
//   e   = exp(S - max)  exact two-pass softmax numerator in fp32 registers (one query column per lane)
//   O^T = V^T E^T       E split in-register into hi/lo of 1024 e (the accumulator tile IS the B operand of the next
//                       MFMA after a pairwise fp16 conversion; its k-order permutation is matched on the V side)
//   O   = O^T / (2^13 l) - v_query          (== (softmax - I) V)
//
// Inputs are the hi/lo fp16 planes the qkv GEMM epilogue writes for temporal blocks (q third pre-multiplied by
// dh^-0.5 = 2^-3, exact); the output goes out as hi/lo planes for the proj GEMM.  One workgroup per (batch, joint,
// head); K and V (both row-major fp16 hi/lo planes, 16-byte chunks XOR-swizzled so that the K fragment reads
// (ds_read_b128) and the V fragment reads (ds_read_b64_tr_b16, the hardware transpose read: 4 keys of one d per lane)
// are bank-conflict free) live in LDS for the whole workgroup; each wave owns 32 queries.  12 + 12 MFMAs of 32 cycles replace 32 + 32 fp32 MFMAs of 64
// cycles per 32x32 score tile: 5.3x less matrix-pipe time than k_attn_temporal_f32.
// The tile arithmetic itself -- query fragments, score tile, key mask, softmax, PV steps, output chunk, register staging -- is
// attn_x3_tile.h: k_attn_temporal_x3 (the base form every other F16X3 attention kernel is pinned to) and k_attn_temporal_x3p are the
// staging, synchronisation, walk and stores around those pieces; k_attn_temporal_x3s states the same arithmetic as its own instruction stream.
#include "d3d_kernels.h"

#include <math.h>
#include <utility>

namespace d3d {

#include "attn_lds.h"       // typedefs, kswz / vkey / vswz, patch_wr / patch_rd, split_pair / split_pair_s / split8_e
#include "attn_x3_tile.h"   // the tile arithmetic: query fragments, score tile, softmax, PV steps, output chunk, register staging

constexpr int XDH = 64;

// MU > 1 (only with NKT == 1, i.e. groups of <= 32 tokens: the spatial blocks): one workgroup carries MU independent
// (group, head) units, one per wave, each in its own LDS slice -- a 64-thread workgroup per unit is bound by the
// workgroup launch rate (124k launches per call at T=243, B=64), not by HBM.
template <int NKT, int MU>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_temporal_x3(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                                    _Float16* __restrict__ out_x3,
                                                                    int T, int J, int H, int D, int units, unsigned* rw) {
  static_assert(MU == 1 || NKT == 1, "several units per workgroup only for single-tile groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  constexpr int TP = 32 * NKT;
  const int lane = threadIdx.x & 63;
  const int sub = (MU > 1) ? (int)(threadIdx.x >> 6) : 0;          // unit of this workgroup
  const int wave = (MU > 1) ? 0 : (int)(threadIdx.x >> 6);         // 32-query tile of the unit
  const int tid = (MU > 1) ? lane : (int)threadIdx.x;              // thread index within the unit
  unsigned char* const lds = lds_all + sub * (4 * TP * 128);
  unsigned char* const sKh = lds;                     // [TP][128 B]
  unsigned char* const sKl = lds + TP * 128;
  unsigned char* const sVh = lds + 2 * TP * 128;
  unsigned char* const sVl = lds + 3 * TP * 128;

  const int unit_raw = blockIdx.x * MU + sub;         // (b*J + j)*H + hd
  const bool unit_ok = unit_raw < units;
  const int unit = unit_ok ? unit_raw : units - 1;    // surplus waves redo the last unit and store nothing
  const int hd = unit % H;
  const int bj = unit / H;
  const int j = bj % J, b = bj / J;
  const int D3 = 3 * D;
  const int r = lane & 31, h = lane >> 5;
  const size_t tok0 = (size_t)b * T * J + j;          // token(t) = tok0 + t*J

  // ---- stage K and V rows of this (batch, joint, head) (pad rows zero): one batch of four slots per thread covers the unit
  __builtin_assume(tid < 64 * NKT);   // (blockDim = 64 NKT MU: the slot bound of the staging loop folds away)
  x3_stage_rows<true>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, hd, 0, NKT, T, tid, 64 * NKT);

  // ---- this lane's query row (rows >= T: zeros)
  const int tq = 32 * wave + r;
  h8 qh[4], ql[4];
  x3_q_global(Ph, Pl, (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * XDH + 8 * h, tq < T, qh, ql);
  __syncthreads();

  // ---- S^T tiles, softmax numerators (in sacc) and their sum, O^T
  f32x16 sacc[NKT];
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile(sKh, sKl, kt * 32, r, h, qh, ql);
  const float l = x3_softmax<NKT>(sacc, h, T);
  f32x16 oacc[2];
#pragma unroll
  for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) x3_pv_tile<false>(sacc[kt], sVh, sVl, 0, kt, T, lane, h, oacc);

  // ---- O = O^T / (2^13 l) - v_query, written as hi/lo planes of 8*o for the proj GEMM
  if (tq < T && unit_ok) {
    float amax = 0.0f;   // range guard
    const float inv = 1.0f / (8192.0f * l);
    const size_t tokq = tok0 + (size_t)tq * J;
    const size_t vo = tokq * D3 + 2 * D + hd * XDH;
    const size_t oo = tokq * 2 * D + hd * 2 * XDH;   // pair layout: a head's 64 columns are two 128-byte lines
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const int d = dt * 32 + 8 * g4 + 4 * h;
        h4 oh, ol;
        x3_out_chunk(oacc[dt], g4, inv, *reinterpret_cast<const h4*>(Ph + vo + d), *reinterpret_cast<const h4*>(Pl + vo + d), amax, oh, ol);
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d)) = oh;
        *reinterpret_cast<h4*>(out_x3 + oo + pair_col(d) + PAIR_LO) = ol;
      }
    if (amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
  }
}

// ---- persistent form for multi-wave units (temporal blocks) ----------------------------------------------------------
// One workgroup per CU walks units u = blockIdx, blockIdx + gridDim, ...; K and V planes are staged by LDS-DMA
// (global_load_lds_dwordx4: no staging registers; the bank swizzles of kswz / vswz are applied to the per-lane SOURCE
// chunk, the LDS image stays lane-linear) and the staging of the NEXT unit flies under the arithmetic of the current one:
//
//   top barrier    K(u), Q(u) landed (the only operations outstanding); V region free
//   issue V(u) DMA; store the outputs of unit u-1 (kept packed in registers over the barrier)
//   S^T = K Q^T, softmax numerators                                   (K from LDS, Q in registers)
//   barrier        V(u) landed, everybody done with K  ->  issue K(u+1) DMA, load Q(u+1) into the dead Q registers
//   O^T = V^T E^T, O = O^T / (2^13 l) - v_query                        (V and v_query from LDS)
//
// Every wait is a plain vmcnt(0): by construction nothing younger than the data waited for is in flight at a barrier.
// The non-persistent kernel above serialises load -> compute -> store per workgroup with ONE workgroup per CU (128 KiB of
// LDS): 0.90 ms per launch at T=243, B=64, of which about 0.15 ms is staging latency nothing overlaps.
// MU > 1 (NKT == 1: groups of <= 32 tokens, the spatial blocks): every wave is its own persistent worker on its own LDS
// slice (units blockIdx * MU + wave, + gridDim * MU, ...); the barriers become wave-local waits, so the MU waves of a
// workgroup drift apart and their load / MFMA / VALU phases overlap.
// The arithmetic is attn_x3_tile.h's, as in the kernel above: what differs is the DMA plan, the syncs, v_query from the V planes in LDS,
// the output patch, and (MU > 1) the V fragments of pad keys masked in registers.
// wave-uniform pointer pinned into an SGPR pair (the DMA then takes the saddr + 32-bit voffset form)
__device__ __forceinline__ const char* sgpr_ptr_x(const char* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

// WIT (wave-private form): 8-row passes of the output patch that carry rows < T -- 3 for groups of <= 24 tokens (the spatial
// blocks: 17 joints), 4 up to 32 (temporal blocks of the T = 27 configuration).
template <int NKT, int MU, int WIT = 3>
__global__ __launch_bounds__(64 * NKT * MU) void k_attn_temporal_x3p(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                                     _Float16* __restrict__ out_x3, int T, int J, int H, int D,
                                                                     int units, unsigned* rw) {
  static_assert(MU == 1 || NKT == 1, "wave-private units only for single-tile groups");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_all[];
  constexpr int TP = 32 * NKT;
  constexpr int PLANE = TP * 128;
  constexpr bool WAVEP = MU > 1;
  // WAVEP: the V planes are double-buffered (6 planes per wave), so that K, V and Q of unit u+1 are all requested at the
  // middle of unit u and awaited ONCE, at the top of unit u+1: with 4 planes a wave had one of K / V in flight at a time,
  // each hidden only by half a unit of arithmetic, and the launch ran at the latency x concurrency limit (3.9 TB/s)
  // -- and its planes hold T rows, not TP: a fragment read of the pad rows [T, TP) runs on into the next plane (the next
  // wave's slice, a zeroed tail behind the last one).  What stands there may be ANOTHER group's planes, NaN / Inf included: the
  // scores of keys >= T are overwritten with -inf before the softmax, so K may hold any bits; their E is an exact 0 in the PV
  // product, and the V fragments of those keys are masked to zeros in registers there (0 x NaN would be NaN).  The whole
  // allocation is zeroed once (the tail behind the last wave stays zero).  13 KiB per wave instead of 24.
  constexpr int NPL = WAVEP ? 6 : 4;
  const int PL = WAVEP ? T * 128 : PLANE;         // plane stride in bytes
  unsigned char* const lds = lds_all + (WAVEP ? (int)(threadIdx.x >> 6) * NPL * PL : 0);
#define D3D_ATTN_SYNC()                                                                     \
  do {                                                                                      \
    if (WAVEP) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");                  \
    else {                                                                                  \
      __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0), stated (see D3D_QKTILE in kernels_gemm_x3p.hip) */ \
      __syncthreads();                                                                      \
    }                                                                                       \
  } while (0)
  unsigned char* const sKh = lds;
  unsigned char* const sKl = lds + PL;
  unsigned char* sVh = lds + 2 * PL;
  unsigned char* sVl = lds + 3 * PL;
  int vb = 0;                                     // WAVEP: V buffer of the current unit
  const int tid = WAVEP ? (int)(threadIdx.x & 63) : (int)threadIdx.x;     // thread index within the unit
  const int wave = WAVEP ? 0 : __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // 32-query tile of the unit
  // lane index behind an opaque barrier, refreshed every iteration: all per-lane LDS / global offsets are then re-derived
  // inside the loop (a few VALU ops) instead of being hoisted out of it and kept in ~80 registers (which spilled)
  int lane = tid & 63;
  asm volatile("" : "+v"(lane));
  int r = lane & 31, h = lane >> 5;
  const int D3 = 3 * D;
  int u = WAVEP ? (int)(blockIdx.x * MU + (threadIdx.x >> 6)) : (int)blockIdx.x;
  const int ustep = (int)gridDim.x * MU;
  if (WAVEP) {   // zero the whole allocation (all waves, before any of them leaves or reads)
    const int total16 = (MU * NPL * PL + (TP - T) * 128) >> 4;
    for (int idx = (int)threadIdx.x; idx < total16; idx += 64 * MU) reinterpret_cast<uint4*>(lds_all)[idx] = make_uint4(0, 0, 0, 0);
    __syncthreads();
  }
  if (u >= units) return;     // wave-uniform (workgroup-uniform when MU == 1)

  if (!WAVEP) {   // pad rows [T, TP) of all four planes: zero once, the DMA never writes them (their lanes are masked off)
    for (int idx = tid; idx < (TP - T) * 8 * NPL; idx += 64 * NKT) {   // (the unit's own threads: 64 * NKT)
      const int pl = idx / ((TP - T) * 8), rem = idx % ((TP - T) * 8);
      *reinterpret_cast<uint4*>(lds + pl * PLANE + (T + (rem >> 3)) * 128 + ((rem & 7) << 4)) = make_uint4(0, 0, 0, 0);
    }
  }

  // DMA plan: a plane is TP/8 = 4*NKT pieces of 8 rows x 128 B; wave w moves pieces w, w + NKT, w + 2 NKT, w + 3 NKT of each
  // plane.  Lane l serves row 8*piece + l/8, LDS slot l%8, and fetches the source chunk the swizzle maps to that slot.
  auto dma = [&](int which, size_t tok0, int hd, int vbuf = 0) {   // which: 1 = K, 2 = V (into V buffer vbuf)
    const int drow = lane >> 3, dslot = lane & 7;
    unsigned char* const dVh = lds + (2 + 2 * vbuf) * PL;
    unsigned char* const dVl = dVh + PL;
    // source address = (wave-uniform base: SGPR pair) + (32-bit per-lane byte offset): no 64-bit per-piece row arithmetic
    const size_t ub = tok0 * D3 + (size_t)which * D + hd * XDH;
    const char* const bh = sgpr_ptr_x(reinterpret_cast<const char*>(Ph + ub));
    const char* const bl = sgpr_ptr_x(reinterpret_cast<const char*>(Pl + ub));
    const int rowstep = J * D3 * 2;      // bytes between consecutive rows of the group
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int piece = wave + NKT * it;
      const int row = 8 * piece + drow;
      const int chunk = (which == 1) ? (dslot ^ ((row >> 1) & 7)) : (dslot ^ vkey(row));
      const unsigned voff = (unsigned)(row * rowstep + chunk * 16);
      unsigned char* dh = (which == 1 ? sKh : dVh) + piece * 1024;
      unsigned char* dl = (which == 1 ? sKl : dVl) + piece * 1024;
      if (row < T) {
        __builtin_amdgcn_global_load_lds(bh + voff, (__attribute__((address_space(3))) void*)(uintptr_t)dh, 16, 0, 0);
        __builtin_amdgcn_global_load_lds(bl + voff, (__attribute__((address_space(3))) void*)(uintptr_t)dl, 16, 0, 0);
      }
    }
  };
  auto unit_of = [&](int uu, int& hd, size_t& tok0) {
    hd = uu % H;
    const int bj = uu / H;
    tok0 = (size_t)(bj / J) * T * J + (bj % J);
  };
  h8 qh[4], ql[4];
  auto load_q = [&](size_t tok0, int hd) {
    const int tq = 32 * wave + r;
    x3_q_global(Ph, Pl, (tok0 + (size_t)(tq < T ? tq : 0) * J) * D3 + hd * XDH + 8 * h, true, qh, ql);   // rows >= T reuse row 0: never stored
  };

  int hd;
  size_t tok0;
  unit_of(u, hd, tok0);
  dma(1, tok0, hd);
  if (WAVEP) dma(2, tok0, hd, 0);
  load_q(tok0, hd);
  size_t po_off = 0; (void)po_off;
  bool po_valid = false;
  // WAVEP: the outputs go through a wave-private 4 KiB LDS patch (32 rows x one 128-byte line, 16-byte chunks XOR-swizzled by
  // row) and leave as whole lines, 16 B per lane, 8 lanes per row: 6 store instructions per unit instead of 16 that each wrote
  // 16-byte pieces of 17 different lines (this kernel is bound by the rate at which a wave gets memory instructions through)
  unsigned char* const patch = lds_all + MU * NPL * PL + (TP - T) * 128 + (int)(threadIdx.x >> 6) * 4096;
  // !WAVEP (T = 81: two 3-wave workgroups per CU by registers): the same 4 KiB patch per wave behind the four planes (it used to be a 1 KiB
  // patch written in four 8-row passes of 8-byte pieces -- 2-way bank conflicts, a quarter of the LDS cycles of the kernel)
  unsigned char* const patch1 = lds_all + 4 * PLANE + (int)(threadIdx.x >> 6) * 4096;
  u32x4 pq[8];                  // [dt * 4 + p]: row 32 wave + 8 p + (lane >> 3), chunk lane & 7 of line dt
  u32x4 pw[2 * WIT];            // [dt * WIT + it]: row 8 it + (lane >> 3), chunk lane & 7 of line dt
  _Float16* pw_ptr = out_x3;    // row (lane >> 3), this lane's chunk of line 0 (row 8 it: + it * pw_stride)
  const size_t pw_stride = (size_t)8 * J * 2 * D;
  int tq = 32 * wave + r;

  for (;;) {
    D3D_ATTN_SYNC();            // K(u), Q(u) landed; V region free
    asm volatile("" : "+v"(lane));
    r = lane & 31; h = lane >> 5; tq = 32 * wave + r;
    if (!WAVEP) dma(2, tok0, hd);
    if (WAVEP) {
      if (po_valid) {
#pragma unroll
        for (int it = 0; it < WIT; ++it)
          if (8 * it + (lane >> 3) < T) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(pw_ptr + it * pw_stride + dt * 64) = pw[dt * WIT + it];
          }
      }
    } else if (po_valid) {
#pragma unroll
      for (int pp = 0; pp < 4; ++pp)
        if (32 * wave + 8 * pp + (lane >> 3) < T) {
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(pw_ptr + pp * pw_stride + dt * 64) = pq[dt * 4 + pp];
        }
    }

    // ---- S^T tiles, softmax numerators (in sacc) and their sum
    f32x16 sacc[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) sacc[kt] = x3_score_tile(sKh, sKl, kt * 32, r, h, qh, ql);
    const float l = x3_softmax<NKT>(sacc, h, T);

    if (WAVEP) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // this wave's K fragments are in registers
    else D3D_ATTN_SYNC();       // V(u) landed (and the stores above acknowledged); everybody is done with K
    const int un = u + ustep;
    const bool has_next = un < units;     // workgroup-uniform
    int hd_n = 0;
    size_t tok0_n = 0;
    if (has_next) {
      unit_of(un, hd_n, tok0_n);
      dma(1, tok0_n, hd_n);
      if (WAVEP) dma(2, tok0_n, hd_n, vb ^ 1);   // (that buffer was last read by unit u-1)
    }

    // ---- O^T.  WAVEP: the planes hold T rows, so the V fragments of the pad keys [T, TP) are whatever follows the plane -- the wave's
    // other V buffer (another unit's V) or the next wave's K: masked in registers
    f32x16 oacc[2];
#pragma unroll
    for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      x3_pv_tile<WAVEP>(sacc[kt], sVh, sVl, 0, kt, T, lane, h, oacc);
      // the next unit's query fragments go into the dead Q registers once two score tiles have been consumed (register room)
      if (kt == (NKT > 2 ? 2 : NKT - 1) && has_next) load_q(tok0_n, hd_n);
    }

    // ---- O = O^T / (2^13 l) - v_query (v_query from the V planes in LDS), packed as hi/lo of 8*o; stored after the next barrier
    {
      const float inv = 1.0f / (8192.0f * l);
      const int tqc = tq < T ? tq : 0;
      float amax = 0.0f;   // range guard (rows tq >= T are never stored)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          const int vo = vswz(tqc, dt * 4 + g4) + 8 * h;
          const h4 vqh = *reinterpret_cast<const h4*>(sVh + vo);
          const h4 vql = *reinterpret_cast<const h4*>(sVl + vo);
          h4 oh, ol;
          x3_out_chunk(oacc[dt], g4, inv, vqh, vql, amax, oh, ol);
          // columns 8 g4 + 4 h .. + 3 of line dt: hi halves in chunk g4, lo halves in chunk 4 + g4 (pair layout)
          patch_wr(WAVEP ? patch : patch1, r, h, g4, oh, ol);
          if (g4 == 3) {
            asm volatile("" ::: "memory");     // (the rows read back were written by other lanes)
            if (WAVEP) {
#pragma unroll
              for (int it = 0; it < WIT; ++it) pw[dt * WIT + it] = patch_rd(patch, 8 * it + (lane >> 3), lane & 7);
            } else {
#pragma unroll
              for (int pp = 0; pp < 4; ++pp) pq[dt * 4 + pp] = patch_rd(patch1, 8 * pp + (lane >> 3), lane & 7);
            }
            asm volatile("" ::: "memory");     // (line dt + 1 reuses the patch)
          }
        }
      }
      if (tq < T && amax > X3_HALF_MAX * 0.125f) range_raise(rw, RANGE_BIT_ACT);
      po_off = (tok0 + (size_t)tqc * J) * 2 * D + hd * 2 * XDH;
      pw_ptr = out_x3 + (tok0 + (size_t)((WAVEP ? 0 : 32 * wave) + (lane >> 3)) * J) * 2 * D + hd * 2 * XDH + 8 * (lane & 7);
      po_valid = true;
    }
    if (!has_next) break;
    u = un; hd = hd_n; tok0 = tok0_n;
    if (WAVEP) {
      vb ^= 1;
      sVh = lds + (2 + 2 * vb) * PL;
      sVl = sVh + PL;
    }
  }
#undef D3D_ATTN_SYNC
  // outputs of the last unit
  if (WAVEP) {
#pragma unroll
    for (int it = 0; it < WIT; ++it)
      if (8 * it + (lane >> 3) < T) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(pw_ptr + it * pw_stride + dt * 64) = pw[dt * WIT + it];
      }
  } else {
#pragma unroll
    for (int pp = 0; pp < 4; ++pp)
      if (32 * wave + 8 * pp + (lane >> 3) < T) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(pw_ptr + pp * pw_stride + dt * 64) = pq[dt * 4 + pp];
      }
  }
}

// ---- persistent form with the two wave halves of the workgroup ONE STEP APART (temporal blocks, 8 key tiles) ----------
// k_attn_temporal_x3p keeps all eight waves of the CU in the same phase: score MFMAs, then softmax VALU, then PV MFMAs, then the
// output arithmetic -- the matrix pipe idles during the VALU phases and the VALU during the products.  Waves w and w + 4 share a
// SIMD; here a unit takes FOUR steps (every step starts with vmcnt(0) + workgroup barrier) and waves 4-7 (half 1) run one step
// behind waves 0-3 (half 0), so that on every SIMD, in every step, one wave is in an MFMA phase and the other in a VALU /
// memory phase:
//
//   step 4i     half 0: scores(i)    [K_i]            half 1: outputs(i-1), stages V_i
//   step 4i+1   half 0: softmax(i), stages V_i        half 1: scores(i)    [K_i]
//   step 4i+2   half 0: products(i)  [V_i]            half 1: softmax(i), stages K_{i+1}
//   step 4i+3   half 0: outputs(i), stages K_{i+1}    half 1: products(i)  [V_i]
//
// One K and one V buffer (128 KiB) + a 4 KiB output patch per wave.  K_i is read in steps 4i, 4i+1 and re-staged in 4i+2, 4i+3;
// V_i is read in steps 4i+2, 4i+3 (v_query goes to registers at the end of the product step) and re-staged in 4i+4, 4i+5.  A
// wave issues the LDS-DMA of its pieces at the start of its own VALU steps (see dma below).  The two halves run two INSTANCES of the
// same statically scheduled loop (HALF is a template parameter: the phase of a wave is never a run-time value), half 1 behind
// one extra barrier; both execute 4n + 1 barriers.  Per wave the arithmetic is that of k_attn_temporal_x3p (same MFMAs in the
// same order, same softmax, same conversions): results are bit-identical, only WHEN and by WHICH instructions differs.
template <int... Js, class F>
__device__ __forceinline__ void static_for_(std::integer_sequence<int, Js...>, F&& f) { (f(std::integral_constant<int, Js>{}), ...); }
template <int N, class F>
__device__ __forceinline__ void static_for(F&& f) { static_for_(std::make_integer_sequence<int, N>{}, f); }
// LDS fragment reads as inline asm: the compiler does not know them as LDS operations, so it inserts no s_waitcnt for them --
// the caller places counted lgkmcnt waits itself (LDS operations of one wave return in order).  Needed because the compiler's
// own waits for a ring of fragment registers came out as lgkmcnt(0) right behind the newest read in several instantiations.
template <int OFF>
__device__ __forceinline__ void lds_read_b128(h8& dst, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int OFF>
__device__ __forceinline__ void lds_read_tr16_b64(s4v& dst, unsigned addr) {
  asm volatile("ds_read_b64_tr_b16 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF));
}
template <int N>
__device__ __forceinline__ void lgkm_wait() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); }


// wave priority per phase (s_setprio): the two waves of a SIMD are in different phases; without it the OLDER wave's VALU stream
// (softmax) wins every issue arbitration and the younger wave's MFMAs starve
constexpr int ATTN_PRIO_S = 2, ATTN_PRIO_PV = 1, ATTN_PRIO_SOFT = 0;
template <int NKT, int HALF>
__device__ __forceinline__ void attn_x3s_half(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, _Float16* __restrict__ out_x3,
                                              int T, int J, int H, int D, int units, unsigned char* const lds, const int wave,
                                              unsigned* rw) {
  constexpr int TP = 32 * NKT;
  constexpr int PLANE = TP * 128;
  unsigned char* const sKh = lds;                 // K hi plane; lo plane at + PLANE
  unsigned char* const sVh = lds + 2 * PLANE;     // V hi plane; lo plane at + PLANE
  unsigned char* const sVl = lds + 3 * PLANE;
  int lane = (int)threadIdx.x & 63;
  asm volatile("" : "+v"(lane));
  int r = lane & 31, h = lane >> 5;
  const int D3 = 3 * D;
  const int u0 = (int)blockIdx.x, ustep = (int)gridDim.x;
  const int n = (units - u0 + ustep - 1) / ustep;              // units of this workgroup (>= 1)
#define D3D_STEP_SYNC(k)                                                                                       \
  do {                                                                                                         \
    __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): last step's DMA has landed, stores are acknowledged */    \
    __syncthreads();                                                                                           \
    asm volatile("" : "+v"(lane));                                                                             \
    r = lane & 31; h = lane >> 5; tq = 32 * wave + r;                                                          \
  } while (0)
  // Staging of K / V by LDS-DMA: every wave moves pieces wave + 8 it, it = 0..3 (8 rows x 128 B each), of the hi and of the lo
  // plane, at the START of one of its VALU steps (the partner wave of the SIMD runs MFMAs meanwhile):
  //   V_i      half 0: in softmax(i)   (step 4i+1)     half 1: in outputs(i-1) (step 4i)       read from step 4i+2 on
  //   K_{i+1}  half 0: in outputs(i)   (step 4i+3)     half 1: in softmax(i)   (step 4i+2)     read from step 4i+4 on
  // The kernel moves 249 KB per unit and runs within 1.4x of the time HBM needs for that, so every vector-memory instruction
  // queues (a wave gets one through per ~250 cycles, LDS-DMA or plain load alike): measured alternatives -- one half issuing a
  // whole K or V, the pieces spread between the MFMAs / the softmax of a step, staging through registers with the LDS writes
  // at the end of the step -- were 0 to 15 % slower.  Source address = (wave-uniform base: SGPR pair) + (one 32-bit per-lane
  // byte offset, advanced by a uniform step per piece); the bank swizzles are applied to the per-lane SOURCE chunk.
  auto dma = [&](int which, size_t tok0, int hd) {   // which: 1 = K, 2 = V
    const int row0 = 8 * wave + (lane >> 3), dslot = lane & 7;
    const int chunk = (which == 1) ? (dslot ^ ((row0 >> 1) & 7)) : (dslot ^ vkey(row0));   // (both swizzles have period 32 in the row)
    const size_t ub = tok0 * D3 + (size_t)which * D + hd * XDH;
    const char* const bh = sgpr_ptr_x(reinterpret_cast<const char*>(Ph + ub));
    const char* const bl = sgpr_ptr_x(reinterpret_cast<const char*>(Pl + ub));
    unsigned voff = (unsigned)((row0 * J * D3 + chunk * 8) * 2);
    const unsigned dst = (unsigned)(uintptr_t)((which == 1 ? sKh : sVh) + wave * 1024);
#pragma unroll
    for (int it = 0; it < 4; ++it) {      // rows row0 + 64 it: only the last piece can reach beyond T (T > 224 with 8 key tiles)
      if (it < 3 || row0 + 192 < T) {
        __builtin_amdgcn_global_load_lds(bh + voff, (__attribute__((address_space(3))) void*)(uintptr_t)(dst + it * 8192), 16, 0, 0);
        __builtin_amdgcn_global_load_lds(bl + voff, (__attribute__((address_space(3))) void*)(uintptr_t)(dst + it * 8192 + PLANE), 16, 0, 0);
      }
      voff += (unsigned)(64 * J * D3 * 2);
    }
  };
  auto unit_of = [&](int i, int& hd, size_t& tok0) {
    const int uu = u0 + i * ustep;
    hd = uu % H;
    const int bj = uu / H;
    tok0 = (size_t)(bj / J) * T * J + (bj % J);
  };
  h8 qh[4], ql[4];
  auto load_q = [&](size_t tok0, int hd) {
    const int tq_ = 32 * wave + r;
    const size_t o = (tok0 + (size_t)(tq_ < T ? tq_ : 0) * J) * D3 + hd * XDH + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      qh[ks] = *reinterpret_cast<const h8*>(Ph + o + 16 * ks);     // rows >= T reuse row 0: their columns are never stored
      ql[ks] = *reinterpret_cast<const h8*>(Pl + o + 16 * ks);
    }
  };

  int hd;
  size_t tok0;
  unit_of(0, hd, tok0);
  dma(1, tok0, hd);                     // K_0
  load_q(tok0, hd);
  // Outputs of a unit: hi/lo halves are transposed through a wave-private 4 KiB LDS patch (32 rows x one 128-byte line, 16-byte
  // chunks XOR-swizzled by row) so that every global store covers whole lines at 16 B per lane -- 8 lanes per row -- instead
  // of 16-byte pieces of 32 different lines per instruction; kept in registers over the step barrier, stored one step later.
  unsigned char* const patch = lds + 4 * PLANE + wave * 4096;
  u32x4 po[8];                  // [dt * 4 + it]: row 32 wave + 8 it + (lane >> 3), chunk lane & 7 of line dt
  _Float16* po_ptr = out_x3;    // that row's line 0, this lane's chunk (row 8 it: + it * po_stride)
  const size_t po_stride = (size_t)8 * J * 2 * D;
  bool po_valid = false;
  int tq = 32 * wave + r;
  if (HALF == 1) {                      // global step 0: half 0's scores(0); half 1 stages its pieces of V_0
    D3D_STEP_SYNC(4);
    dma(2, tok0, hd);
  }

  for (int i = 0; i < n; ++i) {
    const bool has_next = i + 1 < n;    // workgroup-uniform
    int hd_n = 0;
    size_t tok0_n = 0;
    if (has_next) unit_of(i + 1, hd_n, tok0_n);
    // ================= this wave's score step (global step 4i + HALF)
    D3D_STEP_SYNC(0);
    if (po_valid) {
#pragma unroll
      for (int it = 0; it < 4; ++it)
        if (32 * wave + 8 * it + (lane >> 3) < T) {
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(po_ptr + it * po_stride + dt * 64) = po[dt * 4 + it];
        }
    }
    __builtin_amdgcn_s_setprio(ATTN_PRIO_S);
    // ---- S^T tiles (rows = keys, column = query tq); acc = 64 * s.  A step = one 16-deep d-slice of one key tile: two
    // ds_read_b128, three MFMAs; the fragments of step j + 2 are requested before the MFMAs of step j issue, which wait for
    // their own fragments only (lgkmcnt(4): the four younger reads stay in flight).
    f32x16 sacc[NKT];
    {
      h8 kfh[3], kfl[3];
      unsigned kaddr[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) kaddr[ks] = (unsigned)(uintptr_t)(sKh + kswz(r, 2 * ks + h));   // + 4096 kt; lo plane + PLANE
      static_assert(PLANE + (NKT - 1) * 4096 < 65536, "ds offset field");
      lds_read_b128<0>(kfh[0], kaddr[0]); lds_read_b128<PLANE>(kfl[0], kaddr[0]);
      lds_read_b128<0>(kfh[1], kaddr[1]); lds_read_b128<PLANE>(kfl[1], kaddr[1]);
      static_for<4 * NKT>([&](auto jc) {
        constexpr int j = decltype(jc)::value, kt = j >> 2, ks = j & 3, jn = j + 2;
        if constexpr (jn < 4 * NKT) {
          lds_read_b128<(jn >> 2) * 4096>(kfh[jn % 3], kaddr[jn & 3]);
          lds_read_b128<(jn >> 2) * 4096 + PLANE>(kfl[jn % 3], kaddr[jn & 3]);
        }
        lgkm_wait<(jn < 4 * NKT) ? 4 : (j + 1 < 4 * NKT ? 2 : 0)>();
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (ks == 0) {
#pragma unroll
          for (int q = 0; q < 16; ++q) sacc[kt][q] = 0.f;
        }
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfl[j % 3], qh[ks], sacc[kt], 0, 0, 0);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfh[j % 3], ql[ks], sacc[kt], 0, 0, 0);
        sacc[kt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kfh[j % 3], qh[ks], sacc[kt], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    // ================= softmax step (global step 4i + 1 + HALF)
    D3D_STEP_SYNC(1);
    __builtin_amdgcn_s_setprio(ATTN_PRIO_SOFT);
    if (HALF == 0) dma(2, tok0, hd);                                             // V_i
    else if (has_next) dma(1, tok0_n, hd_n);                                     // K_{i+1}
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
    constexpr float C_EXP = 1.4426950408889634f / 64.0f;
    const float mb = m * C_EXP;
    float l = 0.f;
    // numerators e = 2^(...) and, in the same step, their split into fp16 hi / lo of 1024 e (the B operand of the PV product:
    // the accumulator tile IS that operand after the pairwise conversion) -- the PV step then holds MFMAs, V reads and the
    // output arithmetic only.  lo = fp16(1024 e - hi) as ONE fused multiply-add (1024 e is exact, so the value is that of the
    // two-instruction form); the compiler selects v_fma_mix*_f16 for it.
    // (the packed halves go back into the registers of the score tile: slots 0-7 hold the hi pairs, 8-15 the lo pairs)
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      float e[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        e[q] = __builtin_amdgcn_exp2f(fmaf(sacc[kt][q], C_EXP, -mb));
        l += e[q];
      }
#pragma unroll
      for (int pr = 0; pr < 8; ++pr) {
        unsigned hp, lp;
        split_pair_s(e[2 * pr], e[2 * pr + 1], 1024.0f, hp, lp);
        sacc[kt][pr] = __builtin_bit_cast(float, hp);
        sacc[kt][8 + pr] = __builtin_bit_cast(float, lp);
      }
      __builtin_amdgcn_sched_barrier(0);
    }
    l += __shfl_xor(l, 32, 64);
    // ================= PV product step (global step 4i + 2 + HALF)
    D3D_STEP_SYNC(2);
    __builtin_amdgcn_s_setprio(ATTN_PRIO_PV);
    // ---- O^T[d][query] = sum_key V^T[d][key] E^T[key][query]
    f32x16 oacc[2];
#pragma unroll
    for (int q = 0; q < 16; ++q) { oacc[0][q] = 0.f; oacc[1][q] = 0.f; }
    {
      // a step = 16 keys (kt, s2): eight transposing reads (V^T fragments of both d-halves, hi and lo) and six MFMAs; the reads
      // of step j + 1 are requested before the MFMAs of step j, which wait lgkmcnt(8)
      const int gi = lane & 15, tq_ = gi >> 2, tp_ = gi & 3;
      unsigned vaddr[4];     // [dt][row half]: + 2048 per step; lo plane + PLANE
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
        const int d0 = dt * 32 + 16 * ((lane >> 4) & 1);
        const int ch = (d0 >> 3) + (tp_ >> 1), sub = (tp_ & 1) * 8;
        vaddr[2 * dt] = (unsigned)(uintptr_t)(sVh + vswz(4 * h + tq_, ch) + sub);
        vaddr[2 * dt + 1] = (unsigned)(uintptr_t)(sVh + vswz(4 * h + 8 + tq_, ch) + sub);
      }
      s4v vf[2][8];          // [buffer][dt * 4 + {hi rows 0-3, hi rows 8-11, lo rows 0-3, lo rows 8-11}]
      auto vread = [&](auto jc, s4v(&f)[8]) {
        constexpr int off = decltype(jc)::value * 2048;
        static_assert(off + PLANE < 65536, "ds offset field");
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          lds_read_tr16_b64<off>(f[4 * dt], vaddr[2 * dt]);
          lds_read_tr16_b64<off>(f[4 * dt + 1], vaddr[2 * dt + 1]);
          lds_read_tr16_b64<off + PLANE>(f[4 * dt + 2], vaddr[2 * dt]);
          lds_read_tr16_b64<off + PLANE>(f[4 * dt + 3], vaddr[2 * dt + 1]);
        }
      };
      vread(std::integral_constant<int, 0>{}, vf[0]);
      static_for<2 * NKT>([&](auto jc) {
        constexpr int j = decltype(jc)::value, kt = j >> 1, s2 = j & 1;
        if constexpr (j + 1 < 2 * NKT) vread(std::integral_constant<int, j + 1>{}, vf[(j + 1) & 1]);
        typedef float f32x4_ __attribute__((ext_vector_type(4)));
        const h8 eh = __builtin_bit_cast(h8, (f32x4_)__builtin_shufflevector(sacc[kt], sacc[kt], 4 * s2, 4 * s2 + 1, 4 * s2 + 2, 4 * s2 + 3));
        const h8 el = __builtin_bit_cast(h8, (f32x4_)__builtin_shufflevector(sacc[kt], sacc[kt], 8 + 4 * s2, 9 + 4 * s2, 10 + 4 * s2, 11 + 4 * s2));
        lgkm_wait<(j + 1 < 2 * NKT) ? 8 : 0>();
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          h8 vh, vl;
          const h4 a0h = __builtin_bit_cast(h4, vf[j & 1][4 * dt]), a1h = __builtin_bit_cast(h4, vf[j & 1][4 * dt + 1]);
          const h4 c0h = __builtin_bit_cast(h4, vf[j & 1][4 * dt + 2]), c1h = __builtin_bit_cast(h4, vf[j & 1][4 * dt + 3]);
#pragma unroll
          for (int e = 0; e < 4; ++e) { vh[e] = a0h[e]; vh[4 + e] = a1h[e]; vl[e] = c0h[e]; vl[4 + e] = c1h[e]; }
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, eh, oacc[dt], 0, 0, 0);
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, el, oacc[dt], 0, 0, 0);
          oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, eh, oacc[dt], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      });
    }
    // v_query (this wave's own rows of V) into registers: the V planes are released at the end of this step
    h4 vqh[8], vql[8];
    {
      const int tqc = tq < T ? tq : 0;
#pragma unroll
      for (int c = 0; c < 8; ++c) {
        const int vo = vswz(tqc, c) + 8 * h;
        vqh[c] = *reinterpret_cast<const h4*>(sVh + vo);
        vql[c] = *reinterpret_cast<const h4*>(sVl + vo);
      }
    }
    // ================= output step (global step 4i + 3 + HALF); the next queries are fetched here
    D3D_STEP_SYNC(3);
    __builtin_amdgcn_s_setprio(ATTN_PRIO_SOFT);
    if (has_next) dma(HALF == 0 ? 1 : 2, tok0_n, hd_n);
    if (has_next) load_q(tok0_n, hd_n);
    // ---- O = O^T / (2^13 l) - v_query, packed as hi/lo of 8*o; stored in the next score step
    {
      // 8 o = oacc * (8 inv) - (vq_hi + vq_lo): the planes hold 8 v, so this is 8 * fma(oacc, inv, -v) bit for bit (powers of
      // two commute with the rounding), without the two scalings per element; range guard on |8 o| accordingly
      const float inv8 = 8.0f * (1.0f / (8192.0f * l));
      float amax = 0.0f;   // range guard (rows tq >= T are never stored)
#pragma unroll
      for (int dt = 0; dt < 2; ++dt) {
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) {
          // -(vq_hi + vq_lo) by two v_fma_mix_f32 on the packed fp16 halves (exact: the pair sums to <= 22 bits), one fma, then
          // hi = fp16(8 o), lo = fp16(8 o - hi) by v_fma_mixlo / mixhi: 5.5 VALU instructions per value where convert / convert /
          // add / fma / max / clamp / convert / convert back / subtract / convert took 10 (this step is VALU-issue-bound).  Same bits
          // whenever |8 o| is inside the fp16 range; beyond it the range guard fires either way.
          const uint2 ph2 = __builtin_bit_cast(uint2, vqh[dt * 4 + g4]), pl2 = __builtin_bit_cast(uint2, vql[dt * 4 + g4]);
          float o8[4];
#pragma unroll
          for (int pr = 0; pr < 2; ++pr) {
            const unsigned ph_ = pr ? ph2.y : ph2.x, pl_ = pr ? pl2.y : pl2.x;
            float n0, n1;
            asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel_hi:[1,0,0]" : "=v"(n0) : "v"(pl_), "v"(-1.0f));
            asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(n0) : "v"(ph_), "v"(-1.0f), "v"(n0));
            asm("v_fma_mix_f32 %0, %1, %2, 0 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(n1) : "v"(pl_), "v"(-1.0f));
            asm("v_fma_mix_f32 %0, %1, %2, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(n1) : "v"(ph_), "v"(-1.0f), "v"(n1));
            o8[2 * pr] = __builtin_fmaf(oacc[dt][4 * g4 + 2 * pr], inv8, n0);
            o8[2 * pr + 1] = __builtin_fmaf(oacc[dt][4 * g4 + 2 * pr + 1], inv8, n1);
          }
          amax = fmaxf(fmaxf(amax, fabsf(o8[0])), fabsf(o8[1]));
          amax = fmaxf(fmaxf(amax, fabsf(o8[2])), fabsf(o8[3]));
          unsigned h0, l0, h1, l1;
          split_pair(o8[0], o8[1], 1.0f, h0, l0);
          split_pair(o8[2], o8[3], 1.0f, h1, l1);
          const h4 oh = __builtin_bit_cast(h4, make_uint2(h0, h1)), ol = __builtin_bit_cast(h4, make_uint2(l0, l1));
          // columns 8 g4 + 4 h .. + 3 of line dt: hi halves in chunk g4, lo halves in chunk 4 + g4 (pair layout)
          patch_wr(patch, r, h, g4, oh, ol);
        }
        asm volatile("" ::: "memory");     // (the rows read back were written by other lanes)
#pragma unroll
        for (int it = 0; it < 4; ++it) po[dt * 4 + it] = patch_rd(patch, 8 * it + (lane >> 3), lane & 7);
      }
      if (tq < T && amax > X3_HALF_MAX) range_raise(rw, RANGE_BIT_ACT);
      po_ptr = out_x3 + (tok0 + (size_t)(32 * wave + (lane >> 3)) * J) * 2 * D + hd * 2 * XDH + 8 * (lane & 7);
      po_valid = true;
    }
    hd = hd_n; tok0 = tok0_n;
  }
  if (HALF == 0) D3D_STEP_SYNC(4);      // global step 4n: half 1's last output step
#undef D3D_STEP_SYNC
  {   // outputs of the last unit
#pragma unroll
    for (int it = 0; it < 4; ++it)
      if (32 * wave + 8 * it + (lane >> 3) < T) {
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) *reinterpret_cast<u32x4*>(po_ptr + it * po_stride + dt * 64) = po[dt * 4 + it];
      }
  }
}

template <int NKT>
__global__ __launch_bounds__(64 * NKT) void k_attn_temporal_x3s(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl,
                                                                _Float16* __restrict__ out_x3, int T, int J, int H, int D, int units,
                                                                unsigned* rw) {
  static_assert(NKT == 8, "two halves of four waves");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_s[];
  constexpr int TP = 32 * NKT;
  constexpr int PLANE = TP * 128;
  if ((int)blockIdx.x >= units) return;                        // workgroup-uniform
  for (int idx = (int)threadIdx.x; idx < (TP - T) * 8 * 4; idx += 64 * NKT) {   // pad rows [T, TP) of the four planes: zero once
    const int pl = idx / ((TP - T) * 8), rem = idx % ((TP - T) * 8);
    *reinterpret_cast<uint4*>(lds_s + pl * PLANE + (T + (rem >> 3)) * 128 + ((rem & 7) << 4)) = make_uint4(0, 0, 0, 0);
  }
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);   // 32-query tile of the unit
  if (wave < 4) attn_x3s_half<NKT, 0>(Ph, Pl, out_x3, T, J, H, D, units, lds_s, wave, rw);
  else attn_x3s_half<NKT, 1>(Ph, Pl, out_x3, T, J, H, D, units, lds_s, wave, rw);
}

bool attn_temporal_x3_ok(int T, int D, int H) { return T >= 1 && T <= 256 && H > 0 && D == H * XDH; }

template <int NKT, int MU = 1>
static hipError_t launch_x3_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D,
                                int H, hipStream_t s) {
  const size_t lds_bytes = (size_t)MU * 4 * 32 * NKT * 128;   // per unit: K_hi, K_lo, V_hi, V_lo planes of TP rows x 128 B
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL) return hipErrorInvalidValue;
  return launch_lds<k_attn_temporal_x3<NKT, MU>>(dim3((unsigned)((units + MU - 1) / MU)), dim3(64 * NKT * MU), lds_bytes, s, ph, pl, ox, T,
                                                 J, H, D, (int)units, launch_range_word());
}

template <int NKT, int MU = 1, int WIT = 3>
static hipError_t launch_x3p_nkt(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H,
                                 hipStream_t s) {
  // wave-private units (MU > 1, NKT == 1): 6 planes of T rows per wave (V double-buffered) + one zeroed pad behind the last
  const size_t lds_bytes = MU > 1 ? (size_t)MU * 6 * T * 128 + (size_t)(32 * NKT - T) * 128 + (size_t)MU * 4096 : (size_t)4 * 32 * NKT * 128 + (size_t)NKT * 4096;
  const int n_cu = device_cu_count();
  if (n_cu <= 0) return hipErrorUnknown;
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL || lds_bytes > 160 * 1024) return hipErrorInvalidValue;
  // resident workgroups per CU: what registers and LDS allow together (asked from the runtime once per device: sized by the LDS
  // alone, the T = 81 form launched three 3-wave workgroups per CU where the register file held two -- a third of its units
  // then ran as a second pass at half the residency)
  static std::atomic<unsigned long long> per_cu_cache[64];   // (lds_bytes << 8) | workgroups: the wave-private form's LDS varies with T
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return hipErrorUnknown;
  const unsigned long long cached = per_cu_cache[dev & 63].load(std::memory_order_acquire);
  int per_cu = (cached >> 8) == (unsigned long long)lds_bytes ? (int)(cached & 255) : 0;
  if (per_cu <= 0) {
    per_cu = resident_workgroups_per_cu(reinterpret_cast<const void*>(&k_attn_temporal_x3p<NKT, MU, WIT>), 64 * NKT * MU, lds_bytes);
    if (per_cu <= 0) per_cu = 1;
    if (per_cu > 255) per_cu = 255;
    per_cu_cache[dev & 63].store(((unsigned long long)lds_bytes << 8) | (unsigned)per_cu, std::memory_order_release);
  }
  const long long wgs = (units + MU - 1) / MU;
  const long long grid = wgs < (long long)n_cu * per_cu ? wgs : (long long)n_cu * per_cu;
  // the wave-private form's LDS varies with T: it opts in to the whole 160 KiB once
  return launch_lds_optin<k_attn_temporal_x3p<NKT, MU, WIT>>(MU > 1 ? (size_t)160 * 1024 : lds_bytes, dim3((unsigned)grid), dim3(64 * NKT * MU),
                                                             lds_bytes, s, ph, pl, ox, T, J, H, D, (int)units, launch_range_word());
}

static hipError_t launch_x3s(const _Float16* ph, const _Float16* pl, _Float16* ox, int B, int T, int J, int D, int H, hipStream_t s) {
  constexpr int NKT = 8;
  const size_t lds_bytes = (size_t)4 * 32 * NKT * 128 + NKT * 4096;   // K / V planes + one 4 KiB output patch per wave = 160 KiB
  const int n_cu = device_cu_count();
  if (n_cu <= 0) return hipErrorUnknown;
  const long long units = (long long)B * J * H;
  if (units > 0x7fffffffLL / 4) return hipErrorInvalidValue;
  const long long grid = units < n_cu ? units : n_cu;
  return launch_lds<k_attn_temporal_x3s<NKT>>(dim3((unsigned)grid), dim3(64 * NKT), lds_bytes, s, ph, pl, ox, T, J, H, D, (int)units,
                                              launch_range_word());
}

hipError_t launch_attn_temporal_x3(const void* qkv_hi, const void* qkv_lo, void* out_x3, int B, int T, int J,
                                   int D, int H, hipStream_t s) {
  if (!attn_temporal_x3_ok(T, D, H) || !qkv_hi || !qkv_lo || !out_x3) return hipErrorInvalidValue;
  const _Float16 *ph = (const _Float16*)qkv_hi, *pl = (const _Float16*)qkv_lo;
  _Float16* ox = (_Float16*)out_x3;
  // persistent, DMA-staged form where a launch has several units per CU (instantiated for the frame counts of the
  // reference configs: T = 81 -> 3 key tiles, T = 243 -> 8)
  const bool persist = (long long)B * J * H >= 1024;
  switch ((T + 31) / 32) {
    case 1:   // groups of <= 32 tokens (spatial blocks: the 17 joints of a frame).  8 units per workgroup = the 8 heads of one
              // frame at H = 8, so a workgroup reads whole token rows; measured 0.61 ms per launch at T=243, B=64 against
              // 0.82 / 0.68 / 0.69 ms with 1 / 2 / 4 units per workgroup.
      if ((long long)B * J * H >= 4096 && T <= 24 && (size_t)8 * 6 * T * 128 + (size_t)(32 - T) * 128 + 8 * 4096 <= 160 * 1024)
        return launch_x3p_nkt<1, 8>(ph, pl, ox, B, T, J, D, H, s);
      // groups of 25 .. 32 tokens (the temporal blocks of the T = 27 configuration): six wave-private units fit the 160 KiB, and
      // the output patch takes four 8-row passes
      if ((long long)B * J * H >= 4096 && (size_t)6 * 6 * T * 128 + (size_t)(32 - T) * 128 + 6 * 4096 <= 160 * 1024)
        return launch_x3p_nkt<1, 6, 4>(ph, pl, ox, B, T, J, D, H, s);
      if ((long long)B * J * H >= 4096) return launch_x3_nkt<1, 8>(ph, pl, ox, B, T, J, D, H, s);
      return launch_x3_nkt<1, 1>(ph, pl, ox, B, T, J, D, H, s);
    case 2: return launch_x3_nkt<2>(ph, pl, ox, B, T, J, D, H, s);
    case 3: return (persist ? launch_x3p_nkt<3> : launch_x3_nkt<3, 1>)(ph, pl, ox, B, T, J, D, H, s);
    case 4: return launch_x3_nkt<4>(ph, pl, ox, B, T, J, D, H, s);
    case 5: return launch_x3_nkt<5>(ph, pl, ox, B, T, J, D, H, s);
    case 6: return launch_x3_nkt<6>(ph, pl, ox, B, T, J, D, H, s);
    case 7: return launch_x3_nkt<7>(ph, pl, ox, B, T, J, D, H, s);
    default: return (persist ? launch_x3s : launch_x3_nkt<8, 1>)(ph, pl, ox, B, T, J, D, H, s);
  }
}

// ---- helpers for the test hook: fp32 qkv -> planes (q third scaled by 2^-3), planes -> fp32
__global__ __launch_bounds__(256) void k_split_qkv(const float* __restrict__ x, _Float16* __restrict__ hi, _Float16* __restrict__ lo,
                                                   size_t n, int D3, int D) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int col = (int)(i % D3);
  const float s = __builtin_amdgcn_fmed3f(x[i] * (col < D ? 1.0f : 8.0f), -65504.0f, 65504.0f);
  const _Float16 hh = (_Float16)s;
  hi[i] = hh;
  lo[i] = (_Float16)(s - (float)hh);
}

__global__ __launch_bounds__(256) void k_unsplit_pair(const _Float16* __restrict__ pair, float* __restrict__ x, size_t n, int cols) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t row = i / cols;
  const _Float16* p = pair + row * 2 * cols + pair_col((int)(i - row * cols));
  x[i] = ((float)p[0] + (float)p[PAIR_LO]) * 0.125f;
}

hipError_t launch_split_qkv(const float* x, void* hi, void* lo, size_t rows, int D, hipStream_t s) {
  const size_t n = rows * 3 * (size_t)D;
  hipLaunchKernelGGL(k_split_qkv, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, (_Float16*)hi, (_Float16*)lo, n, 3 * D, D);
  return hipGetLastError();
}

hipError_t launch_unsplit_pair(const void* pair, float* x, size_t rows, int cols, hipStream_t s) {
  const size_t n = rows * (size_t)cols;
  hipLaunchKernelGGL(k_unsplit_pair, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const _Float16*)pair, x, n, cols);
  return hipGetLastError();
}

}  // namespace d3d
