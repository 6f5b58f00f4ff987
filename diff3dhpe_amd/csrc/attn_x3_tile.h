// The F16X3 attention arithmetic of the compiler-scheduled kernels, once: k_attn_temporal_x3 and k_attn_temporal_x3p (kernels_attn_x3.hip),
// k_attn_x3_stream (kernels_attn_x3_long.hip) and qm_attention (kernels_qkv_attn_x3_small.hip) are their own staging, walks and
// stores around these pieces, so every rounding-relevant statement -- MFMA order, key mask, exp2 argument, numerator split, output fma,
// clamp and hi / lo split -- has one copy and the forms are bit-identical by construction (tests/test_gpu_attn_x3_digests.py and
// test_gpu_attn_x3_width_digests.py pin the bits).  The statically scheduled kernels (attn_x3s_half, qs_attention, k_qkv_tattn) state the
// same arithmetic as their own instruction streams and are what these pieces are compared against.  Included inside namespace d3d, behind attn_lds.h.
//
//   S^T = K Q^T        rows = keys, column = this lane's query; acc = 64 s (q planes hold q / 8, k planes 8 k)
//   e   = exp(S - max) exact two-pass softmax numerator, fp32, one query column per lane (halves h = 0 / 1 hold different keys)
//   O^T = V^T E^T      E split in-register into hi / lo of 1024 e; acc = 2^13 sum e v (v planes hold 8 v)
//   O   = O^T / (2^13 l) - v_query
#pragma once

#include "attn_lds.h"

constexpr float X3_C_EXP = 1.4426950408889634f / 64.0f;   // acc = 64 s: scale and log2(e) in one fma feeding v_exp_f32
// The same constant for a head width DH.  The planes hold raw q and 8 k whatever the width, so acc = 8 q.k and the exponent argument is
// acc log2(e) / (8 sqrt(DH)): X3_C_EXP itself at 64; at 32 (kernels_attn_x3_h32.hip), at 128 (kernels_attn_x3_h128.hip) and at 48
// and 96 (kernels_attn_x3_hx.hip) evaluated in double and rounded once.  At 16 (kernels_attn_x3_h16.hip) sqrt(DH) = 4 and the constant is
// log2(e) / 32 = 2 * X3_C_EXP, exactly: a power of two times a float.
template <int DH>
constexpr float x3_c_exp() {
  static_assert(DH == 64 || DH == 32 || DH == 128 || DH == 48 || DH == 96 || DH == 16, "head widths with a tile form");
  return DH == 64 ? X3_C_EXP
       : DH == 16 ? 2 * X3_C_EXP
       : DH == 32 ? (float)(1.4426950408889634 / (8.0 * 5.656854249492380195 /* sqrt(32) */))
       : DH == 48 ? (float)(1.4426950408889634 / (8.0 * 6.928203230275509174 /* sqrt(48) */))
       : DH == 96 ? (float)(1.4426950408889634 / (8.0 * 9.797958971132712393 /* sqrt(96) */))
                  : (float)(1.4426950408889634 / (8.0 * 11.313708498984760390 /* sqrt(128) */));
}

// ---- this lane's query row as MFMA B fragments, d = 16 ks + 8 h .. + 7: from the global planes (o: element offset of a real row's
// head columns + 8 h; !valid: zeros instead) or from an LDS Q plane pair at a row.  A row >= T is never stored: its caller gives it
// zeros or a real row.  NKS: the d-steps that belong to the head where it ends inside the 64 columns (widths 48 and 96); the others
// are exact zeros, never the neighbouring head's columns.
template <int NKS = 4>
__device__ __forceinline__ void x3_q_global(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, size_t o, bool valid, h8 (&qh)[4],
                                            h8 (&ql)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    if (valid && ks < NKS) {
      qh[ks] = *reinterpret_cast<const h8*>(Ph + o + 16 * ks);
      ql[ks] = *reinterpret_cast<const h8*>(Pl + o + 16 * ks);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) { qh[ks][e] = (_Float16)0.0f; ql[ks][e] = (_Float16)0.0f; }
    }
  }
}
__device__ __forceinline__ void x3_q_lds(const unsigned char* sQh, const unsigned char* sQl, int row, int h, h8 (&qh)[4], h8 (&ql)[4]) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int qo = kswz(row, 2 * ks + h);
    qh[ks] = *reinterpret_cast<const h8*>(sQh + qo);
    ql[ks] = *reinterpret_cast<const h8*>(sQl + qo);
  }
}

// ---- one 32 x 32 S^T tile of the K rows row0 .. row0 + 31 (r = lane & 31, h = lane >> 5): register q of half h is key
// (q & 3) + 8 (q >> 2) + 4 h of the tile.  Three fp16 MFMAs per 16-deep d-step, small terms first.  KS0 / NKS: the d-steps of the 64-wide
// LDS row that belong to the head (all four; a 32-wide head of a pair takes two).
template <int KS0 = 0, int NKS = 4>
__device__ __forceinline__ f32x16 x3_score_tile(const unsigned char* sKh, const unsigned char* sKl, int row0, int r, int h, const h8 (&qh)[4],
                                                const h8 (&ql)[4]) {
  f32x16 s;
#pragma unroll
  for (int q = 0; q < 16; ++q) s[q] = 0.f;
#pragma unroll
  for (int ks = KS0; ks < KS0 + NKS; ++ks) {
    const int ko = kswz(row0 + r, 2 * ks + h);
    const h8 kh = *reinterpret_cast<const h8*>(sKh + ko);
    const h8 kl = *reinterpret_cast<const h8*>(sKl + ko);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s, 0, 0, 0);
  }
  return s;
}

// The accumulate-into form: the same four d-steps added onto s, for heads wider than one 64-column LDS row (kernels_attn_x3_h128.hip: one
// chain over the row halves in ascending d, each half's K rows in planes of their own).  x3_score_tile is left as it is, so its
// instantiations' code does not change.  NKS: the leading d-steps of the row that belong to the head (a 96-wide head's second row: two).
template <int NKS = 4>
__device__ __forceinline__ void x3_score_acc(f32x16& s, const unsigned char* sKh, const unsigned char* sKl, int row0, int r, int h,
                                             const h8 (&qh)[4], const h8 (&ql)[4]) {
#pragma unroll
  for (int ks = 0; ks < NKS; ++ks) {
    const int ko = kswz(row0 + r, 2 * ks + h);
    const h8 kh = *reinterpret_cast<const h8*>(sKh + ko);
    const h8 kl = *reinterpret_cast<const h8*>(sKl + ko);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kl, qh[ks], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, ql[ks], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_32x32x16_f16(kh, qh[ks], s, 0, 0, 0);
  }
}

// keys >= T score -inf: their numerator is an exact 0, whatever bits the K rows hold.  Register q of lane half h, tile's first key key0.
__device__ __forceinline__ float x3_mask_key(float s, int key0, int q, int h, int T) {
  return key0 + (q & 3) + 8 * (q >> 2) + 4 * h >= T ? -INFINITY : s;
}
__device__ __forceinline__ void x3_mask_keys(f32x16& s, int key0, int h, int T) {
#pragma unroll
  for (int q = 0; q < 16; ++q) s[q] = x3_mask_key(s[q], key0, q, h, T);
}

// numerators of one tile in place, e = 2^((acc - max) log2(e) / 64) with mb = max * X3_C_EXP, summed into l in register order
// (DH: the head width, x3_c_exp<DH>() in place of X3_C_EXP)
template <int DH = 64>
__device__ __forceinline__ void x3_exp_tile(f32x16& s, float mb, float& l) {
#pragma unroll
  for (int q = 0; q < 16; ++q) {
    const float e = __builtin_amdgcn_exp2f(fmaf(s[q], x3_c_exp<DH>(), -mb));
    s[q] = e;
    l += e;
  }
}

// ---- exact (max-subtracted) softmax over the NKT resident tiles of this query column: sacc becomes the numerators, their sum over
// both lane halves is returned.  Only the last key tile can hold keys >= T, so only it pays for the mask.
template <int NKT, int DH = 64>
__device__ __forceinline__ float x3_softmax(f32x16 (&sacc)[NKT], int h, int T) {
  float m = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) {
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      if (kt == NKT - 1) sacc[kt][q] = x3_mask_key(sacc[kt][q], kt * 32, q, h, T);
      m = fmaxf(m, sacc[kt][q]);
    }
  }
  m = fmaxf(m, __shfl_xor(m, 32, 64));
  const float mb = m * x3_c_exp<DH>();
  float l = 0.f;
#pragma unroll
  for (int kt = 0; kt < NKT; ++kt) x3_exp_tile<DH>(sacc[kt], mb, l);
  l += __shfl_xor(l, 32, 64);
  return l;
}

// ---- O^T[d][query] += sum over the 32 keys of key tile kt of V^T[d][key] E^T[key][query]; the group's V rows start at plane row rb.
// k-step s takes numerator registers 8 s .. 8 s + 7: element jj of lane half h is key 32 kt + 16 s + 8 (jj >> 2) + 4 h + (jj & 3), and
// the V^T fragment is read in that order.  ds_read_b64_tr_b16: within a 16-lane group, lane 4 q + p supplies the address of (row k0 + q,
// columns d0 + 4 p .. + 3) and lane i receives column d0 + i of the four rows, i.e. V[k0 .. k0 + 3][d] for this lane's d -- the MFMA A
// fragment.
// VMASK: for planes whose rows behind the group's T are not zeros -- compact planes, where they are the next group's (or the next
// plane's) rows and may hold NaN / Inf of ANOTHER group (the GEMM epilogues store a NaN as a NaN).  E is an exact 0 there, and 0 x NaN is
// NaN: the V bits of keys >= T are masked to +0 in registers; element e of a fragment is key k0 + e (e < 4) / k0 + 4 + e (e >= 4).  Only
// the half-tile that holds keys >= T pays for it (wave-uniform branch).
// DT0 / NDT: the 32-column halves of the 64-wide LDS row that belong to the head (both; a 32-wide head of a pair takes its own one).
template <bool VMASK, int DT0 = 0, int NDT = 2>
__device__ __forceinline__ void x3_pv_tile(const f32x16& e, const unsigned char* sVh, const unsigned char* sVl, int rb, int kt, int T, int lane,
                                           int h, f32x16 (&oacc)[2]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    h8 eh, el;                                                  // e in [0, 1] -> hi / lo of 2^10 e
    {
      float e8[8];
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) e8[jj] = e[8 * s + jj];
      split8_e(e8, eh, el);
    }
    const int k0 = kt * 32 + 16 * s + 4 * h;                    // first key of this lane half's fragment
    const int gi = lane & 15, tq_ = gi >> 2, tp_ = gi & 3;
    const bool vpad = VMASK && kt * 32 + 16 * s + 16 > T;
    u32x4 vmask = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    if (vpad) {
#pragma unroll
      for (int j2 = 0; j2 < 4; ++j2) {
        const int ka = k0 + 8 * (j2 >> 1) + 2 * (j2 & 1);       // key of element 2 j2; element 2 j2 + 1 is the next key
        vmask[j2] = (ka < T ? 0x0000ffffu : 0u) | (ka + 1 < T ? 0xffff0000u : 0u);
      }
    }
#pragma unroll
    for (int dt = DT0; dt < DT0 + NDT; ++dt) {
      const int d0 = dt * 32 + 16 * ((lane >> 4) & 1);
      const int ch = (d0 >> 3) + (tp_ >> 1), sub = (tp_ & 1) * 8;
      const int o0 = vswz(rb + k0 + tq_, ch) + sub, o1 = vswz(rb + k0 + 8 + tq_, ch) + sub;
      const s4v a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o0));
      const s4v a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVh + o1));
      const s4v c0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o0));
      const s4v c1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s4v*)(uintptr_t)(sVl + o1));
      h8 vh, vl;
      {
        const h4 a0h = __builtin_bit_cast(h4, a0), a1h = __builtin_bit_cast(h4, a1);
        const h4 c0h = __builtin_bit_cast(h4, c0), c1h = __builtin_bit_cast(h4, c1);
#pragma unroll
        for (int i = 0; i < 4; ++i) { vh[i] = a0h[i]; vh[4 + i] = a1h[i]; vl[i] = c0h[i]; vl[4 + i] = c1h[i]; }
      }
      if (vpad) {
        vh = __builtin_bit_cast(h8, __builtin_bit_cast(u32x4, vh) & vmask);
        vl = __builtin_bit_cast(h8, __builtin_bit_cast(u32x4, vl) & vmask);
      }
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vl, eh, oacc[dt], 0, 0, 0);
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, el, oacc[dt], 0, 0, 0);
      oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vh, eh, oacc[dt], 0, 0, 0);
    }
    __builtin_amdgcn_sched_barrier(0);   // keep the V^T reads / conversions of later k-steps from being hoisted (VGPR pressure)
  }
}

// ---- the shape of a head of DH columns on the 64-column (128-byte) LDS rows, for a kernel that is written once for every width
// (k_attn_x3_stream, kernels_attn_x3_long.hip).  A unit -- what one workgroup's waves attend over -- is SUB adjacent 64-column segments of
// the plane rows, each in a sub-plane of its own (sub-plane f of a plane starts pl bytes behind sub-plane f - 1), and carries STREAMS
// independent softmax streams, each with its own score tile, maximum and sum:
//   DH = 32    a PAIR of heads in one segment; head p is stream p: d-steps 2 p, 2 p + 1 of the score product, 32-column half p of the PV
//              product and of the output
//   DH = 16    a QUAD of heads in one segment; head p is stream p: d-step p of the score product (a 16-deep d-step is exactly the head's
//              columns), and the 16 rows 16 (p & 1) .. + 15 of an O^T accumulator of its own over 32-column line p >> 1 -- the other 16
//              rows of that tile are the line neighbour's V times this head's E and are never stored
//   DH = 64    one head, one segment, one stream
//   DH = 128   one head in two segments: one score chain over segment 0 then segment 1, one stream, a PV step per segment
// Widths 48 and 96 are no multiple of 64 columns: a head starts at plane column hd DH, wherever that falls, and ends inside its last
// LDS row (x3_stage_cols stages from a column offset; the rest of that row is zeros or not read):
//   DH = 48    one head in one LDS row: three d-steps of the score product, two PV lines of which the second is half used (columns 48 .. 63
//              of the K and V rows are exact zeros)
//   DH = 96    one head in two LDS rows, 64 + 32 columns: the chain of DH = 128 with two d-steps and one PV line in the second row
//              (its upper 32 columns are neither staged nor read)
// The MFMA order of every accumulator is the one of k_attn_x3_h32 / k_attn_temporal_x3 / k_attn_x3_h128 / k_attn_x3_hx / k_attn_x3_h16.
template <int DH>
struct x3_head_shape {
  static_assert(DH == 32 || DH == 64 || DH == 128 || DH == 48 || DH == 96 || DH == 16, "head widths with a tile form");
  static constexpr int SUB = DH > 64 ? 2 : 1;
  static constexpr int STREAMS = DH == 32 ? 2 : DH == 16 ? 4 : 1;
  static constexpr int COLS = DH < 64 && 64 % DH == 0 ? 64 : DH;   // plane columns of a unit (a pair of 32, a quad of 16: one segment)
  static constexpr bool ALIGNED = COLS % 64 == 0;                  // a unit is whole 64-column segments of the plane rows
  static constexpr bool heads_ok(int H) { return H >= 1 && H % STREAMS == 0; }
  static constexpr int units_per_token(int H) { return H / STREAMS; }
  // O^T accumulators, oacc[ACCS][2].  Every width but 16: oacc[f][dt] is 32-column line dt of segment f, shared by nobody or (width 32)
  // owned by one stream.  Width 16: two heads share a line, so head p has oacc[p][p >> 1] to itself (the pair's other entry is never
  // touched) and only rows 16 (p & 1) .. + 15 of it are the head's.
  static constexpr int ACCS = DH == 16 ? 4 : SUB;
  // the stream whose 1 / (2^13 l) scales 32-column line dt of a segment (not at width 16, where a line has two)
  static constexpr int line_stream(int dt) { return DH == 32 ? dt : 0; }
  // the columns of segment f that belong to the unit, and of them those of 32-column line dt
  static constexpr int seg_cols(int f) { return COLS - 64 * f < 64 ? COLS - 64 * f : 64; }
  static constexpr int line_cols(int f, int dt) { return seg_cols(f) - 32 * dt >= 32 ? 32 : seg_cols(f) - 32 * dt > 0 ? seg_cols(f) - 32 * dt : 0; }

  // the S^T tile(s) of the 32 staged K rows from row0 on, unmasked
  static __device__ __forceinline__ void scores(f32x16 (&s)[STREAMS], const unsigned char* sKh, const unsigned char* sKl, int pl, int row0, int r,
                                                int h, const h8 (&qh)[SUB][4], const h8 (&ql)[SUB][4]) {
    if constexpr (DH == 32) {
      s[0] = x3_score_tile<0, 2>(sKh, sKl, row0, r, h, qh[0], ql[0]);
      s[1] = x3_score_tile<2, 2>(sKh, sKl, row0, r, h, qh[0], ql[0]);
    } else if constexpr (DH == 16) {
      s[0] = x3_score_tile<0, 1>(sKh, sKl, row0, r, h, qh[0], ql[0]);
      s[1] = x3_score_tile<1, 1>(sKh, sKl, row0, r, h, qh[0], ql[0]);
      s[2] = x3_score_tile<2, 1>(sKh, sKl, row0, r, h, qh[0], ql[0]);
      s[3] = x3_score_tile<3, 1>(sKh, sKl, row0, r, h, qh[0], ql[0]);
    } else if constexpr (DH == 64) {
      s[0] = x3_score_tile<>(sKh, sKl, row0, r, h, qh[0], ql[0]);
    } else if constexpr (DH == 48) {
      s[0] = x3_score_tile<0, 3>(sKh, sKl, row0, r, h, qh[0], ql[0]);
    } else {
#pragma unroll
      for (int q = 0; q < 16; ++q) s[0][q] = 0.f;
      x3_score_acc(s[0], sKh, sKl, row0, r, h, qh[0], ql[0]);
      x3_score_acc<DH == 96 ? 2 : 4>(s[0], sKh + pl, sKl + pl, row0, r, h, qh[1], ql[1]);
    }
  }
  // O^T += V^T E^T over staged key tile kt; oacc: see ACCS
  static __device__ __forceinline__ void pv(const f32x16 (&e)[STREAMS], const unsigned char* sVh, const unsigned char* sVl, int pl, int kt, int T,
                                            int lane, int h, f32x16 (&oacc)[ACCS][2]) {
    if constexpr (DH == 32) {
      x3_pv_tile<false, 0, 1>(e[0], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
      x3_pv_tile<false, 1, 1>(e[1], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
    } else if constexpr (DH == 16) {
      x3_pv_tile<false, 0, 1>(e[0], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
      x3_pv_tile<false, 0, 1>(e[1], sVh, sVl, 0, kt, T, lane, h, oacc[1]);
      x3_pv_tile<false, 1, 1>(e[2], sVh, sVl, 0, kt, T, lane, h, oacc[2]);
      x3_pv_tile<false, 1, 1>(e[3], sVh, sVl, 0, kt, T, lane, h, oacc[3]);
    } else if constexpr (DH == 64 || DH == 48) {
      x3_pv_tile<false>(e[0], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
    } else if constexpr (DH == 96) {
      x3_pv_tile<false>(e[0], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
      x3_pv_tile<false, 0, 1>(e[0], sVh + pl, sVl + pl, 0, kt, T, lane, h, oacc[1]);
    } else {
      x3_pv_tile<false>(e[0], sVh, sVl, 0, kt, T, lane, h, oacc[0]);
      x3_pv_tile<false>(e[0], sVh + pl, sVl + pl, 0, kt, T, lane, h, oacc[1]);
    }
  }
};

// ---- output columns 8 g4 + 4 h .. + 3 of d half dt (acc: that half's O^T accumulator; vqh / vql: the query row's own V there, hi / lo
// of 8 v): o = acc / (2^13 l) - v_query with inv = 1 / (2^13 l), the range-guard maximum, and hi / lo of 8 o for the proj GEMM.  The one
// place this is rounded: fma, clamp, split.
__device__ __forceinline__ void x3_out_chunk(const f32x16& acc, int g4, float inv, h4 vqh, h4 vql, float& amax, h4& oh, h4& ol) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const float vq = ((float)vqh[e] + (float)vql[e]) * 0.125f;
    const float o = __builtin_fmaf(acc[4 * g4 + e], inv, -vq);
    amax = fmaxf(amax, fabsf(o));
    const float sc = __builtin_amdgcn_fmed3f(o * 8.0f, -65504.0f, 65504.0f);
    oh[e] = (_Float16)sc;
    ol[e] = (_Float16)(sc - (float)oh[e]);
  }
}

// ---- rows [row0, row0 + 32 nkt) of a unit's K (and V) planes, head hd, through registers into rows [0, 32 nkt) of the swizzled LDS
// planes; rows >= T as zeros.  Batches of four 16-byte slots per thread, all global loads of a batch issued before its LDS writes.
// (hd counts heads of 64 columns: for 32-wide heads it is the index of the pair.)
template <bool WITH_V>
__device__ __forceinline__ void x3_stage_rows(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, unsigned char* sKh,
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
        const size_t o = (tok0 + (size_t)(row0 + row) * J) * D3 + hd * 64 + c8 * 8;
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

// ---- the same staging from a plane column: rows [row0, row0 + 32 nkt) of the K (and V) columns col0 .. col0 + 8 NCH - 1 into 16-byte
// chunks 0 .. NCH - 1 of rows [0, 32 nkt) of the swizzled LDS planes, for heads that do not start on a 64-column boundary (widths 48 and
// 96; col0 % 8 == 0, so every load is 16-byte aligned and ends inside the head).  WCH (4 or 8, >= NCH) chunks of a row are written:
// those from NCH on as exact zeros -- never the neighbouring head's columns -- and those from WCH on not at all (nothing may read them).
// Rows >= T as zeros.
template <bool WITH_V, int NCH, int WCH>
__device__ __forceinline__ void x3_stage_cols(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, unsigned char* sKh,
                                              unsigned char* sKl, unsigned char* sVh, unsigned char* sVl, size_t tok0, int J, int D, int col0,
                                              int row0, int nkt, int T, int tid, int nthr) {
  static_assert((WCH == 4 || WCH == 8) && NCH >= 1 && NCH <= WCH, "whole chunks of a 128-byte row");
  constexpr int NIT = 4;
  const int slots = nkt * 32 * WCH;
  const int D3 = 3 * D;
  for (int base = 0; base < slots; base += NIT * nthr) {
    uint4 kh[NIT], kl[NIT], vh[NIT], vl[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int idx = base + tid + it * nthr;
      const int row = idx / WCH, c8 = idx % WCH;
      kh[it] = make_uint4(0, 0, 0, 0); kl[it] = kh[it]; vh[it] = kh[it]; vl[it] = kh[it];
      if (idx < slots && row0 + row < T && c8 < NCH) {
        const size_t o = (tok0 + (size_t)(row0 + row) * J) * D3 + col0 + c8 * 8;
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
      const int row = idx / WCH, c8 = idx % WCH;
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

// A unit's segment f through whichever staging its width takes: whole 64-column segments by index (x3_stage_rows), or from the unit's
// first plane column col0 (x3_stage_cols: the head's columns of the segment, zeros up to the last chunk that is read).
template <int DH, bool WITH_V, int F>
__device__ __forceinline__ void x3_stage_segment(const _Float16* __restrict__ Ph, const _Float16* __restrict__ Pl, unsigned char* sKh,
                                                 unsigned char* sKl, unsigned char* sVh, unsigned char* sVl, size_t tok0, int J, int D, int col0,
                                                 int row0, int nkt, int T, int tid, int nthr) {
  using HS = x3_head_shape<DH>;
  if constexpr (HS::ALIGNED) {
    x3_stage_rows<WITH_V>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, (col0 >> 6) + F, row0, nkt, T, tid, nthr);
  } else {
    constexpr int NCH = HS::seg_cols(F) / 8;
    x3_stage_cols<WITH_V, NCH, (NCH <= 4 ? 4 : 8)>(Ph, Pl, sKh, sKl, sVh, sVl, tok0, J, D, col0 + 64 * F, row0, nkt, T, tid, nthr);
  }
}
