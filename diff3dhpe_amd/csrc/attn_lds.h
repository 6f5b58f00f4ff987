// LDS layout helpers of the attention kernels (kernels_attn_x3.hip, kernels_attn_x3_long.hip, kernels_attn_bf16.hip and the attention steps of the fused
// kernels_qkv_sattn.hip, kernels_qkv_tattn.hip, kernels_qkv_attn_bf16.hip, kernels_qkv_attn_x3_small.hip), included inside namespace d3d: the row
// swizzles of the K / Q and V planes, the hi / lo fp16 splits, the output patch.  The F16X3 tile arithmetic on these layouts is attn_x3_tile.h.
#pragma once

#include "kloop_common.h"   // h8 / h4 / u32x4 / u32x4_alias

// K / Q rows: a fragment read takes 16 consecutive rows at one logical 16-byte chunk
__device__ __forceinline__ int kswz(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }
// V rows: the four key rows k0..k0+3 of one transpose read must land in four different 64-byte bank groups (row parity
// picks the half of the 256-byte bank row, bit 1 of the row flips chunk bit 2); rows 4 apart are additionally rotated
// over the low chunk bits so that the row-parallel v_query reads of the epilogue (32 lanes, 32 rows, same logical
// chunk) are 2-way instead of 16-way conflicted.  (row >> 2) is constant inside a transpose read, so those stay conflict-free.
__device__ __forceinline__ int vkey(int row) { return (((row >> 1) & 1) << 2) ^ ((row >> 2) & 3); }
__device__ __forceinline__ int vswz(int row, int chunk) { return row * 128 + ((chunk ^ vkey(row)) << 4); }

// Output patch, write side.  Lane (row r, half h) of the O^T accumulator layout holds 4 columns of a 16-byte chunk -- hi and lo
// halves (oh, ol: 8 bytes each) of columns 8 g + 4 h .. + 3.  Written as two ds_write_b64 per lane, rows r and r + 1 of a
// 16-lane group share a 16-byte slot (a lane's 8-byte position inside its chunk is fixed by h, the same for the whole group):
// a 2-way bank conflict on every write -- 0.33 (spatial) / 0.13 (temporal) of all LDS cycles of these kernels (rocprofv3
// SQ_LDS_BANK_CONFLICT, round 2).  v_permlane32_swap trades the halves between lanes l and l + 32 instead: lanes < 32 then own
// the WHOLE hi chunk of their row, lanes >= 32 the whole lo chunk, one ds_write_b128 each, 16-byte slots XOR-swizzled by
// (row & 7) -- conflict-free on the write (8 consecutive rows per lane group) and on the ds_read_b128 read-back (patch_rd).
__device__ __forceinline__ void patch_wr(unsigned char* patch, int r, int h, int g, h4 oh, h4 ol) {
  const uint2 a = __builtin_bit_cast(uint2, oh), b = __builtin_bit_cast(uint2, ol);
  const auto s0 = __builtin_amdgcn_permlane32_swap(a.x, b.x, false, false);   // new a[l + 32] = b[l], new b[l] = a[l + 32]
  const auto s1 = __builtin_amdgcn_permlane32_swap(a.y, b.y, false, false);
  u32x4_alias v;
  v[0] = s0[0]; v[1] = s1[0]; v[2] = s0[1]; v[3] = s1[1];
  *reinterpret_cast<u32x4_alias*>(patch + r * 128 + ((((h << 2) + g) ^ (r & 7)) << 4)) = v;
}
__device__ __forceinline__ u32x4 patch_rd(const unsigned char* patch, int row, int chunk) {
  return *reinterpret_cast<const u32x4_alias*>(patch + row * 128 + ((chunk ^ (row & 7)) << 4));
}

// (v0, v1) -> packed fp16 pairs hi = fp16(k v), lo = fp16(k v - hi), k a power of two: v_fma_mixlo/mixhi_f16 do scale,
// subtract (reading the fp16 hi half directly) and convert in one instruction each -- 2 VALU instructions per value where the
// generic lowering (multiply, convert, convert back, subtract, convert, pack) takes 5.  Same values: k v and k v - hi are exact
// in fp32, so every form rounds the same quantity once (the split of split8_x3).
// split_pair: the scale in a VGPR, not volatile (plane writes and output steps: the compiler may schedule them among the LDS writes)
__device__ __forceinline__ void split_pair(float v0, float v1, float k, unsigned& hi, unsigned& lo) {
  asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(v0), "v"(k));
  asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(v1), "v"(k));
  asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(v0), "v"(k), "v"(hi));
  asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(v1), "v"(k), "v"(hi));
}
// split_pair_s: the scale in an SGPR; volatile pins the split to the step it is written in (the softmax numerators)
__device__ __forceinline__ void split_pair_s(float e0, float e1, float k, unsigned& hi, unsigned& lo) {
  asm volatile("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(hi) : "v"(e0), "s"(k));
  asm volatile("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(hi) : "v"(e1), "s"(k));
  asm volatile("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(lo) : "v"(e0), "s"(k), "v"(hi));
  asm volatile("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(lo) : "v"(e1), "s"(k), "v"(hi));
}
// eight numerators (one 16-key k-step of a lane) -> the MFMA B fragments hi / lo of 1024 e
__device__ __forceinline__ void split8_e(const float (&e)[8], h8& eh, h8& el) {
  u32x4 hv, lv;
#pragma unroll
  for (int pr = 0; pr < 4; ++pr) {
    unsigned a, b;
    split_pair_s(e[2 * pr], e[2 * pr + 1], 1024.0f, a, b);
    hv[pr] = a; lv[pr] = b;
  }
  eh = __builtin_bit_cast(h8, hv);
  el = __builtin_bit_cast(h8, lv);
}
