// What the LDS-DMA k-loop kernels share (kernels_gemm_x3p.hip and the kernels on the two-phase loop of qkv_fused_kloop.h), included
// inside namespace d3d like gemm_x3p_prelude.h: the vector typedefs, the SGPR pointer pin, the counted vmcnt wait, the LDS-DMA
// instruction, the DMA plan of a k-tile and the XCD-aware tile order of the persistent walks.
#pragma once

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef short s4v __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
// LDS patches and planes are written as one type and read back as another: through may_alias types, or type-based alias analysis is
// free to move the read-back above the writes (it did, in the four-pass form of the T = 81 attention kernel)
typedef unsigned u32x4_alias __attribute__((ext_vector_type(4), may_alias));
typedef unsigned u32x2_alias __attribute__((ext_vector_type(2), may_alias));

// wave-uniform pointer pinned into an SGPR pair
__device__ __forceinline__ const char* sgpr_ptr(const char* p) {
  const unsigned long long v = reinterpret_cast<unsigned long long>(p);
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const char*>(((unsigned long long)hi << 32) | lo);
}

__device__ __forceinline__ void wait_vm(int n) {   // s_waitcnt vmcnt(n), n wave-uniform
  switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    case 4: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    case 5: asm volatile("s_waitcnt vmcnt(5)" ::: "memory"); break;
    case 6: asm volatile("s_waitcnt vmcnt(6)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(7)" ::: "memory"); break;
  }
}

// LDS-DMA (global_load_lds_dwordx4): the wave drops 64 x 16 bytes, lane l's from SRC, at byte DSTOFF + 16 l of the kernel's `lds`
#define KL_GLDS(SRC, DSTOFF)                                                                                            \
  __builtin_amdgcn_global_load_lds((SRC), (__attribute__((address_space(3))) void*)(uintptr_t)(lds + (DSTOFF)), 16, 0, 0)

// ---- DMA plan (branch-free): the k-tile of a BM x BN tile is (BM + BN)/8 pieces of 8 rows x
// 128 B; wave w moves pieces w, w + NW, ... of A, then of W.  A lane serves row (8 piece + lane/8), LDS slot lane%8,
// and fetches the source chunk the swizzle assigns to that slot (constant per lane: NW is even, so (row>>1)&7 =
// 4 (w&1) + lane/16).  Contract: the A buffer holds >= mtiles*BM rows and the W buffer >= ntiles*BN rows
// (padding rows are staged and multiplied but never stored).
// Source addresses are formed as (wave-uniform byte base: SGPR pair, advanced by scalar adds) + (one 32-bit per-lane byte
// offset, the same for every piece and k-tile), so that the DMA takes the saddr form and needs no per-piece 64-bit VALU
// address arithmetic.
// In scope: lane, wave.  AP_ / WP_: operands of RW_ 16-bit words per row, the tile's first rows ROWA_ / ROWB_; NW_ waves; the W rows
// of a stage start at byte AREG_.  Declares K2_ (= RW_), ubA, ubB (this wave's first piece), lofs_, it_stride (between a wave's pieces), dstA, dstB.
#define KL_DMA_PLAN(AP_, WP_, RW_, ROWA_, ROWB_, NW_, AREG_)                                                            \
  const int lr_ = lane >> 3;                                                                                            \
  const int csrc_ = (lane & 7) ^ (((wave & 1) << 2) | (lr_ >> 1));                                                      \
  const size_t K2_ = (RW_);                                                                                             \
  const char* ubA = reinterpret_cast<const char*>(AP_) + (size_t)((ROWA_) + wave * 8) * K2_ * 2;                        \
  const char* ubB = reinterpret_cast<const char*>(WP_) + (size_t)((ROWB_) + wave * 8) * K2_ * 2;                        \
  unsigned lofs_ = (unsigned)(lr_ * (int)K2_ + csrc_ * 8) * 2u;                                                         \
  const size_t it_stride = (size_t)((NW_) * 8) * K2_ * 2;                 /* bytes */                                   \
  const int dstA = wave * 1024 + lane * 16, dstB = (AREG_) + wave * 1024 + lane * 16

// Tile order of the persistent walks: ordinal o -> (M-tile, N-tile) with all N-tiles of an M-tile on one XCD (workgroup b runs on XCD
// b % 8, and a walk visits b, b + gridDim, ...: gridDim % 8 == 0 keeps it there), M-tiles beyond the last whole eight by columns.
// Declares vfull, mrem and the lambda tile_of(o, mt, nt).
#define KL_XCD_TILE_ORDER(MTILES_, NTILES_)                                                                             \
  const int vfull = ((MTILES_) / 8) * 8 * (NTILES_), mrem = (MTILES_) % 8;                                              \
  auto tile_of = [&](int o, int& mt, int& nt) {                                                                         \
    if (o < vfull) {                                                                                                    \
      const int xcd = o & 7, slot = o >> 3;                                                                             \
      mt = (slot / (NTILES_)) * 8 + xcd;                                                                                \
      nt = slot % (NTILES_);                                                                                            \
    } else {                                                                                                            \
      const int o2 = o - vfull;                                                                                         \
      mt = ((MTILES_) / 8) * 8 + o2 % mrem;                                                                             \
      nt = o2 / mrem;                                                                                                   \
    }                                                                                                                   \
  }
