// Temporal GRAND attention in exact fp32 on the matrix pipe for windows of ANY length, heads of 64 and of 32 columns: the keys stream
// through LDS in chunks of 256 frames instead of all living there (k_attn_temporal_f32<NKT> in kernels_attn.hip and
// k_attn_temporal_f32_h32<NKT> in kernels_attn_f32_h32.hip: K and V of T <= 256 rows).  One kernel template over the head width,
// k_attn_f32_stream3<DH> in attn_f32_tile.h, on the pieces of that header (this unit instantiates and launches DH = 64,
// kernels_attn_f32_h32_long.hip DH = 32), so the arithmetic is the resident kernel's of that width, statement for statement.
//
// Both widths normalise BEFORE the second product (F32Tile::NORM_AT_STORE is false).  An order-preserving streaming form of that needs l
// before the first V product, so three passes over the keys:
//
//   pass 1   per chunk: stage K; per key tile the DH / 2 MFMAs of S^T, keys >= T at -inf, running fmaxf in register order; cross-half
//            shuffle
//   pass 2   per chunk: stage K; the SAME MFMAs again (same bits), e = expf(s - m), l += e with key tiles and registers ascending;
//            cross-half add
//   pass 3   per chunk: stage K and V; the same MFMAs a third time, p = expf(s - m) / l (width 64, T <= 256: - 1 where the global key
//            index is the lane's query), the MFMAs of O^T per tile in the resident kernel's order
//
// So every expf sees the same argument, l is summed in the same order and oacc takes the same MFMAs in the same order as in the resident
// kernel: for T <= 256 the output is bit-identical to launch_attn_temporal_f32 / launch_attn_temporal_f32_h32
// (tests/test_gpu_long_temporal_f32.py, tests/test_gpu_long_f32_h32.py).  The price is the scores computed three times (and expf twice);
// one score tile (16 registers) is live at a time.
//
// The diagonal: v[query] is subtracted at the store, except at width 64 for T <= 256, where the resident kernel to agree with has the
// - 1 in P (F32Tile::DIAG_IN_P_RESIDENT).
//
// One workgroup per (batch, joint, head, query block), f32_launch_stream's geometry.  A chunk is 8 key tiles: 132 KiB at width 64, 68 KiB
// at width 32 (two workgroups per CU by LDS) -- the resident kernel's footprint at NKT = 8.
// Every wave executes every barrier: the chunk and key-tile trip counts depend on T alone, a wave whose queries are all >= T stages
// and synchronises and only skips its stores.
#include "attn_f32_tile.h"

namespace d3d {

// (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
bool attn_temporal_f32_long_ok(int T, int D, int H) { return T >= 1 && H > 0 && D == H * 64; }

hipError_t launch_attn_temporal_f32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  return f32_launch_stream<k_attn_f32_stream3<64>, 64>(qkv, out, B, T, J, D, H, s);
}

}  // namespace d3d
