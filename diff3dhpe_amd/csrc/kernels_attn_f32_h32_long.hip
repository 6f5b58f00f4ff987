// Temporal GRAND attention in exact fp32 on the matrix pipe for heads of 32 columns and windows of ANY length: the width-32
// instantiation of the three-pass key-streaming walk k_attn_f32_stream3<DH> (attn_f32_tile.h; the walk is described in
// kernels_attn_f32_long.hip, which launches it at width 64).  Bit-identical to launch_attn_temporal_f32_h32 for T <= 256
// (tests/test_gpu_long_f32_h32.py): both kernels take the two forms of the exp argument from f32_exp_tile.  A chunk of 256 keys is
// 69 632 B, two workgroups per CU by LDS.
#include "attn_f32_tile.h"

namespace d3d {

// (the workgroup count B J H ceil(T / 256) is checked against 31 bits at the launch, where B and J are known)
bool attn_temporal_f32_h32_long_ok(int T, int D, int H) { return T >= 1 && H > 0 && D == H * 32; }

hipError_t launch_attn_temporal_f32_h32_long(const float* qkv, float* out, int B, int T, int J, int D, int H, hipStream_t s) {
  if (!attn_temporal_f32_h32_long_ok(T, D, H) || !qkv || !out || B <= 0 || J <= 0) return hipErrorInvalidValue;
  return f32_launch_stream<k_attn_f32_stream3<32>, 32>(qkv, out, B, T, J, D, H, s);
}

}  // namespace d3d
