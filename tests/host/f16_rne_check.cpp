// Stand-alone driver of the fp16 side of the host weight packing (diff3dhpe_amd/csrc/weight_pack.hip: f16_rne, pack_bf16's fp16 form), built
// and run as an ordinary program by tests/test_f16_mode_host.py.  Input: fp32 bit patterns as hex words on stdin.  Output: per word
// "<fp16 bits as hex> <nonfinite flag>", which the test compares with torch's .to(float16); then the pack check's verdict.
#include <cstdio>
#include <cstring>
#include <vector>

#include "weight_pack.h"

using namespace d3d;

static int check_pack() {
  // one block of D = 64, Dm = 128: the fp16 images have pack_bf16's layout ([rows padded to 256][K], pad rows zero), every element is
  // f16_rne of its weight, and `clamped` rises for a finite weight whose fp16 image is inf exactly as for a non-finite one
  const size_t D = 64, Dm = 128;
  std::vector<float> qkv(3 * D * D), proj(D * D), fc1(Dm * D), fc2(D * Dm), vec(3 * D + Dm, 0.f);
  auto fill = [](std::vector<float>& w, float scale) {
    for (size_t i = 0; i < w.size(); ++i) w[i] = scale * (float)((int)((i * 2654435761u) >> 9 & 0xffff) - 32768) / 32768.0f;
  };
  fill(qkv, 1.0f); fill(proj, 3.0e-6f); fill(fc1, 1.0e-7f); fill(fc2, 1000.0f);   // (ordinary, subnormal, below-subnormal, large)
  int bad = 0;
  for (int pass = 0; pass < 3; ++pass) {
    if (pass == 1) fc2[77] = 70000.0f;   // finite, beyond the fp16 range
    if (pass == 2) {                     // the last fp32 below the tie 65520: rounds DOWN to 65504, finite
      const unsigned below = 0x477fefffu;
      fc2[77] = 1.0f;
      memcpy(&proj[5], &below, 4);
    }
    BlockSrc s{vec.data(), vec.data(), qkv.data(), vec.data(), proj.data(), vec.data(), vec.data(), vec.data(), fc1.data(), vec.data(), fc2.data(), vec.data()};
    PackedWeights h, b;
    pack_bf16({s}, D, Dm, h, true);
    pack_bf16({s}, D, Dm, b);
    if (h.planes.size() != b.planes.size() || h.blk.size() != 1) { printf("pack: sizes differ\n"); return 1; }
    const BlockOff &ho = h.blk[0], &bo = b.blk[0];
    if (ho.qkv_x3 != bo.qkv_x3 || ho.proj_x3 != bo.proj_x3 || ho.fc1_x3 != bo.fc1_x3 || ho.fc2_x3 != bo.fc2_x3) { printf("pack: offsets differ\n"); return 1; }
    if (h.clamped != (pass == 1) || b.clamped) { printf("pack: pass %d clamped %d (bf16 %d)\n", pass, (int)h.clamped, (int)b.clamped); ++bad; }
    struct { const std::vector<float>* w; size_t off, rows, cols; } m[4] = {
        {&qkv, ho.qkv_x3, 3 * D, D}, {&proj, ho.proj_x3, D, D}, {&fc1, ho.fc1_x3, Dm, D}, {&fc2, ho.fc2_x3, D, Dm}};
    for (auto& x : m) {
      for (size_t i = 0; i < x.rows * x.cols; ++i) bad += h.planes[x.off + i] != f16_rne((*x.w)[i]);
      for (size_t i = x.rows * x.cols; i < pad256(x.rows) * x.cols; ++i) bad += h.planes[x.off + i] != 0;
    }
  }
  if (bad) printf("pack: %d mismatches\n", bad);
  return bad;
}

int main() {
  unsigned u;
  while (scanf("%x", &u) == 1) {
    float f;
    memcpy(&f, &u, 4);
    bool flag = false;
    const uint16_t h = f16_rne(f, &flag);
    if (f16_rne(f) != h) return 2;   // (the flag pointer is optional)
    printf("%04x %d\n", (unsigned)h, (int)flag);
  }
  if (check_pack()) return 1;
  printf("pack: ok\n");
  return 0;
}
