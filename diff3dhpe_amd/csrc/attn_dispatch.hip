// The table of attention kernel families, the option keys that gate them, the attention plan and its info keys (attn_dispatch.h).
// Host code only: the launchers and predicates it refers to live beside their kernels (kernels_attn*.hip).  The device pass of the
// compiler sees an empty unit -- it would otherwise emit the constant tables, whose entries are host functions.
#ifndef __HIP_DEVICE_COMPILE__
#include "attn_dispatch.h"

#include <cstring>

#include "../../include/d3d.h"
#include "d3d_kernels.h"

namespace d3d {

const AttnOption ATTN_OPTIONS[AO_COUNT] = {   // (in the order of AttnOpt)
    {"long_temporal", true},     {"long_temporal_f32", true},     {"attn_h32", true},  {"attn_f32_h32", true},
    {"long_temporal_h32", true}, {"long_temporal_f32_h32", true}, {"attn_h128", true}, {"attn_f32_h128", true},
    {"attn_hx", true},           {"attn_f32_hx", true},           {"attn_h16", ATTN_H16_DEFAULT}, {"attn_f32_h16", ATTN_F32_H16_DEFAULT}};

int attn_option_index(const char* key) {
  for (int i = 0; i < AO_COUNT; ++i)
    if (!strcmp(key, ATTN_OPTIONS[i].key)) return i;
  return -1;
}

unsigned attn_option_defaults() {
  unsigned w = 0;
  for (int i = 0; i < AO_COUNT; ++i) w |= ATTN_OPTIONS[i].def ? 1u << i : 0u;
  return w;
}

namespace {

// ---- the launchers of d3d_kernels.h behind the one signature ----
struct Groups {   // (batches, group length, tokens between a group's members): a spatial block is (B T, J, 1)
  int B, T, J;
  explicit Groups(const AttnArgs& a) : B(a.temporal ? a.B : a.B * a.T), T(a.temporal ? a.T : a.J), J(a.temporal ? a.J : 1) {}
};
template <hipError_t (*F)(const void*, const void*, void*, int, int, int, int, int, hipStream_t)>
hipError_t planes(const AttnArgs& a) {
  const Groups g(a);
  return F(a.qkv, a.qkv_lo, a.out_x3, g.B, g.T, g.J, a.D, a.H, a.s);
}
template <hipError_t (*F)(const float*, float*, int, int, int, int, int, hipStream_t)>
hipError_t rows(const AttnArgs& a) {
  const Groups g(a);
  return F(static_cast<const float*>(a.qkv), a.out, g.B, g.T, g.J, a.D, a.H, a.s);
}
// the launchers that take the block's own (B, T, J): the spatial kernel of width 32 and, with their pair-layout output, those of
// kernels_attn.hip
hipError_t spatial_f32_h32(const AttnArgs& a) {
  return launch_attn_spatial_f32_h32(static_cast<const float*>(a.qkv), a.out, a.B, a.T, a.J, a.D, a.H, a.s);
}
template <hipError_t (*F)(const float*, float*, void*, int, int, int, int, int, hipStream_t)>
hipError_t rows_x3(const AttnArgs& a) {
  return F(static_cast<const float*>(a.qkv), a.out, a.out_x3, a.B, a.T, a.J, a.D, a.H, a.s);
}
hipError_t generic(const AttnArgs& a) {
  return launch_attn_generic(static_cast<const float*>(a.qkv), a.out, a.out_x3, a.B, a.T, a.J, a.D, a.H, a.temporal ? 1 : 0, a.s);
}
bool any_shape(int, int, int) { return true; }

// ---- the regimes: {predicate, launch, option, the op hook's D3D_EUNSUP message} ----
constexpr AttnRegime NONE = {nullptr, nullptr, AO_NONE, nullptr};
constexpr AttnRegime GENERIC = {any_shape, generic, AO_NONE, nullptr};
constexpr AttnRegime X3_H32 = {attn_x3_h32_ok, planes<launch_attn_x3_h32>, AO_ATTN_H32,
                               "F16X3 attention for head_dim 32: an even head count, group length <= 256"};
constexpr AttnRegime X3_H32_LONG = {attn_x3_h32_long_ok, planes<launch_attn_x3_h32_long>, AO_LONG_TEMPORAL_H32,
                                    "key-streaming F16X3 attention for head_dim 32: an even head count"};
constexpr AttnRegime X3_H128 = {attn_x3_h128_ok, planes<launch_attn_x3_h128>, AO_ATTN_H128,
                                "F16X3 attention for head_dim 128: groups of up to 128 tokens"};
constexpr AttnRegime X3_H128_LONG = {attn_x3_h128_long_ok, planes<launch_attn_x3_h128_long>, AO_ATTN_H128,
                                     "key-streaming F16X3 attention: head_dim 128"};
constexpr AttnRegime X3_HX = {attn_x3_hx_ok, planes<launch_attn_x3_hx>, AO_ATTN_HX,
                              "F16X3 attention for head_dim 48 or 96: groups of up to 256 (head_dim 48) / 128 (head_dim 96) tokens"};
constexpr AttnRegime X3_HX_LONG = {attn_x3_hx_long_ok, planes<launch_attn_x3_hx_long>, AO_ATTN_HX,
                                   "key-streaming F16X3 attention: head_dim 48 or 96"};
constexpr AttnRegime X3_H16 = {attn_x3_h16_ok, planes<launch_attn_x3_h16>, AO_ATTN_H16,
                               "F16X3 attention for head_dim 16: a multiple of 4 heads, groups of up to 256 tokens"};
constexpr AttnRegime X3_H16_LONG = {attn_x3_h16_long_ok, planes<launch_attn_x3_h16_long>, AO_ATTN_H16,
                                    "key-streaming F16X3 attention: head_dim 16, a multiple of 4 heads"};
constexpr AttnRegime X3 = {attn_temporal_x3_ok, planes<launch_attn_temporal_x3>, AO_NONE, nullptr};   // (hook: d3d_op_attention)
constexpr AttnRegime X3_LONG = {attn_temporal_x3_long_ok, planes<launch_attn_temporal_x3_long>, AO_LONG_TEMPORAL,
                                "key-streaming F16X3 attention: head_dim 64"};
constexpr AttnRegime F32_H32_SP = {attn_spatial_f32_h32_ok, spatial_f32_h32, AO_ATTN_F32_H32,
                                   "fp32 spatial attention for head_dim 32: 15 to 17 joints"};
constexpr AttnRegime F32_H32_TP = {attn_temporal_f32_h32_ok, rows<launch_attn_temporal_f32_h32>, AO_ATTN_F32_H32,
                                   "fp32 temporal attention for head_dim 32: window length <= 256"};
constexpr AttnRegime F32_H32_LONG = {attn_temporal_f32_h32_long_ok, rows<launch_attn_temporal_f32_h32_long>, AO_LONG_TEMPORAL_F32_H32,
                                     "key-streaming fp32 attention: head_dim 32"};
constexpr AttnRegime F32_H128 = {attn_f32_h128_ok, rows<launch_attn_f32_h128>, AO_ATTN_F32_H128,
                                 "fp32 attention for head_dim 128: groups of up to 128 tokens"};
constexpr AttnRegime F32_H128_LONG = {attn_f32_h128_long_ok, rows<launch_attn_f32_h128_long>, AO_ATTN_F32_H128,
                                      "key-streaming fp32 attention: head_dim 128"};
constexpr AttnRegime F32_HX = {attn_f32_hx_ok, rows<launch_attn_f32_hx>, AO_ATTN_F32_HX,
                               "fp32 attention for head_dim 48 or 96: groups of up to 256 (head_dim 48) / 192 (head_dim 96) tokens"};
constexpr AttnRegime F32_HX_LONG = {attn_f32_hx_long_ok, rows<launch_attn_f32_hx_long>, AO_ATTN_F32_HX,
                                    "key-streaming fp32 attention: head_dim 48 or 96"};
constexpr AttnRegime F32_H16 = {attn_f32_h16_ok, rows<launch_attn_f32_h16>, AO_ATTN_F32_H16,
                                "fp32 attention for head_dim 16: groups of up to 256 tokens"};
constexpr AttnRegime F32_H16_LONG = {attn_f32_h16_long_ok, rows<launch_attn_f32_h16_long>, AO_ATTN_F32_H16,
                                     "key-streaming fp32 attention: head_dim 16"};
constexpr AttnRegime F32_SP = {attn_spatial_fast_ok, rows_x3<launch_attn_spatial_f32>, AO_NONE, nullptr};   // (hook: d3d_op_attention)
constexpr AttnRegime F32_TP = {attn_temporal_fast_ok, rows_x3<launch_attn_temporal_f32>, AO_NONE, nullptr};
constexpr AttnRegime F32_LONG = {attn_temporal_f32_long_ok, rows<launch_attn_temporal_f32_long>, AO_LONG_TEMPORAL_F32,
                                 "key-streaming fp32 attention: head_dim 64"};

}  // namespace

// name, form, narrow, d32, spatial, temporal, streaming, stream_above, key, key_mode, key_stream.  Widths 64 and 32 have a streaming
// option of their own and stream beyond the 256 frames their resident kernels hold; the later widths stream wherever the resident
// predicate fails.  What differs by width inside a launcher -- head-count rule, resident limit, chunk length: the table of d3d_kernels.h.
constexpr AttnFamily ATTN_FAMILIES[AF_COUNT] = {
    {"generic",  ATTN_ROWS,   false, false, GENERIC,    GENERIC,    NONE,          0,   nullptr,              ATTN_KEY_NONE, nullptr},
    {"x3_h32",   ATTN_PLANES, true,  false, X3_H32,     X3_H32,     X3_H32_LONG,   256, "attn_h32_last",      ATTN_KEY_BOTH, "long_temporal_h32_last"},
    {"x3_h128",  ATTN_PLANES, false, false, X3_H128,    X3_H128,    X3_H128_LONG,  0,   "attn_h128_last",     ATTN_KEY_BITS, nullptr},
    {"x3_hx",    ATTN_PLANES, false, false, X3_HX,      X3_HX,      X3_HX_LONG,    0,   "attn_hx_last",       ATTN_KEY_BITS, nullptr},
    {"x3_h16",   ATTN_PLANES, true,  false, X3_H16,     X3_H16,     X3_H16_LONG,   0,   "attn_h16_last",      ATTN_KEY_BITS, nullptr},
    {"x3",       ATTN_PLANES, false, false, X3,         X3,         X3_LONG,       256, nullptr,              ATTN_KEY_NONE, "long_temporal_last"},
    {"f32_h32",  ATTN_ROWS,   false, false, F32_H32_SP, F32_H32_TP, F32_H32_LONG,  256, "attn_f32_h32_last",  ATTN_KEY_BITS, "long_temporal_f32_h32_last"},
    {"f32_h128", ATTN_ROWS,   false, false, F32_H128,   F32_H128,   F32_H128_LONG, 0,   "attn_f32_h128_last", ATTN_KEY_BITS, nullptr},
    {"f32_hx",   ATTN_ROWS,   false, true,  F32_HX,     F32_HX,     F32_HX_LONG,   0,   "attn_f32_hx_last",   ATTN_KEY_BITS, nullptr},
    {"f32_h16",  ATTN_ROWS,   false, false, F32_H16,    F32_H16,    F32_H16_LONG,  0,   "attn_f32_h16_last",  ATTN_KEY_BITS, nullptr},
    {"f32",      ATTN_ROWS,   false, false, F32_SP,     F32_TP,     F32_LONG,      256, nullptr,              ATTN_KEY_NONE, "long_temporal_f32_last"}};

const char* attn_family_name(int family) { return family >= 0 && family < AF_COUNT ? ATTN_FAMILIES[family].name : nullptr; }

namespace {

// The ladders of the plain (row-kernel) flow, first rung that holds: {family, streaming}
struct Rung { AttnFamilyId family; bool stream; };
constexpr Rung PLAIN_SPATIAL[] = {{AF_X3, false}, {AF_F32_H32, false}, {AF_F32_H128, false}, {AF_F32_HX, false}, {AF_F32_H16, false},
                                  {AF_F32, false}, {AF_GENERIC, false}};
constexpr Rung PLAIN_TEMPORAL[] = {{AF_X3, false},      {AF_F32_H32, false}, {AF_F32, true},     {AF_F32_H32, true},
                                   {AF_F32_H128, false}, {AF_F32_H128, true}, {AF_F32_HX, false}, {AF_F32_HX, true},
                                   {AF_F32_H16, false},  {AF_F32_H16, true},  {AF_F32, false},    {AF_GENERIC, false}};

// A rung holds for groups of N tokens.  F16X3 engines take the planes kernel where the group length fits, q / k / v going to it as
// planes; every fp32 kernel behind an option belongs to FP32 engines alone (heads of 48 columns in ones or threes, D % 32 != 0, keep the
// generic kernel in both precisions, bit for bit); the kernels of kernels_attn.hip serve both.
template <size_t R>
AttnPick plain_pick(const Rung (&ladder)[R], bool temporal, int precision, unsigned opts, int N, int D, int H) {
  for (const Rung& g : ladder) {
    const AttnPick pick{g.family, g.stream ? 1 : 0};
    const AttnFamily& f = pick.fam();
    const AttnRegime& r = pick.regime(temporal);
    const bool engine = f.form == ATTN_PLANES ? precision == D3D_PREC_F16X3
                                              : r.opt == AO_NONE || (precision == D3D_PREC_FP32 && (opts >> r.opt & 1u));
    if (engine && !(f.d32 && D % 32 != 0) && !(g.stream && N <= f.stream_above) && r.ok(N, D, H)) return pick;
  }
  return AttnPick{};   // (not reached: the generic rung holds for every shape)
}

}  // namespace

AttnChoice attn_choose(int precision, unsigned opts, bool fold_layernorm, int T, int J, int D, int H) {
  const auto on = [&](AttnOpt o) { return o == AO_NONE || (opts >> o & 1u) != 0; };
  AttnChoice c;
  // The folded flow: the first ATTN_PLANES family (their predicates exclude each other by head width) whose resident kernel takes the
  // spatial groups and which serves the window, resident where its option and predicate allow, else streaming.  The spatial blocks ask no
  // option of their own: at width 32 "long_temporal_h32" alone keeps the flow for a long window, "attn_h32" alone does not.
  if (precision == D3D_PREC_F16X3 && fold_layernorm && D % 32 == 0) {
    for (int i = 0; i < AF_COUNT; ++i) {
      const AttnFamily& f = ATTN_FAMILIES[i];
      if (f.form != ATTN_PLANES || !f.sp.ok(J, D, H)) continue;
      const bool resident = on(f.tp.opt) && f.tp.ok(T, D, H);
      const bool streams = f.stream.ok && on(f.stream.opt) && T > f.stream_above && f.stream.ok(T, D, H);
      if (!resident && !streams) continue;
      c.flow = ATTN_FLOW_FOLD;
      c.sp = AttnPick{i, 0};
      c.tp = AttnPick{i, resident ? 0 : 1};
      return c;
    }
  }
  if (precision == D3D_PREC_BF16 || precision == D3D_PREC_F16) {   // (one flow for both 16-bit operand modes)
    c.flow = ATTN_FLOW_BF16;
    return c;
  }
  c.sp = plain_pick(PLAIN_SPATIAL, false, precision, opts, J, D, H);
  c.tp = plain_pick(PLAIN_TEMPORAL, true, precision, opts, T, D, H);
  return c;
}

bool attn_plan_key(const AttnChoice& c, const char* key, int64_t* value) {
  for (int i = 0; i < AF_COUNT; ++i) {
    const AttnFamily& f = ATTN_FAMILIES[i];
    const bool live = c.flow == (f.form == ATTN_PLANES ? ATTN_FLOW_FOLD : ATTN_FLOW_PLAIN);
    const int sp = live && c.sp.family == i && !c.sp.stream, tp = live && c.tp.family == i && !c.tp.stream,
              tp_stream = live && c.tp.family == i && c.tp.stream;
    if (f.key && !strcmp(key, f.key)) {
      *value = f.key_mode == ATTN_KEY_BOTH ? (sp && tp) : sp | tp << 1 | (f.key_stream ? 0 : tp_stream << 2);
      return true;
    }
    if (f.key_stream && !strcmp(key, f.key_stream)) {
      *value = tp_stream;
      return true;
    }
  }
  return false;
}

}  // namespace d3d
#endif   // !__HIP_DEVICE_COMPILE__
