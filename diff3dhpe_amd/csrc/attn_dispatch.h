// The attention kernel families as ONE table (attn_dispatch.hip), and the choice of a forward's attention kernels as a pure function of
// the engine's precision, options and shapes.  The engine (engine.hip: plan, launch, options, "*_last" info keys) and the single-op hooks
// (engine_ops.hip) read the table; a new head width is one row of it plus its kernels.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace d3d {

// ---- the engine options that gate a family ("key" of d3d_engine_set_option / d3d_engine_get_info; include/d3d.h documents each) ----
enum AttnOpt { AO_LONG_TEMPORAL, AO_LONG_TEMPORAL_F32, AO_ATTN_H32, AO_ATTN_F32_H32, AO_LONG_TEMPORAL_H32, AO_LONG_TEMPORAL_F32_H32,
               AO_ATTN_H128, AO_ATTN_F32_H128, AO_ATTN_HX, AO_ATTN_F32_HX, AO_ATTN_H16, AO_ATTN_F32_H16, AO_COUNT, AO_NONE = AO_COUNT };
// The defaults of "attn_h16" / "attn_f32_h16", decided by the table of DESIGN.md section 5 (experiments/attn_h16.py)
constexpr bool ATTN_H16_DEFAULT = true, ATTN_F32_H16_DEFAULT = true;
struct AttnOption { const char* key; bool def; };
extern const AttnOption ATTN_OPTIONS[AO_COUNT];
int attn_option_index(const char* key);   // the AttnOpt of a key, -1: not an attention option
unsigned attn_option_defaults();          // bit i: the default of option i.  An engine holds its settings as such a word

// ---- one launch signature for every kernel ----
// qkv: the block's q / k / v of B sequences, (B T J, 3 D): fp32 rows (ATTN_ROWS), or the fp16 hi plane with the lo plane at qkv_lo
// (ATTN_PLANES).  out: fp32 rows; out_x3: the pair layout -- the only output of the ATTN_PLANES kernels, written instead of out by the
// kernels_attn.hip launches where it is not null (F16X3 engines), not a form the other fp32 kernels have.  Most kernels attend over the T
// tokens of (batch, joint) groups, J tokens apart; a spatial block is B T batches of J consecutive tokens and one joint: the adapters of
// attn_dispatch.hip make that swap where the launcher takes groups.
struct AttnArgs {
  const void *qkv, *qkv_lo; float* out; void* out_x3;
  int B, T, J, D, H; bool temporal; hipStream_t s;
};
using AttnLaunch = hipError_t (*)(const AttnArgs&);
using AttnPredicate = bool (*)(int N, int D, int H);   // N: the group length, T or J

// One way a family serves a block: resident spatial, resident temporal, or key-streaming temporal.  ok == nullptr: the family has none.
struct AttnRegime {
  AttnPredicate ok;
  AttnLaunch launch;
  AttnOpt opt;         // the option that switches it on, AO_NONE: always on
  const char* unsup;   // the D3D_EUNSUP message of its op hook (nullptr: no hook of its own)
};
enum AttnForm { ATTN_ROWS, ATTN_PLANES };   // fp32 rows in and out / hi and lo planes in, pair layout out
// How a family's "*_last" info key reads the plan: 1 where both block types ran it resident / bit 0 spatial, bit 1 temporal resident
// and, in a family without a key_stream of its own, bit 2 temporal streaming
enum AttnKeyMode { ATTN_KEY_NONE, ATTN_KEY_BOTH, ATTN_KEY_BITS };
struct AttnFamily {
  const char* name;            // golden files, debugging
  AttnForm form;
  bool narrow;                 // heads of 32 / 16 columns sharing a 64-column segment: what "fused_narrow" fuses with the qkv GEMM
  bool d32;                    // the engine takes it only where D % 32 == 0
  AttnRegime sp, tp, stream;
  int stream_above;            // the engine streams only windows of more than this many frames
  const char* key;             // info key of the resident regimes, read as key_mode says (nullptr: none)
  AttnKeyMode key_mode;
  const char* key_stream;      // info key of the streaming regime, 0 / 1 (nullptr: bit 2 of key, or none)
};
// The rows.  AF_GENERIC is 0, so a zeroed choice is the generic kernel; the ATTN_PLANES rows stand in the precedence of the folded flow.
enum AttnFamilyId { AF_GENERIC, AF_X3_H32, AF_X3_H128, AF_X3_HX, AF_X3_H16, AF_X3, AF_F32_H32, AF_F32_H128, AF_F32_HX, AF_F32_H16, AF_F32,
                    AF_COUNT };
extern const AttnFamily ATTN_FAMILIES[AF_COUNT];
const char* attn_family_name(int family);   // nullptr beyond the table

// ---- the choice ----
struct AttnPick {
  int family = AF_GENERIC;   // AttnFamilyId
  int stream = 0;            // 1: the key-streaming regime (temporal blocks only)
  const AttnFamily& fam() const { return ATTN_FAMILIES[family]; }
  const AttnRegime& regime(bool temporal) const { return stream ? fam().stream : temporal ? fam().tp : fam().sp; }
};
enum AttnFlow { ATTN_FLOW_PLAIN, ATTN_FLOW_FOLD, ATTN_FLOW_BF16 };   // run_blocks / run_blocks_fold / run_blocks_bf16
struct AttnChoice {
  int flow = ATTN_FLOW_PLAIN;
  AttnPick sp, tp;           // the spatial / the temporal blocks.  BF16: launch_attn_bf16 runs, both stay generic
};
// precision: D3D_PREC_*; opts: the option word.  No engine, no batch size, no device property: an eager run, a capture and a replay agree.
AttnChoice attn_choose(int precision, unsigned opts, bool fold_layernorm, int T, int J, int D, int H);
// The "*_last" info keys: which block types of the plan ran which family.  The ATTN_PLANES keys are 0 outside the folded flow, the
// ATTN_ROWS keys outside the plain one.  false: not one of the keys.
bool attn_plan_key(const AttnChoice& c, const char* key, int64_t* value);

}  // namespace d3d
