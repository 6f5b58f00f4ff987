// Host side of libd3d_hip.so: engine object, weight registry/repack, DDIM schedule, per-step launch sequence and the
// C ABI declared in include/d3d.h (its engine-free single-op hooks: engine_ops.hip).  No CPU compute path exists here: every tensor operation is a kernel from
// kernels_*.hip; the only host arithmetic is the integer timestep schedule and table bookkeeping.
#include <hip/hip_runtime.h>

#include <cmath>
#include <dlfcn.h>
#include <cstdio>
#include <cstring>
#include <map>
#include <algorithm>
#include <string>
#include <vector>

#include "../../include/d3d.h"
#include "attn_dispatch.h"
#include "d3d_kernels.h"
#include "engine_internal.h"

using namespace d3d;

namespace {

thread_local std::string g_err;

}  // namespace

int d3d::fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

namespace {

struct WeightSlot {
  std::string name;
  int64_t numel = 0;
  std::vector<float> host;
  bool set = false;
  size_t dev_off = 0;  // float offset into the device arena
};

struct BlockW : BlockSrc {   // (the block's fp32 tensors, here in the device arena)
  // F16X3 mode: fp16 hi/lo planes of the four GEMM weights (same [N][K] layout)
  const uint16_t *qkv_x3 = nullptr, *proj_x3 = nullptr, *fc1_x3 = nullptr, *fc2_x3 = nullptr;   // F16X3 pair layout
  // LayerNorm-folded forms (X3Fold, d3d_kernels.h; fold_layernorm, weight_pack.h) for norm1 -> qkv and norm2 -> fc1
  const uint16_t *qkv_f3 = nullptr, *fc1_f3 = nullptr;
  const float *qkv_cs = nullptr, *qkv_fb = nullptr, *fc1_cs = nullptr, *fc1_fb = nullptr;
  // fused qkv + attention kernels (kernels_qkv_sattn.hip, kernels_qkv_tattn.hip, kernels_qkv_attn_x3_small.hip): the folded qkv weight /
  // csum / bias with HEAD-MAJOR rows (tile_order_src_row, weight_pack.h; heads of 32 / 16 columns: by 64-column segment)
  const uint16_t* qkv_f3h = nullptr;
  const float *qkv_csh = nullptr, *qkv_fbh = nullptr;
  // exponent k of each weight's planes (2^k w; 12 unless a weight exceeds 15.99: split_weight_f16x3)
  int qkv_e = 12, proj_e = 12, fc1_e = 12, fc2_e = 12, qkv_fe = 12, fc1_fe = 12;
};

// Which kernels one forward of B sequences runs: every choice the block loops branch on, made once by plan_blocks() from the options,
// the shapes, B and the CU count.  The entry points keep the plan they ran; d3d_engine_get_info reads its "*_last" keys from it.
struct BlockPlan {
  // The flow (run_blocks / run_blocks_fold / run_blocks_bf16) and the attention kernel of the spatial / of the temporal blocks wherever
  // the qkv GEMM and the attention are two launches: attn_choose() of attn_dispatch.h.  A BF16 plan runs launch_attn_bf16.
  AttnChoice attn;
  // FOLD, BF16: the qkv GEMM and the attention of the spatial / temporal blocks as one kernel
  bool fused_sp = false, fused_tp = false;
  // FOLD: block 0's q / k / v from the raw input channels and the commit-time tables instead of the K = D qkv GEMM ("block0_direct")
  bool b0_direct = false;
  // FOLD: fc1 / proj on their own kernels; the post-norm inside the fc2 epilogue
  bool fc1_own = false, proj_own = false, pn = false;
  // FOLD with "latency_mode": the S of the split-K form of each GEMM, 0 = the launches above
  int fc2_split = 0, proj_split = 0, fc1_split = 0;
  // FOLD with "latency_mode" and "small_tiles": the fused qkv + attention step of the spatial / temporal blocks on 128-row tiles
  // (kernels_qkv_attn_x3_small.hip) where the 256-row launch would leave CUs without a workgroup; block 0 keeps its direct form
  bool small_sp = false, small_tp = false;
  // FOLD with "fused_narrow" at head widths 32 / 16: the qkv GEMM and the attention of the spatial blocks (block 0 included) / of the
  // temporal blocks (T <= 127) as one launch of the same kernel's narrow forms, in place of the GEMM + attn.sp / attn.tp pair
  bool narrow_sp = false, narrow_tp = false;
  // BF16: whole-row proj / fc2 with their LayerNorms in the epilogue; qkv / fc1 on the hand-specialised GEMM kernel
  bool rows = false, bf16q_qkv = false, bf16q_fc1 = false;
};

}  // namespace

struct d3d_engine {
  d3d_config cfg{};
  int T = 0, J = 0, D = 0, H = 0, Dm = 0, Dt = 0, depth = 0, cin = 0, nblk = 0;
  std::vector<WeightSlot> slots;
  std::map<std::string, int> index;
  std::vector<float> freqs_host;
  bool freqs_set = false;
  bool committed = false;
  bool weights_clamped = false;   // F16X3: a GEMM weight was not finite at commit (range guard; finite weights get a per-matrix scale)
  // d3d_engine_set_option: the F16X3 block flow with the post-norm inside the fc2 epilogue / with norm1, norm2 folded into
  // the consuming GEMMs (both on by default; experiments/ and the A/B tests switch them off)
  bool opt_fused_postnorm = true, opt_fold_layernorm = true;
  // "fused_spatial": the spatial blocks' qkv GEMM and attention as ONE kernel (q / k / v never leave the chip); bit-identical
  bool opt_fused_spatial = true;
  // "fused_temporal": the same for the temporal blocks where the frame count fits one tile (T in 193..255, or T <= 127 with several joints
  // per tile: kernels_qkv_tattn.hip)
  // BF16 mode: both keys select the bf16 qkv GEMM + attention kernels (kernels_qkv_attn_bf16.hip) for their block type, every T <= 255
  bool opt_fused_temporal = true;
  // "block0_direct": block 0 of the F16X3 fold flow computes Wg x0 as G u + P[j] + Q[b] from the CIN raw channels of a token (the input
  // rows are an affine map of them: kernels_qkv_sattn.hip k_qkv_sattn_direct) -- no qkv GEMM in that block; 0 = the GEMM, for A/B runs
  bool opt_block0_direct = true;
  // its tables, resident like the weights (one allocation): Wg = W_qkv diag(gamma1) of block 0 as fp32 [3 D][D] (the weight of the per-forward
  // small linear that makes Q from the time vector, original row order), G = Wg W_e [3 D][CIN] and P[j] = Wg (b_e + spos[j]) [J][3 D] in the
  // head-major tile order of qkv_f3h / qkv_csh / qkv_fbh, so a tile's slices are contiguous
  DevBuf<float> b0_tab;
  const float *b0_wg = nullptr, *b0_G = nullptr, *b0_P = nullptr;
  // "fc1_kernel": fc1 on its own kernel (kernels_fc1_x3.hip) where the launch fills the chip for a few rounds; bit-identical
  bool opt_fc1_kernel = true;
  // "proj_kernel": the same for proj (kernels_proj_x3.hip: whole 192-row tiles; the rows behind the last whole tile stay with the template)
  bool opt_proj_kernel = true;
  // "streams" = 2 (default): d3d_ddim_sample runs two half-batches concurrently, the second on side_stream (forked / joined by
  // events); 1: the whole batch on the caller's stream
  int opt_streams = 2;
  // "bf16_gemm_kernel": BF16 mode, qkv and fc1 on their own kernel (kernels_gemm_bf16q.hip: the hand-specialised k-loop) from two rounds of
  // 256 x 256 tiles on; bit-identical to the token GEMM's forms
  bool opt_bf16_gemm_kernel = true;
  // "head_inject" (tests only): the head kernel perturbs the FIRST of its two evaluations of row 0's dot products, so that its
  // run-time fence -- compare, third evaluation, D3D_RANGE_RECOMPUTE -- can be seen working (kernels_elem.hip k_head)
  int opt_head_inject = 0;
  // "norm_eps_bits": eps of the constructor's norm_layer -- norm1 / norm2 of every block and the two post-norms (S2S:184: LayerNorm
  // eps = 1e-6 unless the caller passes another norm_layer); the head's own LayerNorm keeps its 1e-5 (S2S:218)
  float ln_eps = 1e-6f;
  // "head_fence": that fence on (round 5's default).  Off since round 6: the deviation it guarded against is identified (a packed fp32
  // form beside another wave's MFMAs) and its absence from every kernel is a build-time test
  int opt_head_fence = 0;
  // "latency_mode" (off by default): in the F16X3 folded flow, fc2 + post-norm of a forward too small to fill one round of whole-row
  // tiles runs as a split-K x split-N GEMM + an ordered reduce / post-norm row kernel (d3d_kernels.h fc2_splitk_choose).  Changes the
  // order of additions: results stay inside the parity gate but are no longer bit-identical to the default path's.
  bool opt_latency_mode = false;
  // The options that gate an attention kernel family, one bit each (AttnOpt, attn_dispatch.h: "long_temporal", "long_temporal_f32",
  // "attn_h32", "attn_f32_h32", "long_temporal_h32", "long_temporal_f32_h32", "attn_h128", "attn_f32_h128", "attn_hx", "attn_f32_hx",
  // "attn_h16", "attn_f32_h16"; what each selects: include/d3d.h).  An F16X3 key off = the plain row-kernel flow with the generic fp32
  // attention; an fp32 key off = the generic one-thread-per-row kernel (the fp32 MFMA kernels change the order of additions: inside the
  // parity gate, not bit-identical to it).
  unsigned attn_opts = attn_option_defaults();
  // "deep_stages" of THIS engine: -1 = follow the process-wide default (the key with a NULL engine), 0 / 1 = this engine's own setting.
  // Read into the calling thread's launch context by EngineScope, so two engines driven from two threads never see each other's value.
  int opt_deep_stages = -1;
  // "proj_split" / "fc1_split" (read only while "latency_mode" is on): -1 = the rules of d3d_kernels.h (proj_splitk_choose /
  // fc1_splitk_choose), 0 / 2 / 4 = that S wherever the call fits the kernel pair (else the present launch): measurements and tests
  int opt_proj_split = -1, opt_fc1_split = -1;
  // "small_tiles" (read only while "latency_mode" is on and the flow is the folded one): 1 = the fused qkv + attention launches of a forward
  // that would run fewer workgroups than the device has CUs take the 128-row tiles of kernels_qkv_attn_x3_small.hip where those run at
  // most 5/8 as many workgroups as the device has CUs (bit-identical to the two-kernel flow, so NOT to the grouped temporal form it
  // replaces); 0 (default) = every launch as without the key
  bool opt_small_tiles = false;
  // "fused_narrow" (off by default): an F16X3 engine whose heads are 32 columns wide in pairs or 16 wide in quads runs the qkv GEMM and the
  // attention of its spatial blocks, and of its temporal blocks for windows of up to 127 frames, as ONE kernel (the narrow forms of
  // kernels_qkv_attn_x3_small.hip: q / k / v never reach HBM); bit-identical to the two launches it replaces.  Not tied to "latency_mode"
  bool opt_fused_narrow = false;
  // fc1's partials (S M Dm floats) fit no region of the workspace that is dead at that point for every S: an engine-owned buffer,
  // FC1_SPLITK_SCRATCH_FLOATS per slot, allocated when "latency_mode" is switched on and freed when it is switched off.  Slot 1 serves
  // the second half-batch of a two-stream sampling (the halves run concurrently), allocated by the first such call.
  DevBuf<float> lat_scratch[2];
  // the plan of the most recent forward (of a two-stream sampling: of the first half-batch, the one that holds sequence 0); all zero
  // before any.  d3d_engine_get_info: "fc2_split_last" / "proj_split_last" / "fc1_split_last" = the S that ran (0: the whole launch),
  // "bf16_fused_spatial_last" / "..temporal_last" = whether a BF16 forward ran kernels_qkv_attn_bf16.hip in those blocks,
  // and the keys of the attention kernels that ran, which attn_plan_key() (attn_dispatch.h) states
  BlockPlan last_plan;
  hipStream_t side_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  int device = -1;                // ordinal of the device the weights were committed on
  DevBuf<unsigned> range_dev;     // F16X3 range guard: THIS engine's sticky word (device memory; every plane-writing kernel launched
                                  // for this engine ORs into it -- d3d_kernels.h LaunchCtx::range_word)
  // d3d_engine_range_post / _take: snapshots of the word without a blocking synchronisation -- a ring of pinned, device-mapped host
  // slots (one per ticket), each with the event recorded behind its snapshot kernel
  static constexpr int RANGE_TICKETS = 256;
  unsigned* range_host = nullptr;      // hipHostMalloc'ed, RANGE_TICKETS words
  unsigned* range_host_dev = nullptr;  // the same memory as the device addresses it
  std::vector<hipEvent_t> range_ev;
  long long range_posted = 0;          // tickets handed out so far (ticket t lives in slot t % RANGE_TICKETS)

  DevBuf<float> arena;  // all weights, device
  DevBuf<uint16_t> arena16;  // F16X3: hi/lo planes of the GEMM weights (BF16: their bf16 copies)
  DevBuf<float> arena_fold;  // F16X3: csum / folded bias vectors of the LN-folded GEMMs
  std::vector<BlockW> blk;  // execution order: STE0, TTE0, STE1, ...
  const float *fus_w = nullptr, *fus_b = nullptr, *spos = nullptr, *tpos = nullptr;
  const float *sn_g = nullptr, *sn_b = nullptr, *tn_g = nullptr, *tn_b = nullptr;
  const float *hd_g = nullptr, *hd_b = nullptr, *hd_w = nullptr, *hd_bias = nullptr;
  const float *tm1_w = nullptr, *tm1_b = nullptr, *tm3_w = nullptr, *tm3_b = nullptr;
  const float *wm_w = nullptr, *wm_b = nullptr;
  DevBuf<float> tblk_w, tblk_b;  // concatenated per-block time projections (nblk*D, Dt), (nblk*D)
  DevBuf<float> freqs_dev;

  // schedule
  bool sched_set = false;
  int num_timesteps = 0, S = 0, clip = 0;
  float eta = 0.f;
  std::vector<float> ac, somac;
  std::vector<int32_t> times;  // S+1, reversed
  DevBuf<float> ac_dev, somac_dev, sqrt_ac_dev;
  DevBuf<float> temb_sched;  // (S, nblk, D)
  bool has_sqrt_ac = false;

  // hipGraph replay of the whole S-step loop (d3d_engine_set_graph_mode): one captured graph per (B, workspace)
  struct GraphEntry { int B; void* ws; hipGraph_t graph; hipGraphExec_t exec; unsigned long long used; };
  static constexpr size_t MAX_GRAPHS = 4;   // least recently used entry is destroyed beyond that (a caller that re-allocates its
                                            // workspace per batch would otherwise grow the cache without bound)
  bool graph_mode = false;
  std::vector<GraphEntry> graphs;
  unsigned long long graph_clock = 0, graphs_captured = 0;
  hipStream_t cap_stream = nullptr;
  void drop_graphs() {
    for (auto& g : graphs) { (void)hipGraphExecDestroy(g.exec); (void)hipGraphDestroy(g.graph); }
    graphs.clear();
  }

  // optional per-kernel-class timing with HIP events on the launch stream (bench.py's roofline leg)
  struct ProfRec { int cls, cls2; hipEvent_t a, b; double flops, bytes; };
  bool profiling = false;
  std::vector<ProfRec> recs;
  std::vector<hipEvent_t> ev_pool;
  double prof_ms[D3D_KC_COUNT] = {0}, prof_flops[D3D_KC_COUNT] = {0}, prof_bytes[D3D_KC_COUNT] = {0};
  int64_t prof_launches[D3D_KC_COUNT] = {0};

  // debug trace (d3d_engine_set_trace): one checksum per buffer a kernel of the F16X3 block flow has just written
  bool tracing = false;
  DevBuf<unsigned long long> trace_dev;
  int trace_cap = 0, trace_n = 0, trace_fwd = 0, trace_views = 1;
  std::vector<uint32_t> trace_tags;

  ~d3d_engine() {   // what is not device memory (the DevBuf members free that)
    drop_graphs();
    if (range_host) (void)hipHostFree(range_host);
    for (auto ev : range_ev) (void)hipEventDestroy(ev);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    if (side_stream) (void)hipStreamDestroy(side_stream);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    for (auto& r : recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto ev : ev_pool) (void)hipEventDestroy(ev);
  }
};

namespace {

// Launches issued while one of these is alive report to the engine's range-guard word and stage their small GEMMs as the engine's
// "deep_stages" says (d3d_kernels.h LaunchCtx: the calling thread's own context, so concurrent calls on distinct engines do not mix).
struct RangeScope {
  unsigned* saved;
  int saved_deep;
  explicit RangeScope(const d3d_engine* e) : saved(tl_launch_ctx.range_word), saved_deep(tl_launch_ctx.deep_stages) {
    tl_launch_ctx.range_word = e->range_dev;
    tl_launch_ctx.deep_stages = e->opt_deep_stages;
  }
  ~RangeScope() { tl_launch_ctx.range_word = saved; tl_launch_ctx.deep_stages = saved_deep; }
};

// registers the tensors of `list` (name suffix, element count) that exist in this model: a count of 0 = not a parameter of it
void add_slots(d3d_engine* e, const std::string& prefix, std::initializer_list<std::pair<const char*, int64_t>> list) {
  for (const auto& t : list) {
    if (!t.second) continue;
    WeightSlot s;
    s.name = prefix + t.first;
    s.numel = t.second;
    e->index[s.name] = (int)e->slots.size();
    e->slots.push_back(std::move(s));
  }
}

void add_block_slots(d3d_engine* e, const std::string& p) {
  const int64_t D = e->D, Dm = e->Dm, Dt = e->Dt;   // (time_mlp only with_time_emb: Dt != 0)
  add_slots(e, p, {{".norm1.weight", D}, {".norm1.bias", D}, {".attn.qkv.weight", 3 * D * D}, {".attn.qkv.bias", 3 * D},
                   {".attn.proj.weight", D * D}, {".attn.proj.bias", D}, {".norm2.weight", D}, {".norm2.bias", D},
                   {".time_mlp.1.weight", D * Dt}, {".time_mlp.1.bias", Dt ? D : 0}, {".mlp.fc1.weight", Dm * D}, {".mlp.fc1.bias", Dm},
                   {".mlp.fc2.weight", D * Dm}, {".mlp.fc2.bias", D}});
}

// Parameter inventory in the reference's registration order (S2S:160-220, S2F:216-218); mirrors diff3dhpe_amd/spec.py.
void build_slots(d3d_engine* e) {
  const int64_t D = e->D, Dt = e->Dt, T = e->T, J = e->J, s2f = e->cfg.seq2frame ? 1 : 0;
  add_slots(e, "", {{"time_mlp.1.weight", Dt * D}, {"time_mlp.1.bias", Dt}, {"time_mlp.3.weight", Dt * Dt}, {"time_mlp.3.bias", Dt},
                    {"fusion_layer.weight", D * e->cin}, {"fusion_layer.bias", D}, {"Spatial_pos_embed", J * D}});
  for (int i = 0; i < e->depth; ++i) add_block_slots(e, "STEblocks." + std::to_string(i));
  add_slots(e, "", {{"Spatial_norm.weight", D}, {"Spatial_norm.bias", D}, {"Temporal_pos_embed", T * D}});
  for (int i = 0; i < e->depth; ++i) add_block_slots(e, "TTEblocks." + std::to_string(i));
  add_slots(e, "", {{"Temporal_norm.weight", D}, {"Temporal_norm.bias", D}, {"head.0.weight", D}, {"head.0.bias", D}, {"head.1.weight", 3 * D},
                    {"head.1.bias", 3}, {"weighted_mean.weight", s2f * T}, {"weighted_mean.bias", s2f}});
}

const float* wptr(const d3d_engine* e, const std::string& name) {
  auto it = e->index.find(name);
  if (it == e->index.end()) return nullptr;
  return e->arena + e->slots[it->second].dev_off;
}

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// RAII bracket: records an event pair around one kernel launch when profiling is on (no-op otherwise).
struct Prof {
  d3d_engine* e; hipStream_t s; bool on; d3d_engine::ProfRec r{};
  Prof(d3d_engine* e_, int cls, double flops, double bytes, hipStream_t s_, int cls2 = -1) : e(e_), s(s_), on(e_->profiling) {
    if (!on) return;
    auto get = [&]() {
      hipEvent_t ev = nullptr;
      if (!e->ev_pool.empty()) { ev = e->ev_pool.back(); e->ev_pool.pop_back(); }
      else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr;
      return ev;
    };
    r.cls = cls; r.cls2 = cls2; r.flops = flops; r.bytes = bytes; r.a = get(); r.b = get();
    if (!r.a || !r.b) { on = false; return; }
    (void)hipEventRecord(r.a, s);
  }
  ~Prof() {
    if (!on) return;
    (void)hipEventRecord(r.b, s);
    e->recs.push_back(r);
  }
};

// debug trace: tag = view << 28 | forward << 16 | block << 8 | kernel << 4 | buffer
//   kernel: 0 embed, 1 stream entry, 2 qkv, 3 attention, 4 proj, 5 fc1, 6 fc2 (+ post-norm), 7 post-norm row kernel, 8 head
//   buffer: 0 = the kernel's main output (rows < M only), 1 = row-statistics partials
int trace(d3d_engine* e, int blk, int kernel, int buf, const void* p, size_t bytes, hipStream_t s) {
  if (!e->tracing) return D3D_OK;
  for (int v = 0; v < e->trace_views && e->trace_n < e->trace_cap; ++v) {
    HIP_TRY(launch_checksum(p, bytes, e->trace_dev + e->trace_n, v, s));
    e->trace_tags.push_back(((uint32_t)v << 28) | ((uint32_t)(e->trace_fwd & 0xFFF) << 16) | ((uint32_t)blk << 8) |
                            ((uint32_t)kernel << 4) | (uint32_t)buf);
    ++e->trace_n;
  }
  return D3D_OK;
}
#define TRACE(blk, kernel, buf, p, bytes)                                  \
  do {                                                                     \
    if (e->tracing) {                                                      \
      int _t = trace(e, (blk), (kernel), (buf), (p), (bytes), s);          \
      if (_t) return _t;                                                   \
    }                                                                      \
  } while (0)

// Workspace carve-up (float offsets).  AO (attention output) aliases HN: norm1(x) is dead once the qkv GEMM has run.
struct Workspace {
  float *X, *HN, *QKV, *HID, *Y0, *Y1, *TEMB, *TSCR, *RED, *TIMES, *XIN, *NIN, *OUTB, *ST1, *ST2, *QT;
  size_t total_bytes;
};

Workspace carve(const d3d_engine* e, int B, void* base) {
  const size_t M = (size_t)B * e->T * e->J;
  const size_t D = e->D;
  size_t off = 0;
  auto take = [&](size_t nfloats) {
    size_t o = off;
    off += align_up(nfloats, 64);
    return o;
  };
  float* b = reinterpret_cast<float*>(base);
  Workspace w{};
  // F16X3 operand planes are read in whole 256-row tiles; the fused spatial kernel's tiles start every 255 rows (15 frames) and
  // stage 256, so the last one may reach 255 * ceil(frames / 15) + 1 rows.  Sized that way whatever J is: the 16-frame tiles of 15 and
  // 16 joints need 240 * ceil(frames / 16) + 16 rows (never more than the above: 15 c >= 15 for every tile count c >= 1) and
  // 256 * ceil(frames / 16) = M rounded up to 256 (what Mp is rounded to anyway), so d3d_workspace_bytes does not depend on the form
  const size_t fr = M / (size_t)e->J, qs_rows = 255 * ((fr + 14) / 15) + 1;
  const size_t Mp = (std::max(std::max(M, qs_rows), (M + 191) / 192 * 192) + 255) / 256 * 256;   // (and whole 192-row tiles)
  size_t oX = take(Mp * D), oHN = take(Mp * D), oQKV = take(M * 3 * D), oHID = take(Mp * e->Dm);
  size_t oY0 = take(M * 3), oY1 = take(M * 3);
  size_t oTE = take((size_t)B * e->nblk * D), oTS = take((size_t)B * (D + 2 * (size_t)e->Dt));
  size_t oRED = take((size_t)B * e->J * D), oTI = take((size_t)B + 64);
  size_t oXI = take(M * e->cfg.in_chans), oNI = take(M * 3), oOB = take(M * 3);   // graph-mode staging copies
  // row statistics of the LN-folded GEMMs; whole 256-row tiles, the persistent walk stages a tile's block of them by LDS-DMA
  size_t oS1 = take(Mp * 2 * (size_t)((D + 63) / 64)), oS2 = take(Mp * 2 * (size_t)((D + 63) / 64));
  // "block0_direct": the time rows Q[b] = Wg tv[b] of this forward, (B, 3 D) -- in the caller's workspace, so the two half-batches of a
  // two-stream sampling and concurrent engines never share them
  size_t oQT = take((size_t)B * 3 * D);
  if (b) {   // (d3d_workspace_bytes asks for the size alone: no arithmetic on a null base -- UBSan, experiments/asan_host.sh)
    w.X = b + oX; w.HN = b + oHN; w.QKV = b + oQKV; w.HID = b + oHID; w.Y0 = b + oY0; w.Y1 = b + oY1;
    w.TEMB = b + oTE; w.TSCR = b + oTS; w.RED = b + oRED; w.TIMES = b + oTI;
    w.XIN = b + oXI; w.NIN = b + oNI; w.OUTB = b + oOB; w.ST1 = b + oS1; w.ST2 = b + oS2; w.QT = b + oQT;
  }
  w.total_bytes = off * sizeof(float);
  return w;
}

// time-embedding table for n timesteps: out (n, nblk, D).  scratch: n*(D + 2*Dt) floats.
int compute_temb(d3d_engine* e, const float* times_dev, int n, float* out, float* scratch, hipStream_t s) {
  float* sin_buf = scratch;
  float* h1 = sin_buf + (size_t)n * e->D;
  float* h2 = h1 + (size_t)n * e->Dt;
  HIP_TRY(launch_sinusoid(times_dev, e->freqs_dev, sin_buf, n, e->D, s));
  HIP_TRY(launch_small_linear(sin_buf, e->tm1_w, e->tm1_b, h1, n, e->Dt, e->D, /*gelu out*/ 1, s));
  HIP_TRY(launch_small_linear(h1, e->tm3_w, e->tm3_b, h2, n, e->Dt, e->Dt, 0, s));
  HIP_TRY(launch_small_linear(h2, e->tblk_w, e->tblk_b, out, n, e->nblk * e->D, e->Dt, /*silu in*/ 2, s));
  return D3D_OK;
}

// The attention launch of a spatial or a temporal block of B sequences.  qkv: the block's q / k / v, (M, 3 D) fp32 rows for the fp32
// kernels; for the planes kernels the fp16 hi plane at the same address and the lo plane M 3 D halves behind it.  out / out_x3: AttnArgs.
int launch_attention(const d3d_engine* e, AttnPick kernel, bool temporal, const void* qkv, float* out, void* out_x3, int B, hipStream_t s) {
  const void* lo = kernel.fam().form == ATTN_PLANES ? static_cast<const uint16_t*>(qkv) + (size_t)B * e->T * e->J * 3 * e->D : nullptr;
  HIP_TRY(kernel.regime(temporal).launch(AttnArgs{qkv, lo, out, out_x3, B, e->T, e->J, e->D, e->H, temporal, s}));
  return D3D_OK;
}

// The plan of a forward of B sequences.  A pure function of the options, the shapes, B and the CU count, so an eager run, a capture
// and a replay agree.
BlockPlan plan_blocks(const d3d_engine* e, int B) {
  const int T = e->T, J = e->J, D = e->D, Dm = e->Dm, H = e->H, M = B * T * J, cus = device_cu_count();
  BlockPlan p;
  p.attn = attn_choose(e->cfg.precision, e->attn_opts, e->opt_fold_layernorm, T, J, D, H);
  if (p.attn.flow == ATTN_FLOW_FOLD) {
    // (heads of 32 columns: no D == 64 H predicate holds there, so the fused kernels, block 0 direct and the post-norm in fc2 stay off by
    // their own predicates; qkv_tattn_ok refuses T > 255: a streaming kernel is always the two-kernel branch)
    p.fused_sp = e->opt_fused_spatial && qkv_sattn_ok(J, D, H, D) && e->blk[0].qkv_f3h != nullptr;
    p.fused_tp = e->opt_fused_temporal && qkv_tattn_ok(T, J, D, H, D) && e->blk[1].qkv_f3h != nullptr;
    // block 0 from the raw channels: every forward of this flow whose block 0 has the tables (fused or not, any B, any time rows)
    p.b0_direct = e->opt_block0_direct && e->b0_G != nullptr && e->blk[0].qkv_csh != nullptr && embed_planes_ok(D, e->cfg.in_chans) &&
                  qkv_sattn_direct_ok(J, D, H, e->cfg.in_chans);
    // the dedicated fc1 kernel runs whole 256-row tiles without guards (a launch of at least two rounds of tiles; smaller ones keep the
    // template's 256 x 128 / sliced forms); the proj kernel whole 192-row tiles (the rows behind the last whole tile stay with the template)
    p.fc1_own = e->opt_fc1_kernel && fc1_x3_ok(Dm, D) && (size_t)((M + 255) / 256) * (size_t)(Dm / 256) >= 512;
    p.proj_own = e->opt_proj_kernel && proj_x3_ok(D, D) && (size_t)(M / 192) * (size_t)(D / 256) >= 512;
    // post-norm inside the fc2 epilogue (X3PostNorm) where the tile shape for it exists; else fp32 + the row kernel
    p.pn = e->opt_fused_postnorm && x3q_postnorm_ok(D, Dm);
    if (e->opt_latency_mode) {
      // fc2 + post-norm as a split-K GEMM + the ordered reduce / post-norm row kernel: d3d_kernels.h fc2_splitk_choose
      if (p.pn) p.fc2_split = fc2_splitk_choose(M, D, Dm, cus);
      // proj and fc1: the forced S of "proj_split" / "fc1_split" where the call fits the kernel pair, else the rule
      if (D == 512) {
        const int ps = e->opt_proj_split, fs = e->opt_fc1_split;
        p.proj_split = ps < 0 ? proj_splitk_choose(M, D, D, cus) : (ps && proj_splitk_ok(D, D, ps) && proj_splitk_fits(M, D, ps, cus) ? ps : 0);
        p.fc1_split = fs < 0 ? fc1_splitk_choose(M, Dm, D, cus) : (fs && fc1_splitk_ok(Dm, D, fs) && fc1_splitk_fits(M, Dm, fs, cus) ? fs : 0);
      }
      if (e->opt_small_tiles) {
        // the 128-row tiles where the present fused launch runs fewer workgroups than the device has CUs AND the small-tile launch at most
        // 5/8 of them.  One 137 KiB workgroup holds a CU, so a launch of more workgroups than CUs runs a second round and loses what the
        // shorter k-loop gained; the 5/8 is the table's: launches of up to 136 workgroups on 256 CUs lead in every
        // alternation, the next shape class (192: a half-batch of two T = 81 sequences, its twin running beside it on the second stream)
        // does not.  Present launches: spatial, ceil(frames / 15) tiles (16 at 15 / 16 joints) x 8 heads; temporal (grouped form,
        // T <= 127), B ceil(J / min(255 / T, J)) x 8
        const int fpt = J == 17 ? 15 : 16;
        const long long wg_sp = (long long)((B * T + fpt - 1) / fpt) * 8;
        const int gj = T <= 127 ? (255 / T < J ? 255 / T : J) : 1;
        const long long wg_tp = (long long)B * ((J + gj - 1) / gj) * 8;
        auto fits = [&](long long groups, int N) { return 8 * qkv_attn_x3_small_workgroups(groups, N) <= 5LL * cus; };
        p.small_sp = p.fused_sp && qkv_attn_x3_small_ok(J, 1, J, D, H, D) && wg_sp < cus && fits((long long)B * T, J);
        p.small_tp = p.fused_tp && qkv_attn_x3_small_ok(T, J, J, D, H, D) && wg_tp < cus && fits((long long)B * J, T);
      }
    }
    if (e->opt_fused_narrow && (long long)M * 4 * D < (1LL << 32)) {   // (the kernel's 32-bit row offsets)
      // wherever the two-kernel branch would run the resident kernel of width 32 / 16 and the commit made the tile-order images
      const auto narrow = [](AttnPick a) { return a.fam().narrow && !a.stream; };
      p.narrow_sp = narrow(p.attn.sp) && qkv_attn_x3_narrow_ok(J, 1, J, D, H, D) && e->blk[0].qkv_f3h != nullptr;
      p.narrow_tp = narrow(p.attn.tp) && qkv_attn_x3_narrow_ok(T, J, J, D, H, D) && e->blk[1].qkv_f3h != nullptr;
    }
  } else if (p.attn.flow == ATTN_FLOW_BF16) {
    p.fused_sp = e->opt_fused_spatial && qkv_sattn_bf16_ok(T, J, D, H, B);
    p.fused_tp = e->opt_fused_temporal && qkv_tattn_bf16_ok(T, J, D, H, B);
    p.rows = e->opt_fused_postnorm && bf16_rows_ok(D, D) && bf16_rows_ok(D, Dm);
    auto own = [&](int N) {   // from two rounds of 256 x 256 tiles on
      return e->opt_bf16_gemm_kernel && gemm_bf16q_ok(N, D) && (long long)((M + 255) / 256) * (N / 256) >= 2LL * cus;
    };
    p.bf16q_qkv = own(3 * D);
    p.bf16q_fc1 = own(Dm);
  }   // (the row-kernel flow: nothing beyond its two attention kernels)
  return p;
}

// The post-norm of block k (S2S:111-135): Spatial_norm / Temporal_norm by parity; Temporal_pos_embed behind block 0 only (row r takes
// entry (r / J) % T); the NEXT block's time vector unless k is the last block.
X3PostNorm block_postnorm(const d3d_engine* e, int k, const float* tvec, int64_t tvec_stride) {
  const bool temporal = (k & 1) != 0;
  X3PostNorm q{};
  q.g = temporal ? e->tn_g : e->sn_g; q.b = temporal ? e->tn_b : e->sn_b; q.eps = e->ln_eps;
  q.pos_div = 1; q.pos_mod = 1; q.rows_per_batch = e->T * e->J;
  if (k == 0) { q.pos = e->tpos; q.pos_div = e->J; q.pos_mod = e->T; }
  if (k + 1 < e->nblk && tvec) { q.tvec = tvec + (size_t)(k + 1) * e->D; q.tvec_stride = tvec_stride; }
  return q;
}
// the same as the arguments of the row kernel, over M rows
LnArgs ln_postnorm(const d3d_engine* e, int M, const X3PostNorm& q) {
  LnArgs a = ln_rows(M, e->D, q.rows_per_batch);
  a.g1 = q.g; a.b1 = q.b; a.eps1 = q.eps;
  a.pos = q.pos; a.pos_div = q.pos_div; a.pos_mod = q.pos_mod;
  a.tvec = q.tvec; a.tvec_stride = q.tvec_stride;
  return a;
}

// the scratch slot a forward with fc1 split needs, allocated outside any capture (the eager pass of a graph call comes first)
int ensure_lat_scratch(d3d_engine* e, int slot) {
  if (!e->lat_scratch[slot]) HIP_TRY(e->lat_scratch[slot].alloc(FC1_SPLITK_SCRATCH_FLOATS));
  return D3D_OK;
}

// F16X3 production flow ("plane-resident, LayerNorm-folded"): the residual stream lives in the GEMM operand (pair) layout
// in w.X, so it is at once the A operand of the qkv / fc1 GEMMs and the residual input of the proj / fc2 epilogues; norm1
// and norm2 are folded into those two GEMMs (X3Fold), their row statistics coming from the producer of the stream (the
// fc2 epilogue, resp. the proj epilogue).  The block's post-norm runs inside the fc2 epilogue (X3PostNorm: whole-row tiles,
// D == 512); for other widths the fc2 output goes to w.HN as fp32 and one stand-alone row kernel per block applies it.
// The hidden activation (w.HID) is in "accumulator order" (pair_col_acc), matched by the fc2 weight split at commit.
// Same op sequence as run_blocks (S2S:222-247, 111-135); leaves the final Temporal_norm output as fp32 in w.X.
int run_blocks_fold(d3d_engine* e, const BlockPlan& pl, const float* x2d, const float* y, int y_bcast, const float* tvec,
                    int64_t tvec_stride, int B, const Workspace& w, hipStream_t s) {
  const int T = e->T, J = e->J, D = e->D;
  const int M = B * T * J;
  const double MD4 = (double)M * D * 4.0;
  uint16_t* XP = reinterpret_cast<uint16_t*>(w.X);      // residual stream, pair layout of 8x
  uint16_t* AOx = reinterpret_cast<uint16_t*>(w.HN);    // attention output (pair layout); w.HN as fp32 = embed / fc2 output
  uint16_t* HIDx = reinterpret_cast<uint16_t*>(w.HID);
  uint16_t* QKVh = reinterpret_cast<uint16_t*>(w.QKV);
  uint16_t* QKVl = QKVh + (size_t)M * 3 * D;
  const size_t MDb = (size_t)M * D * 4;                 // bytes of an (M, D) fp32 tensor = of its pair-layout planes
  auto rowk = [&](LnArgs a, int outs) -> hipError_t {
    Prof p(e, D3D_KC_LAYERNORM, 8.0 * M * D, MD4 * (1 + outs), s);
    return launch_layernorm(a, s);
  };
  if (embed_planes_ok(D, e->cfg.in_chans)) {   // embedding straight into the stream planes + row statistics (one pass over HBM)
    Prof p(e, D3D_KC_EMBED, 2.0 * M * D * e->cin, MD4 + (double)M * e->cin * 4.0, s);
    HIP_TRY(launch_embed_planes(x2d, y, e->fus_w, e->fus_b, e->spos, tvec, tvec_stride, XP, w.ST1, B, T, J, D, e->cfg.in_chans, y_bcast, s));
  } else {
    {
      Prof p(e, D3D_KC_EMBED, 2.0 * M * D * e->cin, MD4 + (double)M * e->cin * 4.0, s);
      HIP_TRY(launch_embed(x2d, y, e->fus_w, e->fus_b, e->spos, tvec, tvec_stride, w.HN, B, T, J, D, e->cfg.in_chans, y_bcast, s));
    }
    TRACE(0, 0, 0, w.HN, MDb);
    {  // stream entry: planes + row statistics of x (no normalisation)
      LnArgs a = ln_rows(M, D, T * J);
      a.x = w.HN; a.skip_ln1 = 1; a.y_x3 = XP; a.stats = w.ST1;
      HIP_TRY(rowk(a, 1));
    }
  }
  TRACE(0, 1, 0, XP, MDb);
  TRACE(0, 1, 1, w.ST1, (size_t)M * 8);
  if (pl.fused_sp || pl.fc1_own) {   // the fused spatial kernel / the fc1 kernel stage (and multiply) rows beyond the matrix: finite values there
    const size_t Mp = (size_t)((reinterpret_cast<char*>(w.HN) - reinterpret_cast<char*>(w.X)) / ((size_t)D * 4));   // rows of w.X as carved
    if (Mp > (size_t)M) HIP_TRY(hipMemsetAsync(XP + (size_t)M * 2 * D, 0, (Mp - (size_t)M) * 2 * D * sizeof(uint16_t), s));
  }
  // block 0 direct: the time rows Q[b] = Wg tv[b] (block 0's slice of the time vector), one row when every batch element shares t
  const float* b0_Q = nullptr;
  const int b0_qstride = tvec_stride ? 3 * D : 0;
  if (pl.b0_direct && tvec) {
    HIP_TRY(launch_small_linear(tvec, e->b0_wg, nullptr, w.QT, tvec_stride ? B : 1, 3 * D, D, 0, s, tvec_stride));
    b0_Q = w.QT;
  }
  auto qkv_direct = [&](void* out_x3, void* ph, void* plo) -> hipError_t {
    const BlockW& b0 = e->blk[0];
    return launch_qkv_sattn_direct(x2d, y, y_bcast, e->cfg.in_chans, e->b0_G, e->b0_P, b0_Q, b0_qstride, b0.qkv_fbh, b0.qkv_csh, w.ST1, 1, e->ln_eps,
                                   out_x3, ph, plo, M, T, J, D, e->H, s);
  };
  // its work: the CIN-deep fill (+ 2 adds) per q / k / v value; M input rows, the tables and the statistics in
  const double b0_flops = 2.0 * M * 3.0 * D * (e->cin + 1), b0_in = (double)M * (e->cin + 2) * 4.0 + 4.0 * 3.0 * D * (e->cin + J + 1);
  const int np2 = x3q_ntiles(M, D);                     // statistics partials per row written by a GEMM epilogue
  int np1 = 1;                                          // ... per row in w.ST1 (1 after a row kernel)
  // latency mode: S k-ranges of fc2 as fp32 partials + the ordered reduce / post-norm row kernel.  The partials take w.HN (the attention
  // output, dead since proj) and on into w.QKV (q / k / v planes, dead since attention): (Mp + 3 M) D floats >= 4 M D, contiguous.
  const int ksplit = pl.fc2_split;
  float* const PART = w.HN;
  // ... and proj / fc1 (kernels_splitk_reduce.hip).  proj's partials take w.QKV (dead since attention) and on into w.HID (dead until
  // fc1): 3 M D + Mp Dm floats >= 4 M D, contiguous -- not w.HN, which holds proj's own A operand.  fc1's take the engine's scratch
  // buffer, the second half-batch of a two-stream sampling its own slot.
  const int psplit = pl.proj_split, fsplit = pl.fc1_split;
  float* const PPART = w.QKV;
  const int fslot = (e->side_stream && s == e->side_stream) ? 1 : 0;
  if (fsplit) {
    const int rc = ensure_lat_scratch(e, fslot);
    if (rc) return rc;
  }
  float* const FPART = e->lat_scratch[fslot];
  for (int k = 0; k < e->nblk; ++k) {
    const BlockW& bw = e->blk[k];
    const bool temporal = (k & 1) != 0;
    auto gemm = [&](const uint16_t* A, const uint16_t* W, int wexp, const float* bias, float* C, uint16_t* Ch, uint16_t* Cl, int outsplit,
                    int N, int K, int epi, int qcols, const X3Fold& f) -> hipError_t {
      const int sub = f.st_in ? (epi == EPI_GELU ? D3D_KC_LINEAR_FC1 : D3D_KC_LINEAR_QKV) : (K == D ? D3D_KC_LINEAR_PROJ : D3D_KC_LINEAR_FC2);
      Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N * (f.Rp ? 2 : 1)), s, sub);
      return launch_linear_x3p(A, W, bias, nullptr, C, Ch, Cl, M, N, K, epi, outsplit, qcols, 0, s, &f, wexp);
    };
    if (temporal ? pl.small_tp : (pl.small_sp && !(k == 0 && pl.b0_direct))) {
      // latency mode, small tiles: the same fused step on 128-row tiles of whole groups (kernels_qkv_attn_x3_small.hip)
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_QKV_TATTN : D3D_KC_QKV_SATTN, 2.0 * M * 3.0 * D * D + 4.0 * M * (double)N * D, 2.0 * MD4 + 4.0 * 3.0 * D * D, s);
      HIP_TRY(launch_qkv_attn_x3_small(XP, bw.qkv_f3h, bw.qkv_fbh, bw.qkv_csh, w.ST1, np1, e->ln_eps, bw.qkv_fe, AOx, temporal ? B * J : B * T, N,
                                       temporal ? J : 1, J, D, D, e->H, s));
      TRACE(k, 3, 0, AOx, MDb);
    } else if (temporal ? pl.narrow_tp : pl.narrow_sp) {
      // "fused_narrow", head widths 32 / 16: the same fused step, a pair / a quad of heads per 64-column segment; block 0 included
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_QKV_TATTN : D3D_KC_QKV_SATTN, 2.0 * M * 3.0 * D * D + 4.0 * M * (double)N * D, 2.0 * MD4 + 4.0 * 3.0 * D * D, s);
      HIP_TRY(launch_qkv_attn_x3_narrow(XP, bw.qkv_f3h, bw.qkv_fbh, bw.qkv_csh, w.ST1, np1, e->ln_eps, bw.qkv_fe, AOx, temporal ? B * J : B * T, N,
                                        temporal ? J : 1, J, D, D, e->H, s));
      TRACE(k, 3, 0, AOx, MDb);
    } else if (temporal && pl.fused_tp) {
      // temporal block: q, k, v of one (batch, joint) group stay in LDS and feed the T-key attention in the same kernel (kernels_qkv_tattn.hip)
      Prof p(e, D3D_KC_QKV_TATTN, 2.0 * M * 3.0 * D * D + 4.0 * M * (double)T * D, 2.0 * MD4 + 4.0 * 3.0 * D * D, s);
      HIP_TRY(launch_qkv_tattn(XP, bw.qkv_f3h, bw.qkv_fbh, bw.qkv_csh, w.ST1, np1, e->ln_eps, bw.qkv_fe, AOx, B, T, J, D, D, e->H, s));
      TRACE(k, 3, 0, AOx, MDb);
    } else if (k == 0 && pl.b0_direct && pl.fused_sp) {
      // block 0: the same kernel with the fill from the raw channels in place of the k-loop
      Prof p(e, D3D_KC_QKV_SATTN, b0_flops + 4.0 * M * (double)J * D, b0_in + MD4, s);
      HIP_TRY(qkv_direct(AOx, nullptr, nullptr));
      TRACE(k, 3, 0, AOx, MDb);
    } else if (!temporal && pl.fused_sp) {
      // spatial block: q, k, v of a frame group stay in LDS and feed the J-key attention in the same kernel (kernels_qkv_sattn.hip)
      Prof p(e, D3D_KC_QKV_SATTN, 2.0 * M * 3.0 * D * D + 4.0 * M * (double)J * D, 2.0 * MD4 + 4.0 * 3.0 * D * D, s);
      HIP_TRY(launch_qkv_sattn(XP, bw.qkv_f3h, bw.qkv_fbh, bw.qkv_csh, w.ST1, np1, e->ln_eps, bw.qkv_fe, AOx, M, D, J, D, e->H, s));
      TRACE(k, 3, 0, AOx, MDb);
    } else {
    if (k == 0 && pl.b0_direct) {   // block 0: the planes from the raw channels, the values the fused form keeps in LDS
      Prof p(e, D3D_KC_LINEAR, b0_flops, b0_in + 3.0 * MD4, s, D3D_KC_LINEAR_QKV);
      HIP_TRY(qkv_direct(nullptr, QKVh, QKVl));
    } else {  // q, k, v planes = norm1(x) Wqkv^T + b   (LayerNorm folded; q third pre-scaled by dh^-0.5)
      X3Fold f{};
      f.st_in = w.ST1; f.st_np = np1; f.csum = bw.qkv_cs; f.eps = e->ln_eps;
      HIP_TRY(gemm(XP, bw.qkv_f3, bw.qkv_fe, bw.qkv_fb, nullptr, QKVh, QKVl, 1, 3 * D, D, EPI_NONE, D, f));
    }
    TRACE(k, 2, 0, QKVh, 3 * MDb);
    {
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_ATTN_TEMPORAL : D3D_KC_ATTN_SPATIAL, 4.0 * M * (double)N * D, 4.0 * MD4, s);
      const int rc = launch_attention(e, temporal ? pl.attn.tp : pl.attn.sp, temporal, QKVh, nullptr, AOx, B, s);
      if (rc) return rc;
    }
    TRACE(k, 3, 0, AOx, MDb);
    }
    {  // x += attn Wproj^T + b, plane to plane in place; row statistics of the new x for the folded norm2
      X3Fold f{};
      f.Rp = XP; f.st_out = w.ST2;
      const int Mw = (M / 192) * 192;     // rows in whole 192-row tiles
      if (psplit) {
        {
          Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)D * D, 4.0 * ((double)M * D + (double)D * D + (double)psplit * M * D), s, D3D_KC_LINEAR_PROJ);
          HIP_TRY(launch_linear_x3p_splitk(AOx, bw.proj_x3, PPART, M, D, D, psplit, s, bw.proj_e));
        }
        TRACE(k, 4, 2, PPART, (size_t)psplit * MDb);
        Prof p(e, D3D_KC_LAYERNORM, 2.0 * M * D * (1 + psplit), MD4 * (2 + psplit), s);
        HIP_TRY(launch_splitk_residual(PPART, psplit, XP, bw.projb, XP, w.ST2, M, D, s));
      } else if (pl.proj_own) {
        Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)D * D, 4.0 * ((double)M * D + (double)D * D + 2.0 * M * D), s, D3D_KC_LINEAR_PROJ);
        HIP_TRY(launch_proj_x3(AOx, bw.proj_x3, bw.projb, XP, w.ST2, bw.proj_e, Mw, D, D, s));
        if (M > Mw) {   // the ragged rest: the template's checked forms, on the sub-matrix behind the whole tiles
          X3Fold fr{};
          fr.Rp = XP + (size_t)Mw * 2 * D; fr.st_out = w.ST2 + (size_t)Mw * np2 * 2;
          HIP_TRY(launch_linear_x3p(AOx + (size_t)Mw * 2 * D, bw.proj_x3, bw.projb, nullptr, nullptr, XP + (size_t)Mw * 2 * D, nullptr, M - Mw, D, D,
                                    EPI_RESIDUAL, 2, 0, 0, s, &fr, bw.proj_e));
        }
      } else {
        HIP_TRY(gemm(AOx, bw.proj_x3, bw.proj_e, bw.projb, nullptr, XP, nullptr, 2, D, D, EPI_RESIDUAL, 0, f));
      }
    }
    TRACE(k, 4, 0, XP, MDb);
    TRACE(k, 4, 1, w.ST2, (size_t)M * 8 * np2);
    {  // hidden = gelu(norm2(x) W1^T + b1), LayerNorm folded
      X3Fold f{};
      f.st_in = w.ST2; f.st_np = np2; f.csum = bw.fc1_cs; f.eps = e->ln_eps;
      if (fsplit) {
        {
          Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)e->Dm * D, 4.0 * ((double)M * D + (double)e->Dm * D + (double)fsplit * M * e->Dm), s, D3D_KC_LINEAR_FC1);
          HIP_TRY(launch_linear_x3p_splitk(XP, bw.fc1_f3, FPART, M, e->Dm, D, fsplit, s, bw.fc1_fe));
        }
        TRACE(k, 5, 2, FPART, (size_t)fsplit * M * e->Dm * 4);
        Prof p(e, D3D_KC_LAYERNORM, 12.0 * M * e->Dm, 4.0 * (double)M * e->Dm * (1 + fsplit), s);
        HIP_TRY(launch_splitk_gelu(FPART, fsplit, w.ST2, np2, bw.fc1_cs, bw.fc1_fb, e->ln_eps, HIDx, M, e->Dm, D, s));
      } else if (pl.fc1_own) {
        Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)e->Dm * D, 4.0 * ((double)M * D + (double)e->Dm * D + (double)M * e->Dm), s, D3D_KC_LINEAR_FC1);
        HIP_TRY(launch_fc1_x3(XP, bw.fc1_f3, bw.fc1_fb, bw.fc1_cs, w.ST2, np2, e->ln_eps, bw.fc1_fe, HIDx, M, e->Dm, D, s));
      } else {
        HIP_TRY(gemm(XP, bw.fc1_f3, bw.fc1_fe, bw.fc1_fb, nullptr, HIDx, nullptr, 2, e->Dm, D, EPI_GELU, 0, f));
      }
    }
    TRACE(k, 5, 0, HIDx, (size_t)M * e->Dm * 4);
    // x = post_norm(x + hidden W2^T + b2) [+ Temporal_pos_embed before TTE0] [+ next block's time vector]
    const X3PostNorm q = block_postnorm(e, k, tvec, tvec_stride);
    const bool last = k + 1 == e->nblk;
    if (ksplit) {
      {
        Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)D * e->Dm, 4.0 * ((double)M * e->Dm + (double)D * e->Dm + (double)ksplit * M * D), s,
               D3D_KC_LINEAR_FC2);
        HIP_TRY(launch_linear_x3p_splitk(HIDx, bw.fc2_x3, PART, M, D, e->Dm, ksplit, s, bw.fc2_e));
      }
      TRACE(k, 6, 0, PART, (size_t)ksplit * MDb);
      {
        Prof p(e, D3D_KC_LAYERNORM, 8.0 * M * D, MD4 * (2 + ksplit), s);
        HIP_TRY(launch_splitk_postnorm(PART, ksplit, XP, bw.fc2b, q, last ? w.X : nullptr, last ? nullptr : XP, last ? nullptr : w.ST1, M, D, s));
      }
      np1 = 1;
      TRACE(k, 7, 0, w.X, MDb);
      if (!last) TRACE(k, 7, 1, w.ST1, (size_t)M * 8);
      continue;
    }
    if (pl.pn) {  // all in the fc2 epilogue
      X3Fold f{};
      f.Rp = XP;
      f.pn = q;
      auto fc2 = [&](float* C, uint16_t* Ch, int outsplit) -> hipError_t {
        return gemm(HIDx, bw.fc2_x3, bw.fc2_e, bw.fc2b, C, Ch, nullptr, outsplit, D, e->Dm, EPI_RESIDUAL, 0, f);
      };
      if (!last) {
        f.st_out = w.ST1;
        HIP_TRY(fc2(nullptr, XP, 2));
        np1 = np2;
        TRACE(k, 6, 1, w.ST1, (size_t)M * 8 * np2);
      } else {
        HIP_TRY(fc2(w.X, nullptr, 0));
      }
      TRACE(k, 6, 0, w.X, MDb);
      continue;
    }
    {  // x + hidden W2^T + b2 -> fp32 (w.HN) for the post-norm
      X3Fold f{};
      f.Rp = XP;
      HIP_TRY(gemm(HIDx, bw.fc2_x3, bw.fc2_e, bw.fc2b, w.HN, nullptr, nullptr, 0, D, e->Dm, EPI_RESIDUAL, 0, f));
    }
    TRACE(k, 6, 0, w.HN, MDb);
    {  // the post-norm as a row kernel -> planes + statistics (or fp32 at the end)
      LnArgs a = ln_postnorm(e, M, q);
      a.x = w.HN;
      if (!last) { a.y_x3 = XP; a.stats = w.ST1; }
      else a.y = w.X;
      HIP_TRY(rowk(a, 1));
    }
    TRACE(k, 7, 0, w.X, MDb);
    if (!last) TRACE(k, 7, 1, w.ST1, (size_t)M * 8);
  }
  return D3D_OK;
}

// bf16 operand mode (D3D_PREC_BF16; SURVEY section 7 step 5, BASELINE configs[1]): the block GEMMs and both attention products take
// bf16 operands (one MFMA per product); the residual stream, LayerNorm / softmax statistics, GELU, time vectors, embedding and
// head stay fp32.  Operand roundings sit exactly where the oracle's bf16-operand emulation puts them: LN output -> bf16 (row
// kernel), q / k / v -> bf16 (qkv epilogue), softmax - I -> bf16 (attention kernel), attention output -> bf16, GELU output ->
// bf16 (fc1 epilogue), weights -> bf16 (commit).  Same op sequence as run_blocks (S2S:222-247, 111-135); leaves the final
// Temporal_norm output as fp32 in w.X.  Measured first with three LayerNorm row kernels per block, then
// given the whole-row proj / fc2 forms below; the row-kernel flow stays behind "fused_postnorm" = 0.
// fp16 operand mode (D3D_PREC_F16): this flow with every launch in its fp16-operand form -- the same rounding points, each now a round to
// nearest even to fp16 (subnormals kept, +-inf beyond 65504: the mode is unscaled and has no range guard), the f16 twin of each bf16
// MFMA.  Plan bits, option and info keys are shared; "bf16" in a name below reads "16-bit operand".
int run_blocks_bf16(d3d_engine* e, const BlockPlan& pl, const float* x2d, const float* y, int y_bcast, const float* tvec,
                    int64_t tvec_stride, int B, const Workspace& w, hipStream_t s) {
  const int T = e->T, J = e->J, D = e->D;
  const int M = B * T * J;
  const double MD4 = (double)M * D * 4.0, MD2 = (double)M * D * 2.0;
  const bool f16 = e->cfg.precision == D3D_PREC_F16;
  uint16_t* HNb = reinterpret_cast<uint16_t*>(w.HN);     // bf16 [Mp][D]: LayerNorm output, then the attention output
  uint16_t* QKVb = reinterpret_cast<uint16_t*>(w.QKV);   // bf16 [M][3D]; in a fused block (below) bf16 [M][D]: the attention output
  uint16_t* HIDb = reinterpret_cast<uint16_t*>(w.HID);   // bf16 [Mp][Dm]
  {
    Prof p(e, D3D_KC_EMBED, 2.0 * M * D * e->cin, MD4 + (double)M * e->cin * 4.0, s);
    HIP_TRY(launch_embed(x2d, y, e->fus_w, e->fus_b, e->spos, tvec, tvec_stride, w.X, B, T, J, D, e->cfg.in_chans, y_bcast, s));
  }
  auto linear = [&](const uint16_t* A, const uint16_t* W, const float* bias, const float* R, float* C, uint16_t* Cb, int N, int K, int epi,
                    int qcols, int sub) -> hipError_t {
    Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)N * K, 2.0 * ((double)M * K + (double)N * K) + (double)M * N * (R ? 8.0 : 2.0), s, sub);
    if (sub == D3D_KC_LINEAR_QKV ? pl.bf16q_qkv : sub == D3D_KC_LINEAR_FC1 && pl.bf16q_fc1)
      return launch_gemm_bf16q(A, W, bias, Cb, M, N, K, epi, qcols, s, f16);
    return launch_linear_bf16(A, W, bias, R, C, Cb, M, N, K, epi, qcols, s, f16);
  };
  auto lnorm = [&](LnArgs a) -> hipError_t {
    Prof p(e, D3D_KC_LAYERNORM, 8.0 * M * D, MD4 * (1 + (a.y ? 1 : 0)) + MD2, s);
    a.h_f16 = f16 ? 1 : 0;
    return launch_layernorm(a, s);
  };
  {  // h = bf16(norm1_0(x))
    LnArgs a = ln_rows(M, D, T * J);
    a.x = w.X; a.h_bf16 = HNb; a.g1 = e->blk[0].n1g; a.b1 = e->blk[0].n1b; a.eps1 = e->ln_eps;
    HIP_TRY(lnorm(a));
  }
  // Whole-row tiles for proj and fc2 (launch_linear_bf16_rows; "fused_postnorm" option, D == 512): the LayerNorm behind each of
  // them -- norm2, resp. post-norm + next norm1 -- runs in the GEMM epilogue and the three row kernels per block are gone
  // (measured first un-fused, as planned: 59 of 323 ms per sampling were LayerNorm kernels at 5 TB/s).
  auto linear_rows = [&](const uint16_t* A, const uint16_t* W, const float* bias, uint16_t* Hb, int K, const X3PostNorm& pn, int sub) -> hipError_t {
    Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)D * K, 2.0 * ((double)M * K + (double)D * K) + (double)M * D * (Hb ? 10.0 : 8.0), s, sub);
    return launch_linear_bf16_rows(A, W, bias, w.X, Hb, M, D, K, pn, s, f16);
  };
  // qkv GEMM + attention of a block in ONE kernel (kernels_qkv_attn_bf16.hip; "fused_spatial" / "fused_temporal"): q / k / v never reach
  // HBM.  Every head's tile reads whole rows of HNb, so the attention output cannot go there: it takes w.QKV, dead in such a block.
  // Bit-identical to the two launches it replaces.
  for (int k = 0; k < e->nblk; ++k) {
    const BlockW& bw = e->blk[k];
    const bool temporal = (k & 1) != 0;
    const uint16_t* AOb = HNb;                             // the attention output: proj's operand
    if (temporal ? pl.fused_tp : pl.fused_sp) {
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_QKV_TATTN : D3D_KC_QKV_SATTN, 2.0 * M * 3.0 * D * D + 4.0 * M * (double)N * D, 2.0 * MD2 + 2.0 * 3.0 * D * D, s);
      HIP_TRY(launch_qkv_attn_bf16(HNb, bw.qkv_x3, bw.qkvb, QKVb, temporal ? B * J : B * T, N, temporal ? J : 1, D, e->H, temporal ? 1 : 0, s, f16));
      AOb = QKVb;
    } else {
    HIP_TRY(linear(HNb, bw.qkv_x3, bw.qkvb, nullptr, nullptr, QKVb, 3 * D, D, EPI_NONE, D, D3D_KC_LINEAR_QKV));
    {
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_ATTN_TEMPORAL : D3D_KC_ATTN_SPATIAL, 4.0 * M * (double)N * D, 4.0 * MD2, s);
      if (temporal) HIP_TRY(launch_attn_bf16(QKVb, HNb, B, T, J, D, e->H, s, f16));
      else HIP_TRY(launch_attn_bf16(QKVb, HNb, B * T, J, 1, D, e->H, s, f16));
    }
    }
    // x = post_norm(x + hidden W2^T + b2) [+ Temporal_pos_embed before TTE0] [+ next block's time vector]; h = bf16(next.norm1(x))
    X3PostNorm post = block_postnorm(e, k, tvec, tvec_stride);
    if (k + 1 < e->nblk) { post.g2 = e->blk[k + 1].n1g; post.b2 = e->blk[k + 1].n1b; post.eps2 = e->ln_eps; }
    if (pl.rows) {
      {  // x += attn Wproj^T + b (fp32 stream in place); h = bf16(norm2(x)) over the attention output's rows (same tile rows: in place)
        X3PostNorm pn{};
        pn.g2 = bw.n2g; pn.b2 = bw.n2b; pn.eps2 = e->ln_eps; pn.pos_div = 1; pn.pos_mod = 1; pn.rows_per_batch = T * J;
        HIP_TRY(linear_rows(AOb, bw.proj_x3, bw.projb, HNb, D, pn, D3D_KC_LINEAR_PROJ));
      }
      HIP_TRY(linear(HNb, bw.fc1_x3, bw.fc1b, nullptr, nullptr, HIDb, e->Dm, D, EPI_GELU, 0, D3D_KC_LINEAR_FC1));
      HIP_TRY(linear_rows(HIDb, bw.fc2_x3, bw.fc2b, k + 1 < e->nblk ? HNb : nullptr, e->Dm, post, D3D_KC_LINEAR_FC2));
      continue;
    }
    HIP_TRY(linear(AOb, bw.proj_x3, bw.projb, w.X, w.X, nullptr, D, D, EPI_RESIDUAL, 0, D3D_KC_LINEAR_PROJ));
    {  // h = bf16(norm2(x))
      LnArgs a = ln_rows(M, D, T * J);
      a.x = w.X; a.h_bf16 = HNb; a.g1 = bw.n2g; a.b1 = bw.n2b; a.eps1 = e->ln_eps;
      HIP_TRY(lnorm(a));
    }
    HIP_TRY(linear(HNb, bw.fc1_x3, bw.fc1b, nullptr, nullptr, HIDb, e->Dm, D, EPI_GELU, 0, D3D_KC_LINEAR_FC1));
    HIP_TRY(linear(HIDb, bw.fc2_x3, bw.fc2b, w.X, w.X, nullptr, D, e->Dm, EPI_RESIDUAL, 0, D3D_KC_LINEAR_FC2));
    {  // the post-norm and the next norm1 as a row kernel
      LnArgs a = ln_postnorm(e, M, post);
      a.x = w.X; a.y = w.X;
      if (k + 1 < e->nblk) { a.h_bf16 = HNb; a.g2 = post.g2; a.b2 = post.b2; a.eps2 = post.eps2; }
      HIP_TRY(lnorm(a));
    }
  }
  return D3D_OK;
}

// One denoiser forward up to (not including) the head: leaves the final Temporal_norm output in w.X.
// tvec: (n, nblk, D) time-embedding table slice or nullptr; tvec_stride = 0 (all rows share entry 0) or nblk*D.
int run_blocks(d3d_engine* e, const BlockPlan& pl, const float* x2d, const float* y, int y_bcast, const float* tvec, int64_t tvec_stride,
               int B, const Workspace& w, hipStream_t s) {
  const int T = e->T, J = e->J, D = e->D;
  const int M = B * T * J;
  const double MD4 = (double)M * D * 4.0;
  if (pl.attn.flow == ATTN_FLOW_FOLD) return run_blocks_fold(e, pl, x2d, y, y_bcast, tvec, tvec_stride, B, w, s);
  if (pl.attn.flow == ATTN_FLOW_BF16) return run_blocks_bf16(e, pl, x2d, y, y_bcast, tvec, tvec_stride, B, w, s);
  {
    Prof p(e, D3D_KC_EMBED, 2.0 * M * D * e->cin, MD4 + (double)M * e->cin * 4.0, s);
    HIP_TRY(launch_embed(x2d, y, e->fus_w, e->fus_b, e->spos, tvec, tvec_stride, w.X, B, T, J, D, e->cfg.in_chans,
                         y_bcast, s));
  }
  const bool x3 = e->cfg.precision == D3D_PREC_F16X3;
  // F16X3: every GEMM A-operand lives in the fp16 hi/lo pair layout (d3d_kernels.h) written by its producer; the pair
  // buffer of an (rows x cols) activation occupies the same bytes as the fp32 tensor would (rows padded to 256, the
  // padding rows are staged by edge tiles but never stored).
  uint16_t* HNx = reinterpret_cast<uint16_t*>(w.HN);
  uint16_t* HIDx = reinterpret_cast<uint16_t*>(w.HID);
  // A: fp32 activation (FP32 mode) or its pair buffer (F16X3 mode).  outsplit (F16X3 only): 1 = C as hi/lo planes
  // Ch/Cl (qkv -> temporal attention), 2 = C in the pair layout at Ch (fc1 -> fc2 hand-off)
  int qcols_ = 0;
  auto linear = [&](const float* A, const uint16_t* Ax, const float* W, const uint16_t* Wx, int wexp, const float* bias, const float* R,
                    float* C, uint16_t* Ch_, uint16_t* Cl_, int outsplit, int N, int K, int epi) -> hipError_t {
    Prof p(e, D3D_KC_LINEAR, 2.0 * M * (double)N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N * (R ? 2 : 1)), s);
    if (x3) return launch_linear_x3p(Ax, Wx, bias, R, C, Ch_, Cl_, M, N, K, epi, outsplit, qcols_, 0, s, nullptr, wexp);
    return launch_linear_f32(A, W, bias, R, C, M, N, K, epi, s);
  };
  auto lnorm = [&](LnArgs a) -> hipError_t {
    if (x3 && a.h) { a.h = nullptr; a.h_x3 = HNx; }   // normalised activations go out as GEMM operands
    Prof p(e, D3D_KC_LAYERNORM, 8.0 * M * D, MD4 * (1 + (a.y ? 1 : 0) + ((a.h || a.h_x3) ? 1 : 0)), s);
    return launch_layernorm(a, s);
  };
  {  // h = norm1_0(x)
    LnArgs a = ln_rows(M, D, T * J);
    a.x = w.X; a.h = w.HN; a.g1 = e->blk[0].n1g; a.b1 = e->blk[0].n1b; a.eps1 = e->ln_eps;
    HIP_TRY(lnorm(a));
  }
  for (int k = 0; k < e->nblk; ++k) {
    const BlockW& bw = e->blk[k];
    const bool temporal = (k & 1) != 0;
    // F16X3: the qkv GEMM hands q/k/v to the fp16-MFMA attention kernel as hi/lo planes.  A spatial block is the same
    // kernel over groups of J consecutive tokens (one "joint", "frames" = the J tokens of a frame, B*T "batches").
    const AttnPick kernel = temporal ? pl.attn.tp : pl.attn.sp;
    const bool attn_x3 = kernel.fam().form == ATTN_PLANES;
    uint16_t* QKVh = reinterpret_cast<uint16_t*>(w.QKV);
    uint16_t* QKVl = QKVh + (size_t)M * 3 * D;
    qcols_ = attn_x3 ? D : 0;
    HIP_TRY(linear(w.HN, HNx, bw.qkvw, bw.qkv_x3, bw.qkv_e, bw.qkvb, nullptr, w.QKV, attn_x3 ? QKVh : nullptr, attn_x3 ? QKVl : nullptr,
                   attn_x3 ? 1 : 0, 3 * D, D, EPI_NONE));
    qcols_ = 0;
    {
      const int N = temporal ? T : J;
      Prof p(e, temporal ? D3D_KC_ATTN_TEMPORAL : D3D_KC_ATTN_SPATIAL, 4.0 * M * (double)N * D, 4.0 * MD4, s);
      const int rc = launch_attention(e, kernel, temporal, w.QKV, w.HN, x3 ? HNx : nullptr, B, s);
      if (rc) return rc;
    }
    HIP_TRY(linear(w.HN, HNx, bw.projw, bw.proj_x3, bw.proj_e, bw.projb, w.X, w.X, nullptr, nullptr, 0, D, D, EPI_RESIDUAL));
    {  // h = norm2(x)
      LnArgs a = ln_rows(M, D, T * J);
      a.x = w.X; a.h = w.HN; a.g1 = bw.n2g; a.b1 = bw.n2b; a.eps1 = e->ln_eps;
      HIP_TRY(lnorm(a));
    }
    HIP_TRY(linear(w.HN, HNx, bw.fc1w, bw.fc1_x3, bw.fc1_e, bw.fc1b, nullptr, w.HID, x3 ? HIDx : nullptr, nullptr, x3 ? 2 : 0, e->Dm, D,
                   EPI_GELU));
    HIP_TRY(linear(w.HID, HIDx, bw.fc2w, bw.fc2_x3, bw.fc2_e, bw.fc2b, w.X, w.X, nullptr, nullptr, 0, D, e->Dm, EPI_RESIDUAL));
    {  // x = post_norm(x) [+ Temporal_pos_embed before TTE0] [+ next block's time vector]; h = next.norm1(x)
      LnArgs a = ln_postnorm(e, M, block_postnorm(e, k, tvec, tvec_stride));
      a.x = w.X; a.y = w.X;
      if (k + 1 < e->nblk) { a.h = w.HN; a.g2 = e->blk[k + 1].n1g; a.b2 = e->blk[k + 1].n1b; a.eps2 = e->ln_eps; }
      HIP_TRY(lnorm(a));
    }
  }
  return D3D_OK;
}

int head_rows(const d3d_engine* e, int B) { return e->cfg.seq2frame ? B * e->J : B * e->T * e->J; }

// fills X / rows for the head (runs the seq2frame frame reduce first when needed)
int prep_head(d3d_engine* e, HeadArgs& h, int B, const Workspace& w, hipStream_t s) {
  h.g = e->hd_g; h.b = e->hd_b; h.eps = 1e-5f; h.Wh = e->hd_w; h.bh = e->hd_bias; h.D = e->D;
  h.inject = e->opt_head_inject; h.fence = e->opt_head_fence;
  h.rows = head_rows(e, B);
  if (e->cfg.seq2frame) {
    Prof p(e, D3D_KC_OTHER, 2.0 * B * e->T * e->J * e->D, 4.0 * B * e->T * e->J * e->D, s);
    HIP_TRY(launch_frame_reduce(w.X, e->wm_w, e->wm_b, w.RED, B, e->T, e->J, e->D, s));
    h.X = w.RED;
  } else {
    h.X = w.X;
  }
  return D3D_OK;
}

int check_ready(const d3d_engine* e, int B, const void* ws, size_t ws_bytes) {
  if (!e) return fail(D3D_EINVAL, "null engine");
  if (!e->committed) return fail(D3D_ESTATE, "weights not committed (d3d_engine_commit_weights)");
  {   // one engine per device: its weights, tables and per-device kernel attributes belong to the device it was committed on
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != e->device)
      return fail(D3D_ESTATE, "engine was committed on device " + std::to_string(e->device) + " but the current device is " +
                                  std::to_string(dev) + " (one engine per device; make its device current before calling)");
  }
  if (B <= 0) return fail(D3D_EINVAL, "B must be positive");
  if ((long long)B * e->T * e->J > 0x7fffffffLL / 4) return fail(D3D_EINVAL, "batch too large for 32-bit token index");
  if (!ws) return fail(D3D_EINVAL, "null workspace");
  if (ws_bytes < d3d_workspace_bytes(e, B)) return fail(D3D_ENOMEM, "workspace smaller than d3d_workspace_bytes(e, B)");
  if ((reinterpret_cast<uintptr_t>(ws) & 255) != 0) return fail(D3D_EINVAL, "workspace must be 256-byte aligned");
  return D3D_OK;
}

}  // namespace

static inline uint32_t range_bits_to_abi(unsigned w, bool weights_clamped) {
  return ((w & d3d::RANGE_BIT_ACT) ? D3D_RANGE_ACT : 0u) | (weights_clamped ? D3D_RANGE_WEIGHT : 0u) |
         ((w & d3d::RANGE_BIT_STATS) ? D3D_RANGE_STATS : 0u) | ((w & d3d::RANGE_BIT_INDEX) ? D3D_RANGE_INDEX : 0u) |
         ((w & d3d::RANGE_BIT_RECOMPUTE) ? D3D_RANGE_RECOMPUTE : 0u);
}

// Range-guard sink of launches that belong to no engine (the single-op hooks): one word per device, written, never read.
unsigned* d3d::range_sink_word() {
  static std::atomic<unsigned*> words[64];   // race-free: the loser of the compare-exchange frees its own allocation and takes the winner's
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  unsigned* w = words[dev & 63].load(std::memory_order_acquire);
  if (w) return w;
  if (hipMalloc(&w, 256) != hipSuccess) return nullptr;
  (void)hipMemset(w, 0, 256);
  unsigned* expect = nullptr;
  if (!words[dev & 63].compare_exchange_strong(expect, w, std::memory_order_acq_rel)) { (void)hipFree(w); w = expect; }
  return w;
}

// ================================================================================================== C ABI
extern "C" {

const char* d3d_last_error(void) { return g_err.c_str(); }
// 141: option / info keys "long_temporal_h32", "long_temporal_f32_h32", info keys "long_temporal_h32_last", "long_temporal_f32_h32_last",
// d3d_op_attention_long_h32, d3d_op_attention_long_f32_h32
// 142: head_dim 128 admitted (FP32 and F16X3), option / info key "attn_h128", info key "attn_h128_last", d3d_op_attention_h128,
// d3d_op_attention_long_h128
// 143: option / info key "attn_f32_h128", info key "attn_f32_h128_last", d3d_op_attention_f32_h128, d3d_op_attention_long_f32_h128
// 145: head_dim 48 and 96 admitted (FP32 and F16X3), option / info key "attn_hx", info key "attn_hx_last", d3d_op_attention_hx,
// d3d_op_attention_long_hx
// 146: option / info key "attn_f32_hx", info key "attn_f32_hx_last", d3d_op_attention_f32_hx, d3d_op_attention_long_f32_hx
// 147: option / info keys "attn_h16" and "attn_f32_h16", info keys "attn_h16_last" and "attn_f32_h16_last", d3d_op_attention_h16,
// d3d_op_attention_long_h16, d3d_op_attention_f32_h16, d3d_op_attention_long_f32_h16
// 148: option / info key "fused_narrow", info key "fused_narrow_last", d3d_op_qkv_attn_x3_narrow
int d3d_version(void) { return 149; }

int d3d_ddim_times(int32_t num_timesteps, int32_t sampling_timesteps, int32_t* out) {
  // torch.linspace(-1, N-1, S+1) in fp32 (two-sided evaluation around the midpoint), .int() truncation, reversed
  // (DIFF:270-272).  A one-sided or fp64 evaluation is off by one for ~200 of the 1000 possible S.
  if (num_timesteps < 1 || sampling_timesteps < 1 || !out) return fail(D3D_EINVAL, "d3d_ddim_times: bad arguments");
  const int steps = sampling_timesteps + 1;
  const float start = -1.0f, end = (float)(num_timesteps - 1);
  volatile float step = (end - start) / (float)(steps - 1);
  const int half = steps / 2;
  for (int i = 0; i < steps; ++i) {
    volatile float prod, v;
    if (i < half) {
      prod = (float)i * step;
      v = start + prod;
    } else {
      prod = (float)(steps - 1 - i) * step;
      v = end - prod;
    }
    out[steps - 1 - i] = (int32_t)v;  // trunc toward zero
  }
  return D3D_OK;
}

int d3d_engine_create(const d3d_config* c, d3d_engine** out) {
  if (!c || !out) return fail(D3D_EINVAL, "null argument");
  if (c->num_frame < 1 || c->num_joints < 1 || c->in_chans < 1 || c->in_chans > 5 || c->embed_dim < 4 || c->depth < 1 ||
      c->num_heads < 1 || c->mlp_hidden < 1)
    return fail(D3D_EINVAL, "d3d_config: non-positive dimension");
  if (c->embed_dim % c->num_heads) return fail(D3D_EINVAL, "embed_dim must be divisible by num_heads");
  // embed_dim 48 h with h odd (heads of 48 columns) is a multiple of 16 alone: the fp32 GEMM zero-fills its last k-tile of 16, the fp16
  // plane forms (pair layout: groups of 32 columns) do not exist there -- such an engine runs the FP32 kernels (below)
  const bool half_tile = c->embed_dim % 32 == 16 && c->embed_dim == 48 * c->num_heads;
  if ((c->embed_dim % 32 && !half_tile) || c->mlp_hidden % 32)
    return fail(D3D_EUNSUP, "embed_dim and mlp_hidden must be multiples of 32 (MFMA k-tile; embed_dim: or 16 more with head_dim 48)");
  if (c->embed_dim > 1024) return fail(D3D_EUNSUP, "embed_dim > 1024 unsupported by the row kernels");
  {
    const int dh = c->embed_dim / c->num_heads;
    if (dh != 4 && dh != 8 && dh != 16 && dh != 32 && dh != 48 && dh != 64 && dh != 96 && dh != 128)
      return fail(D3D_EUNSUP, "head_dim must be 4,8,16,32,48,64,96 or 128");
  }
  if (c->precision != D3D_PREC_FP32 && c->precision != D3D_PREC_F16X3 && c->precision != D3D_PREC_BF16 && c->precision != D3D_PREC_F16)
    return fail(D3D_EUNSUP, "precision must be D3D_PREC_FP32, D3D_PREC_F16X3, D3D_PREC_BF16 or D3D_PREC_F16");
  if (c->precision == D3D_PREC_BF16 &&
      (!attn_bf16_ok(c->num_frame, c->embed_dim, c->num_heads) || !attn_bf16_ok(c->num_joints, c->embed_dim, c->num_heads) ||
       c->num_joints > 32 || c->embed_dim % 64 || c->mlp_hidden % 64))
    return fail(D3D_EUNSUP, "D3D_PREC_BF16 needs head_dim 64, num_frame <= 256, num_joints <= 32 and widths that are multiples of 64");
  if (c->precision == D3D_PREC_F16 &&   // (the bf16 mode's kernels: its admission exactly)
      (!attn_bf16_ok(c->num_frame, c->embed_dim, c->num_heads) || !attn_bf16_ok(c->num_joints, c->embed_dim, c->num_heads) ||
       c->num_joints > 32 || c->embed_dim % 64 || c->mlp_hidden % 64))
    return fail(D3D_EUNSUP, "D3D_PREC_F16 needs head_dim 64, num_frame <= 256, num_joints <= 32 and widths that are multiples of 64");
  d3d_engine* e = new d3d_engine();
  e->cfg = *c;
  if (half_tile) e->cfg.precision = D3D_PREC_FP32;   // F16X3 asked for: every kernel of the engine is the exact FP32 one
  e->T = c->num_frame; e->J = c->num_joints; e->D = c->embed_dim; e->H = c->num_heads; e->Dm = c->mlp_hidden;
  e->Dt = c->with_time_emb ? 2 * c->embed_dim : 0;
  e->depth = c->depth; e->nblk = 2 * c->depth; e->cin = c->in_chans + 3;
  build_slots(e);
  *out = e;
  return D3D_OK;
}

void d3d_engine_destroy(d3d_engine* e) { delete e; }

int d3d_engine_num_weights(const d3d_engine* e) { return e ? (int)e->slots.size() : 0; }

int d3d_engine_weight_info(const d3d_engine* e, int i, const char** name, int64_t* numel) {
  if (!e || i < 0 || i >= (int)e->slots.size()) return fail(D3D_EINVAL, "weight index out of range");
  if (name) *name = e->slots[i].name.c_str();
  if (numel) *numel = e->slots[i].numel;
  return D3D_OK;
}

int d3d_engine_set_weight(d3d_engine* e, const char* name, const float* host, int64_t numel) {
  if (!e || !name || !host) return fail(D3D_EINVAL, "null argument");
  auto it = e->index.find(name);
  if (it == e->index.end()) return fail(D3D_EINVAL, std::string("unknown weight name: ") + name);
  WeightSlot& s = e->slots[it->second];
  if (numel != s.numel)
    return fail(D3D_EINVAL, std::string("size mismatch for ") + name + ": got " + std::to_string(numel) + ", expected " +
                                std::to_string(s.numel));
  s.host.assign(host, host + numel);
  s.set = true;
  e->committed = false;
  return D3D_OK;
}

int d3d_engine_set_time_freqs(d3d_engine* e, const float* host, int32_t n) {
  if (!e || !host) return fail(D3D_EINVAL, "null argument");
  if (n != e->D / 2) return fail(D3D_EINVAL, "time frequency table must have embed_dim/2 entries");
  e->freqs_host.assign(host, host + n);
  e->freqs_set = true;
  e->committed = false;
  return D3D_OK;
}

int d3d_engine_commit_weights(d3d_engine* e) {
  if (!e) return fail(D3D_EINVAL, "null engine");
  for (const auto& s : e->slots)
    if (!s.set) return fail(D3D_ESTATE, "missing weight: " + s.name);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
    return fail(D3D_EHIP, "no HIP device: libd3d_hip has no CPU path");
  // All or nothing: from here to the last line the engine is "not committed, no schedule" and holds no view into a buffer, so a step
  // that fails leaves an engine every entry point refuses (check_ready, "schedule not set"), never one that points at freed memory.
  // The old buffers go before anything is allocated: a re-commit's peak device footprint is one set of images.
  e->committed = e->sched_set = false;
  e->drop_graphs();
  e->blk.clear();
  const std::pair<const float**, const char*> views[] = {
      {&e->fus_w, "fusion_layer.weight"}, {&e->fus_b, "fusion_layer.bias"}, {&e->spos, "Spatial_pos_embed"}, {&e->tpos, "Temporal_pos_embed"},
      {&e->sn_g, "Spatial_norm.weight"}, {&e->sn_b, "Spatial_norm.bias"}, {&e->tn_g, "Temporal_norm.weight"}, {&e->tn_b, "Temporal_norm.bias"},
      {&e->hd_g, "head.0.weight"}, {&e->hd_b, "head.0.bias"}, {&e->hd_w, "head.1.weight"}, {&e->hd_bias, "head.1.bias"},
      {&e->wm_w, "weighted_mean.weight"}, {&e->wm_b, "weighted_mean.bias"}, {&e->tm1_w, "time_mlp.1.weight"}, {&e->tm1_b, "time_mlp.1.bias"},
      {&e->tm3_w, "time_mlp.3.weight"}, {&e->tm3_b, "time_mlp.3.bias"}};   // (a model without the tensor: nullptr)
  for (auto& v : views) *v.first = nullptr;
  e->b0_wg = e->b0_G = e->b0_P = nullptr;
  e->arena.reset(); e->arena16.reset(); e->arena_fold.reset(); e->b0_tab.reset(); e->tblk_w.reset(); e->tblk_b.reset(); e->freqs_dev.reset();

  // ---- host: every image, packed before a byte is allocated (weight_pack.hip)
  const size_t D = e->D, Dt = e->Dt, N3 = 3 * D, half = D / 2;
  const bool x3 = e->cfg.precision == D3D_PREC_F16X3;
  auto blk_name = [](int k) { return std::string((k & 1) ? "TTEblocks." : "STEblocks.") + std::to_string(k / 2); };   // execution order
  auto host_w = [&](const std::string& name) { return e->slots[e->index[name]].host.data(); };                        // (S2S:225-245)
  auto block_tensors = [&](int k, auto get) {   // host_w: what the packing reads; wptr: the same tensors in the device arena
    const std::string p = blk_name(k);
    return BlockSrc{get(p + ".norm1.weight"), get(p + ".norm1.bias"), get(p + ".attn.qkv.weight"), get(p + ".attn.qkv.bias"),
                    get(p + ".attn.proj.weight"), get(p + ".attn.proj.bias"), get(p + ".norm2.weight"), get(p + ".norm2.bias"),
                    get(p + ".mlp.fc1.weight"), get(p + ".mlp.fc1.bias"), get(p + ".mlp.fc2.weight"), get(p + ".mlp.fc2.bias")};
  };
  size_t off = 0;
  for (auto& s : e->slots) { s.dev_off = off; off += align_up((size_t)s.numel, 64); }
  std::vector<BlockSrc> src;
  for (int k = 0; k < e->nblk; ++k) src.push_back(block_tensors(k, host_w));
  PackedWeights pk;
  // the tile-order images: for the fused kernels of width 64 in the order of the H heads; for "fused_narrow" (widths 32 / 16, which no
  // predicate of width 64 admits) in the order of D / 64 pseudo-heads -- a pair / a quad of heads is one 64-column segment
  const bool narrow_s = qkv_attn_x3_narrow_ok(e->J, 1, e->J, e->D, e->H, e->D), narrow_t = qkv_attn_x3_narrow_ok(e->T, e->J, e->J, e->D, e->H, e->D);
  const size_t tile_heads = narrow_s || narrow_t ? D / 64 : (size_t)e->H;
  if (x3 && !pack_f16x3(src, D, e->Dm, tile_heads, narrow_s || qkv_sattn_ok(e->J, e->D, e->H, e->D),
                        narrow_t || qkv_tattn_ok(e->T, e->J, e->D, e->H, e->D), pk))
    return fail(D3D_EHIP, "internal: head-major qkv planes got a different exponent");
  if (e->cfg.precision == D3D_PREC_BF16 || e->cfg.precision == D3D_PREC_F16) pack_bf16(src, D, e->Dm, pk, e->cfg.precision == D3D_PREC_F16);
  e->weights_clamped = pk.clamped;
  // "block0_direct": G and P of block 0 where it can take the direct form (a spatial F16X3 block on the fused kernel's tile geometry,
  // embedding straight into the planes); they follow Wg in one allocation, G padded to whole 64-float lines
  const size_t n_G = align_up(N3 * e->cin, 64);
  std::vector<float> b0;
  if (x3 && embed_planes_ok(e->D, e->cfg.in_chans) && qkv_sattn_direct_ok(e->J, e->D, e->H, e->cfg.in_chans)) {
    b0.resize(n_G + (size_t)e->J * N3);
    block0_tables_host(pk.wg0.data(), host_w("fusion_layer.weight"), host_w("fusion_layer.bias"), host_w("Spatial_pos_embed"), e->D, e->H,
                       e->cin, e->J, b0.data(), b0.data() + n_G);
  }
  if (Dt && !e->freqs_set) {   // SinusoidalPosEmb frequencies (S2S:31-33): exp(k * -(ln 1e4 / (half-1))) with the product formed in fp32
    e->freqs_host.resize(half);
    const float neg = (float)(-(std::log(10000.0) / (double)(half - 1)));
    for (size_t k = 0; k < half; ++k) {
      volatile float arg = (float)k * neg;
      e->freqs_host[k] = (float)std::exp((double)arg);
    }
  }

  // ---- device: allocate, upload
  HIP_TRY(e->arena.alloc(off));
  for (auto& s : e->slots)
    HIP_TRY(hipMemcpy(e->arena + s.dev_off, s.host.data(), (size_t)s.numel * sizeof(float), hipMemcpyHostToDevice));
  HIP_TRY(hipGetDevice(&e->device));
  if (!e->range_dev) {
    HIP_TRY(e->range_dev.alloc(256 / sizeof(unsigned)));
    HIP_TRY(hipMemset(e->range_dev, 0, 256));
  }
  if (!e->range_host) {
    HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e->range_host), d3d_engine::RANGE_TICKETS * sizeof(unsigned), hipHostMallocMapped));
    memset(e->range_host, 0, d3d_engine::RANGE_TICKETS * sizeof(unsigned));
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&e->range_host_dev), e->range_host, 0));
    e->range_ev.resize(d3d_engine::RANGE_TICKETS, nullptr);
    for (auto& ev : e->range_ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  }
  if (x3) HIP_TRY(e->arena_fold.upload(pk.fold.data(), pk.fold.size()));
  if (!pk.planes.empty()) HIP_TRY(e->arena16.upload(pk.planes.data(), pk.planes.size()));
  if (!b0.empty()) {
    HIP_TRY(e->b0_tab.alloc(N3 * D + b0.size()));
    HIP_TRY(hipMemcpy(e->b0_tab, pk.wg0.data(), N3 * D * sizeof(float), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->b0_tab + N3 * D, b0.data(), b0.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  if (Dt) {   // the 2*depth per-block Linear(Dt -> D) layers (S2S:104-107) concatenated into one (nblk*D, Dt) matrix
    HIP_TRY(e->tblk_w.alloc(e->nblk * D * Dt));
    HIP_TRY(e->tblk_b.alloc(e->nblk * D));
    for (int k = 0; k < e->nblk; ++k) {
      const std::string p = blk_name(k) + ".time_mlp.1";
      HIP_TRY(hipMemcpy(e->tblk_w + k * D * Dt, wptr(e, p + ".weight"), D * Dt * sizeof(float), hipMemcpyDeviceToDevice));
      HIP_TRY(hipMemcpy(e->tblk_b + k * D, wptr(e, p + ".bias"), D * sizeof(float), hipMemcpyDeviceToDevice));
    }
    HIP_TRY(e->freqs_dev.upload(e->freqs_host.data(), half));
  }

  // ---- views into the buffers: every upload has succeeded
  auto at16 = [&](size_t o) -> const uint16_t* { return o == NO_OFF ? nullptr : e->arena16 + o; };
  auto atf = [&](size_t o) -> const float* { return o == NO_OFF ? nullptr : e->arena_fold + o; };
  for (int k = 0; k < e->nblk; ++k) {
    BlockW b{};
    static_cast<BlockSrc&>(b) = block_tensors(k, [&](const std::string& name) { return wptr(e, name); });
    const BlockOff f = pk.blk.empty() ? BlockOff{} : pk.blk[k];
    b.qkv_x3 = at16(f.qkv_x3); b.proj_x3 = at16(f.proj_x3); b.fc1_x3 = at16(f.fc1_x3); b.fc2_x3 = at16(f.fc2_x3);
    b.qkv_f3 = at16(f.qkv_f3); b.fc1_f3 = at16(f.fc1_f3); b.qkv_f3h = at16(f.qkv_f3h);
    b.qkv_cs = atf(f.qkv_cs); b.qkv_fb = atf(f.qkv_fb); b.fc1_cs = atf(f.fc1_cs); b.fc1_fb = atf(f.fc1_fb);
    b.qkv_csh = atf(f.qkv_csh); b.qkv_fbh = atf(f.qkv_fbh);
    b.qkv_e = f.qkv_e; b.proj_e = f.proj_e; b.fc1_e = f.fc1_e; b.fc2_e = f.fc2_e; b.qkv_fe = f.qkv_fe; b.fc1_fe = f.fc1_fe;
    e->blk.push_back(b);
  }
  if (e->b0_tab) { e->b0_wg = e->b0_tab; e->b0_G = e->b0_tab + N3 * D; e->b0_P = e->b0_G + n_G; }
  for (auto& v : views) *v.first = wptr(e, v.second);
  e->committed = true;
  return D3D_OK;
}

int d3d_engine_set_schedule(d3d_engine* e, int32_t num_timesteps, const float* ac_host, const float* somac_host,
                            int32_t sampling_timesteps, float eta, int32_t clip_denoised, void* stream) {
  if (!e || !ac_host || !somac_host) return fail(D3D_EINVAL, "null argument");
  if (!e->committed) return fail(D3D_ESTATE, "commit weights before setting the schedule");
  if (num_timesteps < 1 || sampling_timesteps < 1) return fail(D3D_EINVAL, "timesteps must be positive");
  if (sampling_timesteps > num_timesteps) return fail(D3D_EINVAL, "sampling_timesteps <= timesteps required (DIFF:145)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RangeScope range_scope(e);
  e->sched_set = false;   // all or nothing: a step that fails below leaves "no schedule", which every reader of the tables checks
  e->drop_graphs();
  e->num_timesteps = num_timesteps; e->S = sampling_timesteps; e->eta = eta; e->clip = clip_denoised ? 1 : 0;
  e->ac.assign(ac_host, ac_host + num_timesteps);
  e->somac.assign(somac_host, somac_host + num_timesteps);
  e->times.resize(sampling_timesteps + 1);
  int rc = d3d_ddim_times(num_timesteps, sampling_timesteps, e->times.data());
  if (rc) return rc;
  e->ac_dev.reset(); e->somac_dev.reset(); e->temb_sched.reset();
  HIP_TRY(e->ac_dev.upload(ac_host, num_timesteps));
  HIP_TRY(e->somac_dev.upload(somac_host, num_timesteps));
  if (e->Dt) {
    const int S = sampling_timesteps;
    std::vector<float> tf(S);
    for (int i = 0; i < S; ++i) tf[i] = (float)e->times[i];
    DevBuf<float> tdev, scratch;
    HIP_TRY(tdev.upload(tf.data(), S));
    HIP_TRY(scratch.alloc((size_t)S * (e->D + 2 * (size_t)e->Dt)));
    HIP_TRY(e->temb_sched.alloc((size_t)S * e->nblk * e->D));
    rc = compute_temb(e, tdev, S, e->temb_sched, scratch, s);
    const hipError_t se = hipStreamSynchronize(s);   // (before the temporaries go, whatever rc says)
    if (rc) return rc;
    HIP_TRY(se);
  }
  e->sched_set = true;
  return D3D_OK;
}

size_t d3d_workspace_bytes(const d3d_engine* e, int32_t B) {
  if (!e || B <= 0) return 0;
  // one carve-up for the whole batch, or two for its halves ("streams" = 2): sized for either, so the option can change
  // without a new workspace
  size_t one = carve(e, B, nullptr).total_bytes, two = 0;
  if (B >= 2) two = align_up(carve(e, (B + 1) / 2, nullptr).total_bytes, 256) + carve(e, B / 2, nullptr).total_bytes;
  return std::max(one, two) + 256;
}

int d3d_denoise(d3d_engine* e, const float* x2d, const float* y, int32_t y_frames, const float* times_dev,
                int32_t n_times, float* x0, int32_t B, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_ready(e, B, ws, ws_bytes);
  if (rc) return rc;
  if (!x2d || !y || !x0) return fail(D3D_EINVAL, "null tensor");
  if (y_frames != 1 && y_frames != e->T) return fail(D3D_EINVAL, "y_frames must be 1 or num_frame");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RangeScope range_scope(e);
  Workspace w = carve(e, B, ws);
  const BlockPlan plan = e->last_plan = plan_blocks(e, B);
  const float* tvec = nullptr;
  int64_t stride = 0;
  if (e->Dt) {
    if (!times_dev) return fail(D3D_EINVAL, "times required when with_time_emb");
    if (n_times != 1 && n_times != B) return fail(D3D_EINVAL, "n_times must be 1 or B");
    rc = compute_temb(e, times_dev, n_times, w.TEMB, w.TSCR, s);
    if (rc) return rc;
    tvec = w.TEMB;
    stride = (n_times == 1) ? 0 : (int64_t)e->nblk * e->D;
  }
  rc = run_blocks(e, plan, x2d, y, (y_frames == 1 && e->T != 1) ? 1 : 0, tvec, stride, B, w, s);
  if (rc) return rc;
  HeadArgs h{};
  rc = prep_head(e, h, B, w, s);
  if (rc) return rc;
  h.x0_raw = x0; h.mode = 0;
  {
    Prof p(e, D3D_KC_HEAD, 14.0 * h.rows * e->D, 4.0 * h.rows * e->D, s);
    HIP_TRY(launch_head(h, s));
  }
  return D3D_OK;
}

namespace {
// The S-step loop of DIFF:262-300 as a launch sequence on `s` (also what gets captured into a hipGraph).
// step_stride: elements between the draws of consecutive steps in step_noise (the WHOLE batch's rows * 3 when B is a half-batch)
int ddim_loop(d3d_engine* e, const float* x2d, const float* init_noise, const float* step_noise, float* out, float* traj_rev,
              float* traj_x0, int B, const Workspace& w, hipStream_t s, size_t step_stride = 0) {
  const int S = e->S;
  const size_t yel = (size_t)head_rows(e, B) * 3;
  if (!step_stride) step_stride = yel;
  const BlockPlan plan = plan_blocks(e, B);
  for (int i = 0; i < S; ++i) {
    const int t = e->times[i], tn = e->times[i + 1];
    const float* y_cur = (i == 0) ? init_noise : ((i & 1) ? w.Y0 : w.Y1);
    float* y_next = (i == S - 1) ? out : ((i & 1) ? w.Y1 : w.Y0);
    const float* tvec = e->Dt ? e->temb_sched + (size_t)i * e->nblk * e->D : nullptr;
    int rc = run_blocks(e, plan, x2d, y_cur, e->cfg.seq2frame ? 1 : 0, tvec, 0, B, w, s);
    if (rc) return rc;
    HeadArgs h{};
    rc = prep_head(e, h, B, w, s);
    if (rc) return rc;
    h.clip = e->clip;
    h.y_cur = y_cur; h.y_next = y_next;
    h.traj_rev = traj_rev; h.traj_x0 = traj_x0; h.traj_rev_stride = S; h.traj_x0_stride = S; h.traj_idx = i;
    if (tn < 0) {
      h.mode = 2;
    } else {
      h.mode = 1;
      h.alpha = e->ac[t]; h.alpha_next = e->ac[tn]; h.somac = e->somac[t]; h.eta = e->eta;
      h.noise = (e->eta != 0.0f) ? step_noise + (size_t)i * step_stride : nullptr;
    }
    {
      Prof p(e, D3D_KC_HEAD, 14.0 * h.rows * e->D, 4.0 * h.rows * e->D, s);
      HIP_TRY(launch_head(h, s));
    }
    TRACE(0, 8, 0, y_next, yel * sizeof(float));
    if (e->tracing) {   // the head once more from the same inputs into scratch (kernel 9), and its y input (kernel 8, buffer 1)
      TRACE(0, 8, 1, y_cur, yel * sizeof(float));
      HeadArgs h2 = h;
      h2.y_next = w.OUTB; h2.traj_rev = nullptr; h2.traj_x0 = nullptr;
      if (h2.y_cur != h2.y_next) {
        HIP_TRY(launch_head(h2, s));
        TRACE(0, 9, 0, w.OUTB, yel * sizeof(float));
      }
      ++e->trace_fwd;
    }
  }
  return D3D_OK;
}

// "streams" = 2: rows [0, B0) on `s`, rows [B0, B) on the engine's side stream, each half in its own carve-up of the
// workspace; the side stream is forked from and joined back into `s` by events (inside a stream capture this makes two
// branches of the graph).  Every output element is independent of the batch it is computed in, so the result is bit-identical
// to the one-stream call.  The gain is the overlap of one half's partly filled kernel tails with the other half's work.
struct SplitWs { int B0, B1; Workspace w0, w1; };
SplitWs carve_split(const d3d_engine* e, int B, void* base) {
  SplitWs sw{};
  sw.B0 = (B + 1) / 2; sw.B1 = B - sw.B0;
  sw.w0 = carve(e, sw.B0, base);
  sw.w1 = carve(e, sw.B1, reinterpret_cast<char*>(base) + align_up(sw.w0.total_bytes, 256));
  return sw;
}
int ddim_loop_split(d3d_engine* e, const float* x2d0, const float* x2d1, const float* noise0, const float* noise1,
                    const float* step_noise, float* out0, float* out1, float* traj_rev, float* traj_x0, int B, const SplitWs& sw,
                    hipStream_t s) {
  if (!e->side_stream) HIP_TRY(hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking));
  if (!e->ev_fork) HIP_TRY(hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming));
  if (!e->ev_join) HIP_TRY(hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming));
  const size_t rows0 = (size_t)head_rows(e, sw.B0) * 3, rows_all = (size_t)head_rows(e, B) * 3;
  HIP_TRY(hipEventRecord(e->ev_fork, s));
  HIP_TRY(hipStreamWaitEvent(e->side_stream, e->ev_fork, 0));
  struct NoSlices {   // (d3d_kernels.h, LaunchCtx: the other half fills the partly filled rounds)
    bool saved = tl_launch_ctx.tail_slices;
    NoSlices() { tl_launch_ctx.tail_slices = false; }
    ~NoSlices() { tl_launch_ctx.tail_slices = saved; }
  } no_slices;
  int rc = ddim_loop(e, x2d0, noise0, step_noise, out0, traj_rev, traj_x0, sw.B0, sw.w0, s, rows_all);
  if (!rc)
    rc = ddim_loop(e, x2d1, noise1, step_noise ? step_noise + rows0 : nullptr, out1, traj_rev ? traj_rev + rows0 * e->S : nullptr,
                   traj_x0 ? traj_x0 + rows0 * e->S : nullptr, sw.B1, sw.w1, e->side_stream, rows_all);
  // join even after a failed launch, so that `s` never runs ahead of work already queued on the side stream
  hipError_t j1 = hipEventRecord(e->ev_join, e->side_stream);
  hipError_t j2 = hipStreamWaitEvent(s, e->ev_join, 0);
  if (rc) return rc;
  HIP_TRY(j1);
  HIP_TRY(j2);
  return D3D_OK;
}
}  // namespace

int d3d_ddim_sample(d3d_engine* e, const float* x2d, const float* init_noise, const float* step_noise, float* out,
                    float* traj_rev, float* traj_x0, int32_t B, void* ws, size_t ws_bytes, void* stream) {
  int rc = check_ready(e, B, ws, ws_bytes);
  if (rc) return rc;
  if (!e->sched_set) return fail(D3D_ESTATE, "schedule not set (d3d_engine_set_schedule)");
  if (!x2d || !init_noise || !out) return fail(D3D_EINVAL, "null tensor");
  if (e->eta != 0.0f && !step_noise) return fail(D3D_EINVAL, "step_noise required when eta != 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  RangeScope range_scope(e);
  Workspace w = carve(e, B, ws);
  const bool use_graph = e->graph_mode && !traj_rev && !traj_x0 && e->eta == 0.0f && !e->profiling && !e->tracing;
  const bool split = e->opt_streams == 2 && B >= 2 && !e->profiling && !e->tracing;
  const size_t xin_row = (size_t)e->T * e->J * e->cfg.in_chans;                 // x2d elements per sequence
  SplitWs sw{};
  if (split) sw = carve_split(e, B, ws);
  e->last_plan = plan_blocks(e, split ? sw.B0 : B);   // what ddim_loop runs (two half-batches: the first half's, see last_plan)
  const size_t xin0 = split ? (size_t)sw.B0 * xin_row : 0, y0 = split ? (size_t)head_rows(e, sw.B0) * 3 : 0;
  if (!use_graph) {
    if (split)
      return ddim_loop_split(e, x2d, x2d + xin0, init_noise, init_noise + y0, step_noise, out, out + y0, traj_rev, traj_x0, B, sw, s);
    return ddim_loop(e, x2d, init_noise, step_noise, out, traj_rev, traj_x0, B, w, s);
  }

  // Graph replay: the captured launch sequence reads its inputs from / writes its result to fixed staging buffers
  // inside the workspace, so one instantiated graph serves every call with the same (B, workspace).
  const size_t xin_bytes = (size_t)B * e->T * e->J * e->cfg.in_chans * sizeof(float);
  const size_t y_bytes = (size_t)head_rows(e, B) * 3 * sizeof(float);
  // the inputs go to the staging buffers FIRST: the eager warm-up pass below then computes the real result from real inputs
  // (staged behind it, it read uninitialised workspace memory -- large finite garbage could set the sticky range words)
  if (split) {
    HIP_TRY(hipMemcpyAsync(sw.w0.XIN, x2d, xin0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(sw.w1.XIN, x2d + xin0, xin_bytes - xin0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(sw.w0.NIN, init_noise, y0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(sw.w1.NIN, init_noise + y0, y_bytes - y0 * sizeof(float), hipMemcpyDeviceToDevice, s));
  } else {
    HIP_TRY(hipMemcpyAsync(w.XIN, x2d, xin_bytes, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.NIN, init_noise, y_bytes, hipMemcpyDeviceToDevice, s));
  }
  hipGraphExec_t exec = nullptr;
  for (auto& g : e->graphs)
    if (g.B == B && g.ws == ws) { exec = g.exec; g.used = ++e->graph_clock; }
  if (!exec) {
    if (!e->cap_stream) HIP_TRY(hipStreamCreateWithFlags(&e->cap_stream, hipStreamNonBlocking));
    auto run = [&](hipStream_t st) {   // (split: each half stages in its own carve-up -- the whole-batch one overlays them)
      if (split)
        return ddim_loop_split(e, sw.w0.XIN, sw.w1.XIN, sw.w0.NIN, sw.w1.NIN, nullptr, sw.w0.OUTB, sw.w1.OUTB, nullptr, nullptr, B, sw, st);
      return ddim_loop(e, w.XIN, w.NIN, nullptr, w.OUTB, nullptr, nullptr, B, w, st);
    };
    {   // one eager pass first: kernels set their max-LDS attribute on first launch, which must not happen mid-capture
      rc = run(s);
      if (rc) return rc;
      HIP_TRY(hipStreamSynchronize(s));
    }
    HIP_TRY(hipStreamBeginCapture(e->cap_stream, hipStreamCaptureModeThreadLocal));
    rc = run(e->cap_stream);
    hipGraph_t graph = nullptr;
    hipError_t ce = hipStreamEndCapture(e->cap_stream, &graph);
    if (rc) { if (graph) (void)hipGraphDestroy(graph); return rc; }
    HIP_TRY(ce);
    hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    if (ie != hipSuccess) { (void)hipGraphDestroy(graph); HIP_TRY(ie); }
    if (e->graphs.size() >= d3d_engine::MAX_GRAPHS) {   // evict the least recently used (its last replay is complete: the warm-up
      size_t lru = 0;                                    // pass above synchronised the stream)
      for (size_t i = 1; i < e->graphs.size(); ++i)
        if (e->graphs[i].used < e->graphs[lru].used) lru = i;
      (void)hipDeviceSynchronize();   // (a replay of it on another stream of the caller's must be over too; evictions are rare)
      (void)hipGraphExecDestroy(e->graphs[lru].exec);
      (void)hipGraphDestroy(e->graphs[lru].graph);
      e->graphs.erase(e->graphs.begin() + (long)lru);
    }
    e->graphs.push_back({B, ws, graph, exec, ++e->graph_clock});
    ++e->graphs_captured;
  }
  HIP_TRY(hipGraphLaunch(exec, s));
  if (split) {
    HIP_TRY(hipMemcpyAsync(out, sw.w0.OUTB, y0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(out + y0, sw.w1.OUTB, y_bytes - y0 * sizeof(float), hipMemcpyDeviceToDevice, s));
    return D3D_OK;
  }
  HIP_TRY(hipMemcpyAsync(out, w.OUTB, y_bytes, hipMemcpyDeviceToDevice, s));
  return D3D_OK;
}

int d3d_engine_set_option(d3d_engine* e, const char* key, int64_t value) {
  if (!key) return fail(D3D_EINVAL, "null key");
  const std::string k(key);
  // 3 / 4 operand stages in the one-tile-per-workgroup GEMM launches: NULL engine = the process-wide default (the single-op hooks and
  // every engine that has not been given a value of its own), an engine = that engine alone
  if (k == "deep_stages" && !e) { set_x3q_deep_stages(value != 0); return D3D_OK; }
  if (!e) return fail(D3D_EINVAL, "null engine");
  if (k == "deep_stages") e->opt_deep_stages = value != 0 ? 1 : 0;
  else
  if (k == "fused_postnorm") e->opt_fused_postnorm = value != 0;
  else if (k == "fold_layernorm") e->opt_fold_layernorm = value != 0;
  else if (k == "fused_spatial") e->opt_fused_spatial = value != 0;
  else if (k == "fused_temporal") e->opt_fused_temporal = value != 0;
  else if (k == "block0_direct") e->opt_block0_direct = value != 0;
  else if (k == "fc1_kernel") e->opt_fc1_kernel = value != 0;
  else if (k == "proj_kernel") e->opt_proj_kernel = value != 0;
  else if (k == "head_inject") e->opt_head_inject = value != 0;
  else if (k == "head_fence") e->opt_head_fence = value != 0;
  else if (k == "norm_eps_bits") {
    const uint32_t b = (uint32_t)value;
    float v;
    memcpy(&v, &b, 4);
    if (!(v > 0.f) || !(v < 1.f)) return fail(D3D_EINVAL, "norm_eps_bits: the bit pattern of an eps in (0, 1)");
    e->ln_eps = v;
  }
  else if (k == "bf16_gemm_kernel") e->opt_bf16_gemm_kernel = value != 0;
  else if (k == "latency_mode") {
    e->opt_latency_mode = value != 0;
    if (!e->opt_latency_mode) {
      if (e->lat_scratch[0] || e->lat_scratch[1]) (void)hipDeviceSynchronize();   // (a forward that reads the buffer may be in flight)
      for (auto& p : e->lat_scratch) p.reset();
    } else if (e->committed) {        // (an engine that exists on the host only has no device to allocate on: the first forward does it)
      const int rc = ensure_lat_scratch(e, 0);
      if (rc) { e->opt_latency_mode = false; return rc; }
    }
  }
  else if (const int ao = attn_option_index(key); ao >= 0) e->attn_opts = value != 0 ? e->attn_opts | 1u << ao : e->attn_opts & ~(1u << ao);
  else if (k == "proj_split" || k == "fc1_split") {
    const bool proj = k == "proj_split";
    if (value != -1 && value != 0 && !(proj ? proj_splitk_ok(e->D, e->D, (int)value) : fc1_splitk_ok(e->Dm, e->D, (int)value)))
      return fail(D3D_EUNSUP, k + ": -1 (the rule), 0, or S in {2, 4} with embed_dim / 32 / S >= 4 whole k-tiles, embed_dim 512");
    (proj ? e->opt_proj_split : e->opt_fc1_split) = (int)value;
  }
  else if (k == "small_tiles") {
    if (value != 0 && value != 1) return fail(D3D_EINVAL, "small_tiles must be 0 or 1");
    e->opt_small_tiles = value != 0;
  }
  else if (k == "fused_narrow") {
    if (value != 0 && value != 1) return fail(D3D_EINVAL, "fused_narrow must be 0 or 1");
    e->opt_fused_narrow = value != 0;
  }
  else if (k == "streams") {
    if (value != 1 && value != 2) return fail(D3D_EINVAL, "streams must be 1 or 2");
    e->opt_streams = (int)value;
  }
  else return fail(D3D_EINVAL, "unknown option: " + k);
  e->drop_graphs();   // captured launch sequences embody the old setting
  return D3D_OK;
}

int d3d_engine_set_graph_mode(d3d_engine* e, int32_t on) {
  if (!e) return fail(D3D_EINVAL, "null engine");
  e->graph_mode = on != 0;
  if (!e->graph_mode) e->drop_graphs();
  return D3D_OK;
}

int d3d_q_sample(d3d_engine* e, const float* x_start, const float* noise, const int32_t* t_dev, float* out, int32_t B,
                 int64_t n, void* stream) {
  if (!e || !x_start || !noise || !t_dev || !out) return fail(D3D_EINVAL, "null argument");
  if (!e->sched_set) return fail(D3D_ESTATE, "schedule not set");
  if (!e->has_sqrt_ac) return fail(D3D_ESTATE, "sqrt_alphas_cumprod not supplied (d3d_engine_set_sqrt_alphas_cumprod)");
  RangeScope range_scope(e);   // an out-of-table timestep raises D3D_RANGE_INDEX in this engine's word
  HIP_TRY(launch_q_sample(x_start, noise, t_dev, e->sqrt_ac_dev, e->somac_dev, out, B, n, e->num_timesteps, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_weighted_loss(d3d_engine* e, const float* model_out, const float* target, const int32_t* t_dev, float* out, int32_t B,
                      int64_t n, int32_t loss_type, int32_t clip_loss, void* stream) {
  if (!e || !model_out || !target || !t_dev || !out || B < 1 || n < 1) return fail(D3D_EINVAL, "bad argument");
  if (loss_type != 1 && loss_type != 2) return fail(D3D_EINVAL, "loss_type: 1 = l1, 2 = l2 (DIFF:368-375)");
  if (!e->sched_set) return fail(D3D_ESTATE, "schedule not set");
  RangeScope range_scope(e);
  HIP_TRY(launch_weighted_loss(model_out, target, t_dev, e->ac_dev, e->somac_dev, out, B, n, loss_type == 2, clip_loss != 0,
                               e->num_timesteps, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_repeat_batch(const float* x, float* out, int32_t B, int64_t n, int32_t repeat_n, void* stream) {
  if (!x || !out || B < 1 || n < 1 || repeat_n < 1) return fail(D3D_EINVAL, "bad argument");
  HIP_TRY(launch_repeat_rows(x, out, B, n, repeat_n, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_hypothesis_mean(const float* pred, float* out, int32_t B, int64_t n, int32_t repeat_n, void* stream) {
  if (!pred || !out || B < 1 || n < 1 || repeat_n < 1) return fail(D3D_EINVAL, "bad argument");
  HIP_TRY(launch_hypothesis_mean(pred, out, B, n, repeat_n, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_engine_get_info(const d3d_engine* e, const char* key, int64_t* value) {
  if (!e || !key || !value) return fail(D3D_EINVAL, "null argument");
  const std::string k(key);
  if (k == "graphs_cached") *value = (int64_t)e->graphs.size();
  else if (k == "graphs_captured") *value = (int64_t)e->graphs_captured;
  else if (k == "streams") *value = e->opt_streams;
  else if (k == "device") *value = e->device;
  else if (attn_plan_key(e->last_plan.attn, key, value)) {}   // the "*_last" keys of the attention kernels
  else if (k == "latency_mode") *value = e->opt_latency_mode ? 1 : 0;
  else if (const int ao = attn_option_index(key); ao >= 0) *value = e->attn_opts >> ao & 1u;
  else if (k == "deep_stages") *value = e->opt_deep_stages < 0 ? (x3q_deep_stages_default() ? 1 : 0) : e->opt_deep_stages;
  else if (k == "fc2_split_last") *value = e->last_plan.fc2_split;
  else if (k == "proj_split_last") *value = e->last_plan.proj_split;
  else if (k == "fc1_split_last") *value = e->last_plan.fc1_split;
  else if (k == "block0_direct_last") *value = e->last_plan.b0_direct ? 1 : 0;
  else if (k == "proj_split") *value = e->opt_proj_split;
  else if (k == "small_tiles") *value = e->opt_small_tiles ? 1 : 0;
  else if (k == "small_tiles_last")
    *value = e->last_plan.attn.flow == ATTN_FLOW_FOLD ? (e->last_plan.small_sp ? 1 : 0) | (e->last_plan.small_tp ? 2 : 0) : 0;
  else if (k == "fused_narrow") *value = e->opt_fused_narrow ? 1 : 0;
  else if (k == "fused_narrow_last")
    *value = e->last_plan.attn.flow == ATTN_FLOW_FOLD ? (e->last_plan.narrow_sp ? 1 : 0) | (e->last_plan.narrow_tp ? 2 : 0) : 0;
  else if (k == "fc1_split") *value = e->opt_fc1_split;
  else if (k == "fused_spatial_last") *value = e->last_plan.attn.flow == ATTN_FLOW_FOLD && e->last_plan.fused_sp;
  else if (k == "bf16_fused_spatial_last") *value = e->last_plan.attn.flow == ATTN_FLOW_BF16 && e->last_plan.fused_sp;
  else if (k == "bf16_fused_temporal_last") *value = e->last_plan.attn.flow == ATTN_FLOW_BF16 && e->last_plan.fused_tp;
  else return fail(D3D_EINVAL, "unknown info key: " + k);
  return D3D_OK;
}

int d3d_engine_set_sqrt_alphas_cumprod(d3d_engine* e, const float* host, int32_t n) {
  if (!e || !host) return fail(D3D_EINVAL, "null argument");
  if (!e->sched_set || n != e->num_timesteps) return fail(D3D_ESTATE, "set the schedule first; n must equal num_timesteps");
  e->has_sqrt_ac = false;
  HIP_TRY(e->sqrt_ac_dev.upload(host, n));
  e->has_sqrt_ac = true;
  return D3D_OK;
}

int d3d_allgather_pred(void* nccl_comm, const float* send, float* recv, int64_t count_per_rank, void* stream) {
  if (!nccl_comm || !send || !recv || count_per_rank <= 0) return fail(D3D_EINVAL, "bad argument");
  // ncclResult_t ncclAllGather(const void* sendbuff, void* recvbuff, size_t sendcount, ncclDataType_t, ncclComm_t, hipStream_t)
  typedef int (*allgather_fn)(const void*, void*, size_t, int, void*, hipStream_t);
  // resolved lazily; only a SUCCESSFUL lookup is cached (RCCL may be loaded into the process after the first call)
  static std::atomic<allgather_fn> cached{nullptr};
  allgather_fn fn = cached.load(std::memory_order_acquire);
  if (!fn) {
    void* sym = dlsym(RTLD_DEFAULT, "ncclAllGather");
    for (const char* name : {"librccl.so", "librccl.so.1"}) {
      if (sym) break;
      if (void* h = dlopen(name, RTLD_NOW | RTLD_NOLOAD)) sym = dlsym(h, "ncclAllGather");   // only a library the process already holds
    }
    fn = reinterpret_cast<allgather_fn>(sym);
    if (!fn) return fail(D3D_EUNSUP, "no RCCL library is loaded in this process (ncclAllGather not found)");
    cached.store(fn, std::memory_order_release);
  }
  constexpr int NCCL_FLOAT32 = 7;   // ncclDataType_t: ncclFloat32 (rccl.h)
  const int rc = fn(send, recv, (size_t)count_per_rank, NCCL_FLOAT32, nccl_comm, reinterpret_cast<hipStream_t>(stream));
  if (rc != 0) return fail(D3D_EHIP, "ncclAllGather failed");
  return D3D_OK;
}

int d3d_tta_mpjpe(const float* pred, const float* pred_flip, const float* gt, const uint8_t* mask, float scale,
                  const int32_t* jl, const int32_t* jr, int32_t n_lr, float* merged, double* sums, int32_t B, int32_t T,
                  int32_t J, void* stream) {
  if (!pred || !gt || !sums || B <= 0 || T <= 0 || J <= 0) return fail(D3D_EINVAL, "bad argument");
  if (J > JointPerm::MAXJ) return fail(D3D_EUNSUP, "more than 64 joints");
  if (pred_flip && n_lr > 0 && (!jl || !jr)) return fail(D3D_EINVAL, "joint lists required");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  JointPerm perm{};
  for (int j = 0; j < J; ++j) perm.p[j] = j;
  for (int i = 0; i < n_lr; ++i) {  // RUN:584-585: pf[:, :, left+right] = pf[:, :, right+left]
    if (jl[i] < 0 || jl[i] >= J || jr[i] < 0 || jr[i] >= J) return fail(D3D_EINVAL, "joint index out of range");
    perm.p[jl[i]] = jr[i];
    perm.p[jr[i]] = jl[i];
  }
  HIP_TRY(launch_tta_mpjpe(pred, pred_flip, gt, mask, scale, perm, merged, sums, B, T, J, s));   // asynchronous on `stream`
  return D3D_OK;
}

int d3d_pose_metrics(const float* pred, const float* gt, const uint8_t* mask, double* sums, int32_t N, int32_t J, void* stream) {
  if (!pred || !gt || !sums || N <= 0 || J <= 0) return fail(D3D_EINVAL, "bad argument");
  if (J > JointPerm::MAXJ) return fail(D3D_EUNSUP, "more than 64 joints");
  HIP_TRY(launch_pose_metrics(pred, gt, mask, sums, N, J, reinterpret_cast<hipStream_t>(stream)));   // asynchronous on `stream`
  return D3D_OK;
}

int d3d_num_windows(int32_t n_frames, int32_t T) { return (n_frames < 1 || T < 1) ? 0 : (n_frames + T - 1) / T; }

int d3d_window_gather(const float* seq, int32_t n_frames, int32_t T, int32_t J, int32_t C, int32_t flip, const int32_t* jl,
                      const int32_t* jr, int32_t n_lr, float* out, uint8_t* mask, void* stream) {
  if (!seq || !out || n_frames < 1 || T < 1 || J < 1 || C < 1) return fail(D3D_EINVAL, "bad argument");
  if (J > JointPerm::MAXJ) return fail(D3D_EUNSUP, "more than 64 joints");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  JointPerm perm{};
  for (int j = 0; j < J; ++j) perm.p[j] = j;
  if (flip)
    for (int i = 0; i < n_lr; ++i) {  // GEN:274-275: batch[:, left+right] = batch[:, right+left]
      if (!jl || !jr || jl[i] < 0 || jl[i] >= J || jr[i] < 0 || jr[i] >= J) return fail(D3D_EINVAL, "joint index out of range");
      perm.p[jl[i]] = jr[i];
      perm.p[jr[i]] = jl[i];
    }
  HIP_TRY(launch_window_gather(seq, out, mask, perm, n_frames, T, J, C, flip ? 1 : 0, s));
  return D3D_OK;
}

int d3d_window_gather_s2f(const float* seq, int32_t n_frames, int32_t T, int32_t J, int32_t C, int32_t flip, const int32_t* jl,
                          const int32_t* jr, int32_t n_lr, int32_t first, int32_t count, float* out, void* stream) {
  if (!seq || !out || n_frames < 1 || T < 1 || J < 1 || C < 1) return fail(D3D_EINVAL, "bad argument");
  if (!(T & 1)) return fail(D3D_EINVAL, "seq2frame windows need an odd number of frames (pad = (T - 1) / 2 on each side)");
  if (first < 0 || count < 1 || first + (int64_t)count > n_frames) return fail(D3D_EINVAL, "window range outside the sequence");
  if (J > JointPerm::MAXJ) return fail(D3D_EUNSUP, "more than 64 joints");
  JointPerm perm{};
  for (int j = 0; j < J; ++j) perm.p[j] = j;
  if (flip)
    for (int i = 0; i < n_lr; ++i) {
      if (!jl || !jr || jl[i] < 0 || jl[i] >= J || jr[i] < 0 || jr[i] >= J) return fail(D3D_EINVAL, "joint index out of range");
      perm.p[jl[i]] = jr[i];
      perm.p[jr[i]] = jl[i];
    }
  HIP_TRY(launch_window_gather_s2f(seq, out, perm, n_frames, T, J, C, first, count, flip ? 1 : 0, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

// ---- F16X3 range guard ----------------------------------------------------------------------------------------------
int d3d_engine_range_flags(d3d_engine* e, uint32_t* flags, int32_t clear, void* stream) {
  if (!e || !flags) return fail(D3D_EINVAL, "null argument");
  if (!e->committed) return fail(D3D_ESTATE, "weights not committed");
  HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)));
  unsigned w = 0;
  HIP_TRY(hipMemcpy(&w, e->range_dev, sizeof(unsigned), hipMemcpyDeviceToHost));
  if (clear && w) HIP_TRY(hipMemset(e->range_dev, 0, sizeof(unsigned)));
  *flags = range_bits_to_abi(w, e->weights_clamped);
  return D3D_OK;
}

int d3d_engine_range_post(d3d_engine* e, void* stream, int64_t* ticket) {
  if (!e || !ticket) return fail(D3D_EINVAL, "null argument");
  if (!e->committed) return fail(D3D_ESTATE, "weights not committed");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  HIP_TRY(hipStreamIsCapturing(s, &cs));
  if (cs != hipStreamCaptureStatusNone) return fail(D3D_ESTATE, "d3d_engine_range_post inside a stream capture");
  const long long t = e->range_posted;
  const int slot = (int)(t % d3d_engine::RANGE_TICKETS);
  e->range_host[slot] = 0;   // (the slot's previous ticket is RANGE_TICKETS posts old: no longer readable, see _take)
  HIP_TRY(launch_range_snapshot(e->range_dev, e->range_host_dev + slot, s));
  HIP_TRY(hipEventRecord(e->range_ev[slot], s));
  e->range_posted = t + 1;
  *ticket = t;
  return D3D_OK;
}

int d3d_engine_range_take(d3d_engine* e, int64_t ticket, int32_t block, uint32_t* flags, int32_t* ready) {
  if (!e || !flags || !ready) return fail(D3D_EINVAL, "null argument");
  if (ticket < 0 || ticket >= e->range_posted) return fail(D3D_EINVAL, "no such range ticket");
  if (ticket + d3d_engine::RANGE_TICKETS <= e->range_posted) return fail(D3D_EINVAL, "range ticket expired (256 are kept)");
  const int slot = (int)(ticket % d3d_engine::RANGE_TICKETS);
  *ready = 0;
  if (block) {
    HIP_TRY(hipEventSynchronize(e->range_ev[slot]));
  } else {
    const hipError_t q = hipEventQuery(e->range_ev[slot]);
    if (q == hipErrorNotReady) { (void)hipGetLastError(); return D3D_OK; }
    HIP_TRY(q);
  }
  const unsigned w = __atomic_load_n(&e->range_host[slot], __ATOMIC_ACQUIRE);
  if (!(w & 0x80000000u)) return fail(D3D_EHIP, "range snapshot slot not written behind its event");
  *flags = range_bits_to_abi(w, e->weights_clamped);
  *ready = 1;
  return D3D_OK;
}

// ---- debug trace ----------------------------------------------------------------------------------------------------
int d3d_engine_set_trace(d3d_engine* e, int32_t capacity, int32_t views) {
  if (!e || capacity < 0 || views < 1 || views > 8) return fail(D3D_EINVAL, "bad argument");
  e->trace_views = views;
  e->trace_dev.reset();
  e->trace_cap = e->trace_n = e->trace_fwd = 0;
  e->trace_tags.clear();
  e->tracing = capacity > 0;
  if (e->tracing) {
    HIP_TRY(e->trace_dev.alloc((size_t)capacity));
    HIP_TRY(hipMemset(e->trace_dev, 0, (size_t)capacity * sizeof(unsigned long long)));
    e->trace_cap = capacity;
  }
  return D3D_OK;
}

int d3d_engine_trace_read(d3d_engine* e, uint64_t* sums_host, uint32_t* tags_host, int32_t cap, int32_t* n, void* stream) {
  if (!e || !sums_host || !tags_host || !n || cap < 0) return fail(D3D_EINVAL, "bad argument");
  if (!e->tracing) return fail(D3D_ESTATE, "trace is off (d3d_engine_set_trace)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipStreamSynchronize(s));
  const int cnt = std::min(e->trace_n, (int)cap);
  if (cnt) HIP_TRY(hipMemcpy(sums_host, e->trace_dev, (size_t)cnt * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  for (int i = 0; i < cnt; ++i) tags_host[i] = e->trace_tags[i];
  *n = cnt;
  HIP_TRY(hipMemset(e->trace_dev, 0, (size_t)e->trace_cap * sizeof(unsigned long long)));
  e->trace_n = e->trace_fwd = 0;
  e->trace_tags.clear();
  return D3D_OK;
}

// ---- profiling ------------------------------------------------------------------------------------------------------
int d3d_engine_set_profiling(d3d_engine* e, int32_t on) {
  if (!e) return fail(D3D_EINVAL, "null engine");
  e->profiling = on != 0;
  return D3D_OK;
}

int d3d_engine_profile_reset(d3d_engine* e) {
  if (!e) return fail(D3D_EINVAL, "null engine");
  for (auto& r : e->recs) { e->ev_pool.push_back(r.a); e->ev_pool.push_back(r.b); }
  e->recs.clear();
  for (int c = 0; c < D3D_KC_COUNT; ++c) { e->prof_ms[c] = e->prof_flops[c] = e->prof_bytes[c] = 0; e->prof_launches[c] = 0; }
  return D3D_OK;
}

int d3d_engine_profile_read(d3d_engine* e, int32_t cls, double* total_ms, int64_t* launches, double* flops, double* bytes) {
  if (!e || cls < 0 || cls >= D3D_KC_COUNT) return fail(D3D_EINVAL, "bad kernel class");
  for (auto& r : e->recs) {  // resolve pending event pairs (blocks until they have completed)
    HIP_TRY(hipEventSynchronize(r.b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, r.a, r.b));
    e->prof_ms[r.cls] += ms; e->prof_flops[r.cls] += r.flops; e->prof_bytes[r.cls] += r.bytes; e->prof_launches[r.cls] += 1;
    if (r.cls2 >= 0) {   // the same launch under its GEMM sub-class (qkv / proj / fc1 / fc2)
      e->prof_ms[r.cls2] += ms; e->prof_flops[r.cls2] += r.flops; e->prof_bytes[r.cls2] += r.bytes; e->prof_launches[r.cls2] += 1;
    }
    e->ev_pool.push_back(r.a); e->ev_pool.push_back(r.b);
  }
  e->recs.clear();
  if (total_ms) *total_ms = e->prof_ms[cls];
  if (launches) *launches = e->prof_launches[cls];
  if (flops) *flops = e->prof_flops[cls];
  if (bytes) *bytes = e->prof_bytes[cls];
  return D3D_OK;
}

const char* d3d_kernel_class_name(int32_t cls) {
  static const char* names[D3D_KC_COUNT] = {"linear", "attn_spatial", "attn_temporal", "layernorm", "embed", "head", "other",
                                            "linear_qkv", "linear_proj", "linear_fc1", "linear_fc2", "qkv_sattn", "qkv_tattn"};
  return (cls >= 0 && cls < D3D_KC_COUNT) ? names[cls] : "?";
}

// ---- single-op hooks that read engine fields (the others: engine_ops.hip) -----------------------------------------------
int d3d_op_time_embedding(d3d_engine* e, const float* times_dev, int32_t n, float* out, float* scratch, void* stream) {
  if (!e || !times_dev || !out || !scratch || n <= 0) return fail(D3D_EINVAL, "bad argument");
  if (!e->committed) return fail(D3D_ESTATE, "weights not committed");
  if (!e->Dt) return fail(D3D_ESTATE, "engine was built with with_time_emb = 0");
  RangeScope range_scope(e);
  return compute_temb(e, times_dev, n, out, scratch, reinterpret_cast<hipStream_t>(stream));
}

int d3d_op_head(d3d_engine* e, const float* X, float* x0, int32_t rows, void* stream) {
  if (!e || !X || !x0 || rows < 1) return fail(D3D_EINVAL, "bad argument");
  if (!e->committed) return fail(D3D_ESTATE, "weights not committed");
  HeadArgs h{};
  h.g = e->hd_g; h.b = e->hd_b; h.eps = 1e-5f; h.Wh = e->hd_w; h.bh = e->hd_bias; h.D = e->D;
  h.X = X; h.rows = rows; h.x0_raw = x0; h.mode = 0;
  HIP_TRY(launch_head(h, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

}  // extern "C"
