/*
 * d3d.h -- C ABI of libd3d_hip.so, the MI355X (gfx950) engine for Diff3DHPE's DDIM sampling hot path.
 *
 * The reference (csiro-icvg/Diff3DHPE) is pure Python and has no FFI/plugin interface; its boundary for this
 * path is the Python object protocol of two classes.  Each entry point below names the reference code it
 * replaces (paths relative to the reference root):
 *   DIFF = common/conditional_diffusion_ddim_normal_directPredict_variableLoss_both_crossFrames.py
 *   DIFF-S2F = common/conditional_diffusion_s2f_ddim_normal_directPredict_variableLoss_both_crossFrames.py
 *   S2S  = common/nets/model_conditional_diffusion_mixste_s2s_grand_linLift.py
 *   S2F  = common/nets/model_conditional_diffusion_mixste_s2f_grand_linLift.py
 *   LOSS = common/loss.py,  RUN = run_conditionalDiffusionDDIM3dhpeNormalDirectPredictVariableLoss.py
 *
 * Conventions
 *   - plain C types only; every pointer marked "dev" is a device (HBM) pointer owned by the caller;
 *     "host" pointers are ordinary host memory.  `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every function returns 0 on success, a negative D3D_E* code on failure; d3d_last_error() gives the message
 *     (thread-local).  No exception crosses the ABI.  Nothing here falls back to a CPU implementation: without a
 *     HIP device the compute entry points fail with D3D_EHIP.
 *   - one engine per device; see "Threads" below.
 *   - tensors are row-major fp32: x2d (B,T,J,in_chans), y / x0 / out (B,T,J,3) [(B,1,J,3) for seq2frame].
 */
#ifndef D3D_H_
#define D3D_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define D3D_OK 0
#define D3D_EINVAL (-1)   /* bad argument / shape                        */
#define D3D_ESTATE (-2)   /* call order (weights not committed, ...)     */
#define D3D_EHIP (-3)     /* HIP runtime error or no device              */
#define D3D_ENOMEM (-4)   /* workspace too small                         */
#define D3D_EUNSUP (-5)   /* configuration outside what the kernels support */

#define D3D_PREC_FP32 0     /* exact fp32: v_mfma_f32_32x32x2_f32, fp32 everywhere (parity mode) */
#define D3D_PREC_F16X3 1    /* fp32-accurate GEMMs and attention from 3 fp16 MFMAs per product on hi/lo operand splits; the
                             * residual stream lives in the GEMM operand layout and norm1/norm2 are folded into the qkv/fc1
                             * GEMMs.  Same 1e-4 parity gate as FP32 INSIDE its operand range (range guard below); the engine the
                             * Python layer's default precision "auto" starts on -- it reads the guard after every call and repeats a flagged
                             * call on a D3D_PREC_FP32 engine. */
#define D3D_PREC_BF16 2     /* SECOND-CLASS precision (BASELINE configs[1]): bf16 operands for the block GEMMs
                             * and both attention products (one MFMA per product), everything else fp32 (residual stream, LayerNorm /
                             * softmax statistics, GELU, time vectors, embedding, head, DDIM update).  It CANNOT meet the 1e-4 parity
                             * gate (bf16 operands cost ~5e-2 max-abs at random init); it is gated against the CPU
                             * oracle's bf16-operand emulation instead (same rounding points).  Needs head_dim 64, num_frame <= 256,
                             * num_joints <= 32, widths % 64 == 0; never the default of the Python layer or of bench.py. */
#define D3D_PREC_F16 3      /* SECOND-CLASS like D3D_PREC_BF16, and the same engine: fp16 operands at bf16's rounding points (LayerNorm
                             * output, q / k / v with the exact q pre-scale 2^-3, softmax - I, attention output, GELU output, weights at
                             * commit), the f16 twin of each bf16 MFMA, the same kernels instantiated for the other element type.  Three
                             * more mantissa bits: about an eighth of the bf16 mode's distance to fp32, still
                             * outside the 1e-4 gate; gated against the oracle's fp16-operand emulation.  Every conversion rounds to
                             * nearest even and keeps fp16 subnormals, as torch's .to(float16); the operands are UNSCALED and there is NO
                             * range guard: a finite value beyond +-65504 at a rounding point becomes +-inf (a weight: the commit reports
                             * it as it reports a non-finite weight).  Admission, workspace, options and info keys are the bf16 mode's:
                             * "fused_spatial", "fused_temporal", "fused_postnorm", "bf16_gemm_kernel" and "bf16_fused_*_last" serve both
                             * 16-bit operand modes -- wherever this header says "BF16 mode / engines" of an option it holds for
                             * D3D_PREC_F16 engines too.  Never chosen by the Python layer's "auto". */

/*
 * Threads
 *   - Distinct engines may be driven from distinct host threads concurrently, on one device or on several: an engine owns its weights,
 *     tables, streams, events, graph cache, ticket ring and range-guard word, every option is a field of the engine, and the launch
 *     context of a call (range word, "deep_stages", tail slices) is thread-local.  What the library keeps per process is written once
 *     per device and idempotently (the LDS opt-in bits, the CU-count caches, the range sink word, the cached ncclAllGather pointer)
 *     or is a plain atomic default (the NULL-engine form of "deep_stages").
 *   - ONE engine is driven by ONE thread at a time: every entry point that takes a d3d_engine* reads or writes its state without a
 *     lock, and two concurrent calls would share one workspace.  The Python layer enforces this with a lock per engine
 *     (Engine.lock); a C caller must serialise its calls per engine itself.  A ticket of d3d_engine_range_post covers the launches
 *     since the previous post, so a caller that wants a ticket to describe ITS call keeps the engine from before the launch until
 *     the post has returned.
 *   - d3d_last_error() is per thread: it returns the message of the calling thread's most recent failed call.
 */
typedef struct d3d_engine d3d_engine;

/* Shape-defining constructor arguments of the denoiser (S2S:140-142 / S2F ctor; runner passes them at RUN:178-180). */
typedef struct d3d_config {
  int32_t num_frame;     /* T  */
  int32_t num_joints;    /* J  */
  int32_t in_chans;      /* 2  */
  int32_t embed_dim;     /* D  */
  int32_t depth;         /* number of (spatial, temporal) block pairs */
  int32_t num_heads;     /* H  */
  int32_t mlp_hidden;    /* int(D * mlp_ratio) */
  int32_t with_time_emb; /* 0/1: 0 removes every time_mlp (S2S:163-177,104-107) */
  int32_t seq2frame;     /* 0 = ...S2S..., 1 = ...S2F... (LOADNET:5-10) */
  int32_t precision;     /* D3D_PREC_* */
} d3d_config;

const char* d3d_last_error(void);
int d3d_version(void);

/* ---- construction: replaces HPE_model(name)(**kw) + GaussianDiffusion(model=...) (RUN:176-189) ------------------- */
/* Head widths embed_dim / num_heads of 4, 8, 16, 32, 48, 64, 96 and 128 (D3D_PREC_BF16: 64 alone), embed_dim a multiple of 32 and
 * <= 1024; anything else: D3D_EUNSUP.  One exception to the multiple of 32: an odd number of heads of 48 columns (embed_dim 48, 144, ...:
 * a multiple of 16).  The fp16 plane forms of the GEMMs do not exist there (32-deep k-tiles, activations in groups of 32 columns), so
 * such an engine runs the FP32 kernels whether D3D_PREC_FP32 or D3D_PREC_F16X3 was asked for -- the exact arithmetic, the fp32 GEMM
 * zero-filling its last k-tile of 16 columns -- and D3D_PREC_BF16 refuses it.  Widths 48 and 96 (embed_dim 384 / 768 with the runner's 8 heads) run the fp16-MFMA attention
 * kernels of those widths on a D3D_PREC_F16X3 engine (option "attn_hx") and the exact fp32 MFMA attention kernels of those widths on a
 * D3D_PREC_FP32 engine (option "attn_f32_hx").  Width 128 (embed_dim 1024 with the runner's 8 heads) runs the fp16-MFMA attention kernels of that width on a
 * D3D_PREC_F16X3 engine (option "attn_h128") and the exact fp32 MFMA attention kernels of that width on a D3D_PREC_FP32 engine
 * (option "attn_f32_h128"). */
int d3d_engine_create(const d3d_config* cfg, d3d_engine** out);
void d3d_engine_destroy(d3d_engine* e);

/* Number of weight tensors the engine expects, and the i-th expected name / element count (reference state_dict keys
 * without the "model." prefix, e.g. "STEblocks.3.attn.qkv.weight"; S2S:160-220, S2F:216-218). */
int d3d_engine_num_weights(const d3d_engine* e);
int d3d_engine_weight_info(const d3d_engine* e, int i, const char** name, int64_t* numel);

/* Copy one fp32 tensor (host memory, torch layout) into the engine; replaces load_state_dict (RUN:226-235). */
int d3d_engine_set_weight(d3d_engine* e, const char* name, const float* host, int64_t numel);
/* Optional: the (D/2,) frequency table of SinusoidalPosEmb (S2S:29-36) as the host framework computes it; without it
 * the engine uses exp() in double rounded to fp32 (differs from torch's expf in ~1 of 256 entries by 1 ulp). */
int d3d_engine_set_time_freqs(d3d_engine* e, const float* host, int32_t n);
/* Verify every tensor was supplied, upload + repack to kernel layouts.  Must precede any compute call. */
int d3d_engine_commit_weights(d3d_engine* e);

/* Diffusion constants: fp32 buffers `alphas_cumprod` and `sqrt_one_minus_alphas_cumprod` (num_timesteps,) as registered
 * at DIFF:151-161, plus sampling_timesteps / ddim_sampling_eta / clip_denoised (DIFF:100-112).  Builds the integer DDIM
 * schedule (DIFF:270-273) and the per-step time-embedding table (S2S:169-174,104-107).  Weights must be committed. */
int d3d_engine_set_schedule(d3d_engine* e, int32_t num_timesteps, const float* alphas_cumprod_host,
                            const float* sqrt_one_minus_alphas_cumprod_host, int32_t sampling_timesteps, float eta,
                            int32_t clip_denoised, void* stream);

/* Optional fp32 buffer `sqrt_alphas_cumprod` (DIFF:155) -- needed only by d3d_q_sample.  Call after set_schedule. */
int d3d_engine_set_sqrt_alphas_cumprod(d3d_engine* e, const float* host, int32_t n);

/* Host-only, bit-exact restatement of `torch.linspace(-1, N-1, S+1).int()` reversed (DIFF:270-272): writes S+1 values. */
int d3d_ddim_times(int32_t num_timesteps, int32_t sampling_timesteps, int32_t* out);

/* Bytes of device scratch the compute calls need for a batch of B sequences. */
size_t d3d_workspace_bytes(const d3d_engine* e, int32_t B);

/* ---- compute: all asynchronous on `stream` ------------------------------------------------------------------------ */
/* B >= 1 (D3D_EINVAL otherwise): a rank whose shard of a batch is empty skips the call, as the host layer does
 * (diff3dhpe_amd/engine.py returns the empty tensor the reference's torch ops would, evaluate.py does not call). */

/* forward_denoise (S2S:249-257 / S2F:253-266) on cat([x2d, y], -1) (DIFF:255).  times_dev: n_times fp32 timesteps on
 * the device, n_times == 1 (broadcast, the sampling case DIFF:254) or == B (per-row, the p_losses case DIFF:392-408).
 * Ignored when with_time_emb == 0.  y is (B,y_frames,J,3) with y_frames == T, or == 1 to have the kernel broadcast one
 * frame over T (the seq2frame repeat of DIFF-S2F:281).  x0 receives the raw network output (no clamp):
 * (B,T,J,3), or (B,1,J,3) for a seq2frame engine. */
int d3d_denoise(d3d_engine* e, const float* x2d_dev, const float* y_dev, int32_t y_frames, const float* times_dev,
                int32_t n_times, float* x0_dev, int32_t B, void* ws_dev, size_t ws_bytes, void* stream);

/* ddim_sample_loop (DIFF:262-300; DIFF-S2F:263-300).  init_noise replaces torch.randn(target_shape) (DIFF:275);
 * step_noise_dev (nullable; required when eta != 0) is (S, B,T',J,3): the per-step randn_like draws (DIFF:293).
 * traj_rev_dev / traj_x0_dev (nullable) receive x_reverse_diffusion / x_start_est stacked on the last axis,
 * shape (B,T',J,3,S) (DIFF:303-347).  out: (B,T',J,3); T' = 1 for seq2frame else T. */
int d3d_ddim_sample(d3d_engine* e, const float* x2d_dev, const float* init_noise_dev, const float* step_noise_dev,
                    float* out_dev, float* traj_rev_dev, float* traj_x0_dev, int32_t B, void* ws_dev, size_t ws_bytes,
                    void* stream);

/* hipGraph replay of d3d_ddim_sample: when enabled (and eta == 0, no trajectory capture, profiling off) the whole S-step
 * launch sequence is captured once per (B, workspace pointer) and replayed with one hipGraphLaunch per call; inputs and
 * the result go through staging buffers inside the workspace.  Weights / schedule changes drop the captured graphs.  At most
 * FOUR captured graphs are kept per engine: a fifth (B, workspace) pair evicts the least recently used one (a caller that
 * re-allocates its workspace per batch re-captures every time, but does not accumulate graphs). */
int d3d_engine_set_graph_mode(d3d_engine* e, int32_t on);

/* Explicit switches (the library reads NO environment variables).  Engine options (results stay within the parity gate either way;
 * used by the A/B scripts under experiments/ and by tests that exercise the alternative flows):
 *   "fused_postnorm"  1 (default) / 0: F16X3 block flow with the block's post-norm inside the fc2 GEMM epilogue / as a row kernel
 *   "fold_layernorm"  1 (default) / 0: F16X3 flow with norm1 / norm2 folded into the qkv / fc1 GEMMs / as row kernels
 *   "fused_spatial"   1 (default) / 0: F16X3 flow, spatial blocks (15, 16 or 17 joints of a frame, D = 512, 8 heads): the qkv GEMM of a
 *                     group of 15 frames (17 joints; 16 frames of 15 or 16 joints) keeps q / k / v in LDS and runs the frames' attention in
 *                     the same kernel (S2S:67 + 73-83; the q / k / v planes never go to HBM) / qkv GEMM and attention as two kernels.
 *                     Bit-identical either way.  Other joint counts keep the two kernels whatever the key says.  "fused_spatial_last"
 *                     (d3d_engine_get_info) reports what the latest forward ran.
 *   "fused_temporal"  1 (default) / 0: the same for the temporal blocks where the frames of a joint fit one 256-row tile (193 <= T <= 255,
 *                     D = 512, 8 heads): the qkv GEMM of one (batch, joint) group keeps K / V in LDS, exchanges the queries there and runs
 *                     the group's T-key attention in the same kernel (S2S:67 + 73-83 for the per-joint groups) / two kernels.  Bit-identical.
 *                     T <= 127: the frames of 255 / T joints of one batch element per tile, every query on its own joint's keys -- as
 *                     accurate as the two-kernel flow but not bit-identical to it (sums grouped by tile position); a batch element's
 *                     result does not depend on its position in the batch either way.
 *                     BF16 mode: both keys select, for their block type, the bf16 qkv GEMM + attention as ONE kernel (a tile of
 *                     floor(255 / N) whole groups of N tokens x one head; q / k / v are rounded to bf16 where the qkv GEMM rounds them and
 *                     stay in LDS; the attention output goes to the workspace region the q / k / v tensor would have taken) / as two
 *                     kernels.  Shapes: head width 64, D % 128 == 0, D >= 256, T <= 255, J <= 32; others keep the two kernels whatever
 *                     the keys say.  Bit-identical either way, for every T, non-finite activations included (a group's pad keys are
 *                     masked to zeros in registers: a sequence's result depends on its own rows only).  "bf16_fused_spatial_last" / "bf16_fused_temporal_last"
 *                     (d3d_engine_get_info) report what the latest forward ran.
 *   "block0_direct"   1 (default) / 0: F16X3 folded flow, block 0 (D = 512, 15, 16 or 17 joints, 8 heads, in_chans <= 3): its input rows are W_e u + b_e + spos[j] + tv[b]
 *                     with u the in_chans + 3 raw channels of a token, so q / k / v follow from commit-time tables (G = Wg W_e, P[j] =
 *                     Wg (b_e + spos[j]), fp64 sums stored as fp32) and one time row per forward (Q = Wg tv, in the caller's workspace) with
 *                     in_chans + 3 fmas and two adds per value: block 0 runs no qkv GEMM / 0: the K = 512 GEMM like every other block.
 *                     Both "fused_spatial" settings take the same fill function: bit-identical to each other; against 0 the results move
 *                     in the last bits (inside the parity gate).  "block0_direct_last" (d3d_engine_get_info) reports what ran.
 *   "fc1_kernel"      1 (default) / 0: fc1 (LayerNorm-folded, GELU) on its own kernel -- the hand-specialised k-loop of the fused kernels
 *                     with the token GEMM's own epilogue function, from two rounds of 256 x 256 tiles on -- / as a form of the token GEMM.
 *                     Bit-identical.
 *   "proj_kernel"     1 (default) / 0: the same for proj (192 x 256 tiles; rows behind the last whole tile through the token GEMM).
 *   "bf16_gemm_kernel" 1 (default) / 0: BF16 mode, qkv and fc1 on their own kernel (the hand-specialised two-phase k-loop with one bf16
 *                     MFMA per fragment pair, from two rounds of 256 x 256 tiles on) / as forms of the token GEMM.  Bit-identical.
 *   "head_fence"      0 (default) / 1: the head kernel evaluates every row's three dot products twice from independently loaded weight
 *                     fragments, compares them bit for bit, repairs a disagreement by a third evaluation and raises D3D_RANGE_RECOMPUTE
 *                     (round 5's default against a deviation seen on a GPU shared by two processes; since round 6 that deviation is
 *                     identified -- one packed fp32 instruction form beside another wave's MFMAs -- and pinned out of every kernel at
 *                     build time, so the second evaluation is optional: +0.08 ms per launch of 0.21)
 *   "head_inject"     0 (default) / 1, tests only (implies "head_fence"): the head kernel perturbs the first of its two evaluations of
 *                     row 0 -- the fence must repair the row (result unchanged) and raise D3D_RANGE_RECOMPUTE
 *   "norm_eps_bits"   the bit pattern of the float eps of the constructor's norm_layer (S2S:184; default 1e-6): norm1 / norm2 of every block
 *                     and the two post-norms; the head's LayerNorm keeps 1e-5 (S2S:218).  The Python classes set it from
 *                     norm_layer=partial(nn.LayerNorm, eps=...)
 *   "streams"         2 (default) / 1: d3d_ddim_sample runs a batch of B >= 2 as two half-batches on two HIP streams (the caller's and
 *                     one the engine owns, forked and joined by events: the caller sees ONE asynchronous operation on its stream;
 *                     bit-identical to one stream -- every output element is independent of the batch it is computed in; measured
 *                     +2.9 % at T=243 / B=64, neutral at T=81 / T=27).  Per-kernel profiling and the trace force one stream.
 *   "latency_mode"    0 (default) / 1: F16X3 flow, small calls.  Where the whole-row fc2 + post-norm launch cannot fill one round of
 *                     the chip (ceil(M / 64) workgroups < CU count; embedding width 512), each of its workgroups stages all of W2 alone and
 *                     the launch lasts K / 32 k-tiles whatever M.  With the mode on such a forward runs fc2 as a split-K x split-N GEMM
 *                     (128 x 128 tiles, S k-ranges, fp32 partials in workspace regions that are dead at that point) followed by a row kernel
 *                     that adds residual, bias and the partials in a fixed order and applies the post-norm.  S in {2, 4} is a function of
 *                     (M, D, mlp_hidden, CU count) alone -- the same for eager and captured runs; where the rule gives S = 1 (larger
 *                     calls) exactly the default kernels run.  The order of additions differs from the default path's: results stay within
 *                     the parity gate but are NOT bit-identical to the default, nor across calls that get different S; a sequence's
 *                     result is bit-identical across calls that get the same S.  d3d_workspace_bytes does not change.  "fc2_split_last"
 *                     (d3d_engine_get_info) reports the S of the latest forward.  Other precisions ignore it.
 *                     The mode covers proj and fc1 of such a forward too (embedding width 512): each may run as the same split GEMM
 *                     (proj: partials in the workspace's q / k / v and hidden-activation regions, dead at that point; fc1: in a buffer the
 *                     engine owns -- 32 MiB, a second one for the second half-batch of a two-stream sampling -- allocated when the mode
 *                     is switched on and freed when it is switched off or the engine destroyed) plus a row kernel that adds the partials
 *                     in a fixed order and applies the launch's own epilogue (proj: residual, stream planes, row statistics; fc1: the
 *                     folded LayerNorm, GELU, hidden planes).  Each has its own rule, a function of (M, N, K, CU count) alone that
 *                     compares the split against the launch it replaces; "proj_split_last" / "fc1_split_last" report what ran.  A
 *                     sequence's result is bit-identical across calls that get the same three S.
 *   "long_temporal"   1 (default) / 0: F16X3 engines with num_frame > 256.  No F16X3 attention kernel holds the keys of such a window in
 *                     LDS; with the key on, the engine keeps its folded flow (LayerNorm-folded GEMMs, plane-resident residual stream, fused
 *                     spatial qkv + attention, block 0 direct, fc2 + post-norm) and the temporal blocks run the folded qkv GEMM followed by
 *                     the key-streaming attention kernel (keys pass through LDS in chunks of 256 frames, the scores are computed twice: the
 *                     exact two-pass softmax of every other form) / 0: the plain row-kernel flow with the generic fp32 attention kernel,
 *                     as before version 135.  The two differ in the last bits, both inside the parity gate.  num_frame <= 256, FP32 and
 *                     BF16 engines: no effect.  d3d_workspace_bytes does not change.  "long_temporal_last" (d3d_engine_get_info) reports
 *                     what the latest forward ran.
 *   "long_temporal_f32"  1 (default) / 0: FP32 engines with num_frame > 256 (the engine a precision-"auto" model falls back to, and the exact
 *                     reference arithmetic).  The resident fp32 MFMA attention kernel holds K and V of at most 256 frames in LDS; with the key
 *                     on, the temporal blocks of such an engine run the key-streaming fp32 kernel (v_mfma_f32_32x32x2_f32, keys pass
 *                     through LDS in chunks of 256 frames, three passes: maximum, sum, normalised product -- the resident kernel's
 *                     arithmetic in its order, the diagonal's - v[query] applied at the store instead of inside the product) / 0: the generic one-thread-per-row kernel, as before version 136.  The two differ in the
 *                     last bits, both inside the parity gate.  num_frame <= 256, F16X3 and BF16 engines: no effect.  d3d_workspace_bytes
 *                     does not change.  "long_temporal_f32_last" (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_h32"        1 (default) / 0: F16X3 engines whose heads are 32 columns wide with an even head count (embed_dim 256 with the
 *                     runner's 8 heads) and num_frame <= 256.  Every other F16X3 attention kernel needs embed_dim == 64 num_heads; with
 *                     the key on, such an engine runs the folded flow (LayerNorm-folded GEMMs, plane-resident residual stream; the fused
 *                     qkv + attention kernels, block 0 direct and the post-norm in fc2 stay off at this width by their own rules) with the
 *                     attention of every block on the fp16-MFMA kernel for that width: two adjacent heads share the 128-byte LDS rows of
 *                     the 64-wide kernels, the exact two-pass softmax of every other form / 0: the plain row-kernel flow with the generic
 *                     fp32 attention kernel, as before version 139.  The two differ in the last bits, both inside the parity gate.
 *                     num_frame > 256, every embed_dim == 64 num_heads engine, FP32 and BF16 engines: no effect.  d3d_workspace_bytes
 *                     does not change.  "attn_h32_last" (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_f32_h32"    1 (default) / 0: FP32 engines whose heads are 32 columns wide (embed_dim 256 with the runner's 8 heads; any head
 *                     count) -- the exact reference arithmetic, and the engine a precision-"auto" model falls back to.  The fp32
 *                     MFMA / LDS attention kernels need embed_dim == 64 num_heads; with the key on, the spatial blocks of such an engine
 *                     (15 to 17 joints) and its temporal blocks (num_frame <= 256) run the exact fp32 kernels of that width
 *                     (temporal: v_mfma_f32_32x32x2_f32, K and V resident in LDS, exact two-pass softmax; spatial: one lane per query
 *                     row, K and V broadcast from LDS; the scores scaled by 1 / sqrt(32) after the sum, v[query] of the diagonal
 *                     subtracted at the store) / 0: the generic one-thread-per-row kernel, as before version 140.  The two differ in
 *                     the order of additions, so in the last bits, both inside the parity gate.  Other joint counts, num_frame > 256
 *                     (that block type keeps the generic kernel), every embed_dim == 64 num_heads engine, F16X3 and BF16 engines: no
 *                     effect.  d3d_workspace_bytes does not change.  "attn_f32_h32_last" (d3d_engine_get_info) reports what the latest
 *                     forward ran.
 *   "long_temporal_h32"  1 (default) / 0: F16X3 engines whose heads are 32 columns wide with an even head count and num_frame > 256, which
 *                     "attn_h32" does not cover.  With the key on, such an engine keeps the folded flow of "attn_h32": its spatial blocks
 *                     on the fp16-MFMA kernel of that width (groups of num_joints <= 256 tokens) and its temporal blocks on the
 *                     key-streaming kernel of that width (a head pair's keys pass through LDS in chunks of 256 frames, the scores are
 *                     computed twice: the exact two-pass softmax of every other form, bit-identical to the resident kernel wherever that
 *                     runs) / 0: the plain row-kernel flow with the generic fp32 attention kernel in every block, as before version 141.
 *                     The two differ in the last bits, both inside the parity gate.  A 9-step sampling at depth 8, num_frame 300: 43.0
 *                     -> 11.2 ms at B = 1, 1168 -> 308 ms at B = 64.  num_frame <= 256, every embed_dim == 64 num_heads
 *                     engine, FP32 and BF16 engines: no effect.  "attn_h32_last" and "long_temporal_last" stay 0 on such an engine.
 *                     d3d_workspace_bytes does not change.  "long_temporal_h32_last" (d3d_engine_get_info) reports what the latest
 *                     forward ran.
 *   "long_temporal_f32_h32"  1 (default) / 0: FP32 engines whose heads are 32 columns wide (any head count) and num_frame > 256, which the
 *                     temporal kernel of "attn_f32_h32" does not cover.  With the key on, the temporal blocks of such an engine run the
 *                     key-streaming fp32 kernel of that width (v_mfma_f32_32x32x2_f32, keys pass through LDS in chunks of 256 frames,
 *                     three passes: maximum, sum, normalised product -- the resident kernel's arithmetic in its order, bit-identical to
 *                     it wherever that runs) / 0: the generic one-thread-per-row kernel, as before version 141.  The two differ in the
 *                     order of additions, so in the last bits, both inside the parity gate.  A 9-step sampling at depth 8, num_frame 300:
 *                     54.3 -> 30.5 ms at B = 1, 1328 -> 734 ms at B = 64.  The spatial blocks go on choosing by
 *                     num_joints alone ("attn_f32_h32").  num_frame <= 256, every embed_dim == 64 num_heads engine, F16X3 and BF16
 *                     engines: no effect.  d3d_workspace_bytes does not change.  "long_temporal_f32_h32_last" (d3d_engine_get_info)
 *                     reports what the latest forward ran.
 *   "attn_h128"  1 (default) / 0: F16X3 engines whose heads are 128 columns wide (embed_dim == 128 num_heads, e.g. 1024 with 8 heads)
 *                     and num_joints <= 128.  With the key on, such an engine runs the folded flow with the two-kernel attention branch:
 *                     its spatial blocks and, for num_frame <= 128, its temporal blocks on the resident fp16-MFMA kernel of that width (a
 *                     head is two 64-column halves of the plane rows, one score chain and one softmax per head), its temporal blocks
 *                     for num_frame > 128 on the key-streaming kernel of that width (keys pass through LDS in chunks of 128 frames, the
 *                     scores are computed twice: the exact two-pass softmax of every other form, bit-identical to the resident kernel
 *                     wherever that runs) / 0: the plain row-kernel flow with the generic fp32 attention kernel in every block.  The
 *                     two differ in the last bits, both inside the parity gate.  A 9-step sampling at depth 8, embed_dim 1024,
 *                     num_frame 243: 187.5 -> 48.9 ms at B = 1, 6479 -> 1754 ms at B = 64.  Every other head
 *                     width, FP32 engines ("attn_f32_h128") and BF16 engines (refused at this width): no effect.
 *                     d3d_workspace_bytes does not change.  "attn_h128_last" (d3d_engine_get_info) reports what the latest forward
 *                     ran.
 *   "attn_f32_h128"   1 (default) / 0: FP32 engines whose heads are 128 columns wide (embed_dim == 128 num_heads, e.g. 1024 with 8
 *                     heads) -- the exact reference arithmetic, and the engine a precision-"auto" model falls back to.  With the key
 *                     on, the spatial blocks of such an engine (num_joints <= 128) and, for num_frame <= 128, its temporal blocks run
 *                     the resident exact fp32 kernel of that width (v_mfma_f32_32x32x2_f32, K and V of a group resident in LDS, the
 *                     scores scaled by 1 / sqrt(128) after the sum, exact two-pass softmax, the second product on the unnormalised
 *                     numerators, the division by their sum and v[query] of the diagonal at the store), its temporal blocks for
 *                     num_frame > 128 the key-streaming kernel of that width (keys pass through LDS in chunks of 128 frames, the
 *                     scores are computed twice -- the resident kernel's arithmetic in its order, bit-identical to it wherever that
 *                     runs); each block type is decided on its own / 0: the generic one-thread-per-row kernel, as before version 143.
 *                     The two differ in the order of additions, so in the last bits, both inside the parity gate.  A 9-step sampling
 *                     at depth 8, embed_dim 1024: 87.4 -> 61.6 ms at num_frame 27, B = 1; num_frame 243: 270.7 -> 138.6 ms at B = 1,
 *                     2610 -> 1377 ms at B = 16.  Every other head
 *                     width, F16X3 and BF16 engines: no effect.  d3d_workspace_bytes does not change.  "attn_f32_h128_last"
 *                     (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_hx"    1 (default) / 0: F16X3 engines whose heads are 48 or 96 columns wide (embed_dim == 48 num_heads or 96 num_heads, e.g.
 *                     384 or 768 with 8 heads) and num_joints <= 256 / 128.  With the key on, such an engine runs the folded flow with
 *                     the two-kernel attention branch: its spatial blocks and, for num_frame <= 256 (width 48) / 128 (width 96), its
 *                     temporal blocks on the resident fp16-MFMA kernel of these widths (a head is 48 or 96 adjacent columns of the
 *                     plane rows from column 48 h / 96 h on, not whole 64-column segments; the columns behind the head in its last LDS
 *                     row are zeros or not read, never the neighbouring head's), its temporal blocks for longer windows on the
 *                     key-streaming kernel of that width (chunks of 256 / 128 frames, the scores computed twice: the exact two-pass
 *                     softmax, bit-identical to the resident kernel wherever that runs) / 0: the plain row-kernel flow with the generic
 *                     fp32 attention kernel in every block, which is also what a D3D_PREC_FP32 engine of these widths runs.  The two
 *                     differ in the last bits, both inside the parity gate.  Measured: DESIGN.md section 5.  Every other head width,
 *                     FP32 and BF16 engines (BF16: refused at these widths): no effect.  d3d_workspace_bytes does not change.
 *                     "attn_hx_last" (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_f32_hx"     1 (default) / 0: FP32 engines whose heads are 48 or 96 columns wide with embed_dim a multiple of 32 (embed_dim ==
 *                     48 num_heads or 96 num_heads, e.g. 384 or 768 with 8 heads) -- the exact reference arithmetic, and the engine a
 *                     precision-"auto" model falls back to.  With the key on, the spatial blocks of such an engine (num_joints <= 256 at
 *                     width 48, <= 192 at width 96) and, for num_frame up to the same limit, its temporal blocks run the resident exact
 *                     fp32 kernel of these widths (v_mfma_f32_32x32x2_f32, K and V of a group resident in LDS, the scores scaled by
 *                     1 / sqrt(head_dim) after the sum, exact two-pass softmax, the second product on the unnormalised numerators, the
 *                     division by their sum and v[query] of the diagonal at the store: the arithmetic of "attn_f32_h128"; a head reads
 *                     and writes its own columns alone -- at width 48 the half-used second 32-column tile takes zeros, never the
 *                     neighbouring head's columns), its temporal blocks for longer windows the key-streaming kernel of that width
 *                     (chunks of 256 / 192 frames, the scores computed twice, bit-identical to the resident kernel wherever that runs);
 *                     each block type is decided on its own / 0: the generic one-thread-per-row kernel, as before version 146.  The
 *                     two differ in the order of additions, so in the last bits, both inside the parity gate.  A 9-step sampling at
 *                     depth 8, num_frame 243: embed_dim 384 66.5 -> 33.9 ms at B = 1, 456 -> 238 ms at B = 16; embed_dim 768
 *                     144.0 -> 75.8 ms and 1385 -> 820 ms; num_frame 27, B = 1: 35.1 -> 28.3 and 62.9 -> 49.0 ms (DESIGN.md
 *                     section 5).  Every other head width, an odd number of heads of 48 columns (embed_dim 48, 144: they keep the
 *                     generic kernel in both precisions), F16X3 and BF16 engines: no effect.  d3d_workspace_bytes does not change.
 *                     "attn_f32_hx_last" (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_h16"   1 (default) / 0: F16X3 engines whose heads are 16 columns wide and come in quads (embed_dim == 16 num_heads with
 *                     num_heads a multiple of 4, e.g. 128 with 8 heads) and num_joints <= 256.  With the key on, such an engine runs the
 *                     folded flow with the two-kernel attention branch: its spatial blocks and, for num_frame <= 256, its temporal blocks
 *                     on the resident fp16-MFMA kernel of that width (four adjacent heads share a 128-byte LDS row; each head owns one
 *                     16-deep step of the score product and has its own softmax, sum and output accumulator, of which only its own 16
 *                     rows are ever stored), its temporal blocks for longer windows on the key-streaming kernel of that width (chunks of
 *                     256 frames, the scores computed twice, bit-identical to the resident kernel wherever that runs) / 0: the plain
 *                     row-kernel flow with the generic fp32 attention kernel in every block, as before version 147.  The two differ in
 *                     the last bits, both inside the parity gate.  Measured: DESIGN.md section 5.  Other head counts of that width
 *                     (embed_dim 32 with 2 heads, 96 with 6), every other head width, FP32 and BF16 engines: no effect.
 *                     d3d_workspace_bytes does not change.  "attn_h16_last" (d3d_engine_get_info) reports what the latest forward ran.
 *   "attn_f32_h16"    1 (default) / 0: FP32 engines whose heads are 16 columns wide (embed_dim == 16 num_heads, any head count) -- the
 *                     exact reference arithmetic, and the engine a precision-"auto" model falls back to.  With the key on, the spatial
 *                     blocks of such an engine (num_joints <= 256) and, for num_frame <= 256, its temporal blocks run the resident exact
 *                     fp32 kernel at that width (v_mfma_f32_32x32x2_f32, the arithmetic of "attn_f32_hx"; the scores times the exact
 *                     1 / sqrt(16) = 0.25 after the sum; the half-used 32-column output tile takes zeros, never the neighbouring head's
 *                     columns), its temporal blocks for longer windows the key-streaming kernel (chunks of 256 frames, two passes,
 *                     bit-identical to the resident kernel wherever that runs); each block type is decided on its own / 0: the generic
 *                     one-thread-per-row kernel, as before version 147.  The two differ in the order of additions, so in the last
 *                     bits, both inside the parity gate.  Measured: DESIGN.md section 5.  Every other head width, F16X3 and BF16
 *                     engines: no effect.  d3d_workspace_bytes does not change.  "attn_f32_h16_last" (d3d_engine_get_info) reports what
 *                     the latest forward ran.
 *   "proj_split" /    -1 (default): the rule.  0, 2, 4: that S for proj / fc1 in every forward that fits the kernel pair (at most 2 x CUs
 *   "fc1_split"       workgroups; fc1: M S <= 8192 rows), the default kernel elsewhere; any other value, or an S the engine's widths do not
 *                     allow (K / 32 / S >= 4 whole k-tiles, width 512): D3D_EUNSUP.  Read only while "latency_mode" is on; for
 *                     measurements and tests.
 *   "small_tiles"     0 (default) / 1: read only while "latency_mode" is on (F16X3 folded flow, embedding width 512, 8 heads).  The fused
 *                     qkv + attention launches that open every block tile 256 token rows x one head, whatever the call: 48 workgroups at
 *                     num_frame 81, B = 1.  With the key on, a spatial launch (15, 16 or 17 joints) / a temporal launch (num_frame <= 127)
 *                     that would run fewer workgroups than the device has CUs runs on 128-row tiles of whole token groups instead --
 *                     floor(127 / N) groups of N tokens per workgroup, twice the workgroups, half the k-loop per workgroup -- where that
 *                     launch has at most 5/8 as many workgroups as the device has CUs (a workgroup holds a CU; measured).  Block 0 keeps
 *                     its direct form ("block0_direct").  The selection is a function of (options, shapes, B, CU count) alone.  The
 *                     small-tile kernel is bit-identical to the two-kernel flow ("fused_spatial" = "fused_temporal" = 0), which the grouped
 *                     temporal kernel it replaces is not: results stay inside the parity gate, but differ in the last bits from the
 *                     same engine with the key off.  d3d_workspace_bytes does not change.  "small_tiles_last" (d3d_engine_get_info)
 *                     reports what the latest forward ran.  Other values: D3D_EINVAL.
 *   "fused_narrow"    0 (default) / 1: F16X3 engines whose heads are 32 columns wide in pairs (embed_dim == 32 num_heads, num_heads even) or
 *                     16 columns wide in quads (embed_dim == 16 num_heads, num_heads % 4 == 0), embed_dim >= 128.  Such an engine runs the
 *                     folded flow with the qkv GEMM and the attention of every block as two launches, q / k / v planes going through
 *                     HBM ("attn_h32" / "attn_h16").  With the key on, its spatial blocks (num_joints <= 127, block 0 included) and, for
 *                     num_frame <= 127, its temporal blocks run both steps as ONE kernel on 128-row tiles of whole token groups x one
 *                     64-column segment -- a pair / a quad of heads -- with q / k / v kept in LDS; temporal blocks of longer windows keep
 *                     their kernels.  Bit-identical to the key off.  The selection is a function of (options, shapes) alone and does
 *                     not read "latency_mode".  Every other head width, odd head pairs / quads, FP32 and BF16 engines: no effect.
 *                     Measured: DESIGN.md section 5 (ahead at every batch of 64 measured, level for single sequences; the temporal step
 *                     of one-group tiles, T = 81, is slower than its two launches), hence opt-in.  d3d_workspace_bytes does not change.
 *                     "fused_narrow_last" (d3d_engine_get_info) reports what the latest forward ran.  Other values: D3D_EINVAL.
 *   "deep_stages"     1 (default) / 0: the one-tile-per-workgroup F16X3 GEMM launches (batches of a few sequences: proj on 128 x 128
 *                     tiles, qkv / proj / fc1 on 256 x 128) keep three / four k-tiles of operands staged instead of two, the wait in front
 *                     of a k-tile's barrier a counted vmcnt -- a k-tile no longer lasts a DMA round trip (proj at B = 1, T = 243: 20.8 ->
 *                     17.6 us per launch; a 9-step sampling 18.9 -> 18.3 ms at B = 1, 75.7 -> 72.2 at B = 8).  Bit-identical.  Per engine
 *                     since version 133: set on an engine it changes that engine alone (and drops its captured graphs, as every key
 *                     does).  It is the only key accepted with a NULL e: that sets the process-wide default, which the single-op hooks
 *                     use and which an engine follows until it is given a value of its own.
 * Unknown key: D3D_EINVAL. */
int d3d_engine_set_option(d3d_engine* e, const char* key, int64_t value);

/* q_sample (DIFF:360-366, extract DIFF:21-24): out = sqrt_ac[t_b] * x_start + sqrt(1-ac)[t_b] * noise, per row b.
 * n = elements per batch row. */
int d3d_q_sample(d3d_engine* e, const float* x_start_dev, const float* noise_dev, const int32_t* t_dev, float* out_dev,
                 int32_t B, int64_t n, void* stream);

/* p_losses tail (DIFF:411-418): out = loss_fn(model_out, target, reduction='none') * loss_coef[b],
 * loss_coef[b] = 1 + alphas_cumprod[t_b] / sqrt_one_minus_alphas_cumprod[t_b], clamped to <= 3 when clip_loss (clipLoss, DIFF:111).
 * loss_type 1 = l1, 2 = l2 (DIFF:368-375).  model_out / target / out: B rows of n fp32 values; t_dev: B int32 timesteps. */
int d3d_weighted_loss(d3d_engine* e, const float* model_out_dev, const float* target_dev, const int32_t* t_dev, float* out_dev,
                      int32_t B, int64_t n, int32_t loss_type, int32_t clip_loss, void* stream);

/* repeat_n hypotheses of forward() (DIFF:433-448): d3d_repeat_batch writes out[r * B + b, :] = x[b, :] for r < repeat_n
 * (noisy_2d_pose.repeat(repeat_n, 1, 1, 1)); d3d_hypothesis_mean writes out[b, :] = (pred[b, :] + pred[B + b, :] + ...) / repeat_n
 * (torch.mean(pred.view(repeat_n, b, f, p, -1), dim=0)) -- in the operation order of the reference's CPU path: the hypotheses added in
 * order, ONE fp32 division by repeat_n.  (torch.mean on a GPU tensor multiplies the sum by a precomputed 1 / repeat_n instead: one ulp apart
 * for repeat_n not a power of two; parity is defined against the CPU path.)  n = fp32 values per batch row. */
int d3d_repeat_batch(const float* x_dev, float* out_dev, int32_t B, int64_t n, int32_t repeat_n, void* stream);
int d3d_hypothesis_mean(const float* pred_dev, float* out_dev, int32_t B, int64_t n, int32_t repeat_n, void* stream);

/* Read-only engine facts: "graphs_cached" (captured hipGraphs held now, <= 4), "graphs_captured" (captures since creation),
 * "streams", "device", "latency_mode", "fc2_split_last" (the k-split S of fc2 + post-norm in the most recent d3d_denoise /
 * d3d_ddim_sample call, 0 when the default whole-row kernel ran; a sampling run as two half-batches reports the first half's),
 * "proj_split_last" / "fc1_split_last" (the same for proj and fc1), "proj_split" / "fc1_split" (the option values),
 * "fused_spatial_last" (1 when the spatial blocks of the most recent d3d_denoise / d3d_ddim_sample call of a D3D_PREC_F16X3 engine ran
 * the fused qkv + attention kernel -- option "fused_spatial", 15, 16 or 17 joints --, else 0: option off, another joint count, another
 * precision, or before any forward),
 * "bf16_fused_spatial_last" / "bf16_fused_temporal_last" (1 when the spatial / temporal blocks of the most recent d3d_denoise /
 * d3d_ddim_sample call of a D3D_PREC_BF16 engine ran the fused qkv + attention kernel, else 0; 0 before the first call and in the
 * other precisions), "block0_direct_last" (1 when block 0 of the most recent d3d_denoise / d3d_ddim_sample call computed q / k / v from
 * the raw input channels -- option "block0_direct" --, else 0: option off, another precision, or a shape without the tables),
 * "long_temporal" (the option value), "long_temporal_last" (1 when the temporal blocks of the most recent d3d_denoise / d3d_ddim_sample
 * call ran the key-streaming F16X3 attention kernel, else 0: num_frame <= 256, option off, another precision, or before any forward),
 * "long_temporal_f32" (the option value), "long_temporal_f32_last" (the same for a D3D_PREC_FP32 engine and the key-streaming fp32
 * attention kernel; "long_temporal_last" stays 0 on such an engine), "attn_h32" (the option value), "attn_h32_last" (1 when the blocks
 * of the most recent d3d_denoise / d3d_ddim_sample call ran the F16X3 attention kernel for heads of 32 columns, else 0: another head
 * width, num_frame > 256, option off, another precision, or before any forward), "attn_f32_h32" (the option value), "attn_f32_h32_last"
 * (bit 0: the spatial blocks, bit 1: the temporal blocks of the most recent d3d_denoise / d3d_ddim_sample call ran the exact fp32 attention
 * kernels for heads of 32 columns; 0 before any forward, with the option off, on every embed_dim == 64 num_heads engine and in the other
 * precisions), "long_temporal_h32" (the option value), "long_temporal_h32_last" (1 when the temporal blocks of the most recent
 * d3d_denoise / d3d_ddim_sample call ran the key-streaming F16X3 attention kernel for heads of 32 columns, else 0: another head width,
 * num_frame <= 256, option off, another precision, or before any forward), "long_temporal_f32_h32" (the option value),
 * "long_temporal_f32_h32_last" (the same for a D3D_PREC_FP32 engine and the key-streaming fp32 kernel of that width),
 * "attn_h128" (the option value), "attn_h128_last" (bit 0: the spatial blocks, bit 1: the temporal blocks of the most recent
 * d3d_denoise / d3d_ddim_sample call ran the resident F16X3 attention kernel for heads of 128 columns, bit 2: the temporal blocks ran
 * the key-streaming kernel of that width; 0 before any forward, with the option off, at every other head width and in the other
 * precisions), "attn_f32_h128" (the option value), "attn_f32_h128_last" (the same three bits for a D3D_PREC_FP32 engine and the exact
 * fp32 kernels for heads of 128 columns; 0 before any forward, with the option off, at every other head width and in the other
 * precisions), "attn_hx" (the option value), "attn_hx_last" (the same three bits for a D3D_PREC_F16X3 engine with heads of 48 or 96
 * columns and the F16X3 kernels of those widths; 0 before any forward, with the option off, at every other head width and in the other
 * precisions), "attn_f32_hx" (the option value), "attn_f32_hx_last" (the same three bits for a D3D_PREC_FP32 engine with heads of 48 or
 * 96 columns and the exact fp32 kernels of those widths; 0 before any forward, with the option off, at every other head width, where
 * embed_dim is no multiple of 32 and in the other precisions), "attn_h16" (the option value), "attn_h16_last" (the same three bits for a
 * D3D_PREC_F16X3 engine with a multiple of 4 heads of 16 columns and the F16X3 kernels of that width; 0 before any forward, with the
 * option off, at every other head width or head count and in the other precisions), "attn_f32_h16" (the option value),
 * "attn_f32_h16_last" (the same three bits for a D3D_PREC_FP32 engine with heads of 16 columns and the exact fp32 kernels at that width; 0
 * before any forward, with the option off, at every other head width and in the other precisions),
 * "small_tiles" (the option value), "small_tiles_last" (bit 0: the
 * spatial blocks, bit 1: the temporal blocks of the most recent d3d_denoise / d3d_ddim_sample call ran the 128-row fused qkv + attention
 * kernel; 0 before any forward, with the option or "latency_mode" off, and in the other precisions),
 * "fused_narrow" (the option value), "fused_narrow_last" (bit 0: the spatial blocks, bit 1: the temporal blocks of the most recent
 * d3d_denoise / d3d_ddim_sample call ran the fused qkv + attention kernel for heads of 32 or 16 columns; 0 before any forward, with the
 * option off, at every other head width or head count and in the other precisions).
 * Unknown key: D3D_EINVAL. */
int d3d_engine_get_info(const d3d_engine* e, const char* key, int64_t* value);

/* evaluate() tail (RUN:583-590, LOSS:15-22): un-flip + average the TTA pair, multiply by scale, and reduce the masked
 * per-joint L2 error.  sums_dev[0] += sum of joint errors over frames with mask != 0, sums_dev[1] += number of such
 * joints (caller zeroes sums_dev).  merged_dev (nullable) receives the merged, de-normalised prediction (B,T,J,3).
 * pred_flip_dev may be NULL (no TTA).  joints_left/right: host index lists of equal length.
 * Asynchronous on `stream` (since ABI version 110; it used to synchronise): sums_dev / merged_dev are valid only after the stream
 * has been synchronised.  J <= 64 (the joint permutation travels as a kernel argument); more: D3D_EUNSUP. */
int d3d_tta_mpjpe(const float* pred_dev, const float* pred_flip_dev, const float* gt_dev, const uint8_t* mask_dev,
                  float scale, const int32_t* joints_left_host, const int32_t* joints_right_host, int32_t n_lr,
                  float* merged_dev, double* sums_dev, int32_t B, int32_t T, int32_t J, void* stream);

/* evaluate()'s other three protocols (RUN:602-614) on the merged, de-normalised prediction d3d_tta_mpjpe wrote (pred_dev, gt_dev:
 * N frames of J joints x 3 fp32; mask_dev: N bytes, nullable = every frame kept), one thread per kept frame, fp64 inside:
 *   sums_dev[0] += sum over kept frames and joints of |s p - g|, s = <g, p> / <p, p> per frame          (N-MPJPE, LOSS:83-93)
 *   sums_dev[1] += the same for the prediction after the best similarity transform onto its target      (P-MPJPE, LOSS:43-81: scale,
 *                  rotation without reflection, translation; the 3 x 3 SVD by a Jacobi eigen-decomposition)
 *   sums_dev[2] += sum over kept frames WITH a kept predecessor in the flattened batch, and joints, of
 *                  |(p_f - p_prev) - (g_f - g_prev)|                                                      (MPJVE, LOSS:132-142: np.diff
 *                  of the masked batch -- window and sequence boundaries included, as there)
 *   sums_dev[3] += kept frames, sums_dev[4] += frames with a predecessor (caller zeroes the five doubles).
 * A batch's protocol value is sums[k] / (J * sums[3]) (k = 0, 1) and sums[2] / (J * sums[4]) -- 0 / 0 = nan for a batch of one kept
 * frame, as numpy's mean of an empty difference there; evaluate() weights each by the batch's kept frames.  Asynchronous on `stream`.
 * J <= 64; more: D3D_EUNSUP. */
int d3d_pose_metrics(const float* pred_dev, const float* gt_dev, const uint8_t* mask_dev, double* sums_dev, int32_t N, int32_t J,
                     void* stream);

/* The path's one exchange step (RUN:216-218: nn.DataParallel's gather of the replicas' outputs) for hosts that do not go through
 * torch.distributed: all-gather of count_per_rank fp32 values (the rank's predicted sequences) over an RCCL communicator the
 * CALLER owns (nccl_comm: ncclComm_t), asynchronous on `stream`; recv_dev holds world_size * count_per_rank values in rank
 * order.  libd3d_hip.so does not link RCCL: ncclAllGather is resolved at run time from the RCCL library already loaded into the
 * process (D3D_EUNSUP if there is none).  The Python host uses torch.distributed instead (parallel.all_gather_pred). */
int d3d_allgather_pred(void* nccl_comm, const float* send_dev, float* recv_dev, int64_t count_per_rank, void* stream);

/* Evaluation windows of one whole sequence, on the device: ChunkedGenerator(out_all=True, pad=0) (common/nosiy_generators.py:27-48
 * window table, :247-276 slicing, edge padding, target_mask, horizontal flip).  seq (n_frames, J, C) -> out
 * (d3d_num_windows, T, J, C); mask (nullable) (windows, T) uint8, 0 for the frames of the shifted last window that its
 * predecessor already covers.  flip != 0 writes the flipped copy (channel 0 negated, left/right joints swapped).
 * Asynchronous on `stream`: out_dev / mask_dev are valid only after the stream has been synchronised.  J <= 64, else D3D_EUNSUP. */
int d3d_num_windows(int32_t n_frames, int32_t T);
int d3d_window_gather(const float* seq_dev, int32_t n_frames, int32_t T, int32_t J, int32_t C, int32_t flip,
                      const int32_t* joints_left_host, const int32_t* joints_right_host, int32_t n_lr, float* out_dev,
                      uint8_t* mask_dev, void* stream);

/* The seq2frame window table (BASELINE configs[4]: ...S2F... models): ChunkedGenerator / ChunkedGenerator_3dhp with out_all=False and
 * chunk_length = stride = 1 (common/nosiy_generators.py:402-420 pair table, :492-512 slicing; data/load_noisy_data.py:312-316
 * pad = (T - 1) // 2): ONE window per target frame f, holding frames f - pad .. f + pad, edge-replicated at both ends of the sequence.
 * Writes the windows of target frames first .. first + count - 1: out (count, T, J, C).  The window's 3D target is frame f of the
 * 3D sequence itself and its mask the frame's `valid` flag: neither needs a kernel.  T must be odd; flip as in d3d_window_gather.
 * Asynchronous on `stream`. */
int d3d_window_gather_s2f(const float* seq_dev, int32_t n_frames, int32_t T, int32_t J, int32_t C, int32_t flip,
                          const int32_t* joints_left_host, const int32_t* joints_right_host, int32_t n_lr, int32_t first, int32_t count,
                          float* out_dev, void* stream);

/* ---- per-kernel-class timing (HIP events recorded on the launch stream around every kernel of d3d_denoise /
 * d3d_ddim_sample while enabled; used by bench.py for the roofline figures).  flops / bytes are the ALGORITHMIC counts
 * of the launches timed, total_ms the sum of their event-pair durations. ------------------------ */
#define D3D_KC_LINEAR 0
#define D3D_KC_ATTN_SPATIAL 1
#define D3D_KC_ATTN_TEMPORAL 2
#define D3D_KC_LAYERNORM 3
#define D3D_KC_EMBED 4
#define D3D_KC_HEAD 5
#define D3D_KC_OTHER 6
/* the GEMM launches of the F16X3 block flow once more, by kind (each is ALSO counted under D3D_KC_LINEAR: do not add these to it) */
#define D3D_KC_LINEAR_QKV 7
#define D3D_KC_LINEAR_PROJ 8
#define D3D_KC_LINEAR_FC1 9
#define D3D_KC_LINEAR_FC2 10
/* spatial blocks of the F16X3 flow: the LayerNorm-folded qkv GEMM and the 15- / 16- / 17-key attention as ONE kernel ("fused_spatial"); its
 * launches are counted here only (neither under D3D_KC_LINEAR nor D3D_KC_ATTN_SPATIAL) */
#define D3D_KC_QKV_SATTN 11
/* temporal blocks likewise ("fused_temporal": the qkv GEMM of one (batch, joint) group and its T-key attention as ONE kernel); counted
 * here only (neither under D3D_KC_LINEAR nor D3D_KC_ATTN_TEMPORAL) */
#define D3D_KC_QKV_TATTN 12
#define D3D_KC_COUNT 13
int d3d_engine_set_profiling(d3d_engine* e, int32_t on);
int d3d_engine_profile_reset(d3d_engine* e);
int d3d_engine_profile_read(d3d_engine* e, int32_t kernel_class, double* total_ms, int64_t* launches, double* flops,
                            double* bytes);
const char* d3d_kernel_class_name(int32_t kernel_class);

/* ---- F16X3 range guard.  The F16X3 operand planes hold fp16 (hi, lo) pairs of 8*x (activations: residual stream, q/k/v,
 * attention output, MLP hidden) and 2^k*w (GEMM weights; k is chosen per matrix at commit: 12 unless an entry exceeds 15.99 --
 * LayerNorm-folded weights W diag(gamma) of checkpoints with large gains -- then smaller, down to 0: nothing is clamped); activations
 * beyond the fp16 range, |x| > 8188, are not representable (the row and attention kernels clamp them to the range, the GEMM
 * epilogues let them become inf): results are then meaningless.
 * Every kernel that writes such planes raises a sticky flag in a word of device memory that belongs to the ENGINE it was launched
 * for when a value left the range (no cost in a healthy run), and d3d_engine_commit_weights notes weights it cannot represent.
 * d3d_engine_range_flags synchronises `stream` and returns
 *   D3D_RANGE_ACT    an activation of THIS engine left the range since its flag was last cleared
 *   D3D_RANGE_WEIGHT a GEMM weight of this engine was not finite at commit, or larger than 65504 in magnitude (its matrix would need
 *                    k < 0, where the planes of the matrix's ordinary entries are too coarse for fp32 accuracy: DESIGN.md section 4.1)
 *   D3D_RANGE_STATS  a LayerNorm folded into a GEMM met a row with |mean| > 16 standard deviations: the folded form works from
 *                    one-pass row statistics (sum, sum of squares), whose variance loses accuracy like eps (1 + mean^2 / var)
 *                    -- beyond ~25 sigma the 1e-4 parity gate is no longer guaranteed (post-norm biases that dwarf the gains)
 * clear != 0 resets the activation and statistics flags of this engine.  The word is per ENGINE (ABI version 120; it used to be
 * per device): two engines on one device, or evaluate() beside a user's own engine, do not see or consume each other's flags; the
 * two internal streams of one d3d_ddim_sample call report to the same word, which is read behind their join.  The single-op hooks
 * below belong to no engine and report nowhere.  A set flag means the F16X3 result is NOT fp32-accurate for this checkpoint / input:
 * run the engine with D3D_PREC_FP32 (RUN:226-235 loads arbitrary checkpoints; random-init and LayerNorm-ed streams stay far
 * inside the range). */
#define D3D_RANGE_ACT 1u
#define D3D_RANGE_WEIGHT 2u
#define D3D_RANGE_STATS 4u
/* not a precision matter, raised in every mode: a timestep handed to d3d_q_sample / d3d_weighted_loss was outside [0, num_timesteps)
 * (the reference raises IndexError on table[t], DIFF:21-24, 411): the row's output is NaN, no table entry was read */
#define D3D_RANGE_INDEX 8u
/* not a precision matter either, raised in every mode: the head kernel (S2S:217-220 + the DDIM update) forms the three dot products of
 * every row TWICE, from independently loaded weight fragments, and the two evaluations disagreed bit for bit.  They cannot on a healthy
 * machine; this is the signature of the one run-to-run deviation ever seen in this library (one wrong o[0] in ~1 launch of 60, only
 * beside a second process on the GPU, only with an instruction schedule that is pinned out by an ISA test -- mechanism unidentified,
 * experiments/NOTES.md).  The kernel repairs the row by a third evaluation (majority) and raises this bit so that a toolchain or
 * driver change that brings the deviation back is reported by the default guard read instead of silently moving a pose. */
#define D3D_RANGE_RECOMPUTE 16u
int d3d_engine_range_flags(d3d_engine* e, uint32_t* flags, int32_t clear, void* stream);

/* The guard WITHOUT a blocking synchronisation (ABI version 130) -- what the Python layer does by default after every compute call
 * (RUN:226-235 loads arbitrary checkpoints, so the default precision has to notice when one is outside its range by itself).
 * d3d_engine_range_post enqueues on `stream`, behind everything already there, ONE one-lane kernel that exchanges this engine's
 * word with zero and stores the value into a pinned host slot the engine owns, then records an event; *ticket names that snapshot.
 * d3d_engine_range_take returns the flags of a ticket (same bits as d3d_engine_range_flags; D3D_RANGE_WEIGHT is sticky):
 *   block == 0  never waits: *ready = 0 while the snapshot kernel has not run yet (flags untouched), 1 once it has
 *   block != 0  waits for the ticket's event (NOT for the whole stream or device)
 * The flags of a ticket cover every kernel launched for this engine on `stream` since the previous post (or read with clear).
 * 256 tickets are kept; an older one: D3D_EINVAL.  Not legal while `stream` is capturing (D3D_ESTATE).  Measured cost of a post per
 * d3d_ddim_sample at T = 243 / B = 64: one ~2 us launch in 477 ms. */
int d3d_engine_range_post(d3d_engine* e, void* stream, int64_t* ticket);
int d3d_engine_range_take(d3d_engine* e, int64_t ticket, int32_t block, uint32_t* flags, int32_t* ready);

/* ---- debug trace: while on (capacity > 0 slots), every kernel of the F16X3 block flow and the head is followed on `stream`
 * by a checksum launch over the rows it has just written (64-bit position-weighted word sums, order-independent), so two runs
 * of the same call can be compared kernel by kernel (experiments/bisect_two_proc.py).  d3d_engine_trace_read synchronises
 * `stream`, copies out up to cap (sum, tag) pairs in launch order and clears the log;
 * views (1..8): every buffer is summed `views` times, launch v reading each line through a different XCD's L2 (workgroup ->
 * data mapping rotated by v): the views of one buffer must agree -- a cross-XCD coherence check that needs no reference run.
 * tag = view << 28 | forward << 16 | block << 8 | kernel << 4 | buffer (kernel: 0 embed, 1 stream entry, 2 qkv, 3 attention, 4 proj,
 * 5 fc1, 6 fc2 [+ post-norm], 7 post-norm row kernel, 8 head / DDIM update [buffer 1: its y input], 9 the head launched a second
 * time from the same inputs into scratch; buffer: 0 output, 1 row statistics).
 * Graph replay is bypassed while tracing.  capacity 0 turns it off. */
int d3d_engine_set_trace(d3d_engine* e, int32_t capacity, int32_t views);
int d3d_engine_trace_read(d3d_engine* e, uint64_t* sums_host, uint32_t* tags_host, int32_t cap, int32_t* n, void* stream);

/* ---- single-op hooks: the same kernels the engine launches, exposed for the parity tests -------------------------- */
/* Time-embedding table (S2S:29-36,169-174 trunk, then every Block.time_mlp S2S:104-107) for n fp32 timesteps on the
 * device: out (n, 2*depth, D) in execution order STE0, TTE0, STE1, ...  scratch: n*(D + 4*D) floats. */
int d3d_op_time_embedding(d3d_engine* e, const float* times_dev, int32_t n, float* out_dev, float* scratch_dev,
                          void* stream);
/* C[M,N] = epi(A[M,K] @ W[N,K]^T + bias[N]); epi 0 none, 1 erf-GELU (FP32: erff; F16X3: erfc series, |err| < 1e-7 |x|),
 * 2 add residual R[M,N] (R may alias C). */
int d3d_op_linear(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev, float* C_dev,
                  int32_t M, int32_t N, int32_t K, int32_t epi, int32_t precision, void* stream);
/* d3d_op_linear with a choice of tile variant (F16X3: 0 = the engine's choice, 13 = 256x256, 4 = 256x128, 9 = on-the-fly A
 * split)
 * and a timing leg: after one untimed call, `reps` back-to-back launches are timed with HIP events on `stream` and the
 * mean written to *avg_ms (nullable).  Operand conversion for F16X3 happens once, outside the timed launches. */
int d3d_op_linear_bench(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev, float* C_dev,
                        int32_t M, int32_t N, int32_t K, int32_t epi, int32_t precision, int32_t variant, int32_t reps,
                        float* avg_ms, void* stream);
/* Y[M,N] = LayerNorm(R + A[M,K] @ W[N,K]^T + bias; gamma, beta, eps) [+ pos[(m / pos_div) % pos_mod, :]]
 *           [+ tvec[(m / rows_per_batch) * tvec_stride + :]]
 * -- the fc2 GEMM of a block with the block's post-norm applied in its epilogue (S2S:131-135 followed by S2S:236 / 245, and
 * the additions of S2S:238-242 / 113-116), the form the F16X3 engine runs: whole-row tiles, so the sum never leaves the chip
 * un-normalised.  F16X3 only; N == 512, K % 32 == 0 (anything else: D3D_EUNSUP).  pos / tvec nullable.  stats nullable:
 * [M,2] = (sum, sum of squares) of every Y row -- when given, the plane-output form runs (the one inside the engine, which
 * hands these statistics to the next LayerNorm-folded GEMM) and Y is decoded from its planes; otherwise the fp32-output
 * form (last block).  reps / avg_ms: timing leg as d3d_op_linear_bench. */
int d3d_op_linear_postnorm(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev,
                           const float* gamma_dev, const float* beta_dev, float eps, const float* pos_dev, int32_t pos_div,
                           int32_t pos_mod, const float* tvec_dev, int64_t tvec_stride, int32_t rows_per_batch, float* Y_dev,
                           float* stats_dev, int32_t M, int32_t N, int32_t K, int32_t reps, float* avg_ms, void* stream);
/* The same Y from the kernel pair of "latency_mode" (d3d_engine_set_option): a split-K x split-N F16X3 GEMM writes S fp32 partials
 * P[ks][M][N] (128 x 128 tiles, k-range ks of S) into partials_dev (S * M * N floats), and an ordered reduce + post-norm row kernel forms
 * R + bias + P[0] + ... + P[S-1] in exactly that order, then the LayerNorm and additions above.  A row's value depends on S, not on
 * M or on the row's position.  N == 512, S in {2, 4}, (K / 32) % S == 0 (anything else: D3D_EUNSUP).  stats as above (one (sum, sum
 * of squares) per row from the row kernel).  reps / avg_ms: mean time of the pair of launches. */
int d3d_op_linear_splitk_postnorm(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev,
                                  const float* gamma_dev, const float* beta_dev, float eps, const float* pos_dev, int32_t pos_div,
                                  int32_t pos_mod, const float* tvec_dev, int64_t tvec_stride, int32_t rows_per_batch, float* Y_dev,
                                  float* stats_dev, int32_t M, int32_t N, int32_t K, int32_t S, float* partials_dev, int32_t reps,
                                  float* avg_ms, void* stream);
/* proj and fc1 of "latency_mode" alone, fp32 in and out (operands are split and results un-split on the device).  S in {2, 4}: the
 * split-K x split-N GEMM into partials_dev (S * M * N floats) + the ordered reduce; S == 0: the default kernel on the same operands
 * (partials_dev unused).  reps / avg_ms: mean time of one call's launches.  Shapes outside the predicate: D3D_EUNSUP.
 *   _residual: Y = R + bias + A W^T as the stream planes hold it; stats_dev (nullable): (sum, sum of squares) of Y per row and 64-column
 *              block, M * (N / 64) * 2 floats.  N == 512, K % 32 == 0, (K / 32) % S == 0, K / 32 / S >= 4.
 *   _gelu:     H = gelu(LayerNorm(X; gamma, beta, eps) W^T + bias), the LayerNorm folded into the GEMM (S2S:46-48 behind 101), H read
 *              back from the accumulator-order planes fc2 consumes.  N % 512 == 0, K % 64 == 0, (K / 32) % S == 0, K / 32 / S >= 4. */
int d3d_op_linear_splitk_residual(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev, float* Y_dev,
                                  float* stats_dev, int32_t M, int32_t N, int32_t K, int32_t S, float* partials_dev, int32_t reps,
                                  float* avg_ms, void* stream);
int d3d_op_linear_splitk_gelu(const float* X_dev, const float* W_dev, const float* bias_dev, const float* gamma_dev,
                              const float* beta_dev, float eps, float* H_dev, int32_t M, int32_t N, int32_t K, int32_t S,
                              float* partials_dev, int32_t reps, float* avg_ms, void* stream);
/* ONE launch of the F16X3 token GEMM in a LayerNorm-folded form of the engine's plane-resident block, with the CALLER's row statistics:
 *   epi 0 (the qkv form):  LayerNorm(X; gamma, beta, eps) W^T + bias as the hi / lo fp16 planes the attention kernels read -- hi_dev, lo_dev:
 *                          (M, N) fp16 each; columns < qcols hold 1 * value, the others 8 * value, so value = (hi + lo) / scale.  H_dev unused.
 *   epi 1 (the fc1 form):  gelu(the same) read back as fp32 H_dev (M, N) from the accumulator-order planes fc2 consumes.  hi_dev, lo_dev,
 *                          qcols unused.
 * X: (M, K) raw fp32 rows (split into planes of 8 x on the device); W: (N, K), folded with gamma / beta on the host as the weight commit
 * folds it.  st_dev: (M, st_np, 2) fp32 (sum, sum of squares) partials of every X row -- the kernel only adds a row's st_np partials, so
 * st_np is the caller's (>= 1), whatever K; the hook copies them into a buffer of whole 256-row tiles whose pad rows hold NaN (the
 * persistent walk stages them, nothing may read them).  N % 128 == 0, K % 32 == 0 (else D3D_EUNSUP); 0 <= qcols <= N, qcols % 4 == 0. */
int d3d_op_linear_folded(const float* X_dev, const float* W_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev,
                         float eps, const float* st_dev, int32_t st_np, int32_t epi, int32_t qcols, float* H_dev, void* hi_dev,
                         void* lo_dev, int32_t M, int32_t N, int32_t K, void* stream);
/* ONE launch of the F16X3 token GEMM in a plane-residual form: Y = R + bias + A W^T with the residual read from stream planes.
 *   with_stats != 0 (the proj form): Y written as stream planes in place of R's and un-split to fp32 Y_dev; stats_dev (M, N / 64, 2)
 *                   receives the (sum, sum of squares) of every new row per 64-column block (what the folded fc1 reads).
 *   with_stats == 0 (the fc2 form of every width but 512): Y written as fp32; stats_dev unused.
 * The launch shape is the engine's choice from (M, N, K, CU count).  N % 128 == 0, K % 32 == 0 (else D3D_EUNSUP). */
int d3d_op_linear_plane_residual(const float* A_dev, const float* W_dev, const float* bias_dev, const float* R_dev, float* Y_dev,
                                 float* stats_dev, int32_t with_stats, int32_t M, int32_t N, int32_t K, void* stream);
/* Every output form of the LayerNorm row kernel in one launch (d3d_op_layernorm is its plain y = LN(x) form):
 *   y = [LN(x; gamma1, beta1, eps1) unless skip_ln1] [+ pos[(row / pos_div) % pos_mod]] [+ tvec[(row / rows_per_batch) * tvec_stride]]
 *   h = LN(y; gamma2, beta2, eps2)
 * Each output is written where its pointer is given: y_dev fp32; yx3_dev fp32, decoded from the stream planes of 8 y the kernel wrote;
 * stats_dev (rows, 2) the (sum, sum of squares) of every y row; h_dev fp32; hx3_dev fp32, decoded from h's planes; hbf16_dev (rows, D)
 * bf16.  At most one of h_dev / hx3_dev / hbf16_dev, and then y_dev or yx3_dev as well (the kernel forms h from y; gamma2 / beta2
 * required); at least one output.  D % 4 == 0, D <= 1024, D % 32 == 0 for the plane outputs (else D3D_EUNSUP). */
int d3d_op_layernorm_forms(const float* x_dev, const float* gamma1_dev, const float* beta1_dev, float eps1, int32_t skip_ln1,
                           const float* pos_dev, int32_t pos_div, int32_t pos_mod, const float* tvec_dev, int64_t tvec_stride,
                           int32_t rows_per_batch, const float* gamma2_dev, const float* beta2_dev, float eps2, float* y_dev,
                           float* yx3_dev, float* stats_dev, float* h_dev, float* hx3_dev, void* hbf16_dev, int32_t rows, int32_t D,
                           void* stream);
/* Regression head of the engine's weights (S2S:217-220: LayerNorm eps 1e-5 + Linear D -> 3) on rows x D fp32 rows:
 * x0 (rows, 3), raw (no clamp, no DDIM update). */
int d3d_op_head(d3d_engine* e, const float* X_dev, float* x0_dev, int32_t rows, void* stream);
/* Row LayerNorm over the last axis (S2S:95,101,236,245 eps 1e-6; S2S:218 eps 1e-5). */
int d3d_op_layernorm(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* out_dev, int32_t rows,
                     int32_t D, float eps, void* stream);
/* GRAND attention core (S2S:75-83) on a packed qkv buffer (B*T*J, 3*D): out = (softmax(q k^T / sqrt(dh)) - I) v,
 * token-major (B*T*J, D).  temporal = 0: groups are frames (N = J keys); 1: groups are joints (N = T keys).
 * force_generic != 0 selects the slow any-shape kernel (cross-check). */
int d3d_op_attention(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                     int32_t temporal, int32_t precision, int32_t force_generic, void* stream);
/* The temporal core of the F16X3 mode from the key-streaming kernel alone (option "long_temporal"): fp32 qkv in, fp32 out, split into /
 * merged from the hi / lo fp16 planes on the device as in d3d_op_attention (D3D_PREC_F16X3).  Any T >= 1, head width D / H == 64 (else
 * D3D_EUNSUP); for T <= 256 bit for bit the result of d3d_op_attention (temporal = 1, D3D_PREC_F16X3). */
int d3d_op_attention_long(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The F16X3 attention kernel for heads of 32 columns alone (option "attn_h32"): fp32 qkv in, fp32 out, split into / merged from the hi / lo
 * fp16 planes on the device as in d3d_op_attention (D3D_PREC_F16X3).  temporal as there (0: N = J keys, 1: N = T keys).  D == 32 H with H
 * even and N <= 256; anything else (head_dim 32 is the only width it takes): D3D_EUNSUP. */
int d3d_op_attention_h32(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                         void* stream);
/* The exact fp32 attention kernels for heads of 32 columns alone (option "attn_f32_h32"): fp32 qkv in, fp32 out.  temporal as in
 * d3d_op_attention (0: N = J keys, 1: N = T keys).  D == 32 H with T <= 256 (temporal) or 15 <= J <= 17 (spatial); anything else
 * (head_dim 32 is the only width they take): D3D_EUNSUP.  Not the bits of d3d_op_attention, which keeps the generic kernel at this width. */
int d3d_op_attention_f32_h32(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                             void* stream);
/* The temporal core of the FP32 mode from the key-streaming fp32 kernel alone (option "long_temporal_f32"): fp32 qkv in, fp32 out.  Any
 * T >= 1, head width D / H == 64 (else D3D_EUNSUP); for T <= 256 bit for bit the result of d3d_op_attention (temporal = 1,
 * D3D_PREC_FP32, force_generic = 0). */
int d3d_op_attention_long_f32(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The temporal core of an F16X3 engine with heads of 32 columns from the key-streaming kernel of that width alone (option
 * "long_temporal_h32"): fp32 qkv in, fp32 out, split into / merged from the hi / lo fp16 planes on the device as in d3d_op_attention
 * (D3D_PREC_F16X3).  Any T >= 1; D == 32 H with H even, anything else (head_dim 32 is the only width it takes): D3D_EUNSUP.  For
 * T <= 256 bit for bit the result of d3d_op_attention_h32 (temporal = 1). */
int d3d_op_attention_long_h32(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The same for an FP32 engine (option "long_temporal_f32_h32"): fp32 qkv in, fp32 out.  Any T >= 1; D == 32 H, any head count, anything
 * else (head_dim 32 is the only width it takes): D3D_EUNSUP.  For T <= 256 bit for bit the result of d3d_op_attention_f32_h32
 * (temporal = 1). */
int d3d_op_attention_long_f32_h32(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                                  void* stream);
/* The attention core of an F16X3 engine with heads of 128 columns from the resident kernel of that width alone (option "attn_h128"):
 * fp32 qkv in, fp32 out, split into / merged from the hi / lo fp16 planes on the device as in d3d_op_attention (D3D_PREC_F16X3).
 * temporal != 0: groups of T keys, else of J keys.  D == 128 H and a group length N <= 128; anything else (head_dim 128 is the only
 * width it takes): D3D_EUNSUP. */
int d3d_op_attention_h128(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                          void* stream);
/* The temporal core of such an engine from the key-streaming kernel of that width alone.  Any T >= 1; D == 128 H, anything else:
 * D3D_EUNSUP.  For T <= 128 bit for bit the result of d3d_op_attention_h128 (temporal = 1). */
int d3d_op_attention_long_h128(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The attention core of an F16X3 engine with heads of 48 or 96 columns from the resident kernel of those widths alone (option
 * "attn_hx"): fp32 qkv in, fp32 out, split into / merged from the hi / lo fp16 planes on the device as in d3d_op_attention
 * (D3D_PREC_F16X3).  temporal != 0: groups of T keys, else of J keys.  The width is D / H: D == 48 H and a group length N <= 256, or
 * D == 96 H and N <= 128; anything else (it takes head_dim 48 or 96 alone): D3D_EUNSUP. */
int d3d_op_attention_hx(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                        void* stream);
/* The temporal core of such an engine from the key-streaming kernel of its width alone.  Any T >= 1; D == 48 H or 96 H, anything else:
 * D3D_EUNSUP.  Wherever d3d_op_attention_hx (temporal = 1) runs, bit for bit its result. */
int d3d_op_attention_long_hx(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The resident exact fp32 attention kernel for heads of 128 columns alone (option "attn_f32_h128"): fp32 qkv in, fp32 out.  temporal as
 * in d3d_op_attention (0: N = J keys, 1: N = T keys).  D == 128 H and a group length N <= 128; anything else (head_dim 128 is the only
 * width it takes): D3D_EUNSUP.  Not the bits of d3d_op_attention, which keeps the generic kernel at this width. */
int d3d_op_attention_f32_h128(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                              int32_t temporal, void* stream);
/* The temporal core of such an engine from the key-streaming fp32 kernel of that width alone.  Any T >= 1; D == 128 H, anything else
 * (head_dim 128 is the only width it takes): D3D_EUNSUP.  For T <= 128 bit for bit the result of d3d_op_attention_f32_h128
 * (temporal = 1). */
int d3d_op_attention_long_f32_h128(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                                   void* stream);
/* The resident exact fp32 attention kernel for heads of 48 or 96 columns alone (option "attn_f32_hx"): fp32 qkv in, fp32 out.  temporal
 * as in d3d_op_attention (0: N = J keys, 1: N = T keys).  The width is D / H: D == 48 H and a group length N <= 256, or D == 96 H and
 * N <= 192; anything else (it takes head_dim 48 or 96 alone): D3D_EUNSUP.  Not the bits of d3d_op_attention, which keeps the generic
 * kernel at these widths. */
int d3d_op_attention_f32_hx(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                            void* stream);
/* The temporal core of such an engine from the key-streaming fp32 kernel of its width alone.  Any T >= 1; D == 48 H or 96 H, anything
 * else: D3D_EUNSUP.  Wherever d3d_op_attention_f32_hx (temporal = 1) runs, bit for bit its result. */
int d3d_op_attention_long_f32_hx(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                                 void* stream);
/* The attention core of an F16X3 engine with quads of heads of 16 columns from the resident kernel of that width alone (option
 * "attn_h16"): fp32 qkv in, fp32 out, split into / merged from the hi / lo fp16 planes on the device as in d3d_op_attention
 * (D3D_PREC_F16X3).  temporal != 0: groups of T keys, else of J keys.  D == 16 H, H a multiple of 4 and a group length N <= 256; anything
 * else (head_dim 16 is the only width it takes): D3D_EUNSUP. */
int d3d_op_attention_h16(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                         void* stream);
/* The temporal core of such an engine from the key-streaming kernel of that width alone.  Any T >= 1; D == 16 H with H a multiple of 4,
 * anything else: D3D_EUNSUP.  For T <= 256 bit for bit the result of d3d_op_attention_h16 (temporal = 1). */
int d3d_op_attention_long_h16(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream);
/* The resident exact fp32 attention kernel for heads of 16 columns alone (option "attn_f32_h16"): fp32 qkv in, fp32 out.  temporal as in
 * d3d_op_attention (0: N = J keys, 1: N = T keys).  D == 16 H (any head count) and a group length N <= 256; anything else (head_dim 16 is
 * the only width it takes): D3D_EUNSUP.  Not the bits of d3d_op_attention, which keeps the generic kernel at this width. */
int d3d_op_attention_f32_h16(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                             void* stream);
/* The temporal core of such an engine from the key-streaming fp32 kernel at that width alone.  Any T >= 1; D == 16 H, anything else:
 * D3D_EUNSUP.  For T <= 256 bit for bit the result of d3d_op_attention_f32_h16 (temporal = 1). */
int d3d_op_attention_long_f32_h16(const float* qkv_dev, float* out_dev, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H,
                                  void* stream);
/* The fused qkv GEMM + attention kernel of the BF16 mode alone: out = attention(bf16(A) bf16(Wqkv)^T + bias) with q / k / v rounded to
 * bf16 (q third times dh^-1/2) and kept on chip -- bit for bit d3d_op_linear (D3D_PREC_BF16) followed by d3d_op_attention (D3D_PREC_BF16)
 * on the same tensors.  A: (groups * N, D) fp32 token rows; Wqkv: (3 D, D); bias: (3 D); out: (groups * N, D) fp32.  Group u holds the N
 * rows (u / stride) * N * stride + u % stride + t * stride: spatial blocks groups = B * T, N = J, stride = 1, temporal = 0; temporal
 * blocks groups = B * J, N = T, stride = J, temporal = 1.  Head width D / H == 64, D % 128 == 0, D >= 256, N <= 255 (temporal = 0:
 * N <= 32), groups % stride == 0; anything else: D3D_EUNSUP / D3D_EINVAL. */
int d3d_op_qkv_attn_bf16(const float* A_dev, const float* Wqkv_dev, const float* bias_dev, int32_t groups, int32_t N, int32_t stride,
                         int32_t D, int32_t H, int32_t temporal, float* out_dev, void* stream);
/* The same kernel in its fp16-operand form (D3D_PREC_F16): operands, q / k / v, softmax - I and the output rounded to fp16.  q is rounded
 * once, AFTER its scale by dh^-1/2 (as the engine's un-fused qkv GEMM rounds it): bit for bit d3d_op_linear (D3D_PREC_F16, residual form
 * with R = 0: q / k / v not rounded yet) followed by d3d_op_attention (D3D_PREC_F16).  Through d3d_op_linear's fp16 output the q third is
 * rounded twice, which differs where q * dh^-1/2 is an fp16 subnormal.  Arguments and refusals as d3d_op_qkv_attn_bf16. */
int d3d_op_qkv_attn_f16(const float* A_dev, const float* Wqkv_dev, const float* bias_dev, int32_t groups, int32_t N, int32_t stride,
                        int32_t D, int32_t H, int32_t temporal, float* out_dev, void* stream);

/* The fused qkv GEMM + attention kernel of "small_tiles" alone (F16X3): out = attention(LayerNorm(X; gamma, beta, eps) Wqkv^T + bias), the
 * LayerNorm folded into the GEMM as the weight commit folds it, q / k / v kept on chip as hi / lo fp16 planes -- bit for bit the folded
 * qkv GEMM followed by d3d_op_attention (D3D_PREC_F16X3) on the same tensors.  X: (groups * N, D) fp32 token rows; Wqkv: (3 D, D); bias:
 * (3 D); gamma, beta: (D); out: (groups * N, D) fp32.  Groups as d3d_op_qkv_attn_bf16: spatial blocks groups = B * T, N = J in 15 .. 17,
 * stride = 1, temporal = 0; temporal blocks groups = B * J, N = T <= 127, stride = J, temporal = 1.  D == 512, H == 8, groups % stride == 0;
 * anything else: D3D_EUNSUP / D3D_EINVAL. */
int d3d_op_qkv_attn_x3_small(const float* X_dev, const float* Wqkv_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev,
                             float eps, int32_t groups, int32_t N, int32_t stride, int32_t D, int32_t H, int32_t temporal, float* out_dev,
                             void* stream);

/* The fused qkv GEMM + attention kernel of "fused_narrow" alone (F16X3), for heads of 32 columns in pairs or 16 columns in quads: the
 * arithmetic and arguments of d3d_op_qkv_attn_x3_small -- bit for bit the folded qkv GEMM followed by d3d_op_attention_h32 /
 * d3d_op_attention_h16 on the same tensors.  Spatial blocks groups = B * T, N = J <= 127 (any joint count), stride = 1, temporal = 0;
 * temporal blocks groups = B * J, N = T <= 127, stride = J, temporal = 1.  D == 32 H with H even or D == 16 H with H % 4 == 0, D >= 128,
 * groups % stride == 0; anything else: D3D_EUNSUP / D3D_EINVAL. */
int d3d_op_qkv_attn_x3_narrow(const float* X_dev, const float* Wqkv_dev, const float* bias_dev, const float* gamma_dev, const float* beta_dev,
                              float eps, int32_t groups, int32_t N, int32_t stride, int32_t D, int32_t H, int32_t temporal, float* out_dev,
                              void* stream);

/* ---- machine probes (measurement support; no reference counterpart) ------------------------------------------------ */
/* What THIS device sustains for the two resources that co-limit the F16X3 GEMM k-loop, measured over about ms_target
 * milliseconds on `stream` (a bench line can then state its roofline fraction against measured ceilings beside the nominal
 * peaks of MI355X_MICROARCH.md; bench.py's "machine_probes" object).  what 0: *result = TFLOP/s of fp16 MFMA work
 * (v_mfma_f32_16x16x32_f16, two waves per SIMD on every CU, register operands with the statistics of real hi / lo halves --
 * the power-limited clock included); what 1: *result = GB/s, summed over the CUs, of the k-loop's staging stream alone
 * (global_load_lds_dwordx4 pieces of 256 x 256 x 32 stages from L2-resident operand rows, no MFMA).  Needs no engine. */
int d3d_probe_machine(int32_t what, float ms_target, float* result, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* D3D_H_ */
