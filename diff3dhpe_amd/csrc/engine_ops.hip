// Single-op test / bench hooks of the C ABI that need no engine: each allocates its temporaries, brings the fp32 operands into the
// kernel's operand form, runs the launch sequence once (`once`), optionally times `reps` more, converts the result back to fp32 and
// synchronises the caller's stream.  d3d_op_time_embedding and d3d_op_head read engine fields and live in engine.hip.
#include <hip/hip_runtime.h>

#include <functional>
#include <vector>

#include "attn_dispatch.h"
#include "d3d_kernels.h"
#include "engine_internal.h"

using namespace d3d;

namespace {

// F16X3 pair buffer of an fp32 device matrix (rows padded to 256, zero rows).  Weights are split on the host with the same routine the
// engine uses at commit; activations on the device with the producers' split.
struct TmpPair : DevBuf<uint16_t> {
  int wexp = 12;
};
int make_pair(TmpPair& t, const float* src_dev, int rows, int cols, bool weight, hipStream_t s) {
  const size_t n16 = 2 * pad256(rows + 191) * cols;   // (whole 256-row tiles, and whole 192-row ones of proj's walk, as the engine's workspace)
  HIP_TRY(t.alloc(n16));
  HIP_TRY(hipMemsetAsync(t.p, 0, n16 * sizeof(uint16_t), s));
  if (weight) {
    std::vector<float> h((size_t)rows * cols);
    std::vector<uint16_t> pr(2 * h.size());
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipMemcpy(h.data(), src_dev, h.size() * sizeof(float), hipMemcpyDeviceToHost));
    t.wexp = split_weight_f16x3(h.data(), rows, cols, pr.data());
    HIP_TRY(hipMemcpy(t.p, pr.data(), pr.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
  } else {
    HIP_TRY(launch_split_x3(src_dev, t.p, (size_t)rows, cols, s));
  }
  return D3D_OK;
}

// The operand pairs of C = A W^T [+ R]: W [N][K], then A [M][K] and R [M][N] where given, then (with_y) the output planes [M][N] -- any
// initialised pair buffer of that size; a hook reads its residual from r, so repeats see the same input.
struct X3Operands { TmpPair a, w, r, y; };
int make_operands(X3Operands& o, const float* A, const float* W, const float* R, int M, int N, int K, bool with_y, hipStream_t s) {
  int rc = make_pair(o.w, W, N, K, true, s);
  if (!rc && A) rc = make_pair(o.a, A, M, K, false, s);
  if (!rc && R) rc = make_pair(o.r, R, M, N, false, s);
  if (!rc && with_y) rc = make_pair(o.y, R, M, N, false, s);
  return rc;
}

// The LayerNorm fold of the weight commit, on the host: W diag(gamma) as planes wp (rows padded to 256, zero rows), and fd = [csum | b + W beta]
int make_folded(TmpPair& wp, DevBuf<float>& fd, const float* W, const float* bias, const float* gamma, const float* beta, int N, int K,
                hipStream_t s) {
  const size_t nk = (size_t)N * K;
  std::vector<float> hw(nk), hg(K), hb(K), hbias(N), wg(nk), fold(2 * (size_t)N);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(hw.data(), W, nk * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hg.data(), gamma, (size_t)K * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hb.data(), beta, (size_t)K * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hbias.data(), bias, (size_t)N * sizeof(float), hipMemcpyDeviceToHost));
  fold_layernorm(hw.data(), hbias.data(), hg.data(), hb.data(), N, K, wg.data(), fold.data(), fold.data() + N);
  std::vector<uint16_t> pr(2 * pad256(N) * K, 0);
  wp.wexp = split_weight_f16x3(wg.data(), N, K, pr.data());
  HIP_TRY(wp.upload(pr.data(), pr.size()));
  HIP_TRY(fd.upload(fold.data(), fold.size()));
  return D3D_OK;
}

// mean time of `once` over reps launches on s, behind `warm` untimed ones (the op hooks' avg_ms)
hipError_t time_reps(const std::function<hipError_t()>& once, int reps, float* avg_ms, hipStream_t s, int warm = 0) {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t le = hipEventCreate(&e0);
  if (le == hipSuccess) le = hipEventCreate(&e1);
  for (int i = 0; i < warm && le == hipSuccess; ++i) le = once();
  if (le == hipSuccess) le = hipEventRecord(e0, s);
  for (int i = 0; i < reps && le == hipSuccess; ++i) le = once();
  if (le == hipSuccess) le = hipEventRecord(e1, s);
  if (le == hipSuccess) le = hipEventSynchronize(e1);
  float ms = 0.f;
  if (le == hipSuccess) le = hipEventElapsedTime(&ms, e0, e1);
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  if (le == hipSuccess) *avg_ms = ms / reps;
  return le;
}

// `once`, then the timed repeats where the caller asked for them
hipError_t run_timed(const std::function<hipError_t()>& once, int reps, float* avg_ms, hipStream_t s, int warm = 0) {
  const hipError_t le = once();
  return le == hipSuccess && avg_ms ? time_reps(once, reps, avg_ms, s, warm) : le;
}

// the post-norm row arguments of the two post-norm hooks, from the caller's
bool row_class_args_ok(const float* pos, int pos_div, int pos_mod, const float* tvec, int64_t tvec_stride, int rows_per_batch) {
  return !(pos && (pos_div < 1 || pos_mod < 1)) && !(tvec && tvec_stride != 0 && rows_per_batch < 1);
}
X3PostNorm hook_postnorm(const float* gamma, const float* beta, float eps, const float* pos, int pos_div, int pos_mod, const float* tvec,
                         int64_t tvec_stride, int rows_per_batch) {
  X3PostNorm q{};
  q.g = gamma; q.b = beta; q.eps = eps;
  q.pos = pos; q.pos_div = pos ? pos_div : 1; q.pos_mod = pos ? pos_mod : 1;
  q.tvec = tvec; q.tvec_stride = tvec_stride; q.rows_per_batch = rows_per_batch > 0 ? rows_per_batch : 1;
  return q;
}

// the hooks' common tail: the launch status first, then the stream's
int finish(hipError_t le, hipStream_t s) {
  const hipError_t se = hipStreamSynchronize(s);
  HIP_TRY(le);
  HIP_TRY(se);
  return D3D_OK;
}

// The round trip of the single-op hooks of the F16X3 attention kernels: fp32 qkv (rows, 3 D) -> hi / lo planes (as the qkv GEMM
// epilogue writes them) -> the kernel alone, launch(hi, lo, out_pair) -> pair layout -> fp32 out (rows, D).  The pair-layout rows are
// 2 ceil32(D) halves apart: where D is no multiple of 32 (an odd head count at width 48 -- no engine, only these ops) the rows are
// unpacked at that pitch and their first D columns copied out.
template <class Launch>
int attention_x3_round_trip(const float* qkv, float* out, size_t rows, int D, hipStream_t s, Launch launch) {
  const int Dp = (D + 31) & ~31;
  const size_t nq = rows * 3 * D, np = rows * Dp;
  DevBuf<uint16_t> tmp;
  DevBuf<float> wide;
  HIP_TRY(tmp.alloc(2 * nq + 2 * np));
  if (Dp != D) HIP_TRY(wide.alloc(np));
  hipError_t le = Dp != D ? hipMemsetAsync(tmp.p + 2 * nq, 0, 2 * np * sizeof(uint16_t), s) : hipSuccess;   // (columns behind D: read back, not written)
  if (le == hipSuccess) le = launch_split_qkv(qkv, tmp.p, tmp.p + nq, rows, D, s);
  if (le == hipSuccess) le = launch(tmp.p, tmp.p + nq, tmp.p + 2 * nq);
  if (le == hipSuccess) le = launch_unsplit_pair(tmp.p + 2 * nq, Dp != D ? wide.p : out, rows, Dp, s);
  if (le == hipSuccess && Dp != D)
    le = hipMemcpy2DAsync(out, (size_t)D * sizeof(float), wide.p, (size_t)Dp * sizeof(float), (size_t)D * sizeof(float), rows, hipMemcpyDeviceToDevice, s);
  return finish(le, s);
}

// The body of every width-specific attention hook: one regime of one family of attn_dispatch.h (resident, for the spatial or the temporal
// blocks, or key-streaming) on fp32 qkv (B T J, 3 D) -> fp32 out (B T J, D).  The fp32 kernels run in place of the caller's buffers; the
// planes kernels through the round trip above.
int attention_op(AttnFamilyId family, bool streaming, const float* qkv, float* out, int B, int T, int J, int D, int H, bool temporal,
                 void* stream) {
  if (!qkv || !out || B <= 0 || T <= 0 || J <= 0 || D <= 0 || H <= 0 || D % H) return fail(D3D_EINVAL, "bad argument");
  const AttnPick pick{family, streaming ? 1 : 0};
  const AttnRegime& r = pick.regime(temporal);
  if (!r.ok(temporal ? T : J, D, H)) return fail(D3D_EUNSUP, r.unsup);
  AttnArgs a{qkv, nullptr, out, nullptr, B, T, J, D, H, temporal, reinterpret_cast<hipStream_t>(stream)};
  if (pick.fam().form == ATTN_ROWS) {
    HIP_TRY(r.launch(a));
    return D3D_OK;
  }
  return attention_x3_round_trip(qkv, out, (size_t)B * T * J, D, a.s, [&](const uint16_t* hi, const uint16_t* lo, uint16_t* o) {
    a.qkv = hi; a.qkv_lo = lo; a.out_x3 = o;
    return r.launch(a);
  });
}

}  // namespace

extern "C" {

int d3d_probe_machine(int32_t what, float ms_target, float* result, void* stream) {
  if (!result || (what != 0 && what != 1) || !(ms_target > 0.f) || ms_target > 2000.f) return fail(D3D_EINVAL, "bad argument");
  HIP_TRY(launch_probe_machine(what, ms_target, result, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_op_linear(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M, int32_t N,
                  int32_t K, int32_t epi, int32_t precision, void* stream) {
  return d3d_op_linear_bench(A, W, bias, R, C, M, N, K, epi, precision, 0, 1, nullptr, stream);
}

int d3d_op_linear_bench(const float* A, const float* W, const float* bias, const float* R, float* C, int32_t M, int32_t N,
                        int32_t K, int32_t epi, int32_t precision, int32_t variant, int32_t reps, float* avg_ms, void* stream) {
  if (precision != D3D_PREC_FP32 && precision != D3D_PREC_F16X3 && precision != D3D_PREC_BF16 && precision != D3D_PREC_F16)
    return fail(D3D_EUNSUP, "precision not implemented");
  if (!A || !W || !C || reps < 1) return fail(D3D_EINVAL, "bad argument");
  if (K % 32 && !(precision == D3D_PREC_FP32 && K % 16 == 0))
    return fail(D3D_EUNSUP, "K must be a multiple of 32 (D3D_PREC_FP32: of 16, a last k-tile of 16 columns is zero-filled)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (precision == D3D_PREC_BF16 || precision == D3D_PREC_F16) {
    // the bf16 operand mode: operands rounded to bf16 on the device (rows padded to 256, zero), the product through launch_linear_bf16;
    // EPI_NONE / EPI_GELU results come back through the kernel's bf16 output (rounded once more).  D3D_PREC_F16: the same with fp16.
    const bool f16 = precision == D3D_PREC_F16;
    if (K % 64 || N % 8) return fail(D3D_EUNSUP, "bf16 / f16 mode: K % 64 == 0 and N % 8 == 0");
    if (epi == EPI_RESIDUAL && !R) return fail(D3D_EINVAL, "residual required");
    const size_t mp = pad256(M), np = pad256(N);
    DevBuf<uint16_t> ab, wb, cb;
    HIP_TRY(ab.alloc(mp * K));
    HIP_TRY(wb.alloc(np * K));
    HIP_TRY(cb.alloc((size_t)M * N));
    hipError_t le = hipMemsetAsync(ab.p, 0, mp * K * 2, s);
    if (le == hipSuccess) le = hipMemsetAsync(wb.p, 0, np * K * 2, s);
    if (le == hipSuccess) le = launch_f32_to_bf16(A, ab.p, (size_t)M * K, s, f16);
    if (le == hipSuccess) le = launch_f32_to_bf16(W, wb.p, (size_t)N * K, s, f16);
    auto once = [&]() -> hipError_t { return launch_linear_bf16(ab.p, wb.p, bias, R, C, cb.p, M, N, K, epi, 0, s, f16); };
    if (le == hipSuccess) le = run_timed(once, reps, avg_ms, s, /*warm clocks*/ 3);
    if (le == hipSuccess && epi != EPI_RESIDUAL) le = launch_bf16_to_f32(cb.p, C, (size_t)M * N, s, f16);
    return finish(le, s);
  }
  X3Operands o;
  if (precision == D3D_PREC_F16X3 && (N % 4) != 0) variant = 9;   // the plane kernel stores 4 columns at a time
  if (precision == D3D_PREC_F16X3) {
    const int rc = make_operands(o, variant != 9 ? A : nullptr, W, nullptr, M, N, K, false, s);
    if (rc) return rc;
  }
  auto once = [&]() -> hipError_t {
    if (precision == D3D_PREC_FP32) return launch_linear_f32(A, W, bias, R, C, M, N, K, epi, s);
    if (variant == 9) return o.w.wexp == 12 ? launch_linear_f16x3(A, o.w.p, bias, R, C, M, N, K, epi, s) : hipErrorInvalidValue;   // on-the-fly A split
    return launch_linear_x3p(o.a.p, o.w.p, bias, R, C, nullptr, nullptr, M, N, K, epi, 0, 0, variant, s, nullptr, o.w.wexp);
  };
  return finish(run_timed(once, reps, avg_ms, s), s);
}

int d3d_op_linear_postnorm(const float* A, const float* W, const float* bias, const float* R, const float* gamma,
                           const float* beta, float eps, const float* pos, int32_t pos_div, int32_t pos_mod, const float* tvec,
                           int64_t tvec_stride, int32_t rows_per_batch, float* Y, float* stats, int32_t M, int32_t N, int32_t K,
                           int32_t reps, float* avg_ms, void* stream) {
  if (!A || !W || !bias || !R || !gamma || !beta || !Y || M < 1 || reps < 1) return fail(D3D_EINVAL, "bad argument");
  if (!x3q_postnorm_ok(N, K)) return fail(D3D_EUNSUP, "the post-norm GEMM form exists for N == 512, K % 32 == 0");
  if (!row_class_args_ok(pos, pos_div, pos_mod, tvec, tvec_stride, rows_per_batch)) return fail(D3D_EINVAL, "bad row-class arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  X3Operands o;
  const int rc = make_operands(o, A, W, R, M, N, K, stats != nullptr, s);
  if (rc) return rc;
  const int np = x3q_ntiles(M, N);
  DevBuf<float> part;
  if (stats) HIP_TRY(part.alloc((size_t)M * np * 2));
  X3Fold f{};
  f.Rp = o.r.p;
  f.pn = hook_postnorm(gamma, beta, eps, pos, pos_div, pos_mod, tvec, tvec_stride, rows_per_batch);
  f.st_out = part.p;
  auto once = [&]() -> hipError_t {
    if (stats) return launch_linear_x3p(o.a.p, o.w.p, bias, nullptr, nullptr, o.y.p, nullptr, M, N, K, EPI_RESIDUAL, 2, 0, 0, s, &f, o.w.wexp);
    return launch_linear_x3p(o.a.p, o.w.p, bias, nullptr, Y, nullptr, nullptr, M, N, K, EPI_RESIDUAL, 0, 0, 0, s, &f, o.w.wexp);
  };
  hipError_t le = run_timed(once, reps, avg_ms, s);
  if (le == hipSuccess && stats) le = launch_unsplit_x3(o.y.p, Y, (size_t)M, N, part.p, np, stats, s);
  return finish(le, s);
}

int d3d_op_linear_splitk_postnorm(const float* A, const float* W, const float* bias, const float* R, const float* gamma,
                                  const float* beta, float eps, const float* pos, int32_t pos_div, int32_t pos_mod, const float* tvec,
                                  int64_t tvec_stride, int32_t rows_per_batch, float* Y, float* stats, int32_t M, int32_t N, int32_t K,
                                  int32_t S, float* partials, int32_t reps, float* avg_ms, void* stream) {
  if (!A || !W || !bias || !R || !gamma || !beta || !Y || !partials || M < 1 || reps < 1) return fail(D3D_EINVAL, "bad argument");
  if (!fc2_splitk_ok(N, K, S)) return fail(D3D_EUNSUP, "the split-K fc2 + post-norm pair exists for N == 512, S in {2, 4}, (K / 32) % S == 0");
  if (!row_class_args_ok(pos, pos_div, pos_mod, tvec, tvec_stride, rows_per_batch)) return fail(D3D_EINVAL, "bad row-class arguments");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  X3Operands o;
  const int rc = make_operands(o, A, W, R, M, N, K, stats != nullptr, s);
  if (rc) return rc;
  DevBuf<float> st1;
  if (stats) HIP_TRY(st1.alloc((size_t)M * 2));
  const X3PostNorm q = hook_postnorm(gamma, beta, eps, pos, pos_div, pos_mod, tvec, tvec_stride, rows_per_batch);
  auto once = [&]() -> hipError_t {   // (the row kernel reads o.r and writes o.y / Y: repeats see the same input)
    const hipError_t ge = launch_linear_x3p_splitk(o.a.p, o.w.p, partials, M, N, K, S, s, o.w.wexp);
    if (ge != hipSuccess) return ge;
    return launch_splitk_postnorm(partials, S, o.r.p, bias, q, stats ? nullptr : Y, stats ? o.y.p : nullptr, st1.p, M, N, s);
  };
  hipError_t le = run_timed(once, reps, avg_ms, s);
  if (le == hipSuccess && stats) le = launch_unsplit_x3(o.y.p, Y, (size_t)M, N, st1.p, 1, stats, s);
  return finish(le, s);
}

int d3d_op_linear_splitk_residual(const float* A, const float* W, const float* bias, const float* R, float* Y, float* stats, int32_t M,
                                  int32_t N, int32_t K, int32_t S, float* partials, int32_t reps, float* avg_ms, void* stream) {
  if (!A || !W || !bias || !R || !Y || (S != 0 && !partials) || M < 1 || reps < 1) return fail(D3D_EINVAL, "bad argument");
  if (S == 0 ? !(N == 512 && K > 0 && K % 32 == 0) : !proj_splitk_ok(N, K, S))
    return fail(D3D_EUNSUP, "the split-K proj pair exists for N == 512, S in {2, 4}, K / 32 / S >= 4 whole k-tiles (S == 0: the default kernel)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  X3Operands o;
  const int rc = make_operands(o, A, W, R, M, N, K, true, s);
  if (rc) return rc;
  const int np = x3q_ntiles(M, N);
  DevBuf<float> part;   // (whole 256-row tiles, as the engine's statistics buffers)
  HIP_TRY(part.alloc(pad256(M) * np * 2));
  X3Fold f{};
  f.Rp = o.r.p; f.st_out = part.p;
  auto once = [&]() -> hipError_t {
    if (S == 0) return launch_linear_x3p(o.a.p, o.w.p, bias, nullptr, nullptr, o.y.p, nullptr, M, N, K, EPI_RESIDUAL, 2, 0, 0, s, &f, o.w.wexp);
    const hipError_t ge = launch_linear_x3p_splitk(o.a.p, o.w.p, partials, M, N, K, S, s, o.w.wexp);
    return ge == hipSuccess ? launch_splitk_residual(partials, S, o.r.p, bias, o.y.p, part.p, M, N, s) : ge;
  };
  hipError_t le = run_timed(once, reps, avg_ms, s);
  if (le == hipSuccess) le = launch_unsplit_x3(o.y.p, Y, (size_t)M, N, nullptr, 0, nullptr, s);
  if (le == hipSuccess && stats) le = hipMemcpyAsync(stats, part.p, (size_t)M * np * 2 * sizeof(float), hipMemcpyDeviceToDevice, s);
  return finish(le, s);
}

int d3d_op_linear_splitk_gelu(const float* X, const float* W, const float* bias, const float* gamma, const float* beta, float eps,
                              float* H, int32_t M, int32_t N, int32_t K, int32_t S, float* partials, int32_t reps, float* avg_ms,
                              void* stream) {
  if (!X || !W || !bias || !gamma || !beta || !H || (S != 0 && !partials) || M < 1 || reps < 1 || !(eps > 0.f))
    return fail(D3D_EINVAL, "bad argument");
  if (S == 0 ? !(N > 0 && N % 512 == 0 && K > 0 && K % 64 == 0) : !fc1_splitk_ok(N, K, S))
    return fail(D3D_EUNSUP, "the split-K fc1 pair exists for N % 512 == 0, K % 64 == 0, S in {2, 4}, K / 32 / S >= 4 whole k-tiles (S == 0: the default kernel)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  TmpPair wp, xp, hp;
  DevBuf<float> fd, st;
  const int rc = make_folded(wp, fd, W, bias, gamma, beta, N, K, s);
  if (rc) return rc;
  const size_t mpad = pad256(M);
  HIP_TRY(xp.alloc(2 * mpad * K));
  HIP_TRY(hipMemsetAsync(xp.p, 0, 2 * mpad * K * sizeof(uint16_t), s));
  HIP_TRY(hp.alloc(2 * mpad * N));
  HIP_TRY(hipMemsetAsync(hp.p, 0, 2 * mpad * N * sizeof(uint16_t), s));
  HIP_TRY(st.alloc(mpad * 2));
  HIP_TRY(hipMemsetAsync(st.p, 0, mpad * 2 * sizeof(float), s));
  {  // the stream entry row kernel: planes of 8 x + one (sum, sum of squares) per row
    LnArgs a = ln_rows(M, K, M);
    a.x = X; a.skip_ln1 = 1; a.y_x3 = xp.p; a.stats = st.p;
    HIP_TRY(launch_layernorm(a, s));
  }
  X3Fold f{};
  f.st_in = st.p; f.st_np = 1; f.csum = fd.p; f.eps = eps;
  auto once = [&]() -> hipError_t {
    if (S == 0) return launch_linear_x3p(xp.p, wp.p, fd.p + N, nullptr, nullptr, hp.p, nullptr, M, N, K, EPI_GELU, 2, 0, 0, s, &f, wp.wexp);
    const hipError_t ge = launch_linear_x3p_splitk(xp.p, wp.p, partials, M, N, K, S, s, wp.wexp);
    return ge == hipSuccess ? launch_splitk_gelu(partials, S, st.p, 1, fd.p, fd.p + N, eps, hp.p, M, N, K, s) : ge;
  };
  hipError_t le = run_timed(once, reps, avg_ms, s);
  if (le == hipSuccess) le = launch_unsplit_acc(hp.p, H, (size_t)M, N, s);
  return finish(le, s);
}

int d3d_op_linear_folded(const float* X, const float* W, const float* bias, const float* gamma, const float* beta, float eps,
                         const float* st, int32_t st_np, int32_t epi, int32_t qcols, float* H, void* hi, void* lo, int32_t M, int32_t N,
                         int32_t K, void* stream) {
  if (!X || !W || !bias || !gamma || !beta || !st || M < 1 || st_np < 1 || !(eps > 0.f) || (epi != EPI_NONE && epi != EPI_GELU))
    return fail(D3D_EINVAL, "bad argument");
  if (!(N > 0 && N % 128 == 0 && K > 0 && K % 32 == 0)) return fail(D3D_EUNSUP, "the folded forms are exposed for N % 128 == 0, K % 32 == 0");
  if (epi == EPI_NONE ? (!hi || !lo || qcols < 0 || qcols > N || qcols % 64) : !H)
    return fail(D3D_EINVAL, "qkv form: hi / lo planes and 0 <= qcols <= N, qcols % 64 == 0; fc1 form: H");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  TmpPair wp, xp, hp;
  DevBuf<float> fd, stb;
  int rc = make_folded(wp, fd, W, bias, gamma, beta, N, K, s);
  if (!rc) rc = make_pair(xp, X, M, K, false, s);
  if (rc) return rc;
  // the statistics as the engine's buffers hold them: whole 256-row tiles; the pad rows are NaN here (staged by the walk, read by nothing)
  const size_t nst = pad256(M) * st_np * 2, mst = (size_t)M * st_np * 2;
  HIP_TRY(stb.alloc(nst));
  HIP_TRY(hipMemsetAsync(stb.p, 0xff, nst * sizeof(float), s));
  HIP_TRY(hipMemcpyAsync(stb.p, st, mst * sizeof(float), hipMemcpyDeviceToDevice, s));
  if (epi == EPI_GELU) {
    HIP_TRY(hp.alloc(2 * pad256(M) * N));
    HIP_TRY(hipMemsetAsync(hp.p, 0, 2 * pad256(M) * N * sizeof(uint16_t), s));
  }
  X3Fold f{};
  f.st_in = stb.p; f.st_np = st_np; f.csum = fd.p; f.eps = eps;
  hipError_t le = epi == EPI_NONE
                      ? launch_linear_x3p(xp.p, wp.p, fd.p + N, nullptr, nullptr, hi, lo, M, N, K, EPI_NONE, 1, qcols, 0, s, &f, wp.wexp)
                      : launch_linear_x3p(xp.p, wp.p, fd.p + N, nullptr, nullptr, hp.p, nullptr, M, N, K, EPI_GELU, 2, 0, 0, s, &f, wp.wexp);
  if (le == hipSuccess && epi == EPI_GELU) le = launch_unsplit_acc(hp.p, H, (size_t)M, N, s);
  return finish(le, s);
}

int d3d_op_linear_plane_residual(const float* A, const float* W, const float* bias, const float* R, float* Y, float* stats,
                                 int32_t with_stats, int32_t M, int32_t N, int32_t K, void* stream) {
  if (!A || !W || !bias || !R || !Y || (with_stats && !stats) || M < 1) return fail(D3D_EINVAL, "bad argument");
  if (!(N > 0 && N % 128 == 0 && K > 0 && K % 32 == 0))
    return fail(D3D_EUNSUP, "the plane-residual forms are exposed for N % 128 == 0, K % 32 == 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  X3Operands o;
  const int rc = make_operands(o, A, W, R, M, N, K, false, s);
  if (rc) return rc;
  const int np = x3q_ntiles(M, N);
  DevBuf<float> part;   // (whole 256-row tiles, as the engine's statistics buffers)
  if (with_stats) HIP_TRY(part.alloc(pad256(M) * np * 2));
  X3Fold f{};
  f.Rp = o.r.p; f.st_out = part.p;
  // proj form: the stream planes updated in place, as the engine runs it; fc2 form: fp32 out
  hipError_t le = with_stats ? launch_linear_x3p(o.a.p, o.w.p, bias, nullptr, nullptr, o.r.p, nullptr, M, N, K, EPI_RESIDUAL, 2, 0, 0, s, &f, o.w.wexp)
                             : launch_linear_x3p(o.a.p, o.w.p, bias, nullptr, Y, nullptr, nullptr, M, N, K, EPI_RESIDUAL, 0, 0, 0, s, &f, o.w.wexp);
  if (le == hipSuccess && with_stats) le = launch_unsplit_x3(o.r.p, Y, (size_t)M, N, nullptr, 0, nullptr, s);
  if (le == hipSuccess && with_stats) le = hipMemcpyAsync(stats, part.p, (size_t)M * np * 2 * sizeof(float), hipMemcpyDeviceToDevice, s);
  return finish(le, s);
}

// (f16: the fp16 operand mode's form of the kernel, d3d_op_qkv_attn_f16)
static int op_qkv_attn_16(const float* A, const float* Wqkv, const float* bias, int32_t groups, int32_t N, int32_t stride, int32_t D,
                          int32_t H, int32_t temporal, float* out, void* stream, bool f16) {
  if (!A || !Wqkv || !bias || !out || groups <= 0 || N <= 0 || stride <= 0 || D <= 0 || H <= 0 || groups % stride) return fail(D3D_EINVAL, "bad argument");
  const int T = temporal ? N : groups / stride, J = temporal ? stride : N, B = temporal ? groups / stride : 1;
  if (!(temporal ? qkv_tattn_bf16_ok(T, J, D, H, B) : qkv_sattn_bf16_ok(T, J, D, H, B)))
    return fail(D3D_EUNSUP, f16 ? "fused f16 qkv + attention: head_dim 64, D % 128 == 0, D >= 256, groups of <= 255 tokens (spatial: <= 32)"
                                : "fused bf16 qkv + attention: head_dim 64, D % 128 == 0, D >= 256, groups of <= 255 tokens (spatial: <= 32)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // operands rounded to bf16 on the device into buffers of EXACTLY the operand sizes (the kernel reads no pad rows), the fused kernel
  // alone, its bf16 output widened to fp32
  const size_t rows = (size_t)groups * N, na = rows * D, nw = (size_t)3 * D * D;
  DevBuf<uint16_t> ab, wb, ob;
  HIP_TRY(ab.alloc(na));
  HIP_TRY(wb.alloc(nw));
  HIP_TRY(ob.alloc(na));
  hipError_t le = launch_f32_to_bf16(A, ab.p, na, s, f16);
  if (le == hipSuccess) le = launch_f32_to_bf16(Wqkv, wb.p, nw, s, f16);
  if (le == hipSuccess) le = hipMemsetAsync(ob.p, 0xff, na * 2, s);   // (NaN: a row the kernel skipped shows)
  if (le == hipSuccess) le = launch_qkv_attn_bf16(ab.p, wb.p, bias, ob.p, groups, N, stride, D, H, temporal ? 1 : 0, s, f16);
  if (le == hipSuccess) le = launch_bf16_to_f32(ob.p, out, na, s, f16);
  return finish(le, s);
}
int d3d_op_qkv_attn_bf16(const float* A, const float* Wqkv, const float* bias, int32_t groups, int32_t N, int32_t stride, int32_t D,
                         int32_t H, int32_t temporal, float* out, void* stream) {
  return op_qkv_attn_16(A, Wqkv, bias, groups, N, stride, D, H, temporal, out, stream, false);
}
int d3d_op_qkv_attn_f16(const float* A, const float* Wqkv, const float* bias, int32_t groups, int32_t N, int32_t stride, int32_t D,
                        int32_t H, int32_t temporal, float* out, void* stream) {
  return op_qkv_attn_16(A, Wqkv, bias, groups, N, stride, D, H, temporal, out, stream, true);
}

int d3d_op_qkv_attn_x3_small(const float* X, const float* Wqkv, const float* bias, const float* gamma, const float* beta, float eps,
                             int32_t groups, int32_t N, int32_t stride, int32_t D, int32_t H, int32_t temporal, float* out, void* stream) {
  if (!X || !Wqkv || !bias || !gamma || !beta || !out || groups <= 0 || N <= 0 || stride <= 0 || D <= 0 || H <= 0 || groups % stride || !(eps > 0.f))
    return fail(D3D_EINVAL, "bad argument");
  const int J = temporal ? stride : N;
  if ((!temporal && stride != 1) || !qkv_attn_x3_small_ok(N, stride, J, D, H, D) || (long long)groups * N * 4 * D >= (1LL << 32))
    return fail(D3D_EUNSUP, "fused F16X3 qkv + attention on small tiles: D 512, 8 heads, groups of <= 127 tokens (spatial: stride 1, 15 .. 17 joints)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the LayerNorm fold and the tile-order images of the weight commit, on the host
  const size_t R3 = 3 * (size_t)D, nk = R3 * D, rows = (size_t)groups * N;
  std::vector<float> hw(nk), hg(D), hb(D), hbias(R3), wg(nk), fold(2 * R3), fold_t(2 * R3);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(hw.data(), Wqkv, nk * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hg.data(), gamma, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hb.data(), beta, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hbias.data(), bias, R3 * sizeof(float), hipMemcpyDeviceToHost));
  fold_layernorm(hw.data(), hbias.data(), hg.data(), hb.data(), R3, D, wg.data(), fold.data(), fold.data() + R3);
  std::vector<uint16_t> pr(2 * nk, 0);
  const int wexp = tile_order_copy(wg.data(), fold.data(), fold.data() + R3, D, H, pr.data(), fold_t.data(), fold_t.data() + R3);
  // buffers of EXACTLY the operand sizes (the kernel reads no pad rows); the output starts as NaN planes: a row the kernel skipped shows
  DevBuf<uint16_t> wp, xp, op;
  DevBuf<float> fd, st;
  HIP_TRY(wp.upload(pr.data(), pr.size()));
  HIP_TRY(fd.upload(fold_t.data(), fold_t.size()));
  HIP_TRY(xp.alloc(2 * rows * D));
  HIP_TRY(op.alloc(2 * rows * D));
  HIP_TRY(st.alloc(rows * 2));
  hipError_t le = hipMemsetAsync(op.p, 0xff, 2 * rows * D * sizeof(uint16_t), s);
  if (le == hipSuccess) {  // the stream entry row kernel: planes of 8 x + one (sum, sum of squares) per row
    LnArgs a = ln_rows((int)rows, D, (int)rows);
    a.x = X; a.skip_ln1 = 1; a.y_x3 = xp.p; a.stats = st.p;
    le = launch_layernorm(a, s);
  }
  if (le == hipSuccess)
    le = launch_qkv_attn_x3_small(xp.p, wp.p, fd.p + R3, fd.p, st.p, 1, eps, wexp, op.p, groups, N, stride, J, D, D, H, s);
  if (le == hipSuccess) le = launch_unsplit_pair(op.p, out, rows, D, s);
  return finish(le, s);
}

int d3d_op_qkv_attn_x3_narrow(const float* X, const float* Wqkv, const float* bias, const float* gamma, const float* beta, float eps,
                              int32_t groups, int32_t N, int32_t stride, int32_t D, int32_t H, int32_t temporal, float* out, void* stream) {
  if (!X || !Wqkv || !bias || !gamma || !beta || !out || groups <= 0 || N <= 0 || stride <= 0 || D <= 0 || H <= 0 || groups % stride || !(eps > 0.f))
    return fail(D3D_EINVAL, "bad argument");
  const int J = temporal ? stride : N;
  if ((!temporal && stride != 1) || !qkv_attn_x3_narrow_ok(N, stride, J, D, H, D) || (long long)groups * N * 4 * D >= (1LL << 32))
    return fail(D3D_EUNSUP, "fused F16X3 qkv + attention for narrow heads: D = 32 H (H even) or 16 H (H % 4 == 0), D >= 128, groups of <= 127 tokens "
                            "(spatial: stride 1)");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // the LayerNorm fold and the tile-order images of the weight commit (D / 64 pseudo-heads), on the host
  const size_t R3 = 3 * (size_t)D, nk = R3 * D, rows = (size_t)groups * N;
  std::vector<float> hw(nk), hg(D), hb(D), hbias(R3), wg(nk), fold(2 * R3), fold_t(2 * R3);
  HIP_TRY(hipStreamSynchronize(s));
  HIP_TRY(hipMemcpy(hw.data(), Wqkv, nk * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hg.data(), gamma, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hb.data(), beta, (size_t)D * sizeof(float), hipMemcpyDeviceToHost));
  HIP_TRY(hipMemcpy(hbias.data(), bias, R3 * sizeof(float), hipMemcpyDeviceToHost));
  fold_layernorm(hw.data(), hbias.data(), hg.data(), hb.data(), R3, D, wg.data(), fold.data(), fold.data() + R3);
  std::vector<uint16_t> pr(2 * nk, 0);
  const int wexp = tile_order_copy(wg.data(), fold.data(), fold.data() + R3, D, (size_t)D / 64, pr.data(), fold_t.data(), fold_t.data() + R3);
  // buffers of EXACTLY the operand sizes (the kernel reads no pad rows); the output starts as NaN planes: a row the kernel skipped shows
  DevBuf<uint16_t> wp, xp, op;
  DevBuf<float> fd, st;
  HIP_TRY(wp.upload(pr.data(), pr.size()));
  HIP_TRY(fd.upload(fold_t.data(), fold_t.size()));
  HIP_TRY(xp.alloc(2 * rows * D));
  HIP_TRY(op.alloc(2 * rows * D));
  HIP_TRY(st.alloc(rows * 2));
  hipError_t le = hipMemsetAsync(op.p, 0xff, 2 * rows * D * sizeof(uint16_t), s);
  if (le == hipSuccess) {  // the stream entry row kernel: planes of 8 x + one (sum, sum of squares) per row
    LnArgs a = ln_rows((int)rows, D, (int)rows);
    a.x = X; a.skip_ln1 = 1; a.y_x3 = xp.p; a.stats = st.p;
    le = launch_layernorm(a, s);
  }
  if (le == hipSuccess)
    le = launch_qkv_attn_x3_narrow(xp.p, wp.p, fd.p + R3, fd.p, st.p, 1, eps, wexp, op.p, groups, N, stride, J, D, D, H, s);
  if (le == hipSuccess) le = launch_unsplit_pair(op.p, out, rows, D, s);
  return finish(le, s);
}

int d3d_op_layernorm(const float* x, const float* gamma, const float* beta, float* out, int32_t rows, int32_t D, float eps,
                     void* stream) {
  if (!x || !gamma || !beta || !out) return fail(D3D_EINVAL, "null tensor");
  LnArgs a = ln_rows(rows, D, 1);
  a.x = x; a.y = out; a.g1 = gamma; a.b1 = beta; a.eps1 = eps;
  HIP_TRY(launch_layernorm(a, reinterpret_cast<hipStream_t>(stream)));
  return D3D_OK;
}

int d3d_op_layernorm_forms(const float* x, const float* gamma1, const float* beta1, float eps1, int32_t skip_ln1, const float* pos,
                           int32_t pos_div, int32_t pos_mod, const float* tvec, int64_t tvec_stride, int32_t rows_per_batch,
                           const float* gamma2, const float* beta2, float eps2, float* y, float* yx3, float* stats, float* h, float* hx3,
                           void* hbf16, int32_t rows, int32_t D, void* stream) {
  const int nh = (h != nullptr) + (hx3 != nullptr) + (hbf16 != nullptr);
  if (!x || rows < 1 || D < 1 || (!skip_ln1 && (!gamma1 || !beta1)) || nh > 1 || (nh && (!gamma2 || !beta2 || (!y && !yx3))) ||
      (!y && !yx3 && !stats && !nh))
    return fail(D3D_EINVAL, "bad argument");
  if (!row_class_args_ok(pos, pos_div, pos_mod, tvec, tvec_stride, rows_per_batch)) return fail(D3D_EINVAL, "bad row-class arguments");
  if (D % 4 || D > 1024 || ((yx3 || hx3) && D % 32)) return fail(D3D_EUNSUP, "row kernel: D % 4 == 0, D <= 1024, plane outputs D % 32 == 0");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  DevBuf<uint16_t> yp, hp;
  if (yx3) HIP_TRY(yp.alloc(2 * (size_t)rows * D));
  if (hx3) HIP_TRY(hp.alloc(2 * (size_t)rows * D));
  LnArgs a = ln_rows(rows, D, rows_per_batch > 0 ? rows_per_batch : 1);
  a.x = x; a.y = y; a.y_x3 = yp.p; a.stats = stats; a.h = h; a.h_x3 = hp.p; a.h_bf16 = hbf16;
  a.g1 = gamma1; a.b1 = beta1; a.eps1 = eps1; a.skip_ln1 = skip_ln1 ? 1 : 0;
  a.g2 = gamma2; a.b2 = beta2; a.eps2 = eps2;
  a.pos = pos; a.pos_div = pos ? pos_div : 1; a.pos_mod = pos ? pos_mod : 1;
  a.tvec = tvec; a.tvec_stride = tvec_stride;
  hipError_t le = launch_layernorm(a, s);
  if (le == hipSuccess && yx3) le = launch_unsplit_x3(yp.p, yx3, (size_t)rows, D, nullptr, 0, nullptr, s);
  if (le == hipSuccess && hx3) le = launch_unsplit_x3(hp.p, hx3, (size_t)rows, D, nullptr, 0, nullptr, s);
  return finish(le, s);
}

int d3d_op_attention(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal,
                     int32_t precision, int32_t force_generic, void* stream) {
  if (precision != D3D_PREC_FP32 && precision != D3D_PREC_F16X3 && precision != D3D_PREC_BF16 && precision != D3D_PREC_F16)
    return fail(D3D_EUNSUP, "precision not implemented");
  if (!qkv || !out || B <= 0 || T <= 0 || J <= 0 || D <= 0 || H <= 0 || D % H) return fail(D3D_EINVAL, "bad argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const size_t rows = (size_t)B * T * J, nq = rows * 3 * D, no = rows * D;
  if (precision == D3D_PREC_BF16 || precision == D3D_PREC_F16) {
    // fp32 qkv -> bf16 (q third scaled by 2^-3, as the qkv GEMM epilogue writes it) -> bf16-MFMA attention -> fp32; D3D_PREC_F16: fp16
    const bool f16 = precision == D3D_PREC_F16;
    const int N = temporal ? T : J;
    if (!attn_bf16_ok(N, D, H)) return fail(D3D_EUNSUP, "bf16 / f16 attention: head_dim 64, group length <= 256");
    DevBuf<float> qs;
    DevBuf<uint16_t> tmp;
    HIP_TRY(qs.alloc(nq));
    HIP_TRY(tmp.alloc(nq + no));
    hipError_t le = hipMemcpyAsync(qs.p, qkv, nq * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (le == hipSuccess) le = launch_scale_cols(qs.p, rows, 3 * D, D, 0.125f, s);
    if (le == hipSuccess) le = launch_f32_to_bf16(qs.p, tmp.p, nq, s, f16);
    if (le == hipSuccess)
      le = temporal ? launch_attn_bf16(tmp.p, tmp.p + nq, B, T, J, D, H, s, f16) : launch_attn_bf16(tmp.p, tmp.p + nq, B * T, J, 1, D, H, s, f16);
    if (le == hipSuccess) le = launch_bf16_to_f32(tmp.p + nq, out, no, s, f16);
    return finish(le, s);
  }
  if (precision == D3D_PREC_F16X3 && temporal && !force_generic && attn_temporal_x3_ok(T, D, H)) {
    return attention_x3_round_trip(qkv, out, rows, D, s, [&](const uint16_t* hi, const uint16_t* lo, uint16_t* o) {
      return launch_attn_temporal_x3(hi, lo, o, B, T, J, D, H, s);
    });
  }
  if (!force_generic && !temporal && attn_spatial_fast_ok(J, D, H)) {
    HIP_TRY(launch_attn_spatial_f32(qkv, out, nullptr, B, T, J, D, H, s));
  } else if (!force_generic && temporal && attn_temporal_fast_ok(T, D, H)) {
    HIP_TRY(launch_attn_temporal_f32(qkv, out, nullptr, B, T, J, D, H, s));
  } else {
    HIP_TRY(launch_attn_generic(qkv, out, nullptr, B, T, J, D, H, temporal, s));
  }
  return D3D_OK;
}

// The width-specific hooks: (family, streaming) of attn_dispatch.h; the streaming kernels serve temporal blocks alone
int d3d_op_attention_long(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_X3, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_h32(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_X3_H32, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_f32_h32(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_F32_H32, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_f32(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_F32, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_long_h32(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_X3_H32, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_long_f32_h32(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_F32_H32, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_h128(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_X3_H128, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_h128(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_X3_H128, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_hx(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_X3_HX, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_hx(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_X3_HX, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_f32_h128(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_F32_H128, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_f32_h128(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_F32_H128, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_f32_hx(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_F32_HX, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_f32_hx(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_F32_HX, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_h16(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_X3_H16, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_h16(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_X3_H16, true, qkv, out, B, T, J, D, H, true, stream);
}
int d3d_op_attention_f32_h16(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, int32_t temporal, void* stream) {
  return attention_op(AF_F32_H16, false, qkv, out, B, T, J, D, H, temporal != 0, stream);
}
int d3d_op_attention_long_f32_h16(const float* qkv, float* out, int32_t B, int32_t T, int32_t J, int32_t D, int32_t H, void* stream) {
  return attention_op(AF_F32_H16, true, qkv, out, B, T, J, D, H, true, stream);
}

}  // extern "C"
