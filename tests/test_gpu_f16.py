"""fp16 operand mode (D3D_PREC_F16) on the MI355X: the bf16 mode's kernels instantiated for fp16 rows, gated as tests/test_gpu_bf16.py
gates the bf16 mode with every bound scaled by 2^-3 (three more mantissa bits).

  * every kernel against fp64 math on the SAME fp16-rounded operands: per-element one fp16 rounding of the output, and a share of the
    outputs that ARE round-to-nearest-even of the exact value.  The bf16 floor is 0.998; the flips come from the fp32 accumulation
    order landing on a rounding boundary, and fp16's boundaries are 2^3 denser: floor 1 - 8 (1 - 0.998) = 0.984;
  * rounding is torch's .to(float16): nearest even, subnormals kept (a weight matrix a third of whose entries are fp16 subnormals);
  * the fused qkv + attention kernel bit for bit the two launches it replaces;
  * the engine against the oracle's fp16-operand emulation (oracle.operand_rounding(torch.float16): same rounding points): max-abs <=
    2e-2 / 8 and MPJPE <= max(1.5 x the emulation's own fp32-vs-fp64-accumulation distance, 2e-3 / 8); the whole sampling at 2.5 x the
    max-abs gate;
  * the point of the mode: at most a quarter of the bf16 engine's MPJPE to the fp32 oracle on the same inputs;
  * path independence (batch chunks, streams, graph replay, the fused / own-kernel options): torch.equal.

Least share of outputs equal to RNE(exact) measured on the MI355X (printed by the tests; floor 0.984): linear 0.99388 ((517, 1024, 512),
the GELU form), attention 0.99913 ((2, 243, 17) temporal), the fused kernel's q / k / v 0.99913 (T = 2)."""
import pytest
import torch

from helpers import cfg_full, inputs, build_product, product, product_with_engine, maxabs, torch_sd, dev
from diff3dhpe_amd.engine import op_linear, op_attention, op_qkv_attn_f16

pytestmark = pytest.mark.gpu
GATE_MAXABS, GATE_MPJPE = 2e-2 / 8, 2e-3 / 8       # tests/test_gpu_bf16.py's gates times 2^-3
RNE_FLOOR = 1.0 - 8 * (1.0 - 0.998)                # 0.984
D, H = 512, 8


def _h(x):
    return x.to(torch.float16).to(torch.float64)


def _mpjpe(a, b):
    return (a.detach().cpu().double() - b.double()).norm(dim=-1).mean().item()


# ------------------------------------------------------------------------------------------------ one kernel against fp64 math
# (M, N, K, epi, subnormal weights): the 256 x 128 tiles with ragged edges; 70 000 rows: the persistent 256 x 256 walk, ragged last tile
LINEAR = [(300, 512, 512, "none", False), (517, 1024, 512, "gelu", False), (517, 512, 1024, "residual", False),
          (70000, 1536, 512, "none", False), (300, 512, 512, "none", True)]


@pytest.mark.parametrize("M,N,K,epi,subnormal", LINEAR)
def test_f16_linear_matches_rounded_operand_math(M, N, K, epi, subnormal):
    """One fp16 MFMA per product, fp32 accumulation: against fp64 math on the SAME fp16-rounded operands the only differences are the
    fp32 accumulation order and, for the fp16-output forms, the final rounding (<= half an fp16 ulp: |ref| 2^-11).  The subnormal case:
    weights ~ N(0, 1.417e-4), a third of which are fp16 subnormals (|w| < 2^-14), no bias, so that flushing them -- at the operand
    conversion or at the MFMA's inputs -- would move the outputs (~3e-3) by ~5e-4 where the bound allows 2.2e-5."""
    g = torch.Generator().manual_seed(M + N + int(subnormal))
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * (1.417e-4 if subnormal else K ** -0.5)
    b = torch.zeros(N) if subnormal else torch.randn(N, generator=g)
    R = torch.randn(M, N, generator=g) if epi == "residual" else None
    if subnormal:
        w16 = W.to(torch.float16)
        share = ((w16 != 0) & (w16.abs() < 2.0 ** -14)).float().mean().item()
        assert 0.30 <= share <= 0.37, share
    out = op_linear(A.cuda(), W.cuda(), b.cuda(), R.cuda() if R is not None else None, epi=epi, precision="f16").cpu().double()
    ref = _h(A) @ _h(W).T + b.double()
    if epi == "gelu":
        ref = torch.nn.functional.gelu(ref)
    if epi == "residual":
        ref = ref + R.double()
        err = (out - ref).abs().max().item()
        print(f"f16 linear ({M}, {N}, {K}) residual: max-abs vs rounded-operand fp64 {err:.3e}")
        assert err <= 2e-5 * (K / 512) ** 0.5 * 8                                     # fp32 accumulation only (the bf16 test's bound)
        return
    worst = ((out - ref).abs() - ref.abs() * 2.0 ** -11).max().item()
    exact = (out == _h(ref.float())).float().mean().item()
    print(f"f16 linear ({M}, {N}, {K}) {epi}{' subnormal weights' if subnormal else ''}: worst |out - ref| - |ref| 2^-11 = {worst:.3e}, "
          f"{100 * exact:.3f} % of the outputs equal RNE(exact)")
    assert torch.isfinite(out).all()
    assert ((out - ref).abs() <= ref.abs() * 2.0 ** -11 + 2e-5).all()                 # one fp16 rounding of the output
    assert torch.equal(out, _h(out.float()))                                          # the output IS fp16-valued
    assert exact >= RNE_FLOOR, exact


# (B, T, J, temporal): two key tiles; the two-pass (QT = 2) form; the full 256-frame window; the runner's shape; spatial; MU > 1 (units >= 4096)
ATTENTION = [(2, 33, 3, True), (1, 161, 2, True), (1, 256, 1, True), (2, 243, 17, True), (3, 9, 17, False), (70, 27, 17, False)]


@pytest.mark.parametrize("B,T,J,temporal", ATTENTION)
def test_f16_attention_matches_rounded_operand_math(B, T, J, temporal):
    """(softmax(q k^T / 8) - I) v with q / 8, k, v and softmax - I rounded to fp16: the kernel against fp64 math with the same roundings
    (tests/test_gpu_bf16.py's reference with the bf16 round replaced by an fp16 round; q is scaled BEFORE it is rounded, as the mode
    rounds it -- in bf16 the order does not matter, in fp16 it does where q / 8 is subnormal)."""
    g = torch.Generator().manual_seed(B * T)
    qkv = torch.randn(B * T * J, 3 * D, generator=g)
    out = op_attention(qkv.cuda(), B, T, J, H, temporal, precision="f16").cpu().double()
    x = qkv.view(B, T, J, 3, H, 64)
    x = x.permute(3, 0, 2, 4, 1, 5) if temporal else x.permute(3, 0, 1, 4, 2, 5)     # (3, B, J | T, H, N, dh)
    q, k, v = _h(x[0] * 0.125), _h(x[1]), _h(x[2])
    a = q @ k.transpose(-2, -1)
    p = a.softmax(-1) - torch.eye(a.shape[-1], dtype=torch.float64)
    o = _h(_h(p.float()) @ v)                       # the kernel writes fp16
    o = o.permute(0, 3, 1, 2, 4) if temporal else o.permute(0, 1, 3, 2, 4)           # (B, T, J, H, dh)
    ref = o.reshape(B * T * J, D)
    err = (out - ref).abs().max().item()
    exact = (out == ref).float().mean().item()
    print(f"f16 attention B={B} T={T} J={J} temporal={temporal}: max-abs vs rounded-operand fp64 {err:.3e} (|out| max {ref.abs().max():.2f}), "
          f"{100 * exact:.3f} % of the outputs equal RNE(exact)")
    assert torch.isfinite(out).all() and torch.equal(out, _h(out.float()))
    assert err <= 3e-2 / 8 * max(1.0, ref.abs().max().item() / 4) and exact >= RNE_FLOOR, (err, exact)


# ------------------------------------------------------------------------------------------------ the fused kernel
def _fused_operands(rows, seed):
    from diff3dhpe_amd.synth import synth_state_dict
    sd = synth_state_dict(cfg_full(27), 11, family="uniform")
    kw = [k for k in sd if k.endswith("attn.qkv.weight")][2]
    W, b = torch.from_numpy(sd[kw]), torch.from_numpy(sd[kw.replace("weight", "bias")])
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, D, generator=g) * (1.0 + 0.1 * torch.randn(D, generator=g))   # a LayerNorm output with gains
    return (x + 0.1 * torch.randn(D, generator=g)).cuda(), W.cuda(), b.cuda()


FUSED = [(3, T, 3, True) for T in (2, 27, 81, 127, 243, 255)] + [(2, 31, J, False) for J in (1, 15, 17, 32)]


@pytest.mark.parametrize("B,T,J,temporal", FUSED)
def test_f16_fused_equals_linear_then_attention_bit_for_bit(B, T, J, temporal):
    """op_qkv_attn_f16 against op_linear followed by op_attention, both "f16".  The fused kernel rounds q ONCE, after the exact scale by
    2^-3 -- as the engine's un-fused qkv GEMM does (its epilogue scales the q third before it rounds).  The op pair can only show that
    if the q that reaches op_attention is not rounded yet: op_linear's residual form (R = 0) returns the same accumulators + bias as
    fp32, and op_attention then scales and rounds them exactly as the kernel does -- torch.equal.  Through op_linear's fp16 output the
    q third is rounded twice (before and after the scale); the two agree except where q / 8 is an fp16 subnormal, so that composition
    is held to a few fp16 ulps and its share of equal outputs is printed (a property of fp16's range, absent in bf16; measured:
    >= 99.9995 % equal, max-abs <= 2.4e-4).  The torch.equal half failed at T = 81 until every fp16 conversion rounded an fp32 VALUE:
    the compiler had folded the multiply in front of 4 of 16 P conversions per key tile into v_fma_mixlo / mixhi_f16 (one rounding of
    the exact product) in the stand-alone attention kernel and none in the fused one (kernels_attn_bf16.hip f16_point)."""
    A, W, b = _fused_operands(B * T * J, B * T + J)
    groups, N, stride = (B * J, T, J) if temporal else (B * T, J, 1)
    got = op_qkv_attn_f16(A, W, b, groups, N, stride, H, temporal)
    acc = op_linear(A, W, b, torch.zeros(B * T * J, 3 * D, device="cuda"), epi="residual", precision="f16")   # q, k, v before their rounding
    want = op_attention(acc, B, T, J, H, temporal, precision="f16")
    assert torch.isfinite(got).all()
    assert torch.equal(got, want), f"max-abs {maxabs(got, want.cpu()):.3e}"
    qkv = op_linear(A, W, b, epi="none", precision="f16")
    assert torch.equal(qkv, acc.to(torch.float16).float())                              # the GEMM's fp16 output IS the round of those
    lin = (_h(A.cpu()) @ _h(W.cpu()).T + b.cpu().double())
    lin_exact = (qkv.cpu().double() == _h(lin.float())).float().mean().item()
    twice = op_attention(qkv, B, T, J, H, temporal, precision="f16")
    same = (twice == got).float().mean().item()
    print(f"fused f16 B={B} T={T} J={J} temporal={temporal}: q/k/v {100 * lin_exact:.3f} % RNE(exact); through the fp16 qkv output "
          f"{100 * same:.4f} % of the outputs equal, max-abs {maxabs(twice, got.cpu()):.3e}")
    assert lin_exact >= RNE_FLOOR
    assert maxabs(twice, got.cpu()) <= 4 * 2.0 ** -11 * max(1.0, got.abs().max().item()) and same >= 0.99


# ------------------------------------------------------------------------------------------------ the engine against the emulation
def _emulations(fn, sd, *args, dtype=torch.float16, **kw):
    """(emulation with fp32 accumulation, the same with fp64 accumulation, fp32 oracle) of an oracle function."""
    from oracle import d3d_oracle as orc
    f32 = fn(sd, *args, **kw)
    with orc.operand_rounding(dtype):
        e32 = fn(sd, *args, **kw)
    torch.set_default_dtype(torch.float64)
    try:
        dbl = lambda v: v.double() if isinstance(v, torch.Tensor) and v.is_floating_point() else v
        with orc.operand_rounding(dtype):
            e64 = fn({k: v.double() for k, v in sd.items()}, *[({k: dbl(x) for k, x in v.items()} if isinstance(v, dict) else dbl(v)) for v in args], **kw)
    finally:
        torch.set_default_dtype(torch.float32)
    return e32, e64, f32


_DENOISE = {}


def _denoise_case(cfg, B, tag):
    """(xcat, t, emulation fp32-acc, emulation fp64-acc, fp32 oracle) of one denoiser evaluation on weights 91 / inputs 910: computed
    once per module and shared, never written to."""
    if tag not in _DENOISE:
        from oracle import d3d_oracle as orc
        inp = inputs(B, cfg.num_frame, 910)
        xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
        t = torch.tensor([(431 * i + 77) % 1000 for i in range(B)], dtype=torch.long)
        _DENOISE[tag] = (xcat, t) + _emulations(orc.forward_denoise, torch_sd(cfg, 91), xcat, t, depth=cfg.depth, seq2frame=cfg.seq2frame)
    return _DENOISE[tag]


@pytest.fixture(scope="module", autouse=True)
def _drop_cases():
    yield
    _DENOISE.clear()


CASES = [("T27", cfg_full(27), 2, 3), ("T81", cfg_full(81), 1, 2), ("s2f_T27", cfg_full(27, seq2frame=True), 2, 2)]


@pytest.mark.parametrize("tag,cfg,B,S", CASES, ids=[c[0] for c in CASES])
def test_f16_engine_against_the_oracles_fp16_emulation(tag, cfg, B, S):
    from oracle import d3d_oracle as orc
    net, diff = build_product(cfg, 91, sampling=S, precision="f16")
    xcat, t, e32, e64, f32 = _denoise_case(cfg, B, tag)
    assert torch.isfinite(e32).all() and torch.isfinite(e64).all()                   # the emulation itself stays inside fp16's range
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    e1, m1, self_m = maxabs(out, e32), _mpjpe(out, e32), _mpjpe(e32, e64)
    print(f"f16 denoise {tag}: engine vs emulation max-abs {e1:.3e} MPJPE {m1:.3e} | emulation fp32-acc vs fp64-acc max-abs "
          f"{maxabs(e32, e64):.3e} MPJPE {self_m:.3e} | engine vs fp32 oracle max-abs {maxabs(out, f32):.3e} MPJPE {_mpjpe(out, f32):.3e} | "
          f"emulation vs fp32 oracle MPJPE {_mpjpe(e32, f32):.3e}")
    assert torch.isfinite(out).all()
    assert e1 <= GATE_MAXABS and m1 <= max(1.5 * self_m, GATE_MPJPE)
    # the whole sampling
    inp = inputs(B, cfg.num_frame, 910)
    noise = inp["noise"][:, :1].contiguous() if cfg.seq2frame else inp["noise"]
    _, y0 = diff(clean_3d_pose=torch.zeros_like(noise).cuda(), noisy_2d_pose=inp["x2d"].cuda(), output_loss=False, init_noise=noise.cuda())
    kw = dict(num_timesteps=1000, sampling_timesteps=S, depth=cfg.depth, seq2frame=cfg.seq2frame)
    e32, e64, f32 = _emulations(orc.ddim_sample_loop, torch_sd(cfg, 91), orc.diffusion_tables("cosine", 1000), inp["x2d"], noise, **kw)
    assert torch.isfinite(e32).all() and torch.isfinite(e64).all()
    e2, m2, self_m = maxabs(y0, e32), _mpjpe(y0, e32), _mpjpe(e32, e64)
    print(f"f16 ddim {tag} S={S}: engine vs emulation max-abs {e2:.3e} MPJPE {m2:.3e} | emulation fp32-acc vs fp64-acc MPJPE {self_m:.3e} | "
          f"engine vs fp32 oracle max-abs {maxabs(y0, f32):.3e} MPJPE {_mpjpe(y0, f32):.3e}")
    assert e2 <= 2.5 * GATE_MAXABS and m2 <= max(1.5 * self_m, GATE_MPJPE)
    assert y0.abs().max().item() <= 1.0 and torch.isfinite(y0).all()
    eng = diff._engine(dev())
    assert eng.range_flags() == 0                                                    # no precision flag on an f16 engine


def test_f16_is_at_most_a_quarter_of_bf16s_distance_to_fp32():
    """The point of the mode: same weights, same inputs, the same kernels -- the fp16 engine's MPJPE to the fp32 oracle is at most a
    quarter of the bf16 engine's (the emulations give 7.4 x; the factor 4 leaves room for the accumulation order)."""
    cfg = cfg_full(27)
    xcat, t, _, _, f32 = _denoise_case(cfg, 2, "T27")
    dist = {}
    for prec in ("bf16", "f16"):
        net, _ = build_product(cfg, 91, sampling=3, precision=prec)
        dist[prec] = _mpjpe(net.forward_denoise(xcat.cuda(), t.cuda()), f32)
    print(f"MPJPE to the fp32 oracle, cfg_full(27) B=2: bf16 engine {dist['bf16']:.3e}, f16 engine {dist['f16']:.3e} "
          f"(ratio {dist['bf16'] / dist['f16']:.2f})")
    assert dist["f16"] <= dist["bf16"] / 4


def test_f16_mode_on_the_trainedlike_family():
    """Heavy-tailed weights / wide LayerNorm gains (the family of tests/test_gpu_round4.py's bf16 test): the fp16 emulation stays finite
    there -- nothing reaches 65504 at a rounding point -- and the engine meets the gates of the uniform family."""
    from oracle import d3d_oracle as orc
    cfg = cfg_full(27)
    net, _ = product(cfg, 11, "f16", family="trainedlike")
    sd = torch_sd(cfg, 11, family="trainedlike")
    inp = inputs(2, 27, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    e32, e64, f32 = _emulations(orc.forward_denoise, sd, xcat, t, depth=8)
    assert torch.isfinite(e32).all() and torch.isfinite(e64).all()
    out = net.forward_denoise(xcat.cuda(), t.cuda())
    e1, m1, self_m = maxabs(out, e32), _mpjpe(out, e32), _mpjpe(e32, e64)
    print(f"f16 trained-like denoise T=27: engine vs emulation max-abs {e1:.3e} MPJPE {m1:.3e} | emulation self-distance max-abs "
          f"{maxabs(e32, e64):.3e} MPJPE {self_m:.3e} | engine vs fp32 oracle max-abs {maxabs(out, f32):.3e} MPJPE {_mpjpe(out, f32):.3e}")
    assert torch.isfinite(out).all()
    assert e1 <= GATE_MAXABS and m1 <= max(1.5 * self_m, GATE_MPJPE)


def test_f16_unfused_row_kernel_flow_meets_the_same_gates():
    """"fused_postnorm" = 0: stand-alone LayerNorm kernels (their fp16 row output) instead of the whole-row GEMM epilogues -- the same
    rounding points, the same gates."""
    cfg = cfg_full(27)
    net, diff, eng = product_with_engine(cfg, 91, "f16", sampling=3)
    xcat, t, e32, e64, _ = _denoise_case(cfg, 2, "T27")
    fused = net.forward_denoise(xcat.cuda(), t.cuda()).cpu()
    eng.set_option("fused_postnorm", 0)
    plain = net.forward_denoise(xcat.cuda(), t.cuda()).cpu()
    eng.set_option("fused_postnorm", 1)
    self_m = _mpjpe(e32, e64)
    print(f"f16 flows: fused vs emulation MPJPE {_mpjpe(fused, e32):.3e}, row-kernel flow vs emulation {_mpjpe(plain, e32):.3e}, "
          f"fused vs row-kernel flow {_mpjpe(fused, plain):.3e}, emulation self-distance {self_m:.3e}")
    for out in (fused, plain):
        assert maxabs(out, e32) <= GATE_MAXABS and _mpjpe(out, e32) <= max(1.5 * self_m, GATE_MPJPE)
    assert _mpjpe(fused, plain) <= max(1.5 * self_m, GATE_MPJPE) and not torch.equal(fused, plain)


# ------------------------------------------------------------------------------------------------ path independence
def test_f16_paths_agree_bit_for_bit():
    """B = 32 at T = 243: the persistent 256 x 256 walk, the own qkv / fc1 kernel, the fused qkv + attention kernels, the whole-row proj /
    fc2 forms.  Every output element is tile-shape and path independent: ragged chunks of 13, two streams, the fused kernels off, the
    own GEMM kernel off and a hipGraph replay all reproduce the large batch bit for bit."""
    cfg = cfg_full(243)
    _, diff, eng = product_with_engine(cfg, 8, "f16", sampling=1)
    inp = inputs(32, 243, 5)
    x2d, nz = inp["x2d"].cuda(), inp["noise"].cuda()
    big = eng.ddim_sample(x2d, nz).clone()
    assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (1, 1)
    assert torch.isfinite(big).all() and big.abs().max().item() <= 1.0
    assert torch.equal(big, eng.ddim_sample(x2d, nz))
    for lo in (0, 13, 26):
        hi = min(lo + 13, 32)
        assert torch.equal(eng.ddim_sample(x2d[lo:hi].contiguous(), nz[lo:hi].contiguous()), big[lo:hi])
    try:
        eng.set_option("streams", 2)
        assert torch.equal(eng.ddim_sample(x2d, nz), big)
        eng.set_option("streams", 1)
        eng.set_option("fused_spatial", 0)
        eng.set_option("fused_temporal", 0)
        assert torch.equal(eng.ddim_sample(x2d, nz), big)
        assert (eng.info("bf16_fused_spatial_last"), eng.info("bf16_fused_temporal_last")) == (0, 0)
        eng.set_option("bf16_gemm_kernel", 0)                                        # qkv (now a launch of its own) and fc1 on the template
        assert torch.equal(eng.ddim_sample(x2d, nz), big)
        eng.set_option("bf16_gemm_kernel", 1)
        assert torch.equal(eng.ddim_sample(x2d, nz), big)
        eng.set_option("fused_spatial", 1)
        eng.set_option("fused_temporal", 1)
        eng.set_graph_mode(True)
        assert torch.equal(eng.ddim_sample(x2d, nz), big) and torch.equal(eng.ddim_sample(x2d, nz), big)   # capture, then replay
    finally:
        eng.set_graph_mode(False)
        eng.set_option("streams", 2)
        eng.set_option("bf16_gemm_kernel", 1)
        eng.set_option("fused_spatial", 1)
        eng.set_option("fused_temporal", 1)


def test_f16_mode_refuses_shapes_it_has_no_kernels_for():
    import diff3dhpe_amd as d3d
    from diff3dhpe_amd import _lib
    net = d3d.HPE_model(d3d.S2S_NAME)(num_frame=9, embed_dim=32, depth=1)       # head_dim 4
    net.precision = "f16"
    with pytest.raises(_lib.D3DError, match="D3D_PREC_F16"):
        net.engine_for(torch.device("cuda", torch.cuda.current_device()))
