"""Every group length of every attention hook against fp64 math, and every window regime of the default F16X3 engine flow against the
CPU oracle, on the MI355X.

The attention kernels choose their code from the group length N (frames T in temporal blocks, joints J in spatial ones): the key-tile
count ceil(N / 32) and the pad keys of the last tile, resident or key-streaming, and in the fused temporal kernel the grouped form
(T <= 127: min(255 / T, J) joints per tile), the single-group form (T = 193 .. 255) or neither.  tests/group_lengths.py holds the lengths
and the arithmetic; tests/test_group_lengths_host.py keeps them from shrinking.

1. Op level.  Inputs: hashed rows at scale 2.0, 8 heads, B = 2 and J = 3 (the temporal stride), every length the first B N J rows of
   one tensor per width.  One test per hook and key-tile class (beyond 256 keys: per 256-key chunk count, class id 100 x chunks), which
   loops over the class's lengths and reports every failing N at once.
     * fp32, F16X3, head-width-32 and key-streaming hooks: err(N) <= max(5e-6, 2 e32(N)) against attn_ref of helpers.py in fp64.
       5e-6 is test_attention_core's bound for this data; e32(N) is the error of the same formula in plain fp32 torch on the CPU on the
       same input (median 2.3e-6, at most 3.9e-6 for N <= 256: the floor is almost always the active term).  A wrong mask or row map
       costs 1e-2 and more.
     * the small-tile hook: the rule of test_gpu_small_tiles.py, at most 1.5 x the error of the two-kernel ops on the same input.
     * bf16 attention: the bound pair of test_gpu_bf16.py (max-abs and the share of outputs that are RNE of the exact value, on the
       same rounded operands); the fused bf16 hook: bit for bit its two-op composition, as in test_gpu_bf16_fused_attn.py.
     * every hook, every N: finite, a second call gives the same bits; the key-streaming kernels give the resident kernels' bits
       where both run (N <= 256); over a key-tile class the F16X3 result differs from the fp32 kernel's in at least one bit (the hook
       falls back to fp32 silently where its predicate fails: equal bits throughout would mean the F16X3 kernel never ran).
2. Engine level.  DenoiserConfig(num_frame=T, embed_dim=512, depth=2), precision "f16x3", default options, B = 2 with two timesteps:
   inside the 1e-4 gate of the CPU oracle, finite, a clean guard word, reproducible; against "fused_temporal" = 0 bit for bit where the
   contract says so (T = 193 .. 255) or the option is inert (128 .. 192, 256, 257), within 2e-5 and batch-independent in the grouped form;
   and the path proven from the per-kernel trace: the two-kernel flow traces q / k / v planes (kernel id 2) in the odd blocks.

Measured maxima (MI355X), max-abs against the reference named above, per hook and class (the N of the maximum in brackets; e32 there):

  class (key tiles)      1              2              3              4              5              6              7              8
  fp32            1.41e-6 (29)   2.15e-6 (63)   2.50e-6 (90)   2.91e-6 (100)  3.11e-6 (156)  3.75e-6 (191)  4.56e-6 (219)  4.38e-6 (233)
    e32 there     1.41e-6        1.91e-6        2.50e-6        2.67e-6        2.67e-6        3.28e-6        2.15e-6        2.23e-6
  fp32 generic    1.27e-6 (32)   2.15e-6 (63)   2.21e-6 (95)   2.72e-6 (128)  3.00e-6 (160)  3.13e-6 (192)  3.98e-6 (224)  3.57e-6 (256); N = 257: 3.77e-6
  F16X3           1.05e-6 (27)   9.93e-7 (46)   1.13e-6 (84)   1.21e-6 (106)  1.23e-6 (148)  1.34e-6 (184)  1.50e-6 (209)  1.34e-6 (252)
  head width 32   7.83e-7 (30)   7.33e-7 (48)   9.16e-7 (95)   9.33e-7 (115)  1.07e-6 (152)  8.82e-7 (184)  8.29e-7 (218)  8.37e-7 (241)
  small tiles     1.76e-6 (19)   1.83e-6 (61)   1.88e-6 (96)   1.81e-6 (121)      two-kernel ops there: 1.22e-6, 1.46e-6, 1.44e-6, 1.45e-6
  bf16            1.56e-2 in every class (bound 3e-2); least share of RNE(exact) outputs 99.941 % (N = 10), >= 99.975 % from class 2 on
  spatial forms (N = 1 .. 32): F16X3 1.00e-6 (7), head width 32 8.09e-7 (27), small tiles 1.60e-6 (15 joints, 20 groups; two-kernel 1.42e-6)
  fused bf16 hook: bit for bit op_linear + op_attention at all 255 temporal and 32 spatial lengths

  key-streaming      N <= 32        33 .. 64       255, 256       257 .. 512     513 .. 768     769
  F16X3           1.05e-6 (27)   9.93e-7 (46)   1.21e-6 (255)  1.40e-6 (290)  8.86e-7 (545)  9.04e-7
  fp32            1.41e-6 (29)   2.15e-6 (63)   3.81e-6 (256)  2.37e-6 (289)  1.58e-6 (545)  1.24e-6      (e32 at 769: 3.07e-6)

The fp32 key-streaming kernel first ran here at 5.05e-6 (N = 511), 6.29e-6 (768) and 6.43e-6 (769, bound 6.15e-6: red): the - 1 of the
diagonal inside P left the accumulator at |v| for the rest of the key walk.  Beyond 256 keys it now subtracts v[query] at the store
(kernels_attn_f32_long.hip); the figures above are those of the kernel as it stands.  The resident fp32 kernel, whose bits it keeps for
N <= 256, shows the same growth (4.56e-6 at N = 219) inside its bound.

Engine level, max-abs against the oracle: 1.01e-6 (T = 2) .. 1.82e-6 (T = 31) over the 57 cases; grouped form against the two-kernel flow
at most 6.26e-7 (T = 97), 0 at T = 2, 8, 16, 32, 64, 96.
"""
import pytest
import torch

import group_lengths as gl
from helpers import hashed, maxabs, torch_sd, attn_ref
from diff3dhpe_amd.spec import DenoiserConfig
from diff3dhpe_amd.synth import synth_inputs

pytestmark = pytest.mark.gpu
B, J, H = 2, 3, 8
FLOOR = 5e-6          # test_attention_core's bound for hashed qkv at scale 2.0
GATE = 1e-4


def _E():
    from diff3dhpe_amd import engine
    return engine


# ------------------------------------------------------------------------------------------------ inputs and references, made once
_BASE, _REF, _MISC = {}, {}, {}


@pytest.fixture(scope="module", autouse=True)
def _drop_caches():
    yield
    _BASE.clear(), _REF.clear(), _MISC.clear()


def _base(D):
    """(cpu, device) hashed qkv rows at scale 2.0 for the longest group of width D; length N takes the first B N J rows."""
    if D not in _BASE:
        longest = max(gl.SWEEPS["long"]) if D == 512 else gl.RESIDENT_MAX
        x = hashed(f"glqkv{D}", (B * longest * J, 3 * D), 21, 2.0)
        _BASE[D] = (x, x.cuda())
    return _BASE[D]


def _shape(N, spatial):
    """(B, T, J) of the temporal call: stride J = 3, or the spatial form -- B J groups of N consecutive tokens, stride 1."""
    return (B * J, N, 1) if spatial else (B, N, J)


def _case(D, N, spatial):
    """(qkv on the device, fp64 reference on the CPU, e32)."""
    key = (D, N, spatial)
    cpu, dev = _base(D)
    rows = B * N * J
    if key not in _REF:
        ref = attn_ref(cpu[:rows], *_shape(N, spatial), H, True)
        _REF[key] = (ref, maxabs(attn_ref(cpu[:rows], *_shape(N, spatial), H, True, torch.float32), ref))
    return (dev[:rows],) + _REF[key]


# call -> (width, spatial form, the call); the ones tests/group_lengths.py has a sweep for are the hooks under test
CALLS = {
    "fp32": (512, False, lambda E, q, N: E.op_attention(q, B, N, J, H, True, precision="fp32")),
    "fp32_spatial": (512, True, lambda E, q, N: E.op_attention(q, B * J, N, 1, H, True, precision="fp32")),
    "fp32_generic": (512, False, lambda E, q, N: E.op_attention(q, B, N, J, H, True, precision="fp32", force_generic=True)),
    "f16x3": (512, False, lambda E, q, N: E.op_attention(q, B, N, J, H, True, precision="f16x3")),
    "f16x3_spatial": (512, True, lambda E, q, N: E.op_attention(q, B * J, N, 1, H, True, precision="f16x3")),
    "h32": (256, False, lambda E, q, N: E.op_attention_h32(q, B, N, J, H, True)),
    "h32_spatial": (256, True, lambda E, q, N: E.op_attention_h32(q, B, J, N, H, False)),     # (the hook's own spatial branch)
    "long": (512, False, lambda E, q, N: E.op_attention_long(q, B, N, J, H)),
    "long_f32": (512, False, lambda E, q, N: E.op_attention_long_f32(q, B, N, J, H)),
}
HOOKS = [h for h in CALLS if h in gl.SWEEPS]
# the fp32 kernel whose bits an F16X3 result must differ from somewhere in the class (proof of the path) ...
FP32_KERNEL = {"f16x3": "fp32", "f16x3_spatial": "fp32_spatial"}
# ... and the resident kernel whose bits a key-streaming kernel must give for N <= 256
RESIDENT_TWIN = {"long": "f16x3", "long_f32": "fp32"}


def _report(what, c, worst):
    err, N, note = worst
    print(f"group lengths [{what}] class {c}: max err {err:.3e} at N = {N}{note}")


@pytest.mark.parametrize("hook,c", [p for h in HOOKS for p in gl.class_params(h)])
def test_attention_hook_matches_fp64_at_every_length(hook, c):
    E = _E()
    D, spatial, run = CALLS[hook]
    other = CALLS[FP32_KERNEL[hook]][2] if hook in FP32_KERNEL else None
    twin = CALLS[RESIDENT_TWIN[hook]][2] if hook in RESIDENT_TWIN else None
    fails, worst, differs = [], (-1.0, None, ""), False
    for N in gl.class_lengths(hook, c):
        q, ref, e32 = _case(D, N, spatial)
        out = run(E, q, N)
        err, bound = maxabs(out, ref), max(FLOOR, 2 * e32)
        if not err <= worst[0]:
            worst = (err, N, f" (e32 {e32:.3e}, bound {bound:.3e})")
        if not torch.isfinite(out).all():
            fails.append(f"N = {N}: the output is not finite")
        if not err <= bound:
            fails.append(f"N = {N}: err {err:.3e} > {bound:.3e} (e32 {e32:.3e})")
        if not torch.equal(run(E, q, N), out):
            fails.append(f"N = {N}: a second call gives other bits")
        if other is not None and not torch.equal(other(E, q, N), out):
            differs = True
        if twin is not None and N <= gl.RESIDENT_MAX and not torch.equal(twin(E, q, N), out):
            fails.append(f"N = {N}: not the bits of the resident kernel")
    _report(hook, c, worst)
    if other is not None and not differs:
        fails.append("every length gives the fp32 kernel's bits: the F16X3 kernel did not run")
    assert not fails, f"{hook}, class {c}:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------------ small tiles
def _small_operands():
    """The operands of test_gpu_small_tiles.py's op test; x for the longest group, length N takes the first rows."""
    import numpy as np
    if "small" not in _MISC:
        Dm = 512
        x = hashed("glstx", (B * J * gl.SMALL_ROWS, Dm), 41, 2.0)
        W = hashed("stW", (3 * Dm, Dm), 42, 1.0 / np.sqrt(Dm))
        b = hashed("stb", (3 * Dm,), 43, 0.5)
        g = 1 + 0.2 * hashed("stg", (Dm,), 44)
        be = 0.2 * hashed("stbe", (Dm,), 45)
        _MISC["small"] = (x, tuple(t.cuda() for t in (W, b, g, be)), (W, b, g, be))
    return _MISC["small"]


def _small_case(E, N, stride, groups, fails):
    """One (N, stride, groups) of the small-tile hook: (its error, the two-kernel ops' error)."""
    from test_gpu_small_tiles import _fp64_attention
    x, (W, b, g, be), host = _small_operands()
    x = x[:groups * N]
    ref = _fp64_attention(x, *host, 1e-6, groups, N, stride)
    xd = x.cuda()
    run = lambda: E.op_qkv_attn_x3_small(xd, W, b, g, be, 1e-6, groups, N, stride, H, stride != 1)
    got = run()
    qkv = E.op_linear(E.op_layernorm(xd, g, be, 1e-6), W, b, epi="none", precision="f16x3")
    two = E.op_attention(qkv, groups // stride, N, stride, H, True, precision="f16x3")
    e_small, e_two = maxabs(got, ref), maxabs(two, ref)
    tag = f"N = {N}, groups = {groups}"
    if not torch.isfinite(got).all():
        fails.append(f"{tag}: the output is not finite")
    if not e_small <= 1.5 * e_two:
        fails.append(f"{tag}: err {e_small:.3e} > 1.5 x {e_two:.3e} (the two-kernel ops)")
    if not torch.equal(run(), got):
        fails.append(f"{tag}: a second call gives other bits")
    return e_small, e_two


@pytest.mark.parametrize("hook,c", gl.class_params("small"))
def test_small_tile_hook_at_every_length(hook, c):
    """Temporal form, stride J = 3, groups = 2 x 3: N = 1 .. 127 covers every count 127 // N of whole groups per 128-row tile."""
    E = _E()
    fails, worst = [], (-1.0, None, "")
    for N in gl.class_lengths(hook, c):
        e_small, e_two = _small_case(E, N, J, B * J, fails)
        if not e_small <= worst[0]:
            worst = (e_small, N, f" (two-kernel ops {e_two:.3e})")
    _report("small tiles", c, worst)
    assert not fails, f"small tiles, class {c}:\n" + "\n".join(fails)


def test_small_tile_hook_spatial_form():
    """15 / 16 / 17 joints, stride 1: one frame, a tile one frame short of full, full, one frame over, and three tiles."""
    E = _E()
    fails, worst = [], (-1.0, None, "")
    for N, groups in gl.SMALL_SPATIAL:
        e_small, e_two = _small_case(E, N, 1, groups, fails)
        if not e_small <= worst[0]:
            worst = (e_small, N, f", groups = {groups} (two-kernel ops {e_two:.3e})")
    _report("small tiles, spatial", 1, worst)
    assert not fails, "small tiles, spatial form:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------------ bf16
def _bf16_reference(qkv, N):
    """test_bf16_attention_matches_rounded_operand_math's reference (that test forms it inline), temporal form: fp64 math on q, k, v and
    softmax - I rounded to bf16, the output rounded to bf16."""
    from test_gpu_bf16 import _bf
    x = qkv.view(B, N, J, 3, H, 64).permute(3, 0, 2, 4, 1, 5)          # (3, B, J, H, N, dh)
    q, k, v = _bf(x[0]), _bf(x[1]), _bf(x[2])
    a = (q @ k.transpose(-2, -1)) * 0.125
    p = a.softmax(-1) - torch.eye(N, dtype=torch.float64)
    o = _bf(_bf(p.float()) @ v)
    return o.permute(0, 3, 1, 2, 4).reshape(B * N * J, 512)


@pytest.mark.parametrize("hook,c", gl.class_params("bf16"))
def test_bf16_attention_at_every_length(hook, c):
    E = _E()
    cpu, dev = _base(512)
    fails, worst, least = [], (-1.0, None, ""), (2.0, None)
    for N in gl.class_lengths(hook, c):
        rows = B * N * J
        run = lambda: E.op_attention(dev[:rows], B, N, J, H, True, precision="bf16")
        got = run()
        out = got.cpu().double()
        ref = _bf16_reference(cpu[:rows], N)
        err, exact = (out - ref).abs().max().item(), (out == ref).float().mean().item()
        bound = 3e-2 * max(1.0, ref.abs().max().item() / 4)
        if not err <= worst[0]:
            worst = (err, N, f" (bound {bound:.3e})")
        if exact < least[0]:
            least = (exact, N)
        if not torch.isfinite(got).all():
            fails.append(f"N = {N}: the output is not finite")
        if not (err <= bound and exact >= 0.998):
            fails.append(f"N = {N}: err {err:.3e} (bound {bound:.3e}), {100 * exact:.3f} % of the outputs equal RNE(exact) (bound 99.8 %)")
        if not torch.equal(run(), got):
            fails.append(f"N = {N}: a second call gives other bits")
    _report("bf16", c, (worst[0], worst[1], worst[2] + f"; least share of RNE(exact) outputs {100 * least[0]:.3f} % at N = {least[1]}"))
    assert not fails, f"bf16, class {c}:\n" + "\n".join(fails)


@pytest.mark.parametrize("hook,c", gl.class_params("qkv_bf16") + gl.class_params("qkv_bf16_spatial"))
def test_fused_bf16_hook_equals_its_two_op_composition_at_every_length(hook, c):
    from test_gpu_bf16_fused_attn import _qkv_weights, _rows
    E = _E()
    if "qkv_bf16" not in _MISC:
        _MISC["qkv_bf16"] = tuple(t.cuda() for t in _qkv_weights("uniform")) + (_rows(B * J * 255, 77).cuda(),)
    W, b, A = _MISC["qkv_bf16"]
    temporal = hook == "qkv_bf16"
    fails = []
    for N in gl.class_lengths(hook, c):
        a = A[:B * N * J]
        qkv = E.op_linear(a, W, b, epi="none", precision="bf16")
        # spatial: B x 3 frames of N joints
        want = E.op_attention(qkv, B, N, J, H, True, precision="bf16") if temporal else E.op_attention(qkv, B, J, N, H, False, precision="bf16")
        run = lambda: E.op_qkv_attn_bf16(a, W, b, B * J, N, J if temporal else 1, H, temporal)
        got = run()
        if not torch.isfinite(got).all():
            fails.append(f"N = {N}: the output is not finite")
        if not torch.equal(got, want):
            fails.append(f"N = {N}: not the bits of op_linear + op_attention, max-abs {maxabs(got, want.cpu()):.3e}")
        if not torch.equal(run(), got):
            fails.append(f"N = {N}: a second call gives other bits")
    print(f"group lengths [{hook}] class {c}: bit for bit op_linear + op_attention at {len(gl.class_lengths(hook, c))} lengths")
    assert not fails, f"{hook}, class {c}:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------------ engine level
def _engine(cfg, sd, prec="f16x3"):
    """As _engine of test_gpu_isolation.py: an Engine of its own with seeded weights and a 3-step schedule."""
    from diff3dhpe_amd.engine import Engine
    from oracle import d3d_oracle as orc
    eng = Engine(cfg, precision=prec)
    eng.load_weights(sd)
    tabs = orc.diffusion_tables("cosine", 1000)
    eng.set_schedule(tabs["alphas_cumprod"], tabs["sqrt_one_minus_alphas_cumprod"], 3, 0.0, True)
    return eng


def _traced_kernels(eng, call):
    """(result, {(block, kernel id)}) of one forward under the per-kernel trace (include/d3d.h: tag = ... block << 8 | kernel << 4 | buffer)."""
    eng.set_trace(4096, 1)
    try:
        out = call().clone()
        tags = [t for t, _ in eng.trace_read()]
    finally:
        eng.set_trace(0)
    return out, {((t >> 8) & 0xFF, (t >> 4) & 0xF) for t in tags}


@pytest.mark.parametrize("T,Jn", gl.ENGINE_CASES)
def test_engine_window_regime(T, Jn):
    from oracle import d3d_oracle as orc
    cfg = DenoiserConfig(num_frame=T, num_joints=Jn, embed_dim=512, depth=2)
    sd = torch_sd(cfg, 21)
    eng = _engine(cfg, sd)
    inp = {k: torch.from_numpy(v) for k, v in synth_inputs(2, T, Jn, seed=400 + T + Jn).items()}
    t = torch.tensor([77, 508])
    x2d, y, td = inp["x2d"].cuda(), (inp["noise"] * 0.7).cuda(), t.float().cuda()
    denoise = lambda: eng.denoise(x2d, y, td)
    eng.range_flags(clear=True)
    out = denoise().clone()
    flags = eng.range_flags()
    ref = orc.forward_denoise(sd, torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1), t, depth=cfg.depth)
    err = maxabs(out, ref)
    path = gl.temporal_path(T)
    print(f"engine T = {T} J = {Jn} [{path}]: max-abs vs oracle {err:.3e}")
    assert torch.isfinite(out).all() and flags == 0
    assert err <= GATE, err
    assert torch.equal(denoise(), out)
    # the path, from the plan's own words and from the trace
    assert eng.info("long_temporal_last") == int(T > 256)
    assert eng.info("fused_spatial_last") == int(gl.fused_spatial(Jn))
    traced, kernels = _traced_kernels(eng, denoise)
    assert torch.equal(traced, out)
    odd = [k for k in range(2 * cfg.depth) if k & 1]
    assert all((k, 3) in kernels for k in range(2 * cfg.depth)), sorted(kernels)      # every block traced its attention output
    qkv_planes = [(k, 2) in kernels for k in odd]
    assert qkv_planes == [not gl.fused_temporal(T)] * len(odd), (T, path, qkv_planes)
    assert gl.fused_temporal(T) == (2 <= T <= 127 or 193 <= T <= 255)
    # against the two-kernel temporal flow
    eng.set_option("fused_temporal", 0)
    plain, kernels0 = _traced_kernels(eng, denoise)
    eng.set_option("fused_temporal", 1)
    assert all((k, 2) in kernels0 for k in odd)
    if path == "grouped":
        e_plain = maxabs(out, plain.cpu())
        print(f"engine T = {T} J = {Jn}: grouped form vs two-kernel flow {e_plain:.3e}")
        assert e_plain <= 2e-5, e_plain
        for i in range(2):
            alone = eng.denoise(x2d[i:i + 1].contiguous(), y[i:i + 1].contiguous(), td[i:i + 1].contiguous())
            assert torch.equal(alone, out[i:i + 1]), i
    else:       # the single-group form's contract (193 .. 255); elsewhere the option is inert
        assert torch.equal(out, plain), maxabs(out, plain.cpu())
