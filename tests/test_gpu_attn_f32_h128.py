"""Exact fp32 attention for heads of 128 columns on the MI355X ("attn_f32_h128", kernels_attn_f32_h128.hip): embed_dim 1024 with the
runner's 8 heads on an FP32 engine -- the exact mode, and the engine a precision-"auto" model falls back to.
  * op level against fp64 math: the resident kernel at every group length N = 1 .. 128 per key-tile class (finite, the same bits twice,
    not the generic kernel's bits throughout a class), spatial groups of 15 / 16 / 17 / 21 / 33 joints, narrow head counts;
  * the key-streaming kernel on both sides of every chunk boundary (128 frames) and of the query-block boundary (256), and bit for bit
    the resident kernel at every T = 1 .. 128;
  * sharp softmax; a NaN batch element does not reach its neighbour; refusals;
  * engine level against the fp64 oracle with the option on and off, invariances, proof of the path through info("attn_f32_h128_last"),
    each block type deciding alone, the other widths and precisions left alone, the fallback engine of precision "auto".

The op-level bound is that of tests/test_gpu_attn_f32_h32.py: err <= max(5e-6, 2 e32), where e32 is the error of the same formula in
plain fp32 torch on the CPU on the same input.

Measured maxima (MI355X), max-abs against fp64 (e32 on the same input in brackets; the bound was 5e-6 .. 6.1e-6 everywhere):

  resident, key tiles     1                  2                  3                  4
    worst (at N)     1.67e-6 (N = 20)   1.69e-6 (N = 61)   1.78e-6 (N = 71)   1.68e-6 (N = 103)
    e32 there        1.68e-6            2.01e-6            2.05e-6            2.53e-6
  spatial, 1 / 3 / 13 frames: 15 joints 1.26e-6 (1.51e-6), 16 joints 1.68e-6 (1.68e-6), 17 joints 1.81e-6 (1.94e-6);
    (1, 2, 21, 1024, 8) 1.33e-6, (1, 1, 33, 128, 1) 1.04e-6, (2, 5, 17, 1024, 8) 1.38e-6
  narrow head counts: (1, 33, 2, 128, 1) 8.4e-7 (1.24e-6), (2, 27, 3, 384, 3) 1.87e-6 (1.48e-6)
  streaming, B = 1, J = 2, D = 1024: T = 1 0, 31 1.02e-6, 32 1.63e-6, 33 1.03e-6, 127 1.21e-6, 128 1.26e-6, 129 1.63e-6, 160 1.05e-6,
    243 1.44e-6, 255 1.40e-6, 256 1.21e-6, 257 1.12e-6, 300 1.33e-6 (e32 1.3e-6 .. 2.7e-6); (1, 385, 2, 256, 2) 1.31e-6 (3.07e-6),
    (1, 513, 2, 128, 1) 9.1e-7 (2.13e-6), (3, 243, 17, 1024, 8) 2.25e-6 (2.66e-6)
  sharp softmax: spatial 1.77e-4 (generic 1.57e-4, 1.47e-4 apart), resident T = 100 1.64e-4 (1.65e-4, 1.85e-4 apart), streaming T = 243
    1.91e-4 (2.23e-4, 2.22e-4 apart)
  engine against the oracle, option on / off: T = 27 3.71e-6 / 3.61e-6 (oracle fp32 floor 3.62e-6), T = 243 7.26e-6 / 6.71e-6 (3.70e-6)
"""
import warnings

import pytest
import torch

import group_lengths as gl
from helpers import hashed, inputs, maxabs, attn_ref, torch_sd, build_net, product_with_engine, xy
from diff3dhpe_amd._lib import D3DError
from diff3dhpe_amd.spec import DenoiserConfig

pytestmark = pytest.mark.gpu
GATE = 1e-4
FLOOR = 5e-6          # test_attention_core's bound for hashed qkv at scale 2.0
DEPTH = 1
KEY, LAST = "attn_f32_h128", "attn_f32_h128_last"
RESIDENT_MAX = 128                 # the longest group whose keys stay in LDS at this width (4 key tiles)
B, J, H, D = 2, 3, 8, 1024         # the temporal sweep: stride J = 3
# the "*_last" keys of the other attention families: none of them may move on an engine that takes these kernels
OTHER_LAST = ("long_temporal_last", "attn_h32_last", "long_temporal_h32_last", "attn_h128_last", "long_temporal_f32_last",
              "attn_f32_h32_last", "long_temporal_f32_h32_last")


def _eng():
    from diff3dhpe_amd import engine
    return engine


def _bound(qkv_cpu, Bn, T, Jn, Hn, temporal):
    """(fp64 reference, max(5e-6, 2 e32), e32) of one problem, on the CPU."""
    ref = attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal)
    e32 = maxabs(attn_ref(qkv_cpu, Bn, T, Jn, Hn, temporal, torch.float32), ref)
    return ref, max(FLOOR, 2 * e32), e32


_BASE = {}


@pytest.fixture(scope="module", autouse=True)
def _drop_base():
    yield
    _BASE.clear()


def _base(name, rows, Dn=D, seed=21, scale=2.0):
    """(cpu, device) hashed qkv rows, made once; a case takes the first rows it needs."""
    if name not in _BASE:
        x = hashed(name, (rows, 3 * Dn), seed, scale)
        _BASE[name] = (x, x.cuda())
    return _BASE[name]


def _sweep(what, cases, run, generic):
    """cases: [(label, argument of run / generic, reference, bound, e32)].  Every failing case is reported at once; the worst error is
    printed."""
    fails, worst, differs = [], (-1.0, None, ""), False
    for label, q, ref, bound, e32 in cases:
        out = run(q)
        err = maxabs(out, ref)
        if not err <= worst[0]:
            worst = (err, label, f" (e32 {e32:.3e}, bound {bound:.3e})")
        if not torch.isfinite(out).all():
            fails.append(f"{label}: the output is not finite")
        if not err <= bound:
            fails.append(f"{label}: err {err:.3e} > {bound:.3e} (e32 {e32:.3e})")
        if not torch.equal(run(q), out):
            fails.append(f"{label}: a second call gives other bits")
        if not torch.equal(generic(q), out):
            differs = True
    print(f"attn_f32_h128 [{what}]: max err {worst[0]:.3e} at {worst[1]}{worst[2]}")
    if not differs:
        fails.append("every case gives the generic kernel's bits: the new kernel did not run")
    assert not fails, f"{what}:\n" + "\n".join(fails)


# ------------------------------------------------------------------------------------------------ 1. resident, every N = 1 .. 128
@pytest.mark.parametrize("c", range(1, 5))
def test_resident_kernel_matches_fp64_at_every_length(c):
    E = _eng()
    cpu, dev = _base("f32h128_tp", B * RESIDENT_MAX * J)
    lengths = [N for N in range(1, RESIDENT_MAX + 1) if gl.nkt(N) == c]
    assert len(lengths) == 32
    cases = []
    for N in lengths:
        rows = B * N * J
        ref, bound, e32 = _bound(cpu[:rows], B, N, J, H, True)
        cases.append((f"N = {N}", (dev[:rows], N), ref, bound, e32))
    _sweep(f"temporal resident, {c} key tiles", cases, lambda a: E.op_attention_f32_h128(a[0], B, a[1], J, H, True),
           lambda a: E.op_attention(a[0], B, a[1], J, H, True, force_generic=True))


# ------------------------------------------------------------------------------------------------ 2. spatial
SPATIAL_FRAMES = (1, 3, 13)


@pytest.mark.parametrize("Jn", [15, 16, 17])
def test_spatial_groups_match_fp64(Jn):
    """One batch element of 1, 3 and 13 frames x 8 heads: a spatial call is (B T, J, 1), one workgroup of one wave per (frame, head)."""
    E = _eng()
    cpu, dev = _base(f"f32h128_sp{Jn}", max(SPATIAL_FRAMES) * Jn)
    cases = []
    for T in SPATIAL_FRAMES:
        rows = T * Jn
        ref, bound, e32 = _bound(cpu[:rows], 1, T, Jn, H, False)
        cases.append((f"{T} frames", (dev[:rows], T), ref, bound, e32))
    _sweep(f"spatial, {Jn} joints", cases, lambda a: E.op_attention_f32_h128(a[0], 1, a[1], Jn, H, False),
           lambda a: E.op_attention(a[0], 1, a[1], Jn, H, False, force_generic=True))


def _one(E, what, Bn, T, Jn, Dn, Hn, temporal, run=None):
    """One shape against fp64 under the bound of this file; the same bits twice.  Returns the output."""
    cpu = hashed(f"qkv{T}_{Jn}_{Dn}", (Bn * T * Jn, 3 * Dn), 21, 2.0)
    ref, bound, e32 = _bound(cpu, Bn, T, Jn, Hn, temporal)
    run = run or (lambda q: E.op_attention_f32_h128(q, Bn, T, Jn, Hn, temporal))
    dev = cpu.cuda()
    got = run(dev)
    err = maxabs(got, ref)
    print(f"attn_f32_h128 [{what}] B={Bn} T={T} J={Jn} D={Dn} H={Hn} temporal={int(temporal)}: max-abs {err:.3e} (e32 {e32:.3e}, "
          f"bound {bound:.3e})")
    assert torch.isfinite(got).all()
    assert err <= bound
    assert torch.equal(run(dev), got)
    return got


@pytest.mark.parametrize("Bn,T,Jn,Dn,Hn", [(1, 2, 21, 1024, 8), (1, 1, 33, 128, 1), (2, 5, 17, 1024, 8)])
def test_spatial_other_joint_counts(Bn, T, Jn, Dn, Hn):
    """21 joints (no other fp32 spatial kernel takes them); 33 joints: two key tiles, two waves, in a spatial call."""
    _one(_eng(), "spatial", Bn, T, Jn, Dn, Hn, False)


# ------------------------------------------------------------------------------------------------ 3. narrow head counts
@pytest.mark.parametrize("Bn,T,Jn,Dn,Hn", [(1, 33, 2, 128, 1), (2, 27, 3, 384, 3)])
def test_narrow_head_counts(Bn, T, Jn, Dn, Hn):
    _one(_eng(), "narrow", Bn, T, Jn, Dn, Hn, True)


# ------------------------------------------------------------------------------------------------ 4. streaming
STREAM = [(1, T, 2, 1024, 8) for T in (1, 31, 32, 33, 127, 128, 129, 160, 243, 255, 256, 257, 300)] + \
         [(1, 385, 2, 256, 2), (1, 513, 2, 128, 1), (3, 243, 17, 1024, 8)]


@pytest.mark.parametrize("Bn,T,Jn,Dn,Hn", STREAM, ids=[f"B{s[0]}_T{s[1]}_J{s[2]}_D{s[3]}" for s in STREAM])
def test_streaming_kernel_matches_fp64(Bn, T, Jn, Dn, Hn):
    """Chunks of 128 frames, query blocks of at most 256: both sides of every boundary up to 300, four chunks + a tail tile at 513."""
    E = _eng()
    _one(E, "streaming", Bn, T, Jn, Dn, Hn, True, run=lambda q: E.op_attention_long_f32_h128(q, Bn, T, Jn, Hn))


# ------------------------------------------------------------------------------------------------ 5. bit identity
@pytest.mark.parametrize("name,seed,scale", [("f32h128_tp", 21, 2.0), ("f32h128_sharp", 22, 9.0)], ids=["scale2", "sharp"])
def test_streaming_kernel_is_bit_identical_to_the_resident_one(name, seed, scale):
    """Every T = 1 .. 128, so every wave count of the resident kernel and every pad-key count."""
    E = _eng()
    _, dev = _base(name, B * RESIDENT_MAX * J, seed=seed, scale=scale)
    differ = []
    for T in range(1, RESIDENT_MAX + 1):
        q = dev[:B * T * J]
        a = E.op_attention_f32_h128(q, B, T, J, H, True)
        if not torch.equal(E.op_attention_long_f32_h128(q, B, T, J, H), a):
            differ.append(T)
        assert torch.isfinite(a).all(), T
    assert not differ, f"other bits at T = {differ}"


# ------------------------------------------------------------------------------------------------ 6. sharp softmax
@pytest.mark.parametrize("Bn,T,Jn,temporal,stream", [(2, 7, 17, False, False), (1, 100, 3, True, False), (1, 243, 3, True, True)])
def test_sharp_softmax(Bn, T, Jn, temporal, stream):
    """Logits up to ~100 (near one-hot rows): the bound of tests/test_gpu_ops.py::test_attention_fast_kernels_agree_with_generic_on_sharp_softmax."""
    E = _eng()
    qkv = hashed(f"sharp{T}", (Bn * T * Jn, 3 * D), 22, 9.0).cuda()
    ref = attn_ref(qkv, Bn, T, Jn, H, temporal).cpu()
    a = E.op_attention_long_f32_h128(qkv, Bn, T, Jn, H) if stream else E.op_attention_f32_h128(qkv, Bn, T, Jn, H, temporal)
    b = E.op_attention(qkv, Bn, T, Jn, H, temporal, force_generic=True)
    print(f"attn_f32_h128 sharp T={T} J={Jn}: new {maxabs(a, ref):.3e} generic {maxabs(b, ref):.3e} apart {maxabs(a, b.cpu()):.3e}")
    assert torch.isfinite(a).all() and torch.isfinite(b).all()
    assert maxabs(a, ref) < 2e-3 and maxabs(b, ref) < 2e-3
    assert maxabs(a, b.cpu()) < 2e-3


# ------------------------------------------------------------------------------------------------ 7. isolation
@pytest.mark.parametrize("T,Jn,temporal", [(243, 2, True), (100, 2, True), (5, 17, False)])
def test_a_nan_batch_element_does_not_reach_its_neighbour(T, Jn, temporal):
    E = _eng()
    Bn = 2
    run = (lambda q, b: E.op_attention_long_f32_h128(q, b, T, Jn, H)) if T > RESIDENT_MAX else \
          (lambda q, b: E.op_attention_f32_h128(q, b, T, Jn, H, temporal))
    qkv = hashed(f"isoqkv{T}_{Jn}_{D}_{Bn}", (Bn * T * Jn, 3 * D), 21, 2.0).cuda()
    bad = qkv.clone()
    bad[T * Jn:] = float("nan")
    alone = run(qkv[:T * Jn].contiguous(), 1)
    both = run(bad, Bn)
    assert torch.isfinite(both[:T * Jn]).all()
    assert torch.equal(both[:T * Jn], alone)


# ------------------------------------------------------------------------------------------------ 8. refusals
@pytest.mark.parametrize("T,Jn,Dn,Hn,temporal", [(27, 2, 512, 8, True), (27, 2, 256, 8, True), (129, 2, 1024, 8, True),
                                                 (1, 129, 1024, 8, False)],
                         ids=["width64", "width32", "129frames", "129joints"])
def test_resident_entry_refuses(T, Jn, Dn, Hn, temporal):
    qkv = torch.zeros((T * Jn, 3 * Dn), device="cuda")
    with pytest.raises(D3DError, match="head_dim 128"):
        _eng().op_attention_f32_h128(qkv, 1, T, Jn, Hn, temporal)


@pytest.mark.parametrize("Dn,Hn", [(512, 8), (256, 8)], ids=["width64", "width32"])
def test_streaming_entry_refuses_other_widths(Dn, Hn):
    qkv = torch.zeros((27 * 2, 3 * Dn), device="cuda")
    with pytest.raises(D3DError, match="head_dim 128"):
        _eng().op_attention_long_f32_h128(qkv, 1, 27, 2, Hn)


# ------------------------------------------------------------------------------------------------ 9. - 12. engine level
def _cfg(T, Dn=1024, Jn=17):
    return DenoiserConfig(num_frame=T, num_joints=Jn, embed_dim=Dn, depth=DEPTH, num_heads=8)


def _sd(cfg, seed=11):   # this module's weights: seed 11 of the trained-like family
    return torch_sd(cfg, seed, family="trainedlike")


def _net(cfg, seed=11, prec="fp32"):
    return build_net(cfg, seed, prec, family="trainedlike")


def _product(cfg, seed=11, prec="fp32", sampling=2):   # this module's defaults; the weights of _sd
    return product_with_engine(cfg, seed, prec, sampling, family="trainedlike")


def _sample(eng, x2d, nz):   # reads this feature's proof-of-path key, LAST
    out = eng.ddim_sample(x2d, nz).clone()
    return out, eng.info(LAST)


def _others(eng):
    return [eng.info(k) for k in OTHER_LAST]


@pytest.mark.parametrize("T,want", [(27, 3), (243, 5)])
def test_forward_denoise_against_the_oracle_with_the_option_on_and_off(T, want):
    """forward_denoise of an FP32 engine at B = 2, trained-like weights, depth 1, per-row t, against oracle/d3d_oracle.py in fp64: the
    kernels for heads of 128 columns (T = 27: both block types resident; T = 243: the temporal blocks streaming) and the generic kernel
    both inside the project's 1e-4 gate."""
    from oracle import d3d_oracle as orc
    cfg = _cfg(T)
    net, _, eng = _product(cfg)
    sd = _sd(cfg)
    inp = inputs(2, T, 500)
    xcat = torch.cat([inp["x2d"], inp["noise"] * 0.7], dim=-1)
    t = torch.tensor([905, 17], dtype=torch.long)
    ref32 = orc.forward_denoise(sd, xcat, t, depth=DEPTH)
    torch.set_default_dtype(torch.float64)      # (the oracle's sinusoid and identity follow the default dtype)
    try:
        ref64 = orc.forward_denoise({k: v.double() for k, v in sd.items()}, xcat.double(), t, depth=DEPTH)
    finally:
        torch.set_default_dtype(torch.float32)
    assert ref64.dtype == torch.float64
    floor = (ref32.double() - ref64).abs().max().item()
    default = eng.info(KEY)
    assert eng.info(LAST) == 0                         # before any forward
    eng.range_flags(clear=True)
    err = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            out = net.forward_denoise(xcat.cuda(), t.cuda())
            assert eng.info(LAST) == (want if opt else 0)
            assert _others(eng) == [0] * len(OTHER_LAST)
            err[opt] = (out.cpu().double() - ref64).abs().max().item()
    finally:
        eng.set_option(KEY, default)
    print(f"attn_f32_h128 T={T} B=2: err_on {err[1]:.3e} err_off {err[0]:.3e} oracle fp32 floor {floor:.3e}")
    assert eng.range_flags() == 0
    assert err[1] <= GATE and err[0] <= GATE


def test_rows_do_not_depend_on_batch_streams_workspace_contents_or_graph_replay():
    T, Bn = 27, 3
    _, _, eng = _product(_cfg(T))
    eng.set_option(KEY, 1)
    x2d, nz = xy(Bn, T, 80)
    eng.set_option("streams", 2)
    whole, last = _sample(eng, x2d, nz)
    assert last == 3 and torch.isfinite(whole).all()
    for b in range(Bn):
        one, last = _sample(eng, x2d[b:b + 1].contiguous(), nz[b:b + 1].contiguous())
        assert last == 3 and torch.equal(one, whole[b:b + 1])
    eng.set_option("streams", 1)
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_option("streams", 2)
    eng._workspace(Bn).view(torch.float32).fill_(float("nan"))
    assert torch.equal(_sample(eng, x2d, nz)[0], whole)
    eng.set_graph_mode(True)
    try:
        first, l1 = _sample(eng, x2d, nz)          # eager warm-up pass + capture + replay
        again = eng.ddim_sample(x2d, nz).clone()   # replay of the cached graph
        assert eng.info("graphs_cached") >= 1
    finally:
        eng.set_graph_mode(False)
    assert l1 == 3
    assert torch.equal(first, whole) and torch.equal(again, whole)


@pytest.mark.parametrize("T,Jn,want", [(27, 129, 2), (300, 17, 5)])
def test_each_block_type_decides_alone(T, Jn, want):
    """129 joints: the spatial blocks stay on k_attn_generic, the temporal ones run the resident kernel; 300 frames: the spatial blocks
    resident, the temporal ones streaming."""
    _, _, eng = _product(_cfg(T, Jn=Jn))
    eng.set_option(KEY, 1)
    assert eng.info(LAST) == 0                     # before any forward
    out, last = _sample(eng, *xy(1, T, 83, Jn))
    assert last == want and torch.isfinite(out).all()
    assert _others(eng) == [0] * len(OTHER_LAST)


def test_engines_with_heads_of_64_columns_ignore_the_option():
    T = 27
    _, _, eng = _product(_cfg(T, Dn=512))
    x2d, nz = xy(2, T, 82)
    default = eng.info(KEY)
    res = {}
    try:
        for opt in (1, 0):
            eng.set_option(KEY, opt)
            res[opt] = _sample(eng, x2d, nz)
    finally:
        eng.set_option(KEY, default)
    assert (res[1][1], res[0][1]) == (0, 0)
    assert torch.isfinite(res[1][0]).all() and torch.equal(res[1][0], res[0][0])


def test_f16x3_engines_are_left_alone():
    """Neither flow of an F16X3 engine at embed_dim 1024 -- the folded one on the F16X3 kernels of this width, the plain one "attn_h128" = 0
    selects (which calls the same attention dispatch with the generic kernel) -- takes the fp32 kernels, and neither changes a bit."""
    T = 27
    _, _, e3 = _product(_cfg(T), prec="f16x3")
    x2d, nz = xy(1, T, 83)
    default, flow_default = e3.info(KEY), e3.info("attn_h128")
    assert e3.info(LAST) == 0
    try:
        for flow in (1, 0):
            e3.set_option("attn_h128", flow)
            res = {}
            for opt in (1, 0):
                e3.set_option(KEY, opt)
                res[opt] = e3.ddim_sample(x2d, nz).clone()
                assert e3.info("attn_h128_last") == (3 if flow else 0) and e3.info(LAST) == 0
            assert torch.isfinite(res[1]).all() and torch.equal(res[1], res[0])
    finally:
        e3.set_option("attn_h128", flow_default)
        e3.set_option(KEY, default)


def test_the_auto_fallback_engine_runs_the_kernels():
    """precision "auto" at T = 27, embed_dim 1024: an input scaled past the plane range raises the F16X3 guard, the call is repeated on the
    exact-fp32 engine -- ONE warning, the fp32 model's result bit for bit, and that engine's blocks on the kernels for heads of 128
    columns."""
    T, Bn = 27, 2
    cfg = _cfg(T)
    net = _net(cfg, prec="auto").cuda()
    net32 = _net(cfg, prec="fp32").cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    net.engine_for(dev, True).set_option(KEY, 1)       # (whatever the default is)
    net32.engine_for(dev).set_option(KEY, 1)
    x2d, nz = xy(Bn, T, 81)
    big = torch.cat([x2d * 1.0e6, nz], dim=-1)
    t = torch.arange(Bn, device="cuda") * 300 + 11
    want = net32.forward_denoise(big, t).clone()
    with warnings.catch_warnings(record=True) as wlog:
        warnings.simplefilter("always")
        got = net.forward_denoise(big, t).clone()
    ours = [w for w in wlog if issubclass(w.category, RuntimeWarning)]
    assert len(ours) == 1 and "range guard fired" in str(ours[0].message), [str(w.message) for w in wlog]
    assert torch.equal(got, want)
    assert net._on_fallback()
    assert net.engine_for(dev, True).info(LAST) == 3
    assert net32.engine_for(dev).info(LAST) == 3
